/* hello_mi355x.h -- C ABI of the MI355X (gfx950) engine for HELLO's variant-scoring hot path.
 *
 * The reference has no native interface on this path: the network is a pickled torch module that
 * python/caller_calling.py:863-868 loads and :651-652 calls per site, and that
 * python/MixtureOfExpertsDNNFast.py:120-134 calls per batch.  This header is the boundary a
 * maintainer binds instead (ctypes stub in INTEGRATION.md); each entry point names the reference
 * interface it stands in for.  Plain pointers and sizes only; no torch types.
 *
 * Conventions
 *   - every function returns 0 on success or a negative hello_status; it never throws; the message
 *     for the calling thread's last failure is hello_last_error().
 *   - pileup tensors are uint8, channels-last [reads][window][channels], exactly what the C++
 *     featurizer emits (c++/src/AlleleSearcherLiteFiltered.cpp:1045,1172).  HELLO_LAYOUT_RCL accepts
 *     the training-storage layout [reads][channels][window] (python/MemmapDatasetLoader.py:68-74).
 *   - count arrays (reads per allele, alleles per site) are ALWAYS host memory (they are tiny and the
 *     engine builds its CSR offsets from them on the host); the large tensors and the outputs are
 *     host or device memory according to `flags`.
 *   - an engine instance is not re-entrant: one instance per (process, device), calls issued from one
 *     thread at a time, all on the same stream.  With device outputs the call is asynchronous and
 *     stream-ordered; with host outputs it returns after the results have landed.
 */
#ifndef HELLO_MI355X_H
#define HELLO_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HELLO_ABI_VERSION 2      /* 2: CONV1D groups in c1, two-source CONV1D (src1 / seg), XATTN_FRONT, flags 64 / 128 on
                                    READCONV_FUSED only (a CONV1D carrying them is refused), hello_site_records */

typedef enum hello_status {
    HELLO_OK = 0,
    HELLO_ERR_ARG = -1,      /* NULL / negative / inconsistent argument                      */
    HELLO_ERR_SHAPE = -2,    /* counts do not add up (sum reads_per_allele != n_reads, ...)  */
    HELLO_ERR_MODEL = -3,    /* malformed model description                                  */
    HELLO_ERR_HIP = -4,      /* a HIP runtime call failed                                    */
    HELLO_ERR_NOGPU = -5,    /* no gfx950 device visible                                     */
    HELLO_ERR_NOMEM = -6     /* host memory exhausted inside the library (no C++ exception crosses the boundary) */
} hello_status;

/* ---- model description: a flat program over activation buffers ------------------------------
 * The Python host (hello_amd/compiler.py) lowers a MoEAttention model
 * (python/MixtureOfExpertsAdvanced.py:71-252, built from python/NNTools.py:633-657 layer lists) into
 * this program once, with weight-norm / batch-norm already folded into the weights
 * (python/NNTools.py:780-799).  Activations are float32, channels-last [rows][length][channels]. */

typedef enum hello_domain {          /* what a buffer's rows are */
    HELLO_ROWS_READS0 = 0,
    HELLO_ROWS_READS1 = 1,
    HELLO_ROWS_ALLELES = 2,
    HELLO_ROWS_SITES = 3
} hello_domain;

typedef enum hello_segment {         /* which ragged reduction (reduceSlots, MixtureOfExpertsAdvanced.py:23-34) */
    HELLO_SEG_READS0_TO_ALLELES = 0,
    HELLO_SEG_READS1_TO_ALLELES = 1,
    HELLO_SEG_ALLELES_TO_SITES = 2
} hello_segment;

/* reserved buffer ids: the caller's inputs */
#define HELLO_BUF_NONE   (-1)
#define HELLO_BUF_READS0 0           /* uint8 [R0][L][C0] */
#define HELLO_BUF_READS1 1           /* uint8 [R1][L][C1] */
#define HELLO_BUF_REF    2           /* uint8 [S][L][5]  one-hot reference (caller_calling.py:53-97) */
#define HELLO_BUF_FIRST_SCRATCH 3

typedef enum hello_op_kind {
    HELLO_OP_CONV1D = 1,     /* Conv1d + bias (+ReLU) (+ residual add after the activation)          */
    HELLO_OP_MAXPOOL = 2,    /* MaxPool1d(k, stride, pad), floor mode                                 */
    HELLO_OP_SEGSUM = 3,     /* dst[seg] = sum of src rows of the segment (reduceSlots)               */
    HELLO_OP_MIX = 4,        /* dst[a] = a0*src0[a] + a1*src1[site(a)]  (xattn_subtract.py:14-42)      */
    HELLO_OP_HEAD = 5,       /* mean over length, Linear C->cout (terminus, NNTools.py:517-566);      */
                             /* writes output slot `dst`: 0..2 expert logits, 3 meta (+softmax)       */
    HELLO_OP_CONCAT = 6,     /* channel concat of src0 (cin ch) and src1 (c1 ch)                      */
    HELLO_OP_ADD = 7,        /* dst = src0 + src1                                                     */
    HELLO_OP_READCONV_FUSED = 8 /* whole read convolver + reads->alleles segment sum in one kernel:
                                 * canonical architecture (architectures/read_convolver.py) on 150 bp windows
                                 * (+0 | 2 extra blocks in k; from the bytes with FLAG_SRC_U8, else from the
                                 * pooled stem output), or on 250 bp windows (from the bytes, Winograd form);
                                 * dst rows are [36 | 61][64] per allele                                   */
    ,
    HELLO_OP_LAYERNORM = 9   /* LayerNormModule (NNTools.py:802-828) between a convolution and its activation:
                              * dst[r][l][:] = act((src0[r][l][:] - mean) / sqrt(var + a0) * gamma + beta) (+ res), mean and
                              * biased variance over the cin channels of the position; gamma at w_off, beta at b_off,
                              * eps in a0; flags: HELLO_FLAG_RELU | HELLO_FLAG_SOFTPLUS                                */
    ,
    HELLO_OP_COMPRESSOR_FUSED = 10 /* the whole allele-level compressor (architectures/compressor_conv_small.py:8-55) in
                              * one LDS-resident kernel: 1x1 64->64, strided block 64->128 with its 1x1 shortcut, k (2 .. 4)
                              * identity residual blocks; src0 rows [36][64] -> dst rows [18][128]; ReLU; k3/s1 convolutions
                              * in Winograd F(3,3) form, weights packed by hello_amd/readconv_pack.py pack_compressor       */
    ,
    HELLO_OP_XATTN_FRONT = 11 /* the front of the allele-level expert (architectures/xattn_subtract.py:9-60) in one LDS-resident
                              * kernel: x = a0 src0[a] + a1 src1[site(a)] (HELLO_FLAG_MIX_REST: x = src0[a] - (src1[site(a)] - src0[a]), as
                              * MIX) ([18][128] rows; src1 = HELLO_BUF_NONE: the site's row is
                              * the sum of its alleles' src0 rows, formed in the kernel in allele order -- the SEGSUM of src0 over
                              * HELLO_SEG_ALLELES_TO_SITES folded in, same bits), 1x1 128->128 + ReLU, then the strided
                              * block's first convolution (k3 s2 p1 128->256 + ReLU) -> dst and its 1x1 s2 shortcut -> the buffer
                              * named by `res` (an OUTPUT here: the block's second convolution reads it as its residual); both
                              * [9][256] rows; weights packed by hello_amd/readconv_pack.py pack_xattn_front                  */
} hello_op_kind;

#define HELLO_FLAG_RELU     1
#define HELLO_FLAG_SRC_U8   2        /* src0 is one of the uint8 input buffers                       */
#define HELLO_FLAG_SOFTMAX  4        /* HEAD: softmax over cout (meta expert, :229-232)              */
#define HELLO_FLAG_SOFTPLUS 16       /* CONV1D: Softplus(beta 1, threshold 20) instead of ReLU (…_layer_norm.py:16) */
#define HELLO_FLAG_WINOGRAD 32       /* READCONV_FUSED: k3/s1 convolutions in Winograd form (150 bp: residual trunk
                                        F(3,3), stem F(2,3); 250 bp: F(2,3)); weights as hello_amd/readconv_pack.py
                                        packs them for that form and window;
                                        CONV1D (k 3, stride 1, pad 1): weights are the T Winograd taps, packed
                                        [cout][cin/8][T][8]; T = 5 (F(3,3)) when lin % 3 == 0, else 4 (F(2,3)) */
#define HELLO_FLAG_BF16X3   64       /* READCONV_FUSED (whole kernel from the bytes, 150 bp, ReLU, Winograd form, k = 0): arithmetic mode
                                        "bf16x3" -- the seven 64 -> 64 trunk convolutions on the bf16 matrix cores as 3-term
                                        splits x w ~= xh wh + xh wl + xl wh of pre-split operands; their split weights
                                        (hello_amd/readconv_pack.py pack_bf16x3) follow the op's fp32 weight block.  Never
                                        the default: results differ from exact fp32 at the 1e-6 level of the activations */
#define HELLO_FLAG_BF16X3_32 128     /* with HELLO_FLAG_BF16X3 ("bf16x3+32"): the six 32 -> 32 convolutions of the ResidualBlock(32)s too */
#define HELLO_FLAG_MIX_REST 8        /* MIX: dst[a] = src0[a] - (src1[site(a)] - src0[a])  (:372-383)  */
#define HELLO_FLAG_POLYPHASE 2048    /* READCONV_FUSED (an addition within ABI version 2; whole kernel from the bytes, 150 bp, ReLU, Winograd
                                        form, fp32, not the wide trunk): the strided 32 -> 64 convolution runs in polyphase form --
                                        centre tap over the even phase, outer taps over the odd phase as Winograd F(3,2): 7 instead of
                                        9 contractions per 3 outputs.  Its weights (hello_amd/readconv_pack.py pack_polyphase) follow
                                        the op's fp32 weight block.  COMPRESSOR_FUSED: its strided 64 -> 128 convolution likewise
                                        (pack_compressor_polyphase behind the op's block; the compiler sets it on request only).  Same fp32 arithmetic; results differ from
                                        the direct form by float re-association only */
/* Lanes (an addition within ABI version 2): bits 8..10 of `flags` name the stream an op runs on, 0 = the call's own stream.  A model
 * of two read technologies / three experts is several INDEPENDENT chains (MixtureOfExpertsAdvanced.py:161-252: read convolver +
 * compressor + expert per technology, the combined expert, the meta network); a launch of a few sites is latency-bound -- every chain
 * is a handful of workgroups -- so a program for SMALL launches puts the chains on lanes and the engine runs them concurrently,
 * ordering lanes with events wherever an op reads what another lane wrote (derived from the buffer ids).  Such a program must write
 * every scratch buffer from ONE op (no buffer reuse) and read none before its writer: hello_engine_create refuses it otherwise
 * (HELLO_ERR_MODEL, decided on the host before any device is looked up).  The buffer ids are ALL the engine orders lanes by, so
 * whatever device memory an op touches beyond its hello_op buffers is private to that op in a laned engine: the fused read
 * convolver's partial sums get one block per READCONV_FUSED op there (two convolvers of one technology -- readConv0 and
 * readConv0Meta of a separate-meta model -- run on different lanes with no event between them); the sequential program, one
 * stream, keeps one block per read technology.  Same kernels, same bits. */
#define HELLO_FLAG_LANE_SHIFT 8
#define HELLO_FLAG_LANE_MASK  (7 << HELLO_FLAG_LANE_SHIFT)
#define HELLO_MAX_LANES 8

typedef struct hello_op {
    int32_t kind;        /* hello_op_kind */
    int32_t domain;      /* hello_domain of dst rows */
    int32_t src0, src1;  /* buffer ids; CONV1D with src1 != HELLO_BUF_NONE: a CONCAT folded in -- input channels [0, seg) are src0's
                          * rows [lin][seg], channels [seg, cin) src1's rows [lin][cin - seg] (dense Winograd form, ReLU, no residual) */
    int32_t dst;         /* buffer id; HEAD: output slot */
    int32_t res;         /* residual buffer id or HELLO_BUF_NONE */
    int32_t cin, cout;   /* channels */
    int32_t k, stride, pad;     /* READCONV_FUSED: k = extra identity 64-channel blocks after the canonical 3 (0 | 2) */
    int32_t lin, lout;   /* positions per row before / after */
    int32_t flags;
    int32_t seg;         /* hello_segment (SEGSUM / MIX / READCONV_FUSED); two-source CONV1D: channels of src0 */
    int32_t c1;          /* CONCAT: channels of src1; CONV1D: groups of a grouped convolution (nn.Conv1d groups; 0 / 1 = dense):
                          * output block g reads input channels [g cin/groups, (g+1) cin/groups), weights packed per output
                          * channel over ITS group's k * cin/groups inputs; cout/groups a multiple of 128, cin/groups of 16 */
    float a0, a1;        /* MIX coefficients */
    int64_t w_off;       /* float offset of the packed weights in the weight blob */
    int64_t b_off;       /* float offset of the bias */
} hello_op;
/* Buffer rules hello_engine_create checks (HELLO_ERR_MODEL) for every op other than a HEAD, before it looks for a device:
 *   - domains: dst is a buffer of the op's domain; src0 / src1 / res hold rows of the domains the op reads -- its own domain,
 *     except SEGSUM and READCONV_FUSED, whose src0 is READS0 / READS1 / ALLELES according to `seg` (their domain: ALLELES, or
 *     SITES for a SEGSUM over HELLO_SEG_ALLELES_TO_SITES), and MIX (domain ALLELES), whose src1 is SITES; the uint8 inputs
 *     READS0 / READS1 / REF have rows of READS0 / READS1 / SITES;
 *   - sizes: every buffer's floats_per_row covers what the op reads or writes per row: lout*cout (CONV1D dst and res),
 *     lin*cin (CONV1D src0; MAXPOOL src0; SEGSUM, MIX, ADD, LAYERNORM all buffers), lout*cin (MAXPOOL dst), lin*cin,
 *     lin*c1 and lin*(cin+c1) (CONCAT src0, src1, dst), lin*seg and lin*(cin-seg) (the two sources of a two-source CONV1D);
 *   - uint8 inputs: HELLO_FLAG_SRC_U8 is set exactly when src0 is one of the reserved input ids (only CONV1D and
 *     READCONV_FUSED read them; never as src1 or res), and then cin == that input's channels (channels0, channels1, 5 for
 *     HELLO_BUF_REF, which needs uses_ref) and lin == window;
 *   - float4: MAXPOOL, SEGSUM, MIX, CONCAT (cin and c1) and ADD take channel counts that are positive multiples of 4;
 *   - lengths: SEGSUM, MIX, CONCAT, ADD and LAYERNORM keep the row length, lin == lout > 0; a CONV1D's padded row is at least
 *     k long (lin + 2 pad >= k);
 *   - MAXPOOL: k >= 1, stride >= 1, 0 <= pad <= k/2, lout == (lin + 2 pad - k) / stride + 1;
 *   - no op runs in place: dst differs from src0 and src1.
 * A HEAD reads src0 (a float buffer of its domain) holding lin*cin floats per row, lin > 0, cin > 0, and writes a logit row
 * (slot < n_experts: ALLELES domain, cout 1) or meta (slot 3: has_meta, SITES domain, cout <= 3). */

typedef struct hello_buffer {        /* scratch buffer i (i >= HELLO_BUF_FIRST_SCRATCH) */
    int32_t domain;                  /* hello_domain: rows scale with the batch */
    int32_t floats_per_row;          /* max length*channels over all uses */
} hello_buffer;

typedef struct hello_model_desc {
    int32_t abi_version;             /* HELLO_ABI_VERSION */
    int32_t window;                  /* L, 150 for the shipped models (python/call.py:187) */
    int32_t channels0, channels1;    /* 6 (7 with the haplotag channel); channels1 = 0: single tech */
    int32_t n_experts;               /* rows of `logits`: 1 (single expert) or 3 (ensemble) */
    int32_t has_meta;                /* meta mixing weights are produced */
    int32_t uses_ref;                /* HELLO_BUF_REF is read (meta_convolver_ref models) */
    int32_t n_buffers;               /* including the 3 reserved ids */
    const hello_buffer* buffers;     /* [n_buffers]; entries 0..2 ignored */
    int32_t n_ops;
    const hello_op* ops;
} hello_model_desc;

typedef struct hello_engine hello_engine;

/* ---- flags of hello_engine_forward ---------------------------------------------------------- */
#define HELLO_IN_DEVICE   1          /* reads0 / reads1 / ref_onehot are device pointers             */
#define HELLO_OUT_DEVICE  2          /* logits / meta / posteriors are device pointers               */
#define HELLO_LAYOUT_RCL  4          /* reads are [R][C][L] instead of [R][L][C]                     */

/* Stands in for: torch.load(args.network) + network.eval() (caller_calling.py:863-868); the model is
 * replicated per process like the reference's per-worker copy (call.py:215-221).  `folded_weights`
 * (host, nbytes) is copied to the device. */
int hello_engine_create(const hello_model_desc* desc, const void* folded_weights, size_t nbytes,
                        int hip_device, hello_engine** out);

/* Stands in for: MoEAttention.forward(tensors, numAllelesPerSite, numReadsPerAllele,
 * reference_segments) (MixtureOfExpertsAdvanced.py:161; batched callers
 * MixtureOfExpertsDNNFast.py:128-134).
 *   reads0 [R0][L][C0], reads_per_allele0 [A] (host), reads1/reads_per_allele1 likewise or NULL,
 *   alleles_per_site [S] (host), ref_onehot [S][L][5] or NULL,
 *   logits out [n_experts][A], meta out [S][3] or NULL,
 *   posteriors out [4][sum_s A_s(A_s+1)/2] or NULL: the wrapper's pair posteriors (see
 *   hello_engine_posteriors) computed in the same stream-ordered call.
 * Every allele must own >= 1 read (the featurizer inserts an all-zero dummy read,
 * AlleleSearcherLiteFiltered.cpp:1037-1043); violations are HELLO_ERR_SHAPE. */
int hello_engine_forward(hello_engine* engine,
                         const uint8_t* reads0, const int32_t* reads_per_allele0,
                         const uint8_t* reads1, const int32_t* reads_per_allele1,
                         const int32_t* alleles_per_site, const uint8_t* ref_onehot,
                         int32_t n_sites, int32_t n_alleles, int64_t n_reads0, int64_t n_reads1,
                         float* logits, float* meta, float* posteriors, int32_t flags, void* hip_stream);

/* Stands in for: the posterior section of MoEMergedWrapperAdvanced.forward
 * (MixtureOfExpertsAdvanced.py:530-589): sigmoid, probability of every unordered allele pair in
 * first-seen itertools.product order, mixture over experts.  n_pairs_total = sum_s A_s(A_s+1)/2.
 *   logits [n_experts][A] and meta [S][3] as written by hello_engine_forward (meta NULL => [1,0,0]),
 *   out [4][n_pairs_total]: rows mix, expert0, expert1, expert2.
 * `flags`: HELLO_IN_DEVICE for logits/meta, HELLO_OUT_DEVICE for out. */
int hello_engine_posteriors(hello_engine* engine, const float* logits, const float* meta,
                            const int32_t* alleles_per_site, int32_t n_sites, int32_t n_alleles,
                            int64_t n_pairs_total, float* out, int32_t flags, void* hip_stream);

/* Stands in for: AlleleSearcherLite.computeFeaturesColoredSimple (the C++ featurizer behind
 * python/AlleleSearcherLite.py:232-251, c++/src/AlleleSearcherLiteFiltered.cpp:971-1180), batched: every
 * read of every allele of every site in one launch, written as uint8 [n_reads][feature_length][channels]
 * ready to be passed to hello_engine_forward as `reads0` / `reads1`.
 *   bases / quals          all reads' bases (ASCII) and base qualities, concatenated; read_offsets [R+1]
 *   cigars                 BAM packing (length << 4 | operation), concatenated; cigar_offsets [R+1]
 *   ref_starts, mapq, orientation (> 0 forward), hp (0|1|2), site_of_read      per read
 *   ref_windows            all sites' reference windows (ASCII), concatenated; ref_window_offsets [S+1]
 *   window_starts, assembly_starts, assembly_stops                             per site (genome positions)
 * A read with zero CIGAR operations yields the all-zero dummy row of an unsupported allele (:1037-1043).
 * `flags`: HELLO_IN_DEVICE when ALL input arrays are device pointers, HELLO_OUT_DEVICE for `out`. */
int hello_engine_featurize(hello_engine* engine,
                           const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets,
                           const uint32_t* cigars, const int64_t* cigar_offsets,
                           const int64_t* ref_starts, const uint8_t* mapq, const int8_t* orientation,
                           const uint8_t* hp, const int32_t* site_of_read,
                           const uint8_t* ref_windows, const int64_t* ref_window_offsets,
                           const int64_t* window_starts, const int64_t* assembly_starts,
                           const int64_t* assembly_stops,
                           int64_t n_reads, int32_t n_sites, int32_t feature_length, int32_t channels,
                           uint8_t* out, int32_t flags, void* hip_stream);

/* Per-allele read support of a launch (no counterpart in the reference, whose VCF carries GT and QUAL only): for every allele
 * the reads that stand behind it, from the per-read arrays hello_engine_featurize reads.  An addition within ABI version 2.
 *   cigar_offsets [R+1], mapq [R], orientation [R]   as passed to hello_engine_featurize
 *   allele_read_offsets [A+1]                        exclusive scan of the reads_per_allele hello_engine_forward receives
 *                                                    (the dummy read of an unsupported allele counts as 1)
 *   out int64 [A][4]                                 over the reads r of allele a with cigar_offsets[r+1] > cigar_offsets[r] (a
 *                                                    read with zero CIGAR operations is the dummy row and supports nothing):
 *                                                    their number, those with orientation > 0, sum mapq, sum mapq^2
 * One launch of allele_support_kernel, asynchronous on `hip_stream`; integers written by index, so two runs give the same bytes.
 * `flags`: HELLO_IN_DEVICE when ALL input arrays are device pointers, HELLO_OUT_DEVICE for `out`; host pointers are staged
 * through device memory of the engine and the call synchronises.  n_alleles == 0 launches nothing and leaves `out` untouched.
 * Host offsets that do not start at 0, decrease or do not end at n_reads are refused (HELLO_ERR_SHAPE); device offsets cannot
 * be read here: the kernel clamps them to [0, n_reads]. */
int hello_engine_allele_support(hello_engine* engine, const int64_t* cigar_offsets, const uint8_t* mapq,
                                const int8_t* orientation, const int64_t* allele_read_offsets,
                                int64_t n_reads, int64_t n_alleles, int64_t* out, int32_t flags, void* hip_stream);

/* Per-allele base-level read evidence of a launch (no counterpart in the reference; an addition within ABI version 2): what the
 * reads of every allele put inside their site's span [assembly_start, assembly_stop), from the arrays hello_engine_featurize
 * reads plus the allele_read_offsets of hello_engine_allele_support.
 * One read r, n = its bases, reference cursor p = ref_starts[r], read cursor i = 0, its operations in order:
 *   M = X (0 7 8), length L   base i+j sits at p+j and BELONGS iff start <= p+j < stop;  p += L, i += L
 *   I (1), length L           all L bases belong iff start <= p <= stop: the insertion joins the base on its left, so one right
 *                             behind the last span base counts, and so does one at an empty span (start == stop);  i += L
 *   S (4)  i += L, never belongs        D N (2 3)  p += L        H P (5 6) and any code >= 9  nothing
 *   The walk stops in front of the first reference-consuming operation (M = X D N) that begins at p >= stop; what follows it
 *   is not examined.  GUARD: an operation of the walk that would move i past n ends it -- the read counts in column 5 and in
 *   no other column, and no quality outside the read's own is loaded; a site_of_read outside [0, n_sites) does the same.
 *   A read with zero operations is the dummy row of an unsupported allele and counts in no column.
 *   For a read with a belonging base: qmin = its lowest belonging quality; d = min(i0, n-1-i1), i0 / i1 its first / last
 *   belonging read index (the distance in read bases, soft-clipped ones included, to the nearer read end).
 *   out int64 [A][6]   per allele over its reads: 0 reads with a belonging base (nq), 1 sum qmin, 2 sum d,
 *                      3 reads with hp == 1, 4 reads with hp == 2, 5 reads stopped by the guard (0 on valid input)
 * One launch of allele_evidence_kernel, asynchronous on `hip_stream`; integers written by index, so two runs give the same bytes.
 * `flags`: as hello_engine_allele_support.  Host arrays are validated (HELLO_ERR_SHAPE): the three offset arrays start at 0 and
 * never decrease (read_offsets and cigar_offsets end at the sizes of quals and cigars, allele_read_offsets at n_reads) and
 * site_of_read lies in [0, n_sites); device arrays cannot be read here: the kernel clamps allele offsets to [0, n_reads].
 * n_alleles == 0 launches nothing and leaves `out` untouched. */
int hello_engine_allele_evidence(hello_engine* engine, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                                 const int64_t* cigar_offsets, const int64_t* ref_starts, const uint8_t* hp,
                                 const int32_t* site_of_read, const int64_t* assembly_starts, const int64_t* assembly_stops,
                                 const int64_t* allele_read_offsets, int64_t n_reads, int64_t n_sites, int64_t n_alleles,
                                 int64_t* out, int32_t flags, void* hip_stream);

/* ---- BAM input and candidate positions (host BAM reader + one GPU kernel; no engine, no model) ------------------------
 * Additions within ABI version 2.
 *
 * hello_bam_*: stands in for pysam.AlignmentFile.fetch as the reference's read containers use it
 * (python/PileupContainerLite.py:526-570).  BGZF is inflated with zlib on at most 16 host threads.  hello_bam_fetch decodes
 * every record of `chromosome` overlapping [start, stop) (pos < stop and end > start, end = bam_endpos) in file order into
 * flat arrays in the layout hello_engine_featurize takes: ASCII bases and base qualities with read offsets [R+1], CIGARs in
 * BAM packing with CIGAR offsets [R+1], ref_start / ref_end (int64), mapq (uint8), flag (uint16), a 64-bit FNV-1a hash of
 * the read name (uint64) and the strand (uint8, 1 = reverse).  use_index: 1 = the `.bai` next to the file (x.bam.bai or
 * x.bai) must be used, 0 = scan the whole file, -1 = the index when there is one.  A CIGAR of more than 65 535 operations is
 * read from the record's CG:B,I tag (SAM specification 4.2.2).  CRAM input and records without stored
 * base qualities are refused (HELLO_ERR_ARG).  A hello_bam is used from one thread at a time. */
typedef struct hello_bam hello_bam;
typedef struct hello_bam_reads hello_bam_reads;
enum {
    HELLO_BAM_BASES = 0, HELLO_BAM_QUALS = 1, HELLO_BAM_READ_OFFSETS = 2, HELLO_BAM_CIGARS = 3, HELLO_BAM_CIGAR_OFFSETS = 4,
    HELLO_BAM_REF_STARTS = 5, HELLO_BAM_REF_ENDS = 6, HELLO_BAM_MAPQ = 7, HELLO_BAM_FLAGS = 8, HELLO_BAM_NAME_HASH = 9,
    HELLO_BAM_STRAND = 10,
    HELLO_BAM_HP = 11,         /* uint8: the HP integer tag (types c/C/s/S/i/I), 0 when absent or outside 0..255 */
    /* after hello_bam_fetch_mods alone (empty after hello_bam_fetch): the 5mC calls of the MM / ML tags, DESIGN.md section 7m */
    HELLO_BAM_MOD_DELTAS = 12, /* int32: per listed base the bases of its kind skipped before it */
    HELLO_BAM_MOD_PROBS = 13,  /* uint8: its ML byte */
    HELLO_BAM_MOD_OFFSETS = 14, /* int64 [R + 1] into the two */
    HELLO_BAM_MOD_MODE = 15,   /* uint8: 0 implicit ('.' or absent), 1 unknown ('?') */
    HELLO_BAM_MOD_STATE = 16,  /* uint8: 0 no modifications, 1 usable, 2 bad */
    /* after hello_bam_fetch_sa alone (after the other two fetches both selectors are refused, as every selector above 16 was
       before them): the SA tags, DESIGN.md section 7q */
    HELLO_BAM_SA_BYTES = 17,   /* uint8: the bytes of every record's SA:Z tag without the NUL, all records concatenated */
    HELLO_BAM_SA_OFFSETS = 18, /* int64 [R + 1] into them; a record without SA, or with SA of another type than Z, has an empty range */
    /* after hello_bam_fetch_pairs alone, which fills 17 and 18 too (refused after the other fetches): the mate fields of the record's
       fixed core, DESIGN.md section 7s */
    HELLO_BAM_MATE_TID = 19,   /* int32: next_refID */
    HELLO_BAM_MATE_POS = 20,   /* int64: next_pos, 0-based, -1 when absent */
    HELLO_BAM_TLEN = 21        /* int32: tlen, carried; no rule uses it */
};
int hello_bam_open(const char* path, int32_t n_threads, hello_bam** out);
int hello_bam_n_references(const hello_bam* bam);
int hello_bam_reference(const hello_bam* bam, int32_t i, const char** name, int64_t* length);
int hello_bam_fetch(hello_bam* bam, const char* chromosome, int64_t start, int64_t stop, int32_t use_index,
                    hello_bam_reads** out);
/* hello_bam_fetch, and per record the C+m group of MM:Z with its bytes of ML:B:C (hello_amd/csrc/mods.h; never an error) */
int hello_bam_fetch_mods(hello_bam* bam, const char* chromosome, int64_t start, int64_t stop, int32_t use_index,
                         hello_bam_reads** out);
/* hello_bam_fetch, and per record the raw text of its SA:Z tag (never an error) */
int hello_bam_fetch_sa(hello_bam* bam, const char* chromosome, int64_t start, int64_t stop, int32_t use_index,
                       hello_bam_reads** out);
/* hello_bam_fetch_sa, and per record the mate fields of its fixed core as they stand (never an error) */
int hello_bam_fetch_pairs(hello_bam* bam, const char* chromosome, int64_t start, int64_t stop, int32_t use_index,
                          hello_bam_reads** out);
int hello_bam_reads_info(const hello_bam_reads* reads, int64_t* n_reads, int32_t* used_index, int64_t* n_blocks);
/* a pointer into `reads` (valid until hello_bam_reads_free) and its element count */
int hello_bam_reads_array(const hello_bam_reads* reads, int32_t which, const void** data, int64_t* count);
void hello_bam_reads_free(hello_bam_reads* reads);
void hello_bam_close(hello_bam* bam);

/* Stands in for: python/HotspotDetectorDVFiltered.py (doOneChunk / hotspotGenerator*, :31-165) over the C++ allele counter it
 * drives (c++/src/AlleleSearcherLiteFiltered.cpp:19-100 partial resolution, :121-317 counting, :550-646 and :834-890 flagging;
 * python/AlleleSearcherLite.py:112-190 windows).  Every region [region_starts[k], region_stops[k]) is cut into chunks of 400 bp
 * (10 000 bp with HELLO_HOTSPOTS_PACBIO or HELLO_HOTSPOTS_TWO_BAMS) counted from its start; the result is the sorted union of the
 * positions every chunk flags, clipped to the chunk -- the positions the reference writes as {'chromosome', 'position'} lines.
 *   reads: the arrays of hello_bam_fetch, `source` 0 for the first BAM, 1 for the second (two BAMs: Illumina, then PacBio);
 *          each source coordinate-sorted in file order.  Reads outside usability (unmapped, secondary, supplementary,
 *          duplicate, improper pair, mapq 0) are filtered here, as are repeated (name hash, strand) pairs within a chunk.
 *   reference: the chromosome's text (case kept), reference_length bytes.
 *   options: HELLO_HOTSPOTS_TWO_BAMS (two read sets, whether or not the second has reads in the regions), HELLO_HOTSPOTS_PACBIO
 *          (one read set of PacBio reads), HELLO_HOTSPOTS_HYBRID (--hybrid_hotspot).
 * Counting and flagging run in one kernel launch on `device` (hotspots.hip); host memory in and out. */
#define HELLO_HOTSPOTS_PACBIO 1
#define HELLO_HOTSPOTS_HYBRID 2
#define HELLO_HOTSPOTS_TWO_BAMS 4
#define HELLO_HOTSPOTS_STATS 10
typedef struct hello_hotspots hello_hotspots;
int hello_hotspots_find(const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets,
                        const uint32_t* cigars, const int64_t* cigar_offsets, const int64_t* ref_starts,
                        const int64_t* ref_ends, const uint8_t* mapq, const uint16_t* flags, const uint64_t* name_hash,
                        const uint8_t* source, int64_t n_reads, const uint8_t* reference, int64_t reference_length,
                        const int64_t* region_starts, const int64_t* region_stops, int32_t n_regions, int32_t options,
                        int32_t q_threshold, int32_t mapq_threshold, int32_t device, hello_hotspots** out);
/* the sorted positions (valid until hello_hotspots_free) */
int hello_hotspots_positions(const hello_hotspots* hotspots, const int64_t** positions, int64_t* n_positions);
/* stats[HELLO_HOTSPOTS_STATS]: chunks, chunks without reads, chunks out of bounds, chunks at the read cap, reads counted
 * (summed over chunks), tiles, events, kernel ms (HIP events), plan ms, total ms */
int hello_hotspots_stats(const hello_hotspots* hotspots, double* stats);
void hello_hotspots_free(hello_hotspots* hotspots);

/* Stands in for: python/caller_calling.py main (:795-843) up to the featurizer, for ONE Illumina BAM or ONE PacBio BAM --
 * python/PileupDataTools.py
 * hotspotsReader and candidateReader (:207-244,302-384: pass 1, one strict searcher per active region), python/trainDataTools.py
 * clusterLocations and data (:477-514,1039-1103: pass 2, one strict searcher per cluster whose own differing regions are the
 * sites), get_labeled_candidates and createTensors (:557-640,880-977), c++/src/Read.cpp:4-172 (a read's allele in a region) and
 * c++/src/AlleleSearcherLiteFiltered.cpp:495-547,648-666,740-831 (strict runs, supports, partials).  DESIGN.md "Candidate
 * sites" restates the rules, the two defined orders (alternative alleles in ascending byte order after the reference allele,
 * supporting reads in file order) and the deviations (the first reads are kept at the read cap; a cluster whose window leaves
 * the chromosome is skipped and counted; a site whose feature window leaves the chromosome is dropped and counted).
 *   reads: the arrays of hello_bam_fetch, coordinate-sorted, holding every read that overlaps [first position - 90, last
 *          position + 90) (pass 1 fetches 75 bp either side of [first - 15, last + 15]; more reads do no harm); hp = selector
 *          HELLO_BAM_HP.  positions: the sorted positions of a hotspot / shard file on this chromosome.
 *   options: 0 (Illumina reads) or HELLO_HOTSPOTS_PACBIO (PacBio reads, below), either with HELLO_CANDIDATES_RESIDENT (the reads
 *          stay on the device: "Resident candidates" below).  HELLO_HOTSPOTS_TWO_BAMS and
 *          HELLO_HOTSPOTS_HYBRID are refused (HELLO_ERR_ARG): those paths need the two-BAM reassembly.
 * Three kernel launches on `device` with options == 0 (candidates.hip: differing regions of pass 1, of pass 2, alleles and
 * supports), seven with HELLO_HOTSPOTS_PACBIO (two clip launches before the differing regions of either pass); the reads of
 * every allele are gathered on at most 16 host threads.
 * HELLO_HOTSPOTS_PACBIO (caller_calling.py:795-843 with one PacBio BAM: readRate (100, 100), pacbio = True, clipFlank = 200, no
 * reassembly): a searcher keeps at most span reads when its fetch interval [lo, hi) is longer than 100 bases (span = hi - lo),
 * else 100 -- the first in file order, as for Illumina.  Reads are selected on their original alignment; then a copy of every
 * kept read is strictly clipped (python/PileupContainerLite.py:255-468,554-573), left at lo and then right at hi, the right clip
 * seeing the left clip's result, and the window tests, counting, alleles, supports and the returned reads (bases, quals, cigars,
 * ref_start) are those of the clipped copies of pass 2; read_index still names the input read.  A clip at position p happens
 * only while reference_start <= p < reference_end.  The CIGAR is split inside the operation holding p, whose left half ends at
 * p.  From the split outwards operations are kept while fewer than 201 read bases (M I S = X) are counted; the operation in
 * which the count passes 200 is kept up to the 201st base (the left clip counts the base at p, the right clip starts behind
 * it) and everything beyond is discarded: reference_start grows / reference_end shrinks by the discarded M = X D N lengths, the
 * bases and qualities lose the discarded M I S = X lengths, hard clips consume nothing.  An outermost kept I becomes S, also
 * when nothing was discarded, and the two halves are rejoined, equal operations at the centre merged into one (the halves of
 * the split operation, or 20M 20M when p is the first one's last base).  Every read counts in the PacBio table (increment 1;
 * an indel needs 2 reads).  A read without an operation on the reference is refused (HELLO_ERR_ARG); the refusal of a soft
 * clip between aligned operations applies to the clipped CIGARs.  The two clip launches of a pass run one wave per
 * (searcher, read): the clip's plan, then the clipped operations, bases and qualities.
 * The result holds the arrays of a shard (hello_amd/shards.py) without the chromosome table, plus read_index (the input read
 * of every gathered read) and the differing regions of both passes as (start, stop) pairs. */
enum {
    HELLO_CAND_START = 0, HELLO_CAND_STOP = 1, HELLO_CAND_WINDOW_START = 2, HELLO_CAND_REF_OFF = 3,      /* int64 */
    HELLO_CAND_REF = 4,                                                                                  /* uint8 */
    HELLO_CAND_ALLELES_PER_SITE = 5,                                                                     /* int32 */
    HELLO_CAND_ALLELE_TEXT = 6,                                                                          /* uint8 */
    HELLO_CAND_ALLELE_TEXT_OFF = 7,                                                                      /* int64 */
    HELLO_CAND_READS_PER_ALLELE = 8,                                                                     /* int32 */
    HELLO_CAND_BASES = 9, HELLO_CAND_QUALS = 10,                                                         /* uint8 */
    HELLO_CAND_READ_OFF = 11,                                                                            /* int64 */
    HELLO_CAND_CIGARS = 12,                                                                              /* uint32 */
    HELLO_CAND_CIGAR_OFF = 13, HELLO_CAND_REF_START = 14,                                                /* int64 */
    HELLO_CAND_MAPQ = 15,                                                                                /* uint8 */
    HELLO_CAND_ORIENTATION = 16,                                                                         /* int8 */
    HELLO_CAND_HP = 17,                                                                                  /* uint8 */
    HELLO_CAND_READ_INDEX = 18, HELLO_CAND_REGIONS_PASS1 = 19, HELLO_CAND_REGIONS_PASS2 = 20             /* int64 */
};
#define HELLO_CANDIDATES_STATS 22
typedef struct hello_candidates hello_candidates;
int hello_candidates_find(const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets,
                          const uint32_t* cigars, const int64_t* cigar_offsets, const int64_t* ref_starts,
                          const int64_t* ref_ends, const uint8_t* mapq, const uint16_t* flags, const uint64_t* name_hash,
                          const uint8_t* hp, int64_t n_reads, const uint8_t* reference, int64_t reference_length,
                          const int64_t* positions, int64_t n_positions, int32_t options, int32_t feature_length,
                          int32_t q_threshold, int32_t mapq_threshold, int32_t device, hello_candidates** out);
/* a pointer into `candidates` (valid until hello_candidates_free) and its element count */
int hello_candidates_array(const hello_candidates* candidates, int32_t which, const void** data, int64_t* count);
/* stats[HELLO_CANDIDATES_STATS]: active regions, without reads, out of bounds, at the read cap, differing regions of pass 1;
 * clusters, without reads, out of bounds, at the read cap, differing regions of pass 2; sites, sites whose feature window leaves
 * the chromosome, alleles, reads gathered, record slots; ms of the pass-1 kernel, the pass-2 kernel, the allele kernel (HIP
 * events), the host gather, the whole call; ms of the two clip kernels of both passes, (searcher, read) pairs whose read a clip
 * applied to (both 0 without HELLO_HOTSPOTS_PACBIO) */
int hello_candidates_stats(const hello_candidates* candidates, double* stats);
void hello_candidates_free(hello_candidates* candidates);

/* hello_candidates_find for an Illumina BAM (read set 0) and a PacBio BAM (read set 1) together: caller_calling.py:784-843 with
 * two read samplers, python/AlleleSearcherLite.py:100-206,257-268 and the reassembly of c++/src/AlleleSearcherLiteFiltered.cpp:
 * 668-738 / c++/src/Read.cpp:174-323.  DESIGN.md "Two BAMs" states the rules.  Every searcher of both passes holds two
 * containers: the Illumina reads under the Illumina cap, unclipped, and the PacBio reads under the PacBio cap, every kept one
 * strictly clipped with flank 200 as under HELLO_HOTSPOTS_PACBIO; filters, the first-of-(name, strand) rule and the cap apply
 * per container, the window tests to both (a searcher with two empty containers has no regions).  Illumina reads count in
 * table 0, PacBio reads in table 1; both tables are flagged and unioned, or, with HELLO_HOTSPOTS_HYBRID in options
 * (--hybrid_hotspot), flagged by the hybrid rule (the only other bit understood is HELLO_CANDIDATES_RESIDENT, below).  In pass 2 a cluster whose Illumina coverage passes the gate (over the reads
 * of read set 0 that overlap the cluster's fetch interval and are mapped, primary, not QC-fail, not duplicate and a proper pair
 * if paired, before de-duplication and the cap: a column is every position one of them covers with M = X D N; a read counts at
 * a column with mapq >= 10 and base quality >= 13 there, on D N that of its last read base before; the gate is sum of counts >
 * 14 * columns) and that has fewer than `reassembly_size` differing regions (the reference's --reconcilement_size, 10) is
 * reassembled: with [start, stop) = [first region - 6, last region + 6), a clipped PacBio read with reference_start <= start and
 * last_position >= stop whose haplotype there (the reference, every region replaced by the read's Success record) equals the
 * haplotype of one choice of one allele per Illumina site (a region with a passing Illumina record without N) gets exactly
 * those alleles as its records, min_q 60, and loses its records elsewhere; its partials stay.  When several choices spell the
 * haplotype, the sites' strings are ordered by bytes and the smallest index tuple is taken (the reference lets hash order
 * decide).  An allele is kept when its support summed over both technologies is positive; its reads are split by technology.
 * Every read keeps its own hp (the reference passes on the last container's list only).
 * The result answers hello_candidates_array for the site arrays and for technology 0; hello_candidates_array_tech(c, 1, ...)
 * gives technology 1's reads_per_allele, bases ... hp and read_index (HELLO_CAND_READS_PER_ALLELE .. HELLO_CAND_READ_INDEX):
 * the clipped copies of pass 2, read_index naming the reads of read set 1. */
#define HELLO_CANDIDATES_HYBRID_STATS 29
int hello_candidates_find_hybrid(
    const uint8_t* bases0, const uint8_t* quals0, const int64_t* read_offsets0, const uint32_t* cigars0,
    const int64_t* cigar_offsets0, const int64_t* ref_starts0, const int64_t* ref_ends0, const uint8_t* mapq0,
    const uint16_t* flags0, const uint64_t* name_hash0, const uint8_t* hp0, int64_t n_reads0,
    const uint8_t* bases1, const uint8_t* quals1, const int64_t* read_offsets1, const uint32_t* cigars1,
    const int64_t* cigar_offsets1, const int64_t* ref_starts1, const int64_t* ref_ends1, const uint8_t* mapq1,
    const uint16_t* flags1, const uint64_t* name_hash1, const uint8_t* hp1, int64_t n_reads1,
    const uint8_t* reference, int64_t reference_length, const int64_t* positions, int64_t n_positions, int32_t options,
    int32_t reassembly_size, int32_t feature_length, int32_t q_threshold, int32_t mapq_threshold, int32_t device,
    hello_candidates** out);
int hello_candidates_array_tech(const hello_candidates* candidates, int32_t tech, int32_t which, const void** data, int64_t* count);
/* stats[HELLO_CANDIDATES_HYBRID_STATS]: the entries of hello_candidates_stats (reads gathered: both technologies; allele kernel
 * ms: both launches around the reassembly), then clusters whose coverage gate passed, clusters reassembled, PacBio reads
 * eligible, reassigned, reassigned where several choices spelled the haplotype (the tie rule), Illumina sites of the reassembled
 * clusters, ms of the reassembly phase (its plan, its kernel and the copy of its results).  The last seven are 0 for the
 * candidates of hello_candidates_find. */
int hello_candidates_hybrid_stats(const hello_candidates* candidates, double* stats);

/* Resident candidates: the hand-over to the scoring engine without the host.  HELLO_CANDIDATES_RESIDENT is a bit of `options`
 * of hello_candidates_find and hello_candidates_find_hybrid beside the HELLO_HOTSPOTS_* values.  With it the call runs as
 * without it up to the sites: the site arrays, reads_per_allele, read_off, cigar_off, read_index, the regions and the
 * statistics are on the host and identical; the reads of the alleles are NOT gathered on the host -- HELLO_CAND_BASES, QUALS,
 * CIGARS, REF_START, MAPQ, ORIENTATION and HP answer with count 0 and the `ms host gather` statistic is 0.  Instead the result
 * owns, on `device`, the reads of pass 2 (bases, qualities, CIGARs, their offsets, ref_start, mapq; for PacBio the clipped
 * copies where the clip kernel wrote them), per such read the orientation and hp of its input read, and per technology the
 * gather table: for every read the featurizer will see its pass-2 read or -1 (the dummy read of an allele without reads of
 * that technology), the exclusive scans of the output reads' base and CIGAR counts, and the read's site.  The chromosome and
 * all scratch are freed before the call returns.  A result without sites (no reads, no positions, no site) holds no device
 * memory and needs no GPU.  hello_candidates_free releases the device memory, from the creating thread, whatever device is
 * current. */
#define HELLO_CANDIDATES_RESIDENT 64
/* The sizes of technology `tech`'s featurizer input (hello_engine_featurize) with the dummy reads: reads = sum of
 * max(reads_per_allele, 1), bases and CIGAR words of the supporting reads.  Host only; resident and non-resident results. */
int hello_candidates_featurizer_counts(const hello_candidates* candidates, int32_t tech, int64_t* n_reads, int64_t* n_bases,
                                       int64_t* n_cigars);
/* One launch of gather_reads_kernel (candidates.hip, a wave per read) on `hip_stream`, asynchronous: technology `tech`'s
 * featurizer input into DEVICE arrays of the caller.  With n = n_reads of hello_candidates_featurizer_counts it writes
 * ref_start, mapq, orientation, hp, site_of_read [read_shift, read_shift + n); bases / quals from byte base_shift, cigars from
 * word cigar_shift; read_off[read_shift] = base_shift and read_off[read_shift + i + 1] = base_shift + bases of reads 0..i,
 * likewise cigar_off with cigar_shift; site_of_read = the site within these candidates + site_shift -- so consecutive gathers of
 * several results into one block give the coalesced arrays of one featurizer launch.  A dummy read has ref_start 0, mapq 40,
 * orientation 1, hp 0, no bases and no CIGAR.  Nothing outside those ranges is written, every element has one writer, two
 * runs give the same bytes.  The candidates must outlive the launch (free them after the stream has passed it) and the
 * stream's device must be current.  HELLO_ERR_ARG, naming it: candidates built without HELLO_CANDIDATES_RESIDENT, a NULL
 * destination with n > 0, tech 1 on candidates of one technology, a negative shift.  n == 0 launches nothing. */
int hello_candidates_gather(const hello_candidates* candidates, int32_t tech, uint8_t* bases, uint8_t* quals, int64_t* read_off,
                            uint32_t* cigars, int64_t* cigar_off, int64_t* ref_start, uint8_t* mapq, int8_t* orientation,
                            uint8_t* hp, int32_t* site_of_read, int64_t read_shift, int64_t base_shift, int64_t cigar_shift,
                            int64_t site_shift, void* hip_stream);
/* The host half of a gather table from one technology's counts: reads_per_allele[n_alleles] and the offsets
 * read_off / cigar_off [sum reads_per_allele + 1] of its supporting reads -> per featurizer read the supporting read or -1
 * (source[n]), and the scans out_read_off / out_cigar_off [n + 1]; *n_reads = n.  With all three outputs NULL only n is
 * returned; otherwise capacity >= n.  Host only. */
int hello_candidates_gather_table(const int32_t* reads_per_allele, int64_t n_alleles, const int64_t* read_off,
                                  const int64_t* cigar_off, int64_t capacity, int64_t* source, int64_t* out_read_off,
                                  int64_t* out_cigar_off, int64_t* n_reads);

/* The engine's own stream (a hipStream_t): what a call with hip_stream == NULL runs on.  It is created
 * non-blocking, so it is NOT ordered with the legacy default stream: a caller whose other work sits on the default
 * stream (handle 0, indistinguishable from NULL here) orders the two with events on this handle -- the Python
 * binding does (hello_amd/engine.py). */
void* hello_engine_stream(hello_engine* engine);

/* Host memory the GPU reads and writes in place (pinned, mapped, coherent): pointers into such a block may be passed to
 * hello_engine_forward under HELLO_IN_DEVICE / HELLO_OUT_DEVICE -- a small batch then crosses PCIe inside the kernels' own loads and
 * stores, with no staging copy and no copy-engine hop (followed by hello_engine_synchronize before the host reads the outputs).
 * NULL when the allocation fails (no GPU).  An addition within ABI version 2. */
void* hello_pinned_alloc(size_t bytes);
void hello_pinned_free(void* block);

/* Wait for everything the engine has enqueued on its last stream. */
int hello_engine_synchronize(hello_engine* engine);

/* Seconds of device time between the start and end of the most recent forward (HIP events on the
 * call's stream); negative if unavailable.  Used by bench.py's roofline leg. */
int hello_engine_last_forward_ms(hello_engine* engine, float* ms);

/* Per-op device time (HIP events on the call's stream around every op).  set_profiling(n > 0)
 * arms recording for the next n forwards; op_times_ms returns, per op, the SUM over the forwards
 * recorded since then and their number.  set_profiling(0) disarms. */
int hello_engine_set_profiling(hello_engine* engine, int max_forwards);
int hello_engine_op_times_ms(hello_engine* engine, float* ms_sum, int32_t capacity, int32_t* n_ops,
                             int32_t* n_forwards);
/* Restrict the recording to ops of one hello_op_kind (0 = every op): two event records per matching op and
 * forward instead of one per op, cheap enough to stay armed inside a timed region (bench.py times the
 * dominant kernel, HELLO_OP_READCONV_FUSED, this way).  Ops of other kinds then report 0 ms. */
int hello_engine_set_profiling_filter(hello_engine* engine, int32_t op_kind);

/* Debug read-back of one op's output (parity tests of single kernels; the reference's counterpart is a forward
 * hook on the module).  debug_capture(i >= 0) arms: every following forward copies the dst buffer of op i,
 * right after the op has run (scratch buffers are reused by later ops), into an engine-owned device buffer;
 * debug_capture(-1) disarms.  debug_read waits for the last forward and copies that snapshot to the host:
 * float32 [rows of the op's domain][positions][channels], `*n_floats` = its size (also when `out` is NULL or
 * `capacity` too small, which is HELLO_ERR_ARG unless out is NULL). */
int hello_engine_debug_capture(hello_engine* engine, int32_t op_index);
int hello_engine_debug_read(hello_engine* engine, float* out, int64_t capacity, int64_t* n_floats);

/* Diagnostic timeline of the fused read convolver (how its time splits over its barrier-delimited sections; the reference has
 * no counterpart -- its profile is torch's).  debug_stamps(1) arms: following forwards launch a STAMPED instantiation of the kernel
 * (same code, plus per-wave s_memtime records at the start of each group of reads and on both sides of each of its 20 barriers,
 * written to an engine-owned buffer nothing else reads; results are unchanged, the launch is ~10 % slower);  3: the same with ONE
 * workgroup resident per CU (LDS padding); 0 disarms.  Only the canonical fp32 Winograd read convolver from the bytes.
 * debug_read_stamps copies the last stamped forward's records to the host: uint64 [layout[0] workgroups][layout[1] waves]
 * [layout[2] groups per workgroup][layout[3] slots]; layout[4] = how many of the workgroups walk layout[2] groups (the rest, from
 * the second launch, walk one).  Slots: 0 group start, 1 + 2 i / 2 + 2 i arrival at / release from barrier i, 41 HW_ID | XCC_ID << 32,
 * 42 / 43 s_memrealtime (100 MHz) at the group's start / end, 44 (group 0 only) after the workgroup's last flush. */
int hello_engine_debug_stamps(hello_engine* engine, int32_t mode);
int hello_engine_debug_read_stamps(hello_engine* engine, uint64_t* out, int64_t capacity, int64_t* n_words, int32_t* layout);

void hello_engine_destroy(hello_engine* engine);

/* ---- record stage (host only: no engine, no GPU) ---------------------------------------------------------------------
 * Stands in for, per site of a whole launch and on `n_threads` host threads:
 *   - caller_calling.vcfRecords' decision and record (python/caller_calling.py:698-743: best pair of the mixture row,
 *     QUAL = -10 log10(1 - min(p, 1 - 1e-8)), ALT list, genotype, createVcfRecord normalisation
 *     python/vcfFromContigs.py:139-227) with INFO "MixtureOfExpertPrediction" -> the shard's `.vcf` lines;
 *   - its `.features` entry (:743-754) as one pickle stream per shard (the list prepareVcf.py:138 loads);
 *   - prepareVcf.vcfRecords' call on the meta-weighted mean of the experts in float64 (python/prepareVcf.py:154-168) with
 *     INFO "HELLO" -> the lines of the final VCF, with their normalised positions for the final sort;
 *   - the best pair / probability / QUAL of all five rows (mixture, expert 0..2, mean).
 * ALT alleles are written in sorted order; equal pair probabilities are ordered by the pair's allele strings, as Python's
 * sort of (value, key) tuples orders them.  A site whose `keep` byte is 0 is decided but emits nothing. */
typedef struct hello_site_table {
    int32_t n_sites;
    const int32_t* alleles_per_site;         /* [S] */
    const uint8_t* allele_text;              /* every allele string of every site, concatenated (ASCII) */
    const int64_t* allele_text_off;          /* [A + 1] */
    int32_t n_chromosomes;
    const uint8_t* chromosome_text;          /* chromosome names, concatenated */
    const int64_t* chromosome_text_off;      /* [n_chromosomes + 1] */
    const int32_t* chromosome_of_site;       /* [S] index into the names */
    const int64_t* start;                    /* [S] allele span [start, stop) in genome coordinates (0-based) */
    const int64_t* stop;
    const uint8_t* ref_windows;              /* per-site reference windows, concatenated (or NULL with `genome`) */
    const int64_t* ref_window_off;           /* [S + 1] */
    const int64_t* window_start;             /* [S] genome position of each window's first byte */
    const uint8_t* const* genome;            /* [n_chromosomes] whole sequences (entries may be NULL) or NULL */
    const int64_t* genome_len;               /* [n_chromosomes] */
    const uint8_t* keep;                     /* [S] or NULL (= all) */
} hello_site_table;

typedef struct hello_features_format {       /* how `meta` (float32 [3]) is written inside a `.features` entry:     */
    const uint8_t* meta_prefix;              /* pickle opcodes before and after the 12 payload bytes -- the binding  */
    int32_t meta_prefix_len;                 /* takes them from its own NumPy's pickle of such an array, so the file */
    const uint8_t* meta_suffix;              /* loads wherever that NumPy's pickles load                             */
    int32_t meta_suffix_len;
} hello_features_format;

typedef struct hello_records hello_records;

typedef struct hello_records_view {          /* pointers into a hello_records object; valid until it is destroyed */
    int32_t n_sites, n_shards;
    const uint8_t* shard_vcf;                /* record lines ('\n'-terminated) in site order */
    const int64_t* shard_vcf_off;            /* [S + 1]: site s owns bytes [off[s], off[s+1]) (empty: no record) */
    const uint8_t* mean_vcf;                 /* the final VCF's lines for the same sites */
    const int64_t* mean_vcf_off;             /* [S + 1] */
    const int64_t* mean_position;            /* [S] 0-based position of the mean call after normalisation, -1: no record */
    const uint8_t* features;                 /* n_shards pickle streams, concatenated */
    const int64_t* features_off;             /* [n_shards + 1] */
    const int32_t* n_records;                /* [n_shards] */
    const int32_t* best_pair;                /* [5][S] pair index within the site: rows mixture, expert 0..2, mean */
    const double* best_p;                    /* [5][S] */
    const double* qual;                      /* [5][S] */
} hello_records_view;

/*   posteriors [4][n_pairs_total] and meta [S][3] (NULL = [1, 0, 0]) as written by hello_engine_forward, HOST memory;
 *   shard_site_off [n_shards + 1] site offsets of the shards the launch coalesced (NULL = one shard);
 *   fmt NULL = no `.features` streams; n_threads <= 0 = one per hardware thread. */
int hello_site_records(const hello_site_table* sites, const float* posteriors, int64_t n_pairs_total, const float* meta,
                       const int32_t* shard_site_off, int32_t n_shards, const hello_features_format* fmt,
                       int32_t n_threads, hello_records** out);
/* hello_site_records with read support (an addition within ABI version 2): the same decisions and the same lines, with
 * annotations on the shard lines and the final-VCF lines.  support0 / support1: int64 [A][4] per technology as
 * hello_engine_allele_support writes them, HOST memory (support1 NULL = one technology); both technologies are summed.
 *   FORMAT  GT:GQ:DP:AD:ADF:ADR
 *           GQ   min(99, floor(QUAL + 0.5)) of the line's own QUAL
 *           DP   reads over ALL alleles of the site, listed in the record or not
 *           AD   one value for REF and one per ALT in the record's order, each taken from the site allele whose string equals
 *                that allele before normalisation (0 when the reference allele is not among the site's alleles);
 *                ADF those on the forward strand, ADR = AD - ADF
 *   INFO    <as before>;MQ=%.2f with MQ = sqrt(sum mapq^2 / DP) over the reads of DP in double, MQ=. when DP is 0
 * The `.features` streams, the view and every other field are those of hello_site_records. */
int hello_site_records_annotated(const hello_site_table* sites, const int64_t* support0, const int64_t* support1,
                                 const float* posteriors, int64_t n_pairs_total, const float* meta,
                                 const int32_t* shard_site_off, int32_t n_shards, const hello_features_format* fmt,
                                 int32_t n_threads, hello_records** out);
/* hello_site_records_annotated with genotype likelihoods and base-level evidence (an addition within ABI version 2): the same
 * decisions and the same lines, plus the fields below.  evidence0 / evidence1: int64 [A][6] per technology as
 * hello_engine_allele_evidence writes them, HOST memory; evidence1 must be NULL exactly when support1 is NULL.  `fields`: a mask
 * of HELLO_EVIDENCE_* bits.  "Listed alleles": REF, then the record's ALTs in its order, each found among the site's alleles by
 * its string before normalisation, as AD finds it.
 *   FORMAT  GT:GQ:DP:AD:ADF:ADR:PL  [:ADI:ADP with two technologies]  [:AH1:AH2 with HELLO_EVIDENCE_HP]
 *           PL   in VCF order (for k: for j <= k) from the posterior p_jk of the pair of listed alleles {j, k} in the row the
 *                line's QUAL comes from (mixture row on shard lines, meta-weighted mean on final-VCF lines), in double:
 *                min(255, floor(-10 log10(p_jk / p_max) + 0.5)), p_max the largest over the listed pairs; 255 for p_jk <= 0;
 *                the whole field is `.` when a listed allele is not among the site's alleles or p_max <= 0
 *           ADI / ADP   AD from technology 0 alone / technology 1 alone
 *           AH1 / AH2   columns 3 / 4 (reads with haplotag 1 / 2) per listed allele, both technologies summed
 *   INFO    <as annotated>;MBQ=..;MPOS=..   per listed allele (comma separated), with the sum (column 1 for MBQ, column 2 for
 *           MPOS) and nq (column 0) added over both technologies: (2 sum + nq) / (2 nq) in integer division -- the mean,
 *           rounded; `.` when nq is 0 or the allele is not among the site's alleles */
#define HELLO_EVIDENCE_HP 1          /* write AH1 / AH2 */
int hello_site_records_evidence(const hello_site_table* sites, const int64_t* support0, const int64_t* support1,
                                const int64_t* evidence0, const int64_t* evidence1, int32_t fields, const float* posteriors,
                                int64_t n_pairs_total, const float* meta, const int32_t* shard_site_off, int32_t n_shards,
                                const hello_features_format* fmt, int32_t n_threads, hello_records** out);
int hello_records_get(const hello_records* records, hello_records_view* view);
void hello_records_destroy(hello_records* records);

const char* hello_last_error(void);
int hello_abi_version(void);

/* ---- shared scoring server (host only; one per GPU) ------------------------------------------------------------------
 * Stands in for: the model copy every worker process of the reference's pool loads for itself and calls once per site
 * (python/call.py:111,215-221; python/caller_calling.py:863-868,872-891).  The workers keep their loop and their call
 * (hello_amd/shared.py: the client packs a site into its slot of a shared-memory segment, sends one byte on a Unix-domain
 * socket and blocks for the one-byte answer); ONE server process per (model file, GPU) drains all pending slots into one
 * hello_engine_forward launch and scatters logits / meta / pair posteriors back.  An addition within ABI version 2.
 *
 * Slot (offsets: hello_site_slot_layout_of): int32 header [16] = {alleles, reads0, reads1, has_ref, pairs, message length};
 * int32 reads_per_allele0 / 1 [HELLO_SITE_MAX_ALLELES]; uint8 reference one-hot [window][5]; results float32 logits
 * [3][HELLO_SITE_MAX_ALLELES], meta [4], posteriors [4][MAX_ALLELES (MAX_ALLELES + 1) / 2]; a message area (errors, statistics
 * as JSON); then the pileup bytes of technology 0 followed by technology 1.
 * Wire: the client sends <u32 length><JSON with "protocol">, the server answers <u32 length><JSON: slot, slot_bytes, max_clients,
 * shm_path, pid, the model's dimensions, `info_json`>; afterwards one byte each way per request: 'R' (score my slot) or 'S'
 * (statistics into my slot's message area) -> 'K' (done) or 'E' (refused: the reason is in the message area). */
#define HELLO_SITE_PROTOCOL 1
#define HELLO_SITE_MAX_ALLELES 64

typedef struct hello_site_slot_layout {      /* byte offsets inside one slot */
    int64_t header, rpa0, rpa1, ref, logits, meta, post, err, reads, read_capacity;
} hello_site_slot_layout;

typedef struct hello_site_server_config {
    int32_t window, channels0, channels1;    /* the model, as the clients are told (and as every slot is checked against) */
    int32_t n_experts, has_meta, uses_ref;
    int32_t max_clients;                     /* slots of the segment */
    int32_t max_batch_sites;                 /* sites of one launch at most */
    int32_t group_launches;                  /* != 0 with several engines: a launch takes clients / engines sites, the groups run out of phase */
    int32_t reserved;                        /* 0 */
    int64_t slot_bytes;
    double idle_exit_s;                      /* leave after this long without a client; < 0: never */
    double linger_s;                         /* patience for the clients that could still send a site before a launch goes out */
    const char* info_json;                   /* further members of the handshake object ("k": v, ...) or NULL */
} hello_site_server_config;

typedef struct hello_site_server_stats {
    int64_t launches, sites, errors;
    int32_t largest_launch, clients_seen;
} hello_site_server_stats;

/* A scorer other than an engine (tests drive the server without a GPU through this): fill logits [n_experts][A], meta [S][3]
 * (NULL when the model has none) and posteriors [4][sum_s A_s(A_s+1)/2]; return 0, or non-zero with a message in `err`. */
typedef int (*hello_site_scorer)(void* ctx, const uint8_t* reads0, const int32_t* reads_per_allele0, const uint8_t* reads1,
                                 const int32_t* reads_per_allele1, const int32_t* alleles_per_site, const uint8_t* ref_onehot,
                                 int32_t n_sites, int32_t n_alleles, int64_t n_reads0, int64_t n_reads1, float* logits, float* meta,
                                 float* posteriors, char* err, int32_t err_capacity);

typedef struct hello_site_server hello_site_server;

int hello_site_slot_layout_of(int32_t window, int32_t channels0, int32_t channels1, int64_t slot_bytes, hello_site_slot_layout* out);
/* Creates the segment file and the listening socket (a connectable socket = a ready server: add the scorers first or right after). */
int hello_site_server_create(const char* socket_path, const char* shm_path, const hello_site_server_config* config, hello_site_server** out);
/* One scorer thread per engine / scorer added; every engine is used from its own thread only. */
int hello_site_server_add_engine(hello_site_server* server, hello_engine* engine);
int hello_site_server_add_scorer(hello_site_server* server, hello_site_scorer scorer, void* ctx);
/* Blocks: serves until hello_site_server_stop (callable from any thread or a signal handler) or the idle limit. */
int hello_site_server_run(hello_site_server* server);
void hello_site_server_stop(hello_site_server* server);
int hello_site_server_get_stats(hello_site_server* server, hello_site_server_stats* out);
/* Closes the sockets, unmaps and unlinks the segment and the socket file. */
void hello_site_server_destroy(hello_site_server* server);

/* Reference-confidence blocks of a gVCF (not in the reference; DESIGN.md section 7f states the rules, hello_amd/gvcf.py restates
 * them in Python).  Over the span [lo, hi) of one chromosome: per position the bases of the counted reads (n_total) and those that
 * equal the reference case-insensitively (n_ref), then the called / no-call flag, GQ and band of the position, and the maximal
 * runs of consecutive positions of one band that lie in no excluded interval.
 *   reads: the arrays of hello_bam_fetch, `source` 0 / 1 as for hello_hotspots_find, each source coordinate-sorted.  A read counts
 *          when it is usable (as for the hotspot stage), not QC-fail (0x200) and mapq >= mapq_threshold; no de-duplication, no cap.
 *          A counted read whose CIGAR consumes more bases than it has is refused (HELLO_ERR_ARG).
 *   reference: the chromosome's text (case kept), reference_length bytes; 0 <= lo <= hi <= reference_length.
 *   excluded_starts / excluded_stops: n_excluded intervals [start, stop), sorted, not overlapping (they may touch).
 *   gq_binsize >= 1: the band of a called position is GQ / gq_binsize; HELLO_REFBLOCKS_NO_CALL is the band of no-call positions.
 *   options: 0, or HELLO_REFBLOCKS_KEEP_COUNTS (the per-position counters are copied back too).
 * Two kernel launches on `device` (refblocks.hip): counting and the number of runs per tile; then, with exact offsets, the runs.
 * Runs of one band that meet at a tile edge are joined on the host.  Host memory in and out. */
#define HELLO_REFBLOCKS_KEEP_COUNTS 1
#define HELLO_REFBLOCKS_NO_CALL (-1)
#define HELLO_REFBLOCKS_STATS 7
enum {
    HELLO_REFBLOCKS_START = 0,      /* int64 [blocks] */
    HELLO_REFBLOCKS_END = 1,        /* int64 [blocks], exclusive */
    HELLO_REFBLOCKS_BAND = 2,       /* int32 [blocks] */
    HELLO_REFBLOCKS_MIN_DP = 3,     /* int32 [blocks]: the smallest n_total */
    HELLO_REFBLOCKS_GQ = 4,         /* int32 [blocks]: the smallest GQ */
    HELLO_REFBLOCKS_N_REF = 5,      /* int32 [blocks]: n_ref of the first position with that GQ */
    HELLO_REFBLOCKS_N_TOTAL = 6,    /* int32 [blocks]: n_total of that position */
    HELLO_REFBLOCKS_COUNT_REF = 7,  /* int32 [hi - lo] with HELLO_REFBLOCKS_KEEP_COUNTS, else count 0 */
    HELLO_REFBLOCKS_COUNT_TOTAL = 8 /* int32 [hi - lo] with HELLO_REFBLOCKS_KEEP_COUNTS, else count 0 */
};
typedef struct hello_refblocks hello_refblocks;
int hello_refblocks_find(const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets,
                         const uint32_t* cigars, const int64_t* cigar_offsets, const int64_t* ref_starts,
                         const int64_t* ref_ends, const uint8_t* mapq, const uint16_t* flags, const uint64_t* name_hash,
                         const uint8_t* source, int64_t n_reads, const uint8_t* reference, int64_t reference_length,
                         int64_t lo, int64_t hi, const int64_t* excluded_starts, const int64_t* excluded_stops,
                         int64_t n_excluded, int32_t q_threshold, int32_t mapq_threshold, int32_t gq_binsize, int32_t options,
                         int32_t device, hello_refblocks** out);
/* a pointer into `blocks` (valid until hello_refblocks_free) and its element count */
int hello_refblocks_array(const hello_refblocks* blocks, int32_t which, const void** data, int64_t* count);
/* stats[HELLO_REFBLOCKS_STATS]: tiles, reads counted, runs before joining, blocks after joining, kernel ms (HIP events, both
 * launches), plan ms, total ms */
int hello_refblocks_stats(const hello_refblocks* blocks, double* stats);
void hello_refblocks_free(hello_refblocks* blocks);

/* Read-backed phasing of heterozygous records (not in the reference; DESIGN.md section 7g states the rules, hello_amd/phase.py
 * restates them in Python).  One handle per chromosome.
 *   hello_phase_observe: with *handle NULL it creates the handle from the chromosome's phasable records -- record_starts /
 *          record_ends [n_records] (the span [POS - 1, POS - 1 + len(REF)), sorted by start), and `alleles` with allele_offsets
 *          [2 n_records + 1]: allele a then allele b of every record, upper case -- and adds the reads given; with *handle set it
 *          adds a further batch of reads (one span of the chromosome) to it, and the record arguments are not read again.
 *          reads: the arrays of hello_bam_fetch, `source` 0 / 1; a read counts by the rule of hello_refblocks_find, and a counted
 *          read whose CIGAR consumes more bases than it has, or records that are not sorted, are refused (HELLO_ERR_ARG).
 *          Per counted read one int8 slot (-1 none, 0 allele a, 1 allele b) per record whose start it covers (observe kernel),
 *          and link[t][k - 1][0 cis | 1 trans], k = 1..window, counted over the slots of every read (link kernel, integer atomics).
 *   hello_phase_chain: host only, opens no GPU.  link int32 [n_records][window][2], chromosome int32 [n_records] (records of
 *          another chromosome are not linked) -> set [n_records] (the index of the record that opened the set of t) and flip.
 *   hello_phase_tag: with the chained set / flip of the handle's records, hp (1, 2, or 0) and ps (the POS of the read's phase set,
 *          or 0) of every read given to hello_phase_observe, in the order given (tag kernel over the slots kept on the device).
 *   hello_phase_fragments: called once, after the last hello_phase_observe and before any tag call, with
 *          name_hash / flags / source of EVERY read given so far, in the order given (n_reads must equal the handle's, else
 *          HELLO_ERR_ARG).  The counted reads of all batches are grouped by (source, name_hash); a group of exactly two reads with
 *          flag 0x1, one with flag & 0xC0 == 0x40 and one with == 0x80, is a pair, and mate[r] is the other read's index (-1 for
 *          every other read).  The fragment links count every (pair or single read) once over its merged observations; the
 *          per-read arrays 0 - 5 stay as they are.  Pair kernels (an open-addressing table, integer atomics) and fragment-link kernel.
 *   hello_phase_tag_fragments: as hello_phase_tag, the two mates of a pair getting the hp / ps of their fragment (arrays 4 and 5).
 * Host memory in and out; phase.hip. */
#define HELLO_PHASE_MAX_WINDOW 32
#define HELLO_PHASE_STATS 9
#define HELLO_PHASE_FRAGMENT_STATS 5
enum {
    HELLO_PHASE_SLOTS = 0,         /* int8 [slots] */
    HELLO_PHASE_SLOT_OFFSETS = 1,  /* int64 [reads + 1]: an uncounted read has no slot */
    HELLO_PHASE_FIRST = 2,         /* int64 [reads]: the record of the read's first slot */
    HELLO_PHASE_LINKS = 3,         /* int32 [n_records][window][2], summed over the batches */
    HELLO_PHASE_HP = 4,            /* uint8 [reads], after hello_phase_tag */
    HELLO_PHASE_PS = 5             /* int64 [reads], after hello_phase_tag */
};
enum {
    HELLO_PHASE_MATE = 6,            /* int64 [reads], after hello_phase_fragments: the mate's index or -1 */
    HELLO_PHASE_FRAGMENT_LINKS = 7   /* int32 [n_records][window][2], after hello_phase_fragments */
};
typedef struct hello_phase hello_phase;
int hello_phase_observe(const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                        const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends, const uint8_t* mapq,
                        const uint16_t* flags, const uint64_t* name_hash, const uint8_t* source, int64_t n_reads,
                        const int64_t* record_starts, const int64_t* record_ends, const uint8_t* alleles,
                        const int64_t* allele_offsets, int64_t n_records, int32_t q_threshold, int32_t mapq_threshold,
                        int32_t window, int32_t device, hello_phase** handle);
int hello_phase_chain(const int32_t* link, const int32_t* chromosome, int64_t n_records, int32_t window, int32_t min_margin,
                      int32_t* set, uint8_t* flip);
int hello_phase_tag(hello_phase* phase, const int32_t* set, const uint8_t* flip);
/* a pointer into `phase` (valid until the next hello_phase_* call on it) and its element count */
int hello_phase_array(const hello_phase* phase, int32_t which, const void** data, int64_t* count);
/* stats[HELLO_PHASE_STATS]: records, reads given, reads counted, slots, observe / link / tag kernel ms (HIP events), plan ms,
 * total ms of the calls */
int hello_phase_stats(const hello_phase* phase, double* stats);
int hello_phase_fragments(hello_phase* phase, const uint64_t* name_hash, const uint16_t* flags, const uint8_t* source,
                          int64_t n_reads);
int hello_phase_tag_fragments(hello_phase* phase, const int32_t* set, const uint8_t* flip);
/* stats[HELLO_PHASE_FRAGMENT_STATS]: pairs, groups of two or more reads that were not joined, pair / fragment-link / fragment-tag
 * kernel ms (HIP events) */
int hello_phase_fragment_stats(const hello_phase* phase, double* stats);
void hello_phase_free(hello_phase* phase);

/* Haplotags from a phased VCF (not in the reference; DESIGN.md section 7h states the rule, hello_amd/haplotag.py restates it in
 * Python).  One handle per chromosome; it keeps the record table on the device.
 *   hello_haplotag_create: the chromosome's phased records -- record_starts / record_ends [n_records] (the span [POS - 1,
 *          POS - 1 + len(REF)), sorted by start), `alleles` with allele_offsets [2 n_records + 1]: the haplotype-1 then the
 *          haplotype-2 allele of every record, upper case, and ps [n_records], the records' positive phase sets -- validated and
 *          uploaded once.  NULL pointers, n_records < 0, records that are not sorted and a phase set below 1 are refused
 *          (HELLO_ERR_ARG) before the device is opened; n_records == 0 opens none.
 *   hello_haplotag_reads: reads: the arrays of hello_bam_fetch (`source` is not read and may be NULL: a read is tagged alike
 *          whichever BAM it came from); a read counts by the rule of hello_refblocks_find, and a counted read whose CIGAR consumes
 *          more bases than it has is refused (HELLO_ERR_ARG) before any launch.  One fused launch, a wave per read: the read's
 *          candidate records by two searches in the table, the walk of hello_phase_observe at each, and across the wave the phase
 *          set of the read's first observation and the counts n1 / n2 of its observations in that set.  hp [n_reads]: 1, 2, or 0
 *          (a tie, no observation, an uncounted read); ps [n_reads]: that set, also at a tie, or 0.  n_records == 0 or
 *          n_reads == 0 launches nothing and gives zeros.  Any number of calls, in any order: the result of a read depends on
 *          that read and the table alone.
 * Host memory in and out; haplotag.hip. */
#define HELLO_HAPLOTAG_STATS 9
typedef struct hello_haplotag hello_haplotag;
int hello_haplotag_create(const int64_t* record_starts, const int64_t* record_ends, const uint8_t* alleles,
                          const int64_t* allele_offsets, const int64_t* ps, int64_t n_records, int32_t device,
                          hello_haplotag** handle);
int hello_haplotag_reads(hello_haplotag* haplotag, const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets,
                         const uint32_t* cigars, const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends,
                         const uint8_t* mapq, const uint16_t* flags, const uint64_t* name_hash, const uint8_t* source, int64_t n_reads,
                         int32_t q_threshold, int32_t mapq_threshold, uint8_t* hp, int64_t* ps);
/* stats[HELLO_HAPLOTAG_STATS]: records, calls, reads given, reads counted, reads with hp 1, reads with hp 2, kernel ms (HIP
 * events), plan ms (the host's walk over the reads), total ms of create and the calls */
int hello_haplotag_stats(const hello_haplotag* haplotag, double* stats);
void hello_haplotag_free(hello_haplotag* haplotag);

/* PCR duplicates among the reads of one chromosome of one BAM (not in the reference; DESIGN.md section 7j states the rules,
 * hello_amd/markdup.py restates them in Python).  One handle per (BAM, chromosome).
 *   hello_markdup_add: with *handle NULL it creates the handle; every call adds the reads of one span.  reads: the arrays of
 *          hello_bam_fetch (`bases`, `mapq` and `source` are not read and may be NULL).  A read is eligible when
 *          flag & (0x4 | 0x100 | 0x800 | 0x400) == 0.  Offsets that do not start at 0 or decrease, and an eligible read with an
 *          unknown CIGAR operation, a CIGAR that does not consume its bases or a ref_end that its CIGAR does not give, are
 *          refused (HELLO_ERR_ARG) before the device is opened and before any launch; so are more than 2^31 - 1 eligible reads
 *          in one handle.  Ends kernel, a wave per eligible read: e = 2 end5 + strand (end5: ref_start minus the leading S / H
 *          run of a forward read, ref_end - 1 plus the trailing S / H run of a reverse read) and score = the sum of the base
 *          qualities >= 15, saturated at 2^30 - 1.  name_hash, flags, e and score of the eligible reads stay on the device.
 *   hello_markdup_find: called once, after the last hello_markdup_add; a second call, and hello_markdup_add after it, are refused
 *          (HELLO_ERR_ARG).  The eligible reads of all spans are joined into pairs by the mate join of hello_phase_fragments
 *          (source 0 for all); a joined read is of kind 1 (pair), another read without flag 0x1 or with 0x8 of kind 2 (single),
 *          every other eligible read of kind 3 (unresolved: never marked, shields nothing).  Key kernel (a second open-addressing
 *          table, integer atomics): within one (lo, hi) of the mates' packed ends the pair with the largest summed score
 *          survives, ties to the smaller of its smaller read index; within one e, every single is a duplicate where a joined
 *          read has that e, else the single with the largest score survives, ties to the smaller index.  Mark kernel: kind and
 *          duplicate of every read.  More than 2^29 eligible reads are refused (the tables are indexed with 32 bits).
 *   hello_markdup_array: aligned with the reads given, in the order given; e and score after hello_markdup_add, the rest after
 *          hello_markdup_find.  A read that is not eligible has e 0, score 0, mate -1, kind 0, duplicate 0.
 * Host memory in and out; markdup.hip. */
#define HELLO_MARKDUP_STATS 12
enum {
    HELLO_MARKDUP_E = 0,          /* int64 [reads] */
    HELLO_MARKDUP_SCORE = 1,      /* int32 [reads] */
    HELLO_MARKDUP_MATE = 2,       /* int64 [reads]: the mate's index or -1 */
    HELLO_MARKDUP_KIND = 3,       /* uint8 [reads]: 0 not eligible, 1 pair, 2 single, 3 unresolved */
    HELLO_MARKDUP_DUPLICATE = 4   /* uint8 [reads] */
};
typedef struct hello_markdup hello_markdup;
int hello_markdup_add(const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                      const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends, const uint8_t* mapq,
                      const uint16_t* flags, const uint64_t* name_hash, const uint8_t* source, int64_t n_reads, int32_t device,
                      hello_markdup** handle);
int hello_markdup_find(hello_markdup* markdup);
/* a pointer into `markdup` (valid until the next hello_markdup_* call on it) and its element count */
int hello_markdup_array(const hello_markdup* markdup, int32_t which, const void** data, int64_t* count);
/* stats[HELLO_MARKDUP_STATS]: reads given, eligible, pairs, singles, unresolved, groups of two or more reads that were not joined,
 * duplicate pairs, duplicate singles, ends / pair / key / mark kernel ms (HIP events) */
int hello_markdup_stats(const hello_markdup* markdup, double* stats);
void hello_markdup_free(hello_markdup* markdup);

/* Alignment, coverage and insert-size metrics of one chromosome of one BAM (not in the reference; DESIGN.md section 7k states the
 * rules, hello_amd/qc.py restates them in Python).  One handle per (BAM, chromosome); every table is int64.
 *   hello_qc_add: with *handle NULL it creates the handle; every call adds the reads overlapping one span [lo, hi) of the
 *          chromosome whose text is `reference` (all of it, reference_length bytes).  reads: the arrays of hello_bam_fetch
 *          (`source` is not read and may be NULL), coordinate-sorted.  A read BELONGS to the span when lo <= ref_start; it is
 *          MEASURED when flag & (0x4 | 0x100 | 0x800 | 0x400 | 0x200) == 0 and COUNTED by the gVCF's rule at mapq_threshold.
 *          The per-read tables (FLAGS over the belonging reads; MAPQ, LENGTH, CYCLE, QUALITY over the belonging measured reads)
 *          come from the reads kernel, the depth tables (every counted read given, over the positions of [lo, hi)) from the
 *          depth kernel.  targets: sorted intervals [start, stop) with 0 <= start < stop that do not overlap (they may touch,
 *          and may end behind the chromosome).  Refused (HELLO_ERR_ARG) before the device is opened and before any launch:
 *          offsets that do not start at 0 or decrease; unsorted reads; a measured or counted read with a negative ref_start, an
 *          unknown CIGAR operation, a CIGAR that does not consume exactly its bases or a ref_end its CIGAR does not give; a
 *          belonging measured read of more than 2^31 / 255 bases; lo below the previous hi; hi <= lo or hi > reference_length;
 *          window < 1; such targets; a reference length, targets, window, threshold or device other than the first call's.  A
 *          refused call leaves the handle as it was.
 *   hello_qc_finish: called once, after the last hello_qc_add; a second call, and hello_qc_add after it, are refused.  The
 *          belonging measured reads of all spans are joined by the mate join of hello_phase_fragments (source 0 for all) and the
 *          insert kernel fills INSERT.
 *   hello_qc_array: INSERT after hello_qc_finish, the others after any hello_qc_add.
 * Host memory in and out; qc.hip. */
#define HELLO_QC_STATS 12
#define HELLO_QC_FLAG_FIELDS 13      /* reads, unmapped, secondary, supplementary, duplicate, qc_fail, paired, proper_pair, read1,
                                        read2, mate_unmapped, reverse, mapq0 */
#define HELLO_QC_CYCLES 513          /* a base's index in sequencing order, the last bin holding "512 or more" */
#define HELLO_QC_CYCLE_FIELDS 7      /* bases, quality_sum, aligned, mismatches, inserted, soft_clipped, deletions */
#define HELLO_QC_LENGTHS 65536
#define HELLO_QC_DEPTHS 1024
#define HELLO_QC_INSERTS 4096        /* per orientation: FR, RF, TANDEM */
enum {
    HELLO_QC_FLAGS = 0,              /* [HELLO_QC_FLAG_FIELDS] */
    HELLO_QC_MAPQ = 1,               /* [256] */
    HELLO_QC_LENGTH = 2,             /* [HELLO_QC_LENGTHS] */
    HELLO_QC_CYCLE = 3,              /* [2][HELLO_QC_CYCLES][HELLO_QC_CYCLE_FIELDS]: first mates and unpaired reads, then reads with 0x80 */
    HELLO_QC_QUALITY = 4,            /* [256][2]: aligned bases of the reported quality, mismatches among them */
    HELLO_QC_DEPTH_HIST = 5,         /* [HELLO_QC_DEPTHS] */
    HELLO_QC_WINDOW_SUM = 6,         /* [ceil(reference_length / window)] */
    HELLO_QC_TARGET_DEPTH_HIST = 7,  /* [HELLO_QC_DEPTHS] */
    HELLO_QC_TARGET_SUM = 8,         /* [n_targets] */
    HELLO_QC_TARGET_COVERED = 9,     /* [n_targets] */
    HELLO_QC_INSERT = 10             /* [3][HELLO_QC_INSERTS] */
};
typedef struct hello_qc hello_qc;
int hello_qc_add(const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                 const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends, const uint8_t* mapq,
                 const uint16_t* flags, const uint64_t* name_hash, const uint8_t* source, int64_t n_reads, const uint8_t* reference,
                 int64_t reference_length, int64_t lo, int64_t hi, const int64_t* target_starts, const int64_t* target_stops,
                 int64_t n_targets, int32_t mapq_threshold, int64_t window, int32_t device, hello_qc** handle);
int hello_qc_finish(hello_qc* qc);
/* a pointer into `qc` (valid until the next hello_qc_* call on it) and its element count */
int hello_qc_array(const hello_qc* qc, int32_t which, const void** data, int64_t* count);
/* stats[HELLO_QC_STATS]: reads given, belonging, belonging and measured, belonging and counted, measured reads with an aligned
 * base behind the reference's end, positions whose reference byte is not ACGT, pairs, groups of two or more reads that were not
 * joined, reads / depth / pair / insert kernel ms (HIP events) */
int hello_qc_stats(const hello_qc* qc, double* stats);
void hello_qc_free(hello_qc* qc);

/* CpG methylation per haplotype of one chromosome of one BAM, from the MM / ML calls of its reads (not in the reference; DESIGN.md
 * section 7m states the rules, hello_amd/methylation.py restates them in Python).  One handle per (BAM, chromosome).
 *   hello_meth_create: takes a copy of `reference` (all of the chromosome) and needs no device.  The first hello_meth_add that
 *          passes its checks (or hello_meth_array) opens the device, uploads the copy, flags the CpG sites -- position p with
 *          reference[p] & 0xDF == 'C', reference[p + 1] & 0xDF == 'G' -- as a bit vector with the sites before every 64-position
 *          word, writes SITES and drops the copy.
 *   hello_meth_add: the reads overlapping one span [lo, hi), coordinate-sorted: the arrays of hello_bam_fetch with `hp` (the
 *          haplotype of every read: 1 and 2 have a class of their own) in the place of `source`, and those of hello_bam_fetch_mods
 *          with their lengths.  A read BELONGS to the span when lo <= ref_start; a belonging read COUNTS when it is counted by the
 *          gVCF's rule at the handle's mapq_threshold, its CIGAR has no H operation, its state is 1 and its last listed base
 *          exists (found on the device).  Refused (HELLO_ERR_ARG) before any launch: offsets that do not start at 0 or decrease;
 *          unsorted reads; a counted read with a negative ref_start, an unknown CIGAR operation, a CIGAR that does not consume
 *          exactly its bases or a ref_end its CIGAR does not give; lo below the previous hi; hi <= lo or hi > reference_length;
 *          modification offsets that do not start at 0, decrease or do not end at n_deltas; n_probs != n_deltas; a negative
 *          delta; a state above 2 or a mode above 1; more than 2^31 / 255 counting reads in one handle (the device sums are
 *          32-bit).  A refused call leaves the handle as it was.
 *   hello_meth_array: SITES int64 [n_sites]; COUNTS int64 [n_sites][3][3] -- class (all, haplotype 1, haplotype 2) by counter
 *          (modified: value >= 128, unmodified, sum of the values); STATUS uint8 per read of the last hello_meth_add.
 * Host memory in and out; methylation.hip. */
#define HELLO_METH_STATS 10
enum {
    HELLO_METH_SITES = 0,
    HELLO_METH_COUNTS = 1,
    HELLO_METH_STATUS = 2            /* 0 not belonging or not counted, 1 counting, 2 bad modifications, 3 none, 4 hard-clipped */
};
typedef struct hello_meth hello_meth;
int hello_meth_create(const uint8_t* reference, int64_t reference_length, int32_t mapq_threshold, int32_t device, hello_meth** handle);
int hello_meth_add(hello_meth* meth, const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                   const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends, const uint8_t* mapq,
                   const uint16_t* flags, const uint64_t* name_hash, const uint8_t* hp, int64_t n_reads, const int32_t* deltas,
                   int64_t n_deltas, const uint8_t* probs, int64_t n_probs, const int64_t* mod_offsets, const uint8_t* mode,
                   const uint8_t* state, int64_t lo, int64_t hi);
/* a pointer into `meth` (valid until the next hello_meth_* call on it) and its element count */
int hello_meth_array(hello_meth* meth, int32_t which, const void** data, int64_t* count);
/* stats[HELLO_METH_STATS]: reads given, belonging, counting, belonging counted reads without modifications, with bad ones, with
 * a hard clip, observations, sites, sites / reads kernel ms (HIP events) */
int hello_meth_stats(const hello_meth* meth, double* stats);
void hello_meth_free(hello_meth* meth);

/* Base counts per strand at a given list of positions of one chromosome of one BAM -- a pileup at sites -- and on top of it the
 * contamination of the BAM and the identity of two BAMs (not in the reference; DESIGN.md section 7n states the rules,
 * hello_amd/contamination.py restates them in Python).  One handle per (BAM, chromosome).
 *   hello_pileup_create: takes a copy of `pos` (0-based, strictly ascending, inside [0, chromosome_length)) and needs no device.
 *          The first hello_pileup_add that passes its checks (or hello_pileup_array of COUNTS) opens the device and builds the
 *          bit vector of the sites with the sites before every 64-position word.  Refused: NULL, a negative count, a length
 *          outside [0, 2^31 - 1], a position that is not above the one before it or lies outside the chromosome.
 *   hello_pileup_option: HELLO_PILEUP_FORM 0 (the default) runs the reads kernel in two phases -- a lane per read ORs the words
 *          under the read, a wave walks every read that covers a site -- and 1 walks every counting read with a wave.  Both give
 *          the same bytes.  HELLO_PILEUP_SHARE: the counting reads of a workgroup of that kernel, 1 to 1 024, or 0 (the default):
 *          every hello_pileup_add sizes it for about 4 096 workgroups.
 *   hello_pileup_add: the reads overlapping one span [lo, hi), coordinate-sorted: the arrays of hello_bam_fetch.  A read BELONGS
 *          to the span when lo <= ref_start; a belonging read COUNTS when it is counted by the gVCF's rule at the handle's
 *          mapq_threshold.  A counting read observes a site under an M / = / X operation (bins A C G T, OTHER, or LOWQ below
 *          q_threshold, the byte folded with & 0xDF) and under a D operation (bin DEL).  Spans ascend and do not overlap.
 *          Refused, before the device is looked for: what hello_meth_add refuses of the reads and the span, in its words, and
 *          more than 2^31 - 1 counting reads in one handle (the device counters are 32-bit).  A refused call leaves the handle
 *          as it was.
 *   hello_pileup_array: COUNTS int64 [n_sites][2][7] -- strand (flag 0x10) by bin; STATUS uint8 per read of the last add.
 *   hello_contam_estimate / hello_contam_identity: host only, no device.  `r`, `a`, `o`: per site the counts of REF, of ALT and
 *          of the two other bases; `af` the ALT allele's frequency, inside (0, 1).  Refused: NULL, a negative n or count, such
 *          an af.
 * Host memory in and out; pileup.hip, contam.h. */
#define HELLO_PILEUP_STATS 8
#define HELLO_PILEUP_BINS 7          /* A, C, G, T, OTHER, DEL, LOWQ */
#define HELLO_CONTAM_GRID 501        /* alpha_k = k / 1000 */
#define HELLO_CONTAM_OUT 505
enum {
    HELLO_PILEUP_COUNTS = 0,
    HELLO_PILEUP_STATUS = 1          /* 0 not belonging or not counted, 1 counting, 2 counting with an observation */
};
enum { HELLO_PILEUP_FORM = 0, HELLO_PILEUP_SHARE = 1 };
typedef struct hello_pileup hello_pileup;
int hello_pileup_create(const int64_t* pos, int64_t n_sites, int64_t chromosome_length, int32_t q_threshold, int32_t mapq_threshold,
                        int32_t device, hello_pileup** handle);
int hello_pileup_option(hello_pileup* pileup, int32_t which, int32_t value);
int hello_pileup_add(hello_pileup* pileup, const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets,
                     const uint32_t* cigars, const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends,
                     const uint8_t* mapq, const uint16_t* flags, const uint64_t* name_hash, const uint8_t* hp, int64_t n_reads,
                     int64_t lo, int64_t hi);
/* a pointer into `pileup` (valid until the next hello_pileup_* call on it) and its element count */
int hello_pileup_array(hello_pileup* pileup, int32_t which, const void** data, int64_t* count);
/* stats[HELLO_PILEUP_STATS]: reads given, belonging, counting, counting reads with an observation, observations, sites, sites /
 * reads kernel ms (HIP events) */
int hello_pileup_stats(const hello_pileup* pileup, double* stats);
void hello_pileup_free(hello_pileup* pileup);
/* out[HELLO_CONTAM_OUT]: the error rate, k of the greatest likelihood, k_lo, k_hi, LL[HELLO_CONTAM_GRID] */
int hello_contam_estimate(const int64_t* r, const int64_t* a, const int64_t* o, const double* af, int64_t n, double* out);
/* out[2]: LOD, the number of sites used */
int hello_contam_identity(const int64_t* r1, const int64_t* a1, const int64_t* o1, const int64_t* r2, const int64_t* a2,
                          const int64_t* o2, const double* af, int64_t n, double* out);

/* Large deletions and insertions of one chromosome of one BAM from the reads' own CIGARs: every I or D operation of at least
 * min_size bases inside one alignment record, left-aligned against the reference, clustered and genotyped (not in the reference;
 * DESIGN.md section 7p states the rules, hello_amd/sv.py restates them in Python).  Split alignments, clipped ends and discordant
 * pairs are not looked at.  One handle per (BAM, chromosome).
 *   hello_sv_create: takes a copy of `reference` and needs no device.  The first hello_sv_add that passes its checks opens the
 *          device, uploads the text and zeroes the cover's difference array (int32 [length + 1]); both live as long as the handle.
 *          Refused: NULL, a length outside [0, 2^31 - 1], min_size < 1, flank < 1.
 *   hello_sv_add: the reads overlapping one span [lo, hi), coordinate-sorted: the arrays of hello_bam_fetch with `hp`.  A read
 *          belongs and counts by hello_pileup_add's rules.  Every counting, belonging read adds to the cover; those with an I or D
 *          of at least min_size bases are walked by a wave each, and each such operation that keeps `flank` reference bases of the
 *          read on both sides and ends inside the chromosome becomes a signature.  Refused, before the device is looked for: what
 *          hello_pileup_add refuses of the reads and the span, in its words, more than 2^31 - 1 counting reads in one handle, and
 *          a call after hello_sv_finish.  A refused call leaves the handle as it was.
 *   hello_sv_finish: clusters the signatures on the host (cluster_gap >= 0 positions, len_ratio_percent 1 to 100, min_support >= 1
 *          distinct reads), reads the spanning depth of every candidate off the difference array on the device and genotypes it.
 *          Refused a second time.
 *   hello_sv_array: int64 each.  The SIGNATURES columns, sorted by (type, pos, len, ordinal, operation index); the CANDIDATES
 *          columns, after hello_sv_finish, sorted by (pos, type, len); STATUS uint8 per read of the last add.
 *   hello_sv_genotype: host only, no device.  `dv`, `dr`: per candidate the reads with the event and the spanning reads without;
 *          out int64 [n][HELLO_SV_GENOTYPE_COLUMNS]: GT (0, 1, 2 for 0/0, 0/1, 1/1), GQ, PL of the three.  Refused: NULL, a
 *          negative n or count.
 * Split alignments (off unless hello_sv_add_split is called):
 *   hello_sv_contigs: the names of the BAM header's sequences in its order and `own`, the index of the handle's chromosome among
 *          them.  Called once, before the first hello_sv_add_split; host only.  Refused: NULL, n < 1, own outside [0, n), a name
 *          twice, two names of one 64-bit FNV-1a hash, a second call.
 *   hello_sv_add_split: hello_sv_add, and the junctions of the split alignments: `sa_bytes` / `sa_offsets` [n_reads + 1] are the
 *          arrays HELLO_BAM_SA_BYTES / HELLO_BAM_SA_OFFSETS of hello_bam_fetch_sa.  Every counting, belonging read with a
 *          non-empty tag is parsed by a wave (sv_split.h: parse_sa_entry); each pair of segments that follow each other on the
 *          read becomes a row of the SIGNATURES columns -- DEL 0, INS 1, DUP 2, INV 3 (3' ends joined) and 4 (5' ends), BND 5
 *          (LEN: the mate's contig index or -1, SHIFT: its breakpoint) -- with the operation index -(k + 1).  A handle may mix
 *          the two adds, one call per span.  Refused: what hello_sv_add refuses, a handle without contigs, offsets that begin
 *          below 0, decrease or run past n_sa_bytes.  The text itself is never a refusal: it sets the read's SPLIT_STATUS.
 *          A refused call leaves the handle as it was.
 *   hello_sv_cluster_split: hello_sv_cluster over the types 0 to 4, with SR (the distinct reads with a split row) as 14th column.
 * Host memory in and out; sv.hip, sv.h, sv_split.h. */
#define HELLO_SV_STATS 19
#define HELLO_SV_GENOTYPE_COLUMNS 5
enum {
    HELLO_SV_SIGNATURES_TYPE = 0,        /* 0 DEL, 1 INS */
    HELLO_SV_SIGNATURES_POS = 1,         /* 0-based, after the move to the left */
    HELLO_SV_SIGNATURES_LEN = 2,
    HELLO_SV_SIGNATURES_SHIFT = 3,
    HELLO_SV_SIGNATURES_ORDINAL = 4,     /* the read's index among the handle's counting reads */
    HELLO_SV_SIGNATURES_OP = 5,          /* the operation's index in the read's CIGAR */
    HELLO_SV_SIGNATURES_STRAND = 6,      /* flag 0x10 */
    HELLO_SV_SIGNATURES_HP = 7,
    HELLO_SV_CANDIDATES_TYPE = 8,
    HELLO_SV_CANDIDATES_POS = 9,
    HELLO_SV_CANDIDATES_LEN = 10,
    HELLO_SV_CANDIDATES_DV = 11,
    HELLO_SV_CANDIDATES_DV_FWD = 12,
    HELLO_SV_CANDIDATES_DV_REV = 13,
    HELLO_SV_CANDIDATES_HP0 = 14,
    HELLO_SV_CANDIDATES_HP1 = 15,
    HELLO_SV_CANDIDATES_HP2 = 16,
    HELLO_SV_CANDIDATES_POS_MIN = 17,
    HELLO_SV_CANDIDATES_POS_MAX = 18,
    HELLO_SV_CANDIDATES_LEN_MIN = 19,
    HELLO_SV_CANDIDATES_LEN_MAX = 20,
    HELLO_SV_CANDIDATES_DP = 21,
    HELLO_SV_CANDIDATES_DR = 22,
    HELLO_SV_CANDIDATES_GT = 23,
    HELLO_SV_CANDIDATES_GQ = 24,
    HELLO_SV_CANDIDATES_PL0 = 25,
    HELLO_SV_CANDIDATES_PL1 = 26,
    HELLO_SV_CANDIDATES_PL2 = 27,
    HELLO_SV_STATUS = 28,                /* 0 not belonging or not counted, 1 counting, 2 walked, 3 walked with a signature */
    HELLO_SV_CANDIDATES_SR = 29,         /* int64: the distinct supporting reads with a row of a split alignment */
    HELLO_SV_SPLIT_STATUS = 30           /* uint8 per read of the last add: 0 no tag or not counting, 1 parsed without a row, 2 with a
                                            row, 3 BAD_SA, 4 TOO_MANY (more than 7 entries) */
};
typedef struct hello_sv hello_sv;
int hello_sv_create(const uint8_t* reference, int64_t reference_length, int32_t min_size, int32_t flank, int32_t mapq_threshold,
                    int32_t device, hello_sv** handle);
int hello_sv_add(hello_sv* sv, const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                 const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends, const uint8_t* mapq,
                 const uint16_t* flags, const uint64_t* name_hash, const uint8_t* hp, int64_t n_reads, int64_t lo, int64_t hi);
int hello_sv_finish(hello_sv* sv, int64_t cluster_gap, int32_t len_ratio_percent, int32_t min_support);
/* a pointer into `sv` (valid until the next hello_sv_* call on it) and its element count */
int hello_sv_array(hello_sv* sv, int32_t which, const void** data, int64_t* count);
/* stats[HELLO_SV_STATS]: reads given, belonging, counting, walked, walked reads with a signature, signatures of CIGAR operations,
 * candidates, cover / reads / finish kernel ms (HIP events); then of hello_sv_add_split: reads with a tag, BAD_SA reads, TOO_MANY
 * reads, junctions, junctions dropped / small / unplaced, rows of junctions, split kernel ms */
int hello_sv_stats(const hello_sv* sv, double* stats);
void hello_sv_free(hello_sv* sv);
int hello_sv_genotype(const int64_t* dv, const int64_t* dr, int64_t n, int64_t* out);
/* The clustering of hello_sv_finish alone, host only: signatures int64 [n][8] in the SIGNATURES columns' order, any row order ->
 * out int64 [*n_out][HELLO_SV_CLUSTER_COLUMNS], the CANDIDATES columns TYPE .. LEN_MAX; `out` has room for n rows. */
#define HELLO_SV_CLUSTER_COLUMNS 13
int hello_sv_cluster(const int64_t* signatures, int64_t n, int64_t cluster_gap, int32_t len_ratio_percent, int32_t min_support,
                     int64_t* out, int64_t* n_out);
#define HELLO_SV_CLUSTER_SPLIT_COLUMNS 14
int hello_sv_cluster_split(const int64_t* signatures, int64_t n, int64_t cluster_gap, int32_t len_ratio_percent, int32_t min_support,
                           int64_t* out, int64_t* n_out);
int hello_sv_contigs(hello_sv* sv, const char* const* names, int64_t n, int64_t own);
int hello_sv_add_split(hello_sv* sv, const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                       const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends, const uint8_t* mapq,
                       const uint16_t* flags, const uint64_t* name_hash, const uint8_t* hp, const uint8_t* sa_bytes,
                       const int64_t* sa_offsets, int64_t n_sa_bytes, int64_t n_reads, int64_t lo, int64_t hi);

/* Discordant read pairs and clipped ends (off unless hello_sv_add_pairs is called):
 *   hello_sv_library: the library's inner distances (median, lo, hi), once, before the first hello_sv_add_pairs; host only.  The
 *          unset triple (0, INT32_MIN, INT32_MAX) is valid too: then only orientation and BND rows arise, which is how a library is
 *          sampled.  Refused: NULL, lo > median, median > hi, a second call.
 *   hello_sv_clip_min: the fewest bases of a soft clip that counts (default 20), before the first hello_sv_add_pairs; host only.
 *   hello_sv_add_pairs: hello_sv_add_split, and per belonging read the pair rules: `mate_tid` / `mate_pos` are the arrays
 *          HELLO_BAM_MATE_TID / HELLO_BAM_MATE_POS of hello_bam_fetch_pairs.  A pair-counted read (flag 0x1, none of 0x4 0x8 0x100
 *          0x800 0x400 0x200, mapq at the threshold; 0x2 is not consulted) needs mate_pos in [0, 2^31 - 1], mate_pos <= length
 *          when mate_tid is the handle's chromosome, and its own end inside the chromosome: else its PAIR_STATUS is BAD_MATE, it
 *          emits nothing and is counted.  The host checks this before any launch; no kernel indexes with an unchecked value.
 *          Refused: what hello_sv_add_split refuses, a handle without a library.  A refused call leaves the handle as it was.  A
 *          handle may mix the three adds.
 *   hello_sv_pairs_array / hello_sv_pairs_stats: new getters; hello_sv_array and hello_sv_stats keep their selectors and meanings,
 *          and with pairs on SIGNATURES_* and CANDIDATES_* of hello_sv_array also hold the pair rows (OP = -16) and the pair-only
 *          candidates.
 *   hello_sv_cluster_pairs: host only.  signatures int64 [n][8] of all kinds -> out int64 [*n_out][HELLO_SV_CLUSTER_PAIRS_COLUMNS]:
 *          the 14 columns of hello_sv_cluster_split, then PR, END_MIN, END_MAX, IMPRECISE; `out` has room for n rows.
 *   hello_sv_library_of: host only.  inner int64 [4096] -> out[3] = (median, lo, hi) with hi - median = median - lo = k max(mad, 1). */
#define HELLO_SV_PAIRS_STATS 13
#define HELLO_SV_CLUSTER_PAIRS_COLUMNS 18
enum {
    HELLO_SV_PAIRS_INNER = 0,            /* int64 [4096]: bin clamp(mate_pos - ref_end + 1024, 0, 4095) of the left FR records */
    HELLO_SV_PAIRS_CLIP_LEFT = 1,        /* int32 [length + 1]: reads whose aligned part ends here before a counting soft clip */
    HELLO_SV_PAIRS_CLIP_RIGHT = 2,       /* int32 [length + 1]: reads whose aligned part starts here behind a counting soft clip */
    HELLO_SV_PAIRS_STATUS = 3,           /* uint8 per read of the last add: 0 not pair-counted, 1 BAD_MATE, 2 right record, 3 normal,
                                            4 short, 5 small, 6 unplaced, 7 with a row, 8 with a BND row */
    HELLO_SV_PAIRS_CANDIDATES_PR = 4,    /* int64, after hello_sv_finish: the supporting pairs */
    HELLO_SV_PAIRS_CANDIDATES_CE = 5,    /* the clipped ends within flank of the candidate's two ends */
    HELLO_SV_PAIRS_CANDIDATES_END_MIN = 6,
    HELLO_SV_PAIRS_CANDIDATES_END_MAX = 7,
    HELLO_SV_PAIRS_CANDIDATES_IMPRECISE = 8      /* 1: from pair rows alone */
};
int hello_sv_library(hello_sv* sv, int32_t median, int32_t lo, int32_t hi);
int hello_sv_clip_min(hello_sv* sv, int32_t clip_min);
int hello_sv_add_pairs(hello_sv* sv, const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                       const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends, const uint8_t* mapq,
                       const uint16_t* flags, const uint64_t* name_hash, const uint8_t* hp, const uint8_t* sa_bytes,
                       const int64_t* sa_offsets, int64_t n_sa_bytes, const int32_t* mate_tid, const int64_t* mate_pos, int64_t n_reads,
                       int64_t lo, int64_t hi);
int hello_sv_pairs_array(hello_sv* sv, int32_t which, const void** data, int64_t* count);
/* stats[HELLO_SV_PAIRS_STATS]: pair-counted belonging reads, left records, right records, normal, short, small, unplaced, BAD_MATE,
 * pair rows, reads with a counting clip, pair rows a cluster took, pair-only candidates (the last two after hello_sv_finish), the
 * pairs kernel's ms */
int hello_sv_pairs_stats(const hello_sv* sv, double* stats);
int hello_sv_cluster_pairs(const int64_t* signatures, int64_t n, int64_t cluster_gap, int32_t len_ratio_percent, int32_t min_support,
                           int32_t median, int32_t lo, int32_t hi, int32_t flank, int64_t* out, int64_t* n_out);
int hello_sv_library_of(const int64_t* inner, int64_t k, int64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* HELLO_MI355X_H */
