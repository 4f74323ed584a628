// Alignment, coverage and insert-size metrics (include/hello_mi355x.h: hello_qc_*): the aligned reads of one chromosome of one BAM,
// span after span, and the chromosome's text -> integer tables.  Not in the reference; DESIGN.md section 7k states the rules and
// hello_amd/qc.py restates them in Python, integer for integer.
//
// Host: the three read classes and the validation of every measured or counted read (cigar.h: qc_walk; the kernels index with
// its CIGAR, bases and qualities), the reads kernel's chunks, and per tile of kQcTile positions the range of counted reads and of
// targets that can touch it.  Device, per hello_qc_add two kernels:
//   reads: a workgroup per chunk of belonging reads, a wave per read.  Lane 0 counts the flags, mapq and length; the wave walks
//     the CIGAR operation by operation (wave-uniform loop) with the lanes on an operation's bases.  CYCLE, QUALITY, MAPQ, FLAGS and
//     the lengths below 1 024 are int32 tables in LDS (36 KB); a chunk of bases that lies in the last cycle bin as a whole is summed
//     in the wave first.  After a barrier every non-zero entry goes to the global int64 table with one 64-bit add.
//   depth: a workgroup per tile, as the count launch of refblocks.hip: the four waves walk the tile's counted reads, the lanes take
//     the positions of an M/=/X or D operation, one int32 counter per position in LDS.  After a barrier a thread takes four
//     positions: the depth histogram, the window and target sums of the tile build up in LDS, and after another barrier the tile
//     issues one global add per non-zero bin, window and target.
// and per hello_qc_finish, over the belonging measured reads of ALL spans:
//   pair (two kernels): the mate join of section 7i, phase_pair.h; `source` is 0 for every read.
//   insert: a thread per read, acting for the pair when its mate has the larger index; a 48 KB histogram in LDS and one flush.
// Every output is an integer sum, so no result depends on the order of the atomic adds: two runs give the same bytes.
#include <memory>

#include "phase_pair.h"
#include "read_walk.h"
#include "stage_host.h"

namespace hello {
namespace {

constexpr int kQcThreads = 256;
constexpr int kQcWaves = kQcThreads / 64;
constexpr int kQcTile = 1024;
constexpr int kQcPer = kQcTile / kQcThreads;
constexpr int kQcLastCycle = HELLO_QC_CYCLES - 1;
constexpr int kQcLdsLengths = 1024;

// The reads kernel's table, in LDS (int32, lengths below kQcLdsLengths) and in global memory (int64, every length): the same index.
constexpr int kQcCycle = 0;
constexpr int kQcQuality = kQcCycle + 2 * HELLO_QC_CYCLES * HELLO_QC_CYCLE_FIELDS;
constexpr int kQcMapq = kQcQuality + 256 * 2;
constexpr int kQcFlags = kQcMapq + 256;                 // HELLO_QC_FLAG_FIELDS, then reads_past_reference
constexpr int kQcLength = kQcFlags + 16;
constexpr int kQcLdsInts = kQcLength + kQcLdsLengths;   // 8 990 int32 = 35 960 bytes
constexpr int kQcTableInts = kQcLength + HELLO_QC_LENGTHS;
enum { F_BASES = 0, F_QSUM, F_ALIGNED, F_MISMATCH, F_INSERTED, F_SOFT, F_DELETIONS };

// Reads per workgroup: enough that the flush of up to 8 990 entries is small beside the walk, few enough that 200 k reads fill the
// chip.  A chunk also ends before its bases pass kQcMaxReadBases = 2^31 / 255 -- a quality is at most 255, so no int32 sum of
// qualities in LDS can overflow (no read is longer than that either: qc_walk).
constexpr int64_t kQcChunkReads = 256;

struct QcReadsArgs {
    const uint8_t* bases;
    const uint8_t* quals;
    const int64_t* read_off;
    const uint32_t* cigars;
    const int64_t* cigar_off;
    const int64_t* ref_start;
    const uint16_t* flags;
    const uint8_t* mapq;
    const int64_t* list;         // the belonging reads, in input order
    const int64_t* chunk;        // [blocks + 1]: workgroup b takes list[chunk[b] .. chunk[b + 1])
    const uint8_t* ref;          // reference text of [ref_lo, ref_hi)
    int64_t ref_lo, ref_length;  // ref_hi covers every aligned base below ref_length
    unsigned long long* table;   // [kQcTableInts]
};

__device__ __forceinline__ bool qc_acgt(unsigned u) { return u == 'A' || u == 'C' || u == 'G' || u == 'T'; }

__device__ __forceinline__ int qc_wave_sum(int v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;                                                            // lane 0 holds the sum
}

__global__ __launch_bounds__(kQcThreads) void qc_reads_kernel(QcReadsArgs a) {
    __shared__ int t[kQcLdsInts];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int j = tid; j < kQcLdsInts; j += kQcThreads) t[j] = 0;
    __syncthreads();
    const int64_t k1 = a.chunk[blockIdx.x + 1];
    for (int64_t k = a.chunk[blockIdx.x] + wave; k < k1; k += kQcWaves) {
        const int64_t r = a.list[k];
        const int flag = a.flags[r], mq = a.mapq[r];
        const int64_t q0 = a.read_off[r];
        const int len = (int)(a.read_off[r + 1] - q0);                    // at most kQcMaxReadBases where the read is measured
        const bool measured = !(flag & kQcNotMeasured);
        if (lane == 0) {
            int* f = t + kQcFlags;
            atomicAdd(&f[0], 1);
            if (flag & 0x4) atomicAdd(&f[1], 1);
            if (flag & 0x100) atomicAdd(&f[2], 1);
            if (flag & 0x800) atomicAdd(&f[3], 1);
            if (flag & 0x400) atomicAdd(&f[4], 1);
            if (flag & 0x200) atomicAdd(&f[5], 1);
            if (flag & 0x1) atomicAdd(&f[6], 1);
            if ((flag & 0x3) == 0x3) atomicAdd(&f[7], 1);
            if (flag & 0x40) atomicAdd(&f[8], 1);
            if (flag & 0x80) atomicAdd(&f[9], 1);
            if ((flag & 0x9) == 0x9) atomicAdd(&f[10], 1);
            if (flag & 0x10) atomicAdd(&f[11], 1);
            if (!(flag & 0x4) && mq == 0) atomicAdd(&f[12], 1);
            if (measured) {
                atomicAdd(&t[kQcMapq + mq], 1);
                if (len < kQcLdsLengths) atomicAdd(&t[kQcLength + len], 1);
                else atomicAdd(&a.table[kQcLength + (len < HELLO_QC_LENGTHS - 1 ? len : HELLO_QC_LENGTHS - 1)], 1ull);
            }
        }
        if (!measured) continue;                                          // the whole wave; its CIGAR was not validated
        int* cyc = t + kQcCycle + ((flag & 0x80) ? HELLO_QC_CYCLES * HELLO_QC_CYCLE_FIELDS : 0);
        const bool reverse = (flag & 0x10) != 0;
        const uint8_t* bases = a.bases + q0;
        const uint8_t* quals = a.quals + q0;
        const int64_t c0 = a.cigar_off[r], n_ops = a.cigar_off[r + 1] - c0;
        int64_t rf = a.ref_start[r];
        int rd = 0;
        bool past = false;
        for (int64_t ci = 0; ci < n_ops; ++ci) {
            const CigarOp o = decode_op(a.cigars[c0 + ci]);
            const int op = o.op, n = o.n;
            const bool m = o.m;
            if (o.on_read()) {
                const int field = m ? F_ALIGNED : op == BAM_CINS ? F_INSERTED : F_SOFT;
                for (int j0 = 0; j0 < n; j0 += 64) {
                    const int j = j0 + lane;
                    const bool on = j < n;
                    const int i = rd + (on ? j : j0);                      // a base of the read in either case
                    const int raw = reverse ? len - 1 - i : i;
                    const int q = on ? quals[i] : 0;
                    bool aligned = false, mismatch = false;
                    if (on && m) {
                        const int64_t p = rf + j;
                        if (p >= a.ref_length) {
                            past = true;
                        } else {
                            const unsigned u = bases[i] & 0xDF, v = a.ref[p - a.ref_lo] & 0xDF;
                            aligned = qc_acgt(u) && qc_acgt(v);
                            mismatch = aligned && u != v;
                        }
                    }
                    const int last = j0 + 63 < n ? j0 + 63 : n - 1;
                    const int lowest = reverse ? len - 1 - (rd + last) : rd + j0;   // the smallest cycle of the chunk's bases
                    if (lowest >= kQcLastCycle) {                          // wave-uniform: 64 adds to one bin become one
                        const int n_on = __popcll(__ballot(on)), q_sum = qc_wave_sum(q);
                        const int n_al = __popcll(__ballot(aligned)), n_mm = __popcll(__ballot(mismatch));
                        if (lane == 0) {
                            int* b = cyc + kQcLastCycle * HELLO_QC_CYCLE_FIELDS;
                            atomicAdd(&b[F_BASES], n_on);
                            atomicAdd(&b[F_QSUM], q_sum);
                            if (!m) atomicAdd(&b[field], n_on);
                            if (n_al) atomicAdd(&b[F_ALIGNED], n_al);
                            if (n_mm) atomicAdd(&b[F_MISMATCH], n_mm);
                        }
                    } else if (on) {
                        int* b = cyc + (raw < kQcLastCycle ? raw : kQcLastCycle) * HELLO_QC_CYCLE_FIELDS;
                        atomicAdd(&b[F_BASES], 1);
                        atomicAdd(&b[F_QSUM], q);
                        if (!m) atomicAdd(&b[field], 1);
                        if (aligned) atomicAdd(&b[F_ALIGNED], 1);
                        if (mismatch) atomicAdd(&b[F_MISMATCH], 1);
                    }
                    if (aligned) {                                         // every lane for itself: section 7k has the measurement
                        atomicAdd(&t[kQcQuality + 2 * q], 1);
                        if (mismatch) atomicAdd(&t[kQcQuality + 2 * q + 1], 1);
                    }
                }
                rd += n;
                if (m) rf += n;
            } else if (op == BAM_CDEL) {
                if (lane == 0 && len > 0) {
                    const int i = rd < len - 1 ? rd : len - 1;
                    const int raw = reverse ? len - 1 - i : i;
                    atomicAdd(&cyc[(raw < kQcLastCycle ? raw : kQcLastCycle) * HELLO_QC_CYCLE_FIELDS + F_DELETIONS], 1);
                }
                rf += n;
            } else if (op == BAM_CREF_SKIP) {
                rf += n;
            }
        }
        if (__ballot(past) && lane == 0) atomicAdd(&t[kQcFlags + HELLO_QC_FLAG_FIELDS], 1);
    }
    __syncthreads();
    for (int j = tid; j < kQcLdsInts; j += kQcThreads)
        if (t[j]) atomicAdd(&a.table[j], (unsigned long long)t[j]);
}

struct QcDepthArgs {
    const uint32_t* cigars;
    const int64_t* cigar_off;
    const int64_t* ref_start;
    const int64_t* list;         // the counted reads that touch [lo, hi), in coordinate order
    const int64_t* list_end;     // reference end of list[k], from its CIGAR
    const int64_t* tile_reads;   // [tiles][2]: the range of `list`
    const int64_t* tile_targets; // [tiles][2]: the range of targets that touch the tile, at most kQcTile of them
    const int64_t* t_start;
    const int64_t* t_stop;
    const uint8_t* ref;          // reference text from lo on
    int64_t lo, hi, window;
    unsigned long long* hist;    // [HELLO_QC_DEPTHS]
    unsigned long long* t_hist;
    unsigned long long* w_sum;   // [windows of the chromosome]
    unsigned long long* t_sum;   // [targets]
    unsigned long long* t_cov;
    unsigned long long* excluded;
};

__global__ __launch_bounds__(kQcThreads) void qc_depth_kernel(QcDepthArgs a) {
    __shared__ int depth[kQcTile];
    __shared__ int hist[HELLO_QC_DEPTHS];
    __shared__ int t_hist[HELLO_QC_DEPTHS];
    __shared__ unsigned long long w_sum[kQcTile];                         // a tile touches at most kQcTile windows and targets
    __shared__ unsigned long long t_sum[kQcTile];
    __shared__ int t_cov[kQcTile];
    __shared__ int excluded;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t tile = blockIdx.x;
    const int64_t lo = a.lo + tile * kQcTile, hi = lo + kQcTile < a.hi ? lo + kQcTile : a.hi;
    const int n = (int)(hi - lo);
    for (int j = tid; j < kQcTile; j += kQcThreads) {
        depth[j] = 0; hist[j] = 0; t_hist[j] = 0; w_sum[j] = 0; t_sum[j] = 0; t_cov[j] = 0;
    }
    if (tid == 0) excluded = 0;
    __syncthreads();
    const int64_t b0 = a.tile_reads[2 * tile], n0 = a.tile_reads[2 * tile + 1] - b0;
    for (int64_t k = wave; k < n0; k += kQcWaves) {
        if (a.list_end[b0 + k] <= lo) continue;
        const int64_t r = a.list[b0 + k];
        const int64_t c0 = a.cigar_off[r], n_ops = a.cigar_off[r + 1] - c0;
        int64_t rf = a.ref_start[r];
        for (int64_t ci = 0; ci < n_ops && rf < hi; ++ci) {
            const unsigned c = a.cigars[c0 + ci];
            const int op = c & 15u;
            const int64_t len = c >> 4;
            if (op == BAM_CMATCH || op == BAM_CEQUAL || op == BAM_CDIFF || op == BAM_CDEL) {
                const int64_t j0 = lo > rf ? lo - rf : 0, j1 = hi - rf < len ? hi - rf : len;
                for (int64_t j = j0 + lane; j < j1; j += 64) atomicAdd(&depth[rf + j - lo], 1);
                rf += len;
            } else if (op == BAM_CREF_SKIP) {
                rf += len;
            }
        }
    }
    __syncthreads();

    // ---- thread t owns positions [kQcPer t, kQcPer (t + 1)): consecutive positions of one window are summed before the LDS add
    const int64_t w0 = lo / a.window, tb = a.tile_targets[2 * tile], te = a.tile_targets[2 * tile + 1];
    int64_t w_at = -1;
    unsigned long long w_acc = 0;
    for (int i = 0; i < kQcPer; ++i) {
        const int j = tid * kQcPer + i;
        if (j >= n) break;
        const int64_t p = lo + j;
        const int d = depth[j];
        const bool acgt = qc_acgt(a.ref[p - a.lo] & 0xDF);
        const int bin = d < HELLO_QC_DEPTHS - 1 ? d : HELLO_QC_DEPTHS - 1;
        if (acgt) atomicAdd(&hist[bin], 1); else atomicAdd(&excluded, 1);
        const int64_t w = p / a.window - w0;
        if (w != w_at) {
            if (w_acc) atomicAdd(&w_sum[w_at], w_acc);
            w_at = w;
            w_acc = 0;
        }
        w_acc += (unsigned long long)d;
        int64_t x = tb, y = te;                                            // the last target that starts at or before p
        while (x < y) {
            const int64_t mid = (x + y) >> 1;
            if (a.t_start[mid] <= p) x = mid + 1; else y = mid;
        }
        if (x > tb && p < a.t_stop[x - 1]) {
            if (acgt) atomicAdd(&t_hist[bin], 1);
            if (d) {
                atomicAdd(&t_sum[x - 1 - tb], (unsigned long long)d);
                atomicAdd(&t_cov[x - 1 - tb], 1);
            }
        }
    }
    if (w_acc) atomicAdd(&w_sum[w_at], w_acc);
    __syncthreads();

    const int64_t n_windows = n > 0 ? (hi - 1) / a.window - w0 + 1 : 0;
    for (int j = tid; j < kQcTile; j += kQcThreads) {
        if (hist[j]) atomicAdd(&a.hist[j], (unsigned long long)hist[j]);
        if (t_hist[j]) atomicAdd(&a.t_hist[j], (unsigned long long)t_hist[j]);
        if (j < n_windows && w_sum[j]) atomicAdd(&a.w_sum[w0 + j], w_sum[j]);
        if (j < te - tb && t_sum[j]) {
            atomicAdd(&a.t_sum[tb + j], t_sum[j]);
            atomicAdd(&a.t_cov[tb + j], (unsigned long long)t_cov[j]);
        }
    }
    if (tid == 0 && excluded) atomicAdd(a.excluded, (unsigned long long)excluded);
}

struct QcInsertArgs {
    const int32_t* mate;         // the join's answer
    const uint16_t* flags;
    const int64_t* start;
    const int64_t* end;
    int64_t n;
    unsigned long long* table;   // [3][HELLO_QC_INSERTS]: FR, RF, TANDEM
};

__global__ __launch_bounds__(kQcThreads) void qc_insert_kernel(QcInsertArgs a) {
    __shared__ int h[3 * HELLO_QC_INSERTS];                               // 48 KB
    for (int j = threadIdx.x; j < 3 * HELLO_QC_INSERTS; j += kQcThreads) h[j] = 0;
    __syncthreads();
    for (int64_t c = (int64_t)blockIdx.x * kQcThreads + threadIdx.x; c < a.n; c += (int64_t)gridDim.x * kQcThreads) {
        const int64_t m = a.mate[c];
        if (m <= c) continue;                                             // no mate (-1), or the mate acts for the pair
        const int64_t s0 = a.start[c], s1 = a.start[m], e0 = a.end[c], e1 = a.end[m];
        const int64_t insert = (e0 > e1 ? e0 : e1) - (s0 < s1 ? s0 : s1);
        const bool r0 = (a.flags[c] & 0x10) != 0, r1 = (a.flags[m] & 0x10) != 0;
        int orientation = 2;
        if (r0 != r1) orientation = (r0 ? s1 < e0 : s0 < e1) ? 0 : 1;     // the forward mate's start below the reverse mate's end: FR
        atomicAdd(&h[orientation * HELLO_QC_INSERTS + (int)(insert < HELLO_QC_INSERTS - 1 ? insert : HELLO_QC_INSERTS - 1)], 1);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < 3 * HELLO_QC_INSERTS; j += kQcThreads)
        if (h[j]) atomicAdd(&a.table[j], (unsigned long long)h[j]);
}

template <class T> std::vector<int64_t> fetch_table(const T* device, size_t n) {
    static_assert(sizeof(T) == sizeof(int64_t), "the device tables are 64-bit");
    std::vector<int64_t> out(n);
    if (n) HS_HIP(hipMemcpy(out.data(), device, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    return out;
}

void add_into(std::vector<int64_t>& total, const std::vector<int64_t>& part) {
    for (size_t i = 0; i < part.size(); ++i) total[i] += part[i];
}

}  // namespace
}  // namespace hello

struct hello_qc {
    int device = 0;
    bool finished = false;
    int64_t reference_length = 0, window = 0, last_hi = 0;
    int32_t mapq_threshold = 0;
    std::vector<int64_t> target_starts, target_stops;
    std::vector<int64_t> reads_table, depth_hist, target_hist, window_sum, target_sum, target_covered, insert;
    std::vector<uint64_t> name;                  // of the belonging measured reads of all spans: what hello_qc_finish joins
    std::vector<uint16_t> flags;
    std::vector<int64_t> start, end;
    double stats[HELLO_QC_STATS] = {0};
};

extern "C" {

int hello_qc_add(const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                 const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends, const uint8_t* mapq,
                 const uint16_t* flags, const uint64_t* name_hash, const uint8_t* source, int64_t n_reads, const uint8_t* reference,
                 int64_t reference_length, int64_t lo, int64_t hi, const int64_t* target_starts, const int64_t* target_stops,
                 int64_t n_targets, int32_t mapq_threshold, int64_t window, int32_t device, hello_qc** handle) try {
    using namespace hello;
    (void)source;
    if (!handle || !read_offsets || !cigar_offsets || !reference || (n_reads > 0 && (!bases || !quals || !cigars || !ref_starts ||
        !ref_ends || !mapq || !flags || !name_hash)) || (n_targets > 0 && (!target_starts || !target_stops)))
        return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (n_reads < 0 || n_targets < 0 || reference_length < 0) return set_last_error(HELLO_ERR_ARG, "negative count");
    hello_qc* h = *handle;
    if (h && h->finished) return set_last_error(HELLO_ERR_ARG, "reads cannot be added after hello_qc_finish");
    if (h && device != h->device) return set_last_error(HELLO_ERR_ARG, "a further call names another device than the first");
    check_span(lo, hi, reference_length, h ? h->last_hi : 0);
    if (window < 1) return set_last_error(HELLO_ERR_ARG, "window %lld: at least 1", (long long)window);
    for (int64_t i = 0; i < n_targets; ++i)
        if (target_starts[i] < 0 || target_starts[i] >= target_stops[i] || (i > 0 && target_starts[i] < target_stops[i - 1]))
            return set_last_error(HELLO_ERR_ARG, "target %lld: [%lld, %lld) is empty, or not sorted behind its predecessor",
                                  (long long)i, (long long)target_starts[i], (long long)target_stops[i]);
    if (h && (reference_length != h->reference_length || window != h->window || mapq_threshold != h->mapq_threshold ||
              n_targets != (int64_t)h->target_starts.size() || !std::equal(h->target_starts.begin(), h->target_starts.end(), target_starts) ||
              !std::equal(h->target_stops.begin(), h->target_stops.end(), target_stops)))
        return set_last_error(HELLO_ERR_ARG, "reference length, targets, window or mapq threshold differ from the first call's");

    // ---- the reads: validated (cigar.h), then the reads kernel's list and chunks and the depth kernel's list
    const ReadsView in{bases, quals, read_offsets, cigars, cigar_offsets, ref_starts, ref_ends, mapq, flags, name_hash, n_reads};
    const std::vector<uint8_t> kind = qc_walk(in, lo, mapq_threshold);
    std::vector<int64_t> list, chunk{0}, d_list, d_end, d_start, d_max_end;
    std::vector<uint64_t> p_name;
    std::vector<uint16_t> p_flags;
    std::vector<int64_t> p_start, p_end;
    int64_t n_measured = 0, n_counted = 0, chunk_bases = 0, ref_hi = hi;
    for (int64_t r = 0; r < n_reads; ++r) {
        const uint8_t k = kind[(size_t)r];
        if ((k & kQcCounted) && ref_ends[r] > lo && ref_starts[r] < hi) {
            d_list.push_back(r);
            d_end.push_back(ref_ends[r]);
            d_start.push_back(ref_starts[r]);
            d_max_end.push_back(d_max_end.empty() ? ref_ends[r] : std::max(d_max_end.back(), ref_ends[r]));
        }
        if (!(k & kQcBelongs)) continue;
        n_counted += (k & kQcCounted) ? 1 : 0;
        const int64_t n_bases = (k & kQcMeasured) ? read_offsets[r + 1] - read_offsets[r] : 0;
        // a chunk ends at kQcChunkReads reads, or before its bases pass 2^31 / 255: the bound on a workgroup's int32 sums
        if ((int64_t)list.size() - chunk.back() >= kQcChunkReads || chunk_bases + n_bases > kQcMaxReadBases) {
            chunk.push_back((int64_t)list.size());
            chunk_bases = 0;
        }
        chunk_bases += n_bases;
        list.push_back(r);
        if (k & kQcMeasured) {
            ++n_measured;
            ref_hi = std::max(ref_hi, std::min(ref_ends[r], reference_length));
            p_name.push_back(name_hash[r]);
            p_flags.push_back(flags[r]);
            p_start.push_back(ref_starts[r]);
            p_end.push_back(ref_ends[r]);
        }
    }
    chunk.push_back((int64_t)list.size());
    const int64_t n_chunks = list.empty() ? 0 : (int64_t)chunk.size() - 1;
    if ((h ? (int64_t)h->name.size() : 0) + n_measured > kPairMaxReads)
        return set_last_error(HELLO_ERR_ARG, "more than %lld measured reads in one handle", (long long)kPairMaxReads);

    // ---- tiles: the contiguous range from the first read whose running-max end exceeds the tile's low edge to the last read
    // that starts below its high edge (as hello_refblocks_find plans them), and the targets that touch the tile
    const int64_t span = hi - lo, n_tiles = (span + kQcTile - 1) / kQcTile;
    if (n_tiles > INT32_MAX || n_chunks > INT32_MAX) return set_last_error(HELLO_ERR_ARG, "span of %lld positions", (long long)span);
    std::vector<int64_t> tile_reads((size_t)n_tiles * 2), tile_targets((size_t)n_tiles * 2);
    for (int64_t t = 0; t < n_tiles; ++t) {
        const int64_t tl = lo + t * kQcTile, th = std::min(tl + kQcTile, hi);
        const int64_t b = std::upper_bound(d_max_end.begin(), d_max_end.end(), tl) - d_max_end.begin();
        const int64_t e = std::lower_bound(d_start.begin(), d_start.end(), th) - d_start.begin();
        tile_reads[2 * t] = b;
        tile_reads[2 * t + 1] = std::max(b, e);
        const int64_t tb = std::upper_bound(target_stops, target_stops + n_targets, tl) - target_stops;
        const int64_t te = std::lower_bound(target_starts, target_starts + n_targets, th) - target_starts;
        tile_targets[2 * t] = tb;
        tile_targets[2 * t + 1] = std::max(tb, te);                        // each has a position in the tile: at most kQcTile
    }
    const int64_t n_windows = (reference_length + window - 1) / window;

    std::unique_ptr<hello_qc> own;
    if (!h) {
        open_device(device);
        own.reset(new hello_qc());
        h = own.get();
    } else {
        HS_HIP(hipSetDevice(h->device));
    }

    // ---- the device: tables of this call alone, added into the handle's once everything has come back
    DevMem m;
    const DeviceReads d = upload_reads(m, in);
    const uint8_t* d_ref = m.put(reference + lo, (size_t)(ref_hi - lo));
    float reads_ms = 0.0f, depth_ms = 0.0f;
    KernelTimer timer;
    unsigned long long* table = m.zeros<unsigned long long>(kQcTableInts);
    if (n_chunks > 0) {
        QcReadsArgs a{};
        a.bases = d.bases; a.quals = d.quals; a.read_off = d.read_off; a.cigars = d.cigars; a.cigar_off = d.cigar_off;
        a.ref_start = d.ref_start;
        a.flags = m.put(flags, (size_t)n_reads);
        a.mapq = m.put(mapq, (size_t)n_reads);
        a.list = m.put(list.data(), list.size());
        a.chunk = m.put(chunk.data(), chunk.size());
        a.ref = d_ref;
        a.ref_lo = lo;
        a.ref_length = reference_length;
        a.table = table;
        timer.start();
        hipLaunchKernelGGL(qc_reads_kernel, dim3((unsigned)n_chunks), dim3(kQcThreads), 0, 0, a);
        reads_ms = timer.stop();
    }
    QcDepthArgs g{};
    g.cigars = d.cigars; g.cigar_off = d.cigar_off; g.ref_start = d.ref_start;
    g.list = m.put(d_list.data(), d_list.size());
    g.list_end = m.put(d_end.data(), d_end.size());
    g.tile_reads = m.put(tile_reads.data(), tile_reads.size());
    g.tile_targets = m.put(tile_targets.data(), tile_targets.size());
    g.t_start = m.put(target_starts, (size_t)n_targets);
    g.t_stop = m.put(target_stops, (size_t)n_targets);
    g.ref = d_ref;
    g.lo = lo; g.hi = hi; g.window = window;
    g.hist = m.zeros<unsigned long long>(HELLO_QC_DEPTHS);
    g.t_hist = m.zeros<unsigned long long>(HELLO_QC_DEPTHS);
    g.w_sum = m.zeros<unsigned long long>((size_t)n_windows);
    g.t_sum = m.zeros<unsigned long long>((size_t)n_targets);
    g.t_cov = m.zeros<unsigned long long>((size_t)n_targets);
    g.excluded = m.zeros<unsigned long long>(1);
    timer.start();
    hipLaunchKernelGGL(qc_depth_kernel, dim3((unsigned)n_tiles), dim3(kQcThreads), 0, 0, g);
    depth_ms = timer.stop();
    const std::vector<int64_t> got_reads = fetch_table(table, kQcTableInts), got_hist = fetch_table(g.hist, HELLO_QC_DEPTHS),
                               got_t_hist = fetch_table(g.t_hist, HELLO_QC_DEPTHS), got_w = fetch_table(g.w_sum, (size_t)n_windows),
                               got_t_sum = fetch_table(g.t_sum, (size_t)n_targets), got_t_cov = fetch_table(g.t_cov, (size_t)n_targets),
                               got_excluded = fetch_table(g.excluded, 1);

    // ---- nothing can fail from here on
    if (own) {
        h->device = device;
        h->reference_length = reference_length;
        h->window = window;
        h->mapq_threshold = mapq_threshold;
        h->target_starts.assign(target_starts, target_starts + n_targets);
        h->target_stops.assign(target_stops, target_stops + n_targets);
        h->reads_table.assign(kQcTableInts, 0);
        h->depth_hist.assign(HELLO_QC_DEPTHS, 0);
        h->target_hist.assign(HELLO_QC_DEPTHS, 0);
        h->window_sum.assign((size_t)n_windows, 0);
        h->target_sum.assign((size_t)n_targets, 0);
        h->target_covered.assign((size_t)n_targets, 0);
    }
    add_into(h->reads_table, got_reads);
    add_into(h->depth_hist, got_hist);
    add_into(h->target_hist, got_t_hist);
    add_into(h->window_sum, got_w);
    add_into(h->target_sum, got_t_sum);
    add_into(h->target_covered, got_t_cov);
    h->name.insert(h->name.end(), p_name.begin(), p_name.end());
    h->flags.insert(h->flags.end(), p_flags.begin(), p_flags.end());
    h->start.insert(h->start.end(), p_start.begin(), p_start.end());
    h->end.insert(h->end.end(), p_end.begin(), p_end.end());
    h->last_hi = hi;
    h->stats[0] += (double)n_reads;
    h->stats[1] += (double)list.size();
    h->stats[2] += (double)n_measured;
    h->stats[3] += (double)n_counted;
    h->stats[4] = (double)h->reads_table[kQcFlags + HELLO_QC_FLAG_FIELDS];
    h->stats[5] += (double)got_excluded[0];
    h->stats[8] += reads_ms;
    h->stats[9] += depth_ms;
    if (own) *handle = own.release();
    return HELLO_OK;
} HS_ENTRY_END("hello_qc_add")

int hello_qc_finish(hello_qc* h) try {
    using namespace hello;
    if (!h) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (h->finished) return set_last_error(HELLO_ERR_ARG, "hello_qc_finish is called once, after the last hello_qc_add");
    const int64_t n = (int64_t)h->name.size();
    std::vector<int64_t> insert(3 * HELLO_QC_INSERTS, 0);
    int32_t joined[2] = {0, 0};
    float pair_ms = 0.0f, insert_ms = 0.0f;
    if (n > 0) {
        HS_HIP(hipSetDevice(h->device));
        DevMem m;
        const uint64_t* name = m.put(h->name.data(), (size_t)n);
        QcInsertArgs a{};
        a.flags = m.put(h->flags.data(), (size_t)n);
        a.start = m.put(h->start.data(), (size_t)n);
        a.end = m.put(h->end.data(), (size_t)n);
        int32_t* mate = m.room<int32_t>((size_t)n);
        pair_ms = pair_join(m, name, a.flags, m.zeros<uint8_t>((size_t)n), n, mate, joined);
        a.mate = mate;
        a.n = n;
        a.table = m.zeros<unsigned long long>(3 * HELLO_QC_INSERTS);
        KernelTimer timer;
        timer.start();
        hipLaunchKernelGGL(qc_insert_kernel, dim3(std::min(blocks_for(n, kQcThreads), 256u)), dim3(kQcThreads), 0, 0, a);
        insert_ms = timer.stop();
        insert = fetch_table(a.table, insert.size());
    }
    h->insert = std::move(insert);
    h->stats[6] = (double)joined[0];
    h->stats[7] = (double)joined[1];
    h->stats[10] = pair_ms;
    h->stats[11] = insert_ms;
    h->finished = true;
    return HELLO_OK;
} HS_ENTRY_END("hello_qc_finish")

int hello_qc_array(const hello_qc* h, int32_t which, const void** data, int64_t* count) {
    using namespace hello;
    if (!h || !data || !count) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    const int64_t* t = h->reads_table.data();
    switch (which) {
        case HELLO_QC_FLAGS: *data = t + kQcFlags; *count = HELLO_QC_FLAG_FIELDS; break;
        case HELLO_QC_MAPQ: *data = t + kQcMapq; *count = 256; break;
        case HELLO_QC_LENGTH: *data = t + kQcLength; *count = HELLO_QC_LENGTHS; break;
        case HELLO_QC_CYCLE: *data = t + kQcCycle; *count = 2 * HELLO_QC_CYCLES * HELLO_QC_CYCLE_FIELDS; break;
        case HELLO_QC_QUALITY: *data = t + kQcQuality; *count = 256 * 2; break;
        case HELLO_QC_DEPTH_HIST: *data = h->depth_hist.data(); *count = (int64_t)h->depth_hist.size(); break;
        case HELLO_QC_WINDOW_SUM: *data = h->window_sum.data(); *count = (int64_t)h->window_sum.size(); break;
        case HELLO_QC_TARGET_DEPTH_HIST: *data = h->target_hist.data(); *count = (int64_t)h->target_hist.size(); break;
        case HELLO_QC_TARGET_SUM: *data = h->target_sum.data(); *count = (int64_t)h->target_sum.size(); break;
        case HELLO_QC_TARGET_COVERED: *data = h->target_covered.data(); *count = (int64_t)h->target_covered.size(); break;
        case HELLO_QC_INSERT:
            if (!h->finished) return set_last_error(HELLO_ERR_ARG, "the insert sizes exist after hello_qc_finish");
            *data = h->insert.data(); *count = (int64_t)h->insert.size(); break;
        default: return set_last_error(HELLO_ERR_ARG, "array selector %d", which);
    }
    return HELLO_OK;
}

int hello_qc_stats(const hello_qc* h, double* stats) {
    if (!h || !stats) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    std::copy(h->stats, h->stats + HELLO_QC_STATS, stats);
    return HELLO_OK;
}

void hello_qc_free(hello_qc* h) { delete h; }

}  // extern "C"
