// Large deletions and insertions from the reads' own CIGARs (include/hello_mi355x.h: hello_sv_*): the chromosome's text and, span
// after span, its reads -> signatures (one per I or D operation of at least min_size bases, left-aligned against the reference),
// clusters of them and a genotype per cluster.  Not in the reference; DESIGN.md section 7p states the rules and hello_amd/sv.py
// restates them in Python, integer for integer.
//
// Host: the classes of the reads, the validation of every counted read and the walk list (cigar.h: sv_walk) -- the kernels index
// with it -- and at finish the clusters and genotypes (sv.h).
// Device, per hello_sv_add two kernels:
//   cover: a lane per counting, belonging read adds +1 and -1 to the difference array of the spanning depth.
//   reads: a wave per read of the walk list, the workgroup's waves sharing its reads.  The lanes sit on 64 operations per step
//     (read_walk.h: the decoder); two inclusive scans by shuffles turn the operations' advances into the reference and the query
//     cursor of every lane, their totals carrying into the next step.  A ballot marks the signatures; for each, in a wave-uniform
//     loop, the whole wave tests cond(j) of the move to the left 64 at a time, and the first failing lane ends it.  Lane 0 takes a
//     slot of the output with one returning atomicAdd: there are as many slots as sv_walk counted operations.
//   split (hello_sv_add_split alone): a wave per counting read with an SA tag.  A ballot of ';' hands the
//     tag's entries to lanes 1 .. 7, which parse them (sv_split.h: parse_sa_entry); the wave sums the primary's CIGAR into lane 0's
//     segment; shuffles rank the segments along the read, a lane per pair of neighbours classifies the junction (sv_junction), and
//     each DEL moves to the left with the loop the reads kernel uses (sv_wave_left_shift).  Lane 0 takes the rows' slots with one
//     returning atomicAdd: the host counted at most 7 per read.  Status and junction counts go to per-read arrays.
//   pairs (hello_sv_add_pairs alone): a lane per read.  The host has marked the pair-counted reads with valid
//     mate fields and the reads whose clips count; sv_pair_classify (sv_pairs.h) turns own and mate fields into an outcome.  The
//     workgroup counts the inner distances in 4 096 LDS counters and flushes the non-zero ones to the 64-bit histogram once; a
//     ballot of "emits a row" and one returning atomicAdd per wave hand out the rows' slots; the clips add to two int32 arrays.
// and at hello_sv_finish two more:
//   tile: a workgroup per 1 024 positions sums the difference array into a 64-bit sum; the host scans the sums.
//   span: a wave per candidate adds its tile's prefix to the lanes' sum of diff[tile start .. pos].
//   clips (with pairs): a wave per candidate sums the two clip arrays over the windows around its two ends.
// The cover is an integer sum and the signatures are sorted by the host before anyone sees them: two runs give the same bytes.
#include <memory>

#include "read_walk.h"
#include "stage_host.h"
#include "sv.h"
#include "sv_pairs.h"
#include "sv_split.h"

namespace hello {
namespace {

constexpr int kSvThreads = 256;
constexpr int kSvWaves = kSvThreads / 64;
constexpr int kSvShare = 1024;               // the most walked reads of a workgroup
constexpr int kSvGroups = 4096;              // the share of a launch is sized for about so many workgroups (pileup.hip)
constexpr int kSvTile = 1024;
constexpr int64_t kSvMaxReads = INT32_MAX;   // counting reads of one handle: the difference array is 32-bit

struct SvCoverArgs {
    const int64_t* ref_start;
    const int64_t* ref_end;
    const int64_t* list;         // [n_list]: the belonging counted reads, in input order
    int64_t n_list, length;
    int flank;
    int* diff;                   // [length + 1]
};

// e = ref_end: it is s + rlen but for a read without a reference operation (s + 1), which is shorter than 2 flank either way.
__global__ __launch_bounds__(kSvThreads) void sv_cover_kernel(SvCoverArgs a) {
    const int64_t k = (int64_t)blockIdx.x * kSvThreads + threadIdx.x;
    if (k >= a.n_list) return;
    const int64_t r = a.list[k];
    const int64_t s = a.ref_start[r], e = a.ref_end[r];                   // 0 <= s < e: sv_walk
    const int64_t from = s + a.flank;
    if (e - s < 2 * (int64_t)a.flank || from >= a.length) return;
    const int64_t last = e - a.flank < a.length - 1 ? e - a.flank : a.length - 1;     // from <= last <= length - 1
    atomicAdd(a.diff + from, 1);
    atomicAdd(a.diff + last + 1, -1);
}

struct SvReadsArgs {
    const uint8_t* bases;
    const int64_t* read_off;
    const uint32_t* cigars;
    const int64_t* cigar_off;
    const int64_t* ref_start;
    const int64_t* ref_end;
    const uint16_t* flags;
    const uint8_t* hp;
    const int64_t* list;         // [n_list]: the walk list
    const int64_t* ordinal;      // [n_list]: the read's index among the handle's counting reads
    uint8_t* seen;               // [n_list], zeroed: 1 when the read gave a signature
    int64_t n_list;
    const uint8_t* ref;          // [length]
    int64_t length;
    int min_size, flank, share;
    SvSig* out;                  // [capacity]
    unsigned long long* cursor;  // zeroed: the slots taken
    unsigned long long capacity;
};

__device__ __forceinline__ long long sv_scan(long long v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const long long up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

// The move to the left of an event of n bases at reference position sp (an insertion's bases begin at bases[sq]), by the whole wave:
// the greatest k with cond(j) for all j < k, over j < bound only.  cond(j) is tested 64 at a time and the first failing lane ends
// it.  The caller's bounds: sp - bound >= 0 keeps every index at or above 0, and sp + n <= length (a deletion) or sp <= length
// (an insertion, with sq + n inside the read's bases) keeps it below length.
__device__ __forceinline__ long long sv_wave_left_shift(const uint8_t* ref, const uint8_t* bases, long long sp, long long sq, long long n,
                                                        bool ins, long long bound, int lane) {
    for (long long j0 = 0;; j0 += 64) {
        const long long j = j0 + lane;
        bool holds = false;
        if (j < bound) {
            const int left = ref[sp - 1 - j] & 0xDF;
            const int right = ins && j < n ? bases[sq + n - 1 - j] : ref[sp - 1 - j + n];
            holds = left == (right & 0xDF);
        }
        const unsigned long long all = __ballot(holds);
        if (all != ~0ull) return j0 + (__ffsll((long long)~all) - 1);     // the lane at j = bound fails at the latest
    }
}

__global__ __launch_bounds__(kSvThreads) void sv_reads_kernel(SvReadsArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t k_lo = (int64_t)blockIdx.x * a.share;
    const int64_t k_hi = k_lo + a.share < a.n_list ? k_lo + a.share : a.n_list;
    for (int64_t k = k_lo + wave; k < k_hi; k += kSvWaves) {
        const int64_t r = a.list[k];
        const int64_t s = a.ref_start[r], e = a.ref_end[r];               // a walked read has a D or an aligned base: e = s + rlen
        const uint8_t* bases = a.bases + a.read_off[r];
        const int64_t c0 = a.cigar_off[r], n_ops = a.cigar_off[r + 1] - c0;
        long long rf = s, rd = 0;
        bool any = false;
        for (int64_t i0 = 0; i0 < n_ops; i0 += 64) {
            const int64_t i = i0 + lane;
            const CigarOp o = i < n_ops ? decode_op(a.cigars[c0 + i]) : CigarOp{BAM_CPAD, 0, false};
            const long long on_ref = o.m || o.op == BAM_CDEL || o.op == BAM_CREF_SKIP ? o.n : 0;
            const long long on_read = o.on_read() ? o.n : 0;
            const long long ref_sum = sv_scan(on_ref, lane), read_sum = sv_scan(on_read, lane);
            const long long p = rf + ref_sum - on_ref, q = rd + read_sum - on_read;     // where the lane's operation begins
            rf += __shfl(ref_sum, 63, 64);
            rd += __shfl(read_sum, 63, 64);
            const bool event = (o.op == BAM_CINS || o.op == BAM_CDEL) && o.n >= a.min_size;
            const long long pe = o.op == BAM_CDEL ? p + o.n : p;
            const bool is_signature = event && p - s >= a.flank && e - pe >= a.flank && pe <= a.length;
            unsigned long long todo = __ballot(is_signature);
            any = any || todo != 0ull;
            while (todo) {                                                // wave-uniform
                const int src = __ffsll((long long)todo) - 1;
                todo &= todo - 1ull;
                const long long sp = __shfl(p, src, 64), sq = __shfl(q, src, 64);
                const int n = __shfl(o.n, src, 64);
                const bool ins = __shfl(o.op, src, 64) == BAM_CINS;
                // the move to the left: j < sp - s keeps every index at or above s >= 0; sp <= pe <= length keeps it below length
                const long long shift = sv_wave_left_shift(a.ref, bases, sp, sq, n, ins, sp - s, lane);
                if (lane == 0) {
                    const unsigned long long slot = atomicAdd(a.cursor, 1ull);
                    if (slot < a.capacity) {                              // always: sv_walk counted the operations
                        SvSig g;
                        g.pos = sp - shift;
                        g.ordinal = a.ordinal[k];
                        g.op_index = i0 + src;
                        g.len = n;
                        g.shift = (int32_t)shift;                         // shift <= pos < 2^31
                        g.type = ins ? kSvIns : kSvDel;
                        g.strand = (a.flags[r] & 0x10) ? 1 : 0;
                        g.hp = a.hp[r];
                        g.pad = 0;
                        a.out[slot] = g;
                    }
                }
            }
        }
        if (lane == 0 && any) a.seen[k] = 1;
    }
}

struct SvSplitArgs {
    const uint32_t* cigars;
    const int64_t* cigar_off;
    const int64_t* ref_start;
    const uint8_t* mapq;
    const uint16_t* flags;
    const uint8_t* hp;
    const uint8_t* sa;           // the SA texts of the reads
    const int64_t* sa_off;       // [n_reads + 1]: validated by the host, monotone and inside `sa`
    const int64_t* list;         // [n_list]: the split list, the counting, belonging reads with a tag
    const int64_t* ordinal;      // [n_list]
    int64_t n_list;
    const uint64_t* contigs;     // [n_contigs]: FNV-1a of the names, all different
    int n_contigs, own;
    const uint8_t* ref;          // [length]
    int64_t length;
    int min_size, flank, mapq_threshold, share;
    uint8_t* status;             // [n_list]: kSplitParsed .. kSplitTooMany
    uint32_t* counts;            // [n_list]: junctions | dropped << 8 | small << 16 | unplaced << 24, each at most 7
    SvSig* out;                  // [capacity]
    unsigned long long* cursor;  // zeroed: the slots taken
    unsigned long long capacity;
};

__device__ __forceinline__ long long sv_wave_sum(long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// The segment lane `src` holds (every lane may name another one).
__device__ __forceinline__ SvSegment sv_shfl_segment(const SvSegment& g, int src) {
    SvSegment o;
    o.s = __shfl((long long)g.s, src, 64);
    o.e = __shfl((long long)g.e, src, 64);
    o.a = __shfl((long long)g.a, src, 64);
    o.m = __shfl((long long)g.m, src, 64);
    o.b = __shfl((long long)g.b, src, 64);
    o.qs = __shfl((long long)g.qs, src, 64);
    o.qe = __shfl((long long)g.qe, src, 64);
    o.hash = 0;
    o.tid = __shfl(g.tid, src, 64);
    o.mapq = __shfl(g.mapq, src, 64);
    o.strand = __shfl(g.strand, src, 64);
    o.ok = 1;
    return o;
}

// A wave per read of the split list.  Lane 0 holds the primary's segment, lanes 1 .. n the entries of the
// tag in their order.  Every byte index lies inside the tag's own [t0, t1); every reference index is sv_wave_left_shift's, whose
// bounds sv_junction guarantees: an own segment lies inside [0, length], a DEL's pos - bound is its left segment's start and its
// pos + len the other breakpoint.
__global__ __launch_bounds__(kSvThreads) void sv_split_kernel(SvSplitArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t k_lo = (int64_t)blockIdx.x * a.share;
    const int64_t k_hi = k_lo + a.share < a.n_list ? k_lo + a.share : a.n_list;
    for (int64_t k = k_lo + wave; k < k_hi; k += kSvWaves) {
        const int64_t r = a.list[k];
        const int64_t t0 = a.sa_off[r], t1 = a.sa_off[r + 1];             // t0 < t1: the host lists reads with a tag
        // ---- the entries' extents: a ballot of ';' per 64 bytes, the count carrying across the steps
        int n_semi = 0;
        long long my_begin = t0, my_end = t0, next_begin = t0, last_semi = -1;
        for (int64_t i0 = t0; i0 < t1; i0 += 64) {
            const int64_t i = i0 + lane;
            unsigned long long mask = __ballot(i < t1 && a.sa[i] == ';');
            while (mask && n_semi < kMaxSegments - 1) {                   // wave-uniform
                const long long at = i0 + (__ffsll((long long)mask) - 1);
                mask &= mask - 1ull;
                if (lane == n_semi + 1) { my_begin = next_begin; my_end = at; }
                next_begin = at + 1;
                last_semi = at;
                ++n_semi;
            }
            if (mask) {                                                   // an eighth entry: only counted
                n_semi += __popcll(mask);
                last_semi = i0 + 63 - __clzll((long long)mask);
            }
        }
        if (n_semi > kMaxSegments - 1 || n_semi == 0 || last_semi != t1 - 1) {
            if (lane == 0) {
                a.status[k] = n_semi > kMaxSegments - 1 ? kSplitTooMany : kSplitBadSa;
                a.counts[k] = 0u;
            }
            continue;
        }
        const int n_seg = n_semi + 1;
        // ---- the segments: lanes 1 .. n parse an entry each; the wave sums the primary's CIGAR and lane 0 takes its clips
        SvSegment g{};
        g.ok = 1;
        g.tid = -1;
        if (lane >= 1 && lane < n_seg) g = parse_sa_entry(a.sa, my_begin, my_end);
        const int64_t c0 = a.cigar_off[r], n_ops = a.cigar_off[r + 1] - c0;
        long long pm = 0, pr = 0, clipped = 0;
        for (int64_t i = lane; i < n_ops; i += 64) {
            const uint32_t c = a.cigars[c0 + i];
            const int op = c & 15;
            const long long n = c >> 4;
            if (op == BAM_CMATCH || op == BAM_CEQUAL || op == BAM_CDIFF) { pm += n; pr += n; }
            else if (op == BAM_CINS) pm += n;
            else if (op == BAM_CDEL || op == BAM_CREF_SKIP) pr += n;
            else if (op == BAM_CSOFT_CLIP || op == BAM_CHARD_CLIP) clipped += n;
        }
        pm = sv_wave_sum(pm);
        pr = sv_wave_sum(pr);
        clipped = sv_wave_sum(clipped);
        if (lane == 0) {
            int64_t i = 0, j = n_ops;
            long long lead = 0, trail = 0;
            for (; i < n_ops; ++i) {
                const uint32_t c = a.cigars[c0 + i];
                if ((c & 15) != BAM_CSOFT_CLIP && (c & 15) != BAM_CHARD_CLIP) break;
                lead += c >> 4;
            }
            for (; j > i; --j) {
                const uint32_t c = a.cigars[c0 + j - 1];
                if ((c & 15) != BAM_CSOFT_CLIP && (c & 15) != BAM_CHARD_CLIP) break;
                trail += c >> 4;
            }
            g.s = a.ref_start[r];
            g.e = g.s + pr;
            g.a = lead;
            g.m = pm;
            g.b = trail;
            g.tid = a.own;
            g.mapq = a.mapq[r];
            g.strand = (a.flags[r] & 0x10) ? 1 : 0;
            sv_orient(g);
            g.ok = pm >= 1 && pr >= 1 && lead + trail == clipped && g.e <= a.length;
        }
        const long long L = __shfl((long long)(g.a + g.m + g.b), 0, 64);
        if (lane >= 1 && lane < n_seg && g.a + g.m + g.b != L) g.ok = 0;
        for (int e = 1; e < n_seg; ++e) {                                 // the contig of every entry: the lanes on the table
            const unsigned long long h = __shfl((unsigned long long)g.hash, e, 64);
            int tid = -1;
            for (int c1 = 0; c1 < a.n_contigs && tid < 0; c1 += 64) {
                const int c = c1 + lane;
                const unsigned long long hit = __ballot(c < a.n_contigs && a.contigs[c] == h);
                if (hit) tid = c1 + (__ffsll((long long)hit) - 1);
            }
            if (lane == e) g.tid = tid;
        }
        if (lane >= 1 && lane < n_seg && g.tid == a.own && g.e > a.length) g.ok = 0;
        if (__ballot(lane < n_seg && !g.ok)) {
            if (lane == 0) {
                a.status[k] = kSplitBadSa;
                a.counts[k] = 0u;
            }
            continue;
        }
        // ---- the ranks by (qs, qe, lane): at most 8 segments, all against all
        int rank = 0;
        for (int j = 0; j < n_seg; ++j) {
            const long long qs = __shfl((long long)g.qs, j, 64), qe = __shfl((long long)g.qe, j, 64);
            const bool before = qs != g.qs ? qs < g.qs : qe != g.qe ? qe < g.qe : j < lane;
            rank += j != lane && before;
        }
        int holder = 0;                                                   // lane k: the lane whose segment has rank k
        for (int j = 0; j < n_seg; ++j)
            if (__shfl(rank, j, 64) == lane) holder = j;
        const int next = __shfl_down(holder, 1, 64);
        const bool mine = lane < n_seg - 1;                               // a lane per pair of neighbours
        const SvSegment A = sv_shfl_segment(g, mine ? holder : 0), B = sv_shfl_segment(g, mine ? next : 0);
        SvJunction j{};
        if (mine) j = sv_junction(A, B, a.own, a.length, a.min_size, a.flank, a.mapq_threshold);
        // ---- the move to the left of every deletion without bases between its segments
        long long moved = 0;
        unsigned long long todo = __ballot(mine && j.outcome == kJunctionRow && j.bound > 0);
        while (todo) {                                                    // wave-uniform
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const long long sp = __shfl((long long)j.pos, src, 64), n = __shfl((long long)j.len, src, 64);
            const long long bound = __shfl((long long)j.bound, src, 64);
            const long long shift = sv_wave_left_shift(a.ref, nullptr, sp, 0, n, false, bound, lane);
            if (lane == src) moved = shift;
        }
        // ---- the rows: lane 0 takes the slots of all of them at once
        const bool is_row = mine && j.outcome == kJunctionRow;
        const unsigned long long rows = __ballot(is_row);
        unsigned long long base = 0;
        if (lane == 0 && rows) base = atomicAdd(a.cursor, (unsigned long long)__popcll(rows));
        base = __shfl(base, 0, 64);
        const unsigned long long slot = base + (unsigned long long)__popcll(rows & ((1ull << lane) - 1ull));
        if (is_row && slot < a.capacity) {                                // always: the host counted the ';' of the tags
            SvSig o;
            o.pos = j.pos - moved;
            o.ordinal = a.ordinal[k];
            o.op_index = -(int64_t)(lane + 1);
            o.len = (int32_t)j.len;
            o.shift = j.type == kSvBnd ? (int32_t)j.shift : (int32_t)moved;
            o.type = (uint8_t)j.type;
            o.strand = (a.flags[r] & 0x10) ? 1 : 0;
            o.hp = a.hp[r];
            o.pad = 0;
            a.out[slot] = o;
        }
        const unsigned n_dropped = (unsigned)__popcll(__ballot(mine && j.outcome == kJunctionDropped));
        const unsigned n_small = (unsigned)__popcll(__ballot(mine && j.outcome == kJunctionSmall));
        const unsigned n_unplaced = (unsigned)__popcll(__ballot(mine && j.outcome == kJunctionUnplaced));
        if (lane == 0) {
            a.status[k] = rows ? kSplitRow : kSplitParsed;
            a.counts[k] = (unsigned)(n_seg - 1) | n_dropped << 8 | n_small << 16 | n_unplaced << 24;
        }
    }
}

struct SvPairsArgs {
    const uint32_t* cigars;
    const int64_t* cigar_off;
    const int64_t* ref_start;
    const int64_t* ref_end;
    const uint16_t* flags;
    const uint8_t* hp;
    const int32_t* mate_tid;
    const int64_t* mate_pos;
    const uint8_t* todo;         // [n_reads]: kPairClassify | kPairClips, by the host's checks
    int64_t n_reads, n_contigs;
    int own, min_size, clip_min;
    SvLibrary lib;
    unsigned long long* inner;   // [kInnerBins]
    int* clip_left;              // [length + 1]
    int* clip_right;             // [length + 1]
    uint8_t* status;             // [n_reads]: PAIR_STATUS | clips << 4
    SvSig* out;                  // [capacity]
    unsigned long long* cursor;  // zeroed: the slots taken
    unsigned long long capacity;
};

// A lane per read.  Every lane reaches both barriers.  The indices: a bin is clamped by sv_pair_classify;
// s and e of a kPairClips read lie inside [0, length] by the host's walk; a slot is below capacity by the guard.
__global__ __launch_bounds__(kSvThreads) void sv_pairs_kernel(SvPairsArgs a) {
    __shared__ int inner[kInnerBins];
    const int lane = threadIdx.x & 63;
    for (int b = threadIdx.x; b < kInnerBins; b += kSvThreads) inner[b] = 0;
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * kSvThreads + threadIdx.x;
    const uint8_t todo = r < a.n_reads ? a.todo[r] : 0;
    SvPairOutcome o;
    if (todo & kPairClassify) {
        o = sv_pair_classify(a.flags[r], a.ref_start[r], a.ref_end[r], a.own, a.mate_tid[r], a.mate_pos[r], a.n_contigs, a.lib, a.min_size);
        if (o.inner) atomicAdd(&inner[o.bin], 1);
    }
    int clips = 0;
    if (todo & kPairClips) {
        const int64_t c0 = a.cigar_off[r];
        clips = sv_clips(a.cigars + c0, a.cigar_off[r + 1] - c0, a.clip_min);
        if (clips & 1) atomicAdd(a.clip_right + a.ref_start[r], 1);
        if (clips & 2) atomicAdd(a.clip_left + a.ref_end[r], 1);
    }
    const bool is_row = o.status == kPairRow || o.status == kPairBndRow;
    const unsigned long long rows = __ballot(is_row);
    unsigned long long base = 0;
    if (lane == 0 && rows) base = atomicAdd(a.cursor, (unsigned long long)__popcll(rows));
    base = __shfl(base, 0, 64);
    const unsigned long long slot = base + (unsigned long long)__popcll(rows & ((1ull << lane) - 1ull));
    if (is_row && slot < a.capacity) {                                    // always: a slot per kPairClassify read
        SvSig g;
        g.pos = o.pos;
        g.ordinal = r;                                                    // the read: the host puts its pair ordinal here
        g.op_index = kPairOp;
        g.len = (int32_t)o.len;
        g.shift = (int32_t)o.shift;
        g.type = (uint8_t)o.type;
        g.strand = (a.flags[r] & 0x10) ? 1 : 0;
        g.hp = a.hp[r];
        g.pad = 0;
        a.out[slot] = g;
    }
    if (r < a.n_reads) a.status[r] = (uint8_t)(o.status | clips << 4);
    __syncthreads();
    for (int b = threadIdx.x; b < kInnerBins; b += kSvThreads) {
        const int n = inner[b];
        if (n) atomicAdd(a.inner + b, (unsigned long long)n);
    }
}

struct SvSpanArgs {
    const int* diff;             // [length + 1]
    int64_t n_diff, n_tiles;
    long long* tile_sum;         // [n_tiles]; for the span kernel the sums before every tile
    const int64_t* pos;          // [n_candidates], each inside [0, length]
    int64_t n_candidates;
    long long* depth;            // [n_candidates]
};

__global__ __launch_bounds__(kSvThreads) void sv_tile_kernel(SvSpanArgs a) {
    __shared__ long long part[kSvWaves];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t t0 = (int64_t)blockIdx.x * kSvTile;
    long long sum = 0;
    for (int j = tid; j < kSvTile; j += kSvThreads)
        if (t0 + j < a.n_diff) sum += a.diff[t0 + j];
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
    if (lane == 0) part[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        long long total = 0;
        for (int w = 0; w < kSvWaves; ++w) total += part[w];
        a.tile_sum[blockIdx.x] = total;
    }
}

__global__ __launch_bounds__(kSvThreads) void sv_span_kernel(SvSpanArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * kSvWaves + wave;
    if (c >= a.n_candidates) return;                                      // the whole wave
    const int64_t pos = a.pos[c], tile = pos / kSvTile, t0 = tile * kSvTile;      // pos < n_diff
    long long sum = 0;
    for (int64_t j = t0 + lane; j <= pos; j += 64) sum += a.diff[j];
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
    if (lane == 0) a.depth[c] = a.tile_sum[tile] + sum;
}

struct SvClipArgs {
    const int* clip_left;        // [length + 1]
    const int* clip_right;
    const int64_t* pos;          // [n_candidates]
    const int64_t* end;
    int64_t n_candidates, length;
    int flank;
    long long* ce;               // [n_candidates]
};

__global__ __launch_bounds__(kSvThreads) void sv_clips_kernel(SvClipArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * kSvWaves + wave;
    if (c >= a.n_candidates) return;                                      // the whole wave
    const SvClipWindows w = sv_clip_windows(a.pos[c], a.end[c], a.flank, a.length);     // inside [0, length]
    long long sum = 0;
    for (int64_t j = w.lo1 + lane; j <= w.hi1; j += 64) sum += (long long)a.clip_left[j] + a.clip_right[j];
    for (int64_t j = w.lo2 + lane; j <= w.hi2; j += 64) sum += (long long)a.clip_left[j] + a.clip_right[j];
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
    if (lane == 0) a.ce[c] = sum;
}

constexpr int kSvSigColumns = 8, kSvCandColumns = 20;

}  // namespace
}  // namespace hello

struct hello_sv : hello::SpanHandle<HELLO_SV_STATS> {
    int32_t min_size = 0, flank = 0, mapq_threshold = 0;
    hello::DevMem mem;                           // the reference text and the difference array live as long as the handle
    const uint8_t* ref = nullptr;
    int* diff = nullptr;
    bool built = false, finished = false, sorted = true;
    std::vector<uint8_t> reference;              // until the device side is built
    std::vector<hello::SvSig> sigs;
    std::vector<int64_t> sig_cols[hello::kSvSigColumns], cand_cols[hello::kSvCandColumns], cand_sr;
    std::vector<uint64_t> contigs;               // hello_sv_contigs: FNV-1a of the names; empty until then
    int32_t own = -1;
    std::vector<uint8_t> split_status;           // of the last add, per read
    // ---- discordant pairs and clipped ends
    bool has_library = false, pairs_built = false;
    hello::SvLibrary library;
    int32_t clip_min = 20;
    int64_t pairs_given = 0;                     // the belonging pair-counted reads so far: the ordinal of the next
    int64_t pairs_given_adds = 0;                // the calls of hello_sv_add_pairs that passed
    unsigned long long* inner = nullptr;         // [kInnerBins]
    int* clip_left = nullptr;                    // [length + 1]
    int* clip_right = nullptr;
    std::vector<uint8_t> pair_status;            // of the last add, per read
    std::vector<int64_t> inner_host, cand_pairs[5];      // PR, CE, END_MIN, END_MAX, IMPRECISE
    std::vector<int32_t> clip_host[2];
    double pair_stats[hello::kPairStats] = {0};
};

extern "C" {

// The device side of a handle, built when the first hello_sv_add has passed its checks.
static void sv_build(hello_sv* h) {
    using namespace hello;
    if (h->built) return;
    open_device(h->device);
    DevMem keep;
    const uint8_t* ref = keep.put(h->reference.data(), h->reference.size());
    int* diff = keep.zeros<int>((size_t)h->length + 1);
    // ---- nothing can fail from here on
    h->mem.ptrs.swap(keep.ptrs);
    h->ref = ref;
    h->diff = diff;
    std::vector<uint8_t>().swap(h->reference);
    h->built = true;
}

// The device side of the pairs, built when the first hello_sv_add_pairs has passed its checks.
static void sv_build_pairs(hello_sv* h) {
    using namespace hello;
    if (h->pairs_built) return;
    DevMem keep;
    unsigned long long* inner = keep.zeros<unsigned long long>(kInnerBins);
    int* left = keep.zeros<int>((size_t)h->length + 1);
    int* right = keep.zeros<int>((size_t)h->length + 1);
    // ---- nothing can fail from here on
    h->mem.ptrs.insert(h->mem.ptrs.end(), keep.ptrs.begin(), keep.ptrs.end());
    keep.ptrs.clear();
    h->inner = inner;
    h->clip_left = left;
    h->clip_right = right;
    h->pairs_built = true;
}

// The SIGNATURES columns of the handle, in sv_sort's order.
static void sv_signature_columns(hello_sv* h) {
    using namespace hello;
    if (h->sorted) return;
    sv_sort(h->sigs);
    for (auto& c : h->sig_cols) c.resize(h->sigs.size());
    for (size_t i = 0; i < h->sigs.size(); ++i) {
        const SvSig& g = h->sigs[i];
        const int64_t row[kSvSigColumns] = {g.type, g.pos, g.len, g.shift, g.ordinal, g.op_index, g.strand, g.hp};
        for (int c = 0; c < kSvSigColumns; ++c) h->sig_cols[c][i] = row[c];
    }
    h->sorted = true;
}

int hello_sv_create(const uint8_t* reference, int64_t reference_length, int32_t min_size, int32_t flank, int32_t mapq_threshold,
                    int32_t device, hello_sv** handle) try {
    using namespace hello;
    if (!reference || !handle) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    *handle = nullptr;
    if (reference_length < 0 || reference_length > INT32_MAX)
        return set_last_error(HELLO_ERR_ARG, "reference of %lld bases: 0 to %d", (long long)reference_length, INT32_MAX);
    if (min_size < 1) return set_last_error(HELLO_ERR_ARG, "min_size %d: at least 1", min_size);
    if (flank < 1) return set_last_error(HELLO_ERR_ARG, "flank %d: at least 1", flank);
    std::unique_ptr<hello_sv> h(new hello_sv());
    h->device = device;
    h->min_size = min_size;
    h->flank = flank;
    h->mapq_threshold = mapq_threshold;
    h->length = reference_length;
    h->reference.assign(reference, reference + reference_length);
    *handle = h.release();
    return HELLO_OK;
} HS_ENTRY_END("hello_sv_create")

// hello_sv_add (sa_offsets == nullptr), hello_sv_add_split and hello_sv_add_pairs (mate_tid != nullptr): refusals are thrown.
static void sv_add(hello_sv* h, const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                   const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends, const uint8_t* mapq,
                   const uint16_t* flags, const uint64_t* name_hash, const uint8_t* hp, const uint8_t* sa_bytes,
                   const int64_t* sa_offsets, int64_t n_sa_bytes, int64_t n_reads, int64_t lo, int64_t hi,
                   const int32_t* mate_tid = nullptr, const int64_t* mate_pos = nullptr) {
    using namespace hello;
    const char* entry = mate_tid ? "hello_sv_add_pairs" : sa_offsets ? "hello_sv_add_split" : "hello_sv_add";
    if (!h || !read_offsets || !cigar_offsets || (n_reads > 0 && (!bases || !cigars || !ref_starts || !ref_ends || !mapq || !flags || !hp)))
        raise(HELLO_ERR_ARG, "NULL pointer");
    if (n_reads < 0) raise(HELLO_ERR_ARG, "negative count");
    if (h->finished) raise(HELLO_ERR_ARG, "%s after hello_sv_finish: the handle takes no more reads", entry);
    if (sa_offsets) {
        if (h->contigs.empty()) raise(HELLO_ERR_ARG, "%s before hello_sv_contigs: the handle knows no contig names", entry);
        if (n_sa_bytes < 0 || (n_sa_bytes > 0 && !sa_bytes)) raise(HELLO_ERR_ARG, "%lld SA bytes", (long long)n_sa_bytes);
        if (sa_offsets[0] < 0) raise(HELLO_ERR_ARG, "SA offsets begin at %lld", (long long)sa_offsets[0]);
        for (int64_t r = 0; r < n_reads; ++r)
            if (sa_offsets[r + 1] < sa_offsets[r]) raise(HELLO_ERR_ARG, "read %lld: SA offsets decrease", (long long)r);
        if (sa_offsets[n_reads] > n_sa_bytes)
            raise(HELLO_ERR_ARG, "SA offsets end at %lld, %lld SA bytes", (long long)sa_offsets[n_reads], (long long)n_sa_bytes);
    }
    if (mate_tid && !h->has_library)
        raise(HELLO_ERR_ARG, "hello_sv_add_pairs before hello_sv_library: the handle knows no insert sizes");
    h->check_span(lo, hi);

    // ---- the reads: validated, then the kernels' lists
    const ReadsView in{bases, quals, read_offsets, cigars, cigar_offsets, ref_starts, ref_ends, mapq, flags, name_hash, n_reads};
    const SvWalk walk = sv_walk(in, lo, h->mapq_threshold, h->min_size);
    std::vector<int64_t> list, ordinal, split_list, split_ordinal;
    std::vector<uint8_t> status((size_t)n_reads, 0), split_status((size_t)n_reads, kSplitNone);
    int64_t split_capacity = 0;                      // min(7, the ';' of the tag) per read of the split list: no more rows
    int64_t n_belonging = 0;
    size_t next = 0;
    for (int64_t r = 0; r < n_reads; ++r) {
        if (!(walk.kind[(size_t)r] & kPileBelongs)) continue;
        ++n_belonging;
        if (!(walk.kind[(size_t)r] & kPileCounted)) continue;
        if (next < walk.walk.size() && walk.walk[next] == r) {
            ordinal.push_back(h->counting_given + (int64_t)list.size());
            ++next;
        }
        if (sa_offsets && sa_offsets[r + 1] > sa_offsets[r]) {
            split_list.push_back(r);
            split_ordinal.push_back(h->counting_given + (int64_t)list.size());
            const int64_t n_semi = std::count(sa_bytes + sa_offsets[r], sa_bytes + sa_offsets[r + 1], (uint8_t)';');
            split_capacity += std::min<int64_t>(kMaxSegments - 1, n_semi);
        }
        status[(size_t)r] = 1;
        list.push_back(r);
    }
    const int64_t n_list = (int64_t)list.size(), n_walk = (int64_t)walk.walk.size(), n_split = (int64_t)split_list.size();
    h->take_counting(n_list, kSvMaxReads, "cover sums");
    // ---- the pairs: what the kernel may classify and whose clips count, by the host's checks alone (sv_pairs.h)
    SvPairMarks marks;
    if (mate_tid) marks = sv_pairs_mark(in, walk.kind, sa_offsets, mate_tid, mate_pos, h->own, h->length, h->mapq_threshold, h->pairs_given);
    std::vector<uint8_t>&pair_todo = marks.todo, &pair_state = marks.state;
    std::vector<int64_t>& pair_ordinal = marks.ordinal;
    const int64_t n_pair_reads = marks.n_pair_reads, n_bad_mate = marks.n_bad_mate, n_classify = marks.n_classify, n_pair_work = marks.n_work;
    // room for every row this add can give, so that no insert below the kernels can fail; grown by doubling
    const size_t need = h->sigs.size() + (size_t)walk.n_ops + (size_t)split_capacity + (size_t)n_classify;
    if (need > h->sigs.capacity()) h->sigs.reserve(std::max(need, 2 * h->sigs.capacity()));
    const int64_t share = std::min<int64_t>(kSvShare, std::max<int64_t>(kSvWaves, (n_walk + kSvGroups - 1) / kSvGroups));
    const int64_t n_blocks = (n_walk + share - 1) / share;

    sv_build(h);
    HS_HIP(hipSetDevice(h->device));
    if (mate_tid) sv_build_pairs(h);
    std::vector<SvSig> paired;
    float pairs_ms = 0.0f;
    std::vector<uint8_t> seen((size_t)n_walk, 0);
    std::vector<SvSig> found, joined;
    std::vector<uint8_t> split_state((size_t)n_split, 0);
    std::vector<uint32_t> split_counts((size_t)n_split, 0);
    float cover_ms = 0.0f, reads_ms = 0.0f, split_ms = 0.0f;
    // One copy of a per-read array on the device for all the kernels of this add: uploaded by the first that needs it.
    DevMem m;
    const int64_t *d_start = nullptr, *d_end = nullptr, *d_cigar_off = nullptr;
    const uint32_t* d_cigars = nullptr;
    const uint16_t* d_flags = nullptr;
    const uint8_t* d_hp = nullptr;
    auto shared = [&m](auto*& on_device, auto* host, size_t n) {
        if (!on_device) on_device = m.put(host, n);
        return on_device;
    };
    const size_t n_cigar_ops = (size_t)cigar_offsets[n_reads];
    if (n_list > 0) {
        shared(d_start, ref_starts, (size_t)n_reads);
        shared(d_end, ref_ends, (size_t)n_reads);
        SvReadsArgs a{};
        SvSig* got = nullptr;
        if (n_walk > 0) {                            // every upload before the first kernel: a failure leaves the cover as it was
            a.bases = m.put(bases, (size_t)read_offsets[n_reads]);
            a.read_off = m.put(read_offsets, (size_t)n_reads + 1);
            a.cigars = shared(d_cigars, cigars, n_cigar_ops);
            a.cigar_off = shared(d_cigar_off, cigar_offsets, (size_t)n_reads + 1);
            a.ref_start = d_start;
            a.ref_end = d_end;
            a.flags = shared(d_flags, flags, (size_t)n_reads);
            a.hp = shared(d_hp, hp, (size_t)n_reads);
            a.list = m.put(walk.walk.data(), walk.walk.size());
            a.ordinal = m.put(ordinal.data(), ordinal.size());
            a.seen = m.zeros<uint8_t>((size_t)n_walk);
            a.n_list = n_walk;
            a.ref = h->ref;
            a.length = h->length;
            a.min_size = h->min_size;
            a.flank = h->flank;
            a.share = (int)share;
            a.out = got = m.room<SvSig>((size_t)walk.n_ops);
            a.cursor = m.zeros<unsigned long long>(1);
            a.capacity = (unsigned long long)walk.n_ops;
        }
        KernelTimer timer;
        if (n_walk > 0) {                            // the reads first: a refusal here has not touched the cover
            timer.start();
            hipLaunchKernelGGL(sv_reads_kernel, dim3((unsigned)n_blocks), dim3(kSvThreads), 0, 0, a);
            reads_ms = timer.stop();
            unsigned long long taken = 0;
            HS_HIP(hipMemcpy(&taken, a.cursor, sizeof(taken), hipMemcpyDeviceToHost));
            if (taken > a.capacity) raise(HELLO_ERR_HIP, "%llu signatures for %llu counted operations", taken, a.capacity);
            found.resize((size_t)taken);
            if (taken) HS_HIP(hipMemcpy(found.data(), got, (size_t)taken * sizeof(SvSig), hipMemcpyDeviceToHost));
            HS_HIP(hipMemcpy(seen.data(), a.seen, (size_t)n_walk, hipMemcpyDeviceToHost));
        }
        if (n_split > 0) {                           // the split alignments: nothing of the handle is touched either
            SvSplitArgs p{};
            p.cigars = shared(d_cigars, cigars, n_cigar_ops);
            p.cigar_off = shared(d_cigar_off, cigar_offsets, (size_t)n_reads + 1);
            p.ref_start = d_start;
            p.mapq = m.put(mapq, (size_t)n_reads);
            p.flags = shared(d_flags, flags, (size_t)n_reads);
            p.hp = shared(d_hp, hp, (size_t)n_reads);
            p.sa = m.put(sa_bytes, (size_t)sa_offsets[n_reads]);
            p.sa_off = m.put(sa_offsets, (size_t)n_reads + 1);
            p.list = m.put(split_list.data(), split_list.size());
            p.ordinal = m.put(split_ordinal.data(), split_ordinal.size());
            p.n_list = n_split;
            p.contigs = m.put(h->contigs.data(), h->contigs.size());
            p.n_contigs = (int)h->contigs.size();
            p.own = h->own;
            p.ref = h->ref;
            p.length = h->length;
            p.min_size = h->min_size;
            p.flank = h->flank;
            p.mapq_threshold = h->mapq_threshold;
            const int64_t part = std::min<int64_t>(kSvShare, std::max<int64_t>(kSvWaves, (n_split + kSvGroups - 1) / kSvGroups));
            p.share = (int)part;
            p.status = m.zeros<uint8_t>((size_t)n_split);
            p.counts = m.zeros<uint32_t>((size_t)n_split);
            SvSig* rows = m.room<SvSig>((size_t)split_capacity);
            p.out = rows;
            p.cursor = m.zeros<unsigned long long>(1);
            p.capacity = (unsigned long long)split_capacity;
            timer.start();
            hipLaunchKernelGGL(sv_split_kernel, dim3((unsigned)((n_split + part - 1) / part)), dim3(kSvThreads), 0, 0, p);
            split_ms = timer.stop();
            unsigned long long taken = 0;
            HS_HIP(hipMemcpy(&taken, p.cursor, sizeof(taken), hipMemcpyDeviceToHost));
            if (taken > p.capacity) raise(HELLO_ERR_HIP, "%llu rows for %llu entries of the SA tags", taken, p.capacity);
            joined.resize((size_t)taken);
            if (taken) HS_HIP(hipMemcpy(joined.data(), rows, (size_t)taken * sizeof(SvSig), hipMemcpyDeviceToHost));
            HS_HIP(hipMemcpy(split_state.data(), p.status, (size_t)n_split, hipMemcpyDeviceToHost));
            HS_HIP(hipMemcpy(split_counts.data(), p.counts, (size_t)n_split * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
        SvCoverArgs c{d_start, d_end, m.put(list.data(), list.size()), n_list, h->length, h->flank, h->diff};
        timer.start();
        hipLaunchKernelGGL(sv_cover_kernel, dim3((unsigned)((n_list + kSvThreads - 1) / kSvThreads)), dim3(kSvThreads), 0, 0, c);
        cover_ms = timer.stop();
    }
    // The pairs come last, like the cover: only a failing HIP call can stop them, and the handle is of no use after one.
    if (n_pair_work > 0) {                           // a span without a paired or a clipped read launches nothing
        SvPairsArgs p{};                             // the reads' arrays are those the kernels above uploaded, where they did
        p.cigars = shared(d_cigars, cigars, n_cigar_ops);
        p.cigar_off = shared(d_cigar_off, cigar_offsets, (size_t)n_reads + 1);
        p.ref_start = shared(d_start, ref_starts, (size_t)n_reads);
        p.ref_end = shared(d_end, ref_ends, (size_t)n_reads);
        p.flags = shared(d_flags, flags, (size_t)n_reads);
        p.hp = shared(d_hp, hp, (size_t)n_reads);
        p.mate_tid = m.put(mate_tid, (size_t)n_reads);
        p.mate_pos = m.put(mate_pos, (size_t)n_reads);
        p.todo = m.put(pair_todo.data(), (size_t)n_reads);
        p.n_reads = n_reads;
        p.n_contigs = (int64_t)h->contigs.size();
        p.own = h->own;
        p.min_size = h->min_size;
        p.clip_min = h->clip_min;
        p.lib = h->library;
        p.inner = h->inner;
        p.clip_left = h->clip_left;
        p.clip_right = h->clip_right;
        p.status = m.zeros<uint8_t>((size_t)n_reads);
        SvSig* rows = m.room<SvSig>((size_t)n_classify);
        p.out = rows;
        p.cursor = m.zeros<unsigned long long>(1);
        p.capacity = (unsigned long long)n_classify;
        std::vector<uint8_t> state((size_t)n_reads);
        paired.reserve((size_t)n_classify);
        KernelTimer timer;
        timer.start();
        hipLaunchKernelGGL(sv_pairs_kernel, dim3((unsigned)((n_reads + kSvThreads - 1) / kSvThreads)), dim3(kSvThreads), 0, 0, p);
        pairs_ms = timer.stop();
        unsigned long long taken = 0;
        HS_HIP(hipMemcpy(&taken, p.cursor, sizeof(taken), hipMemcpyDeviceToHost));
        if (taken > p.capacity) raise(HELLO_ERR_HIP, "%llu pair rows for %llu pair-counted reads", taken, p.capacity);
        paired.resize((size_t)taken);
        if (taken) HS_HIP(hipMemcpy(paired.data(), rows, (size_t)taken * sizeof(SvSig), hipMemcpyDeviceToHost));
        for (SvSig& g : paired) {                    // the kernel names the read; its ordinal is the host's
            if (g.ordinal < 0 || g.ordinal >= n_reads) raise(HELLO_ERR_HIP, "a pair row of read %lld of %lld", (long long)g.ordinal, (long long)n_reads);
            g.ordinal = pair_ordinal[(size_t)g.ordinal];
        }
        HS_HIP(hipMemcpy(state.data(), p.status, (size_t)n_reads, hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < n_reads; ++r)
            if (pair_todo[(size_t)r] & kPairClassify) pair_state[(size_t)r] = state[(size_t)r];
            else if (pair_todo[(size_t)r]) pair_state[(size_t)r] |= state[(size_t)r] & 0xF0;        // a BAD_MATE read's clips still count
    }

    // ---- nothing can fail from here on
    int64_t n_seen = 0;
    for (int64_t k = 0; k < n_walk; ++k) {
        status[(size_t)walk.walk[(size_t)k]] = seen[(size_t)k] ? 3 : 2;
        n_seen += seen[(size_t)k] ? 1 : 0;
    }
    if (!found.empty() || !joined.empty() || !paired.empty()) {
        h->sigs.insert(h->sigs.end(), found.begin(), found.end());
        h->sigs.insert(h->sigs.end(), joined.begin(), joined.end());
        h->sigs.insert(h->sigs.end(), paired.begin(), paired.end());
        h->sorted = false;
    }
    if (mate_tid) {                                  // the statistics of the pairs: reduced here from the per-read outcomes
        double* st = h->pair_stats;
        for (int64_t r = 0; r < n_reads; ++r) {
            const uint8_t state = pair_state[(size_t)r] & 15;
            const bool same = state >= kPairNormal && state <= kPairRow && state != kPairUnplaced;
            st[1] += same;                           // pairs_left
            st[2] += state == kPairRight;
            st[3] += state == kPairNormal;
            st[4] += state == kPairShort;
            st[5] += state == kPairSmall;
            st[6] += state == kPairUnplaced;
            st[9] += (pair_state[(size_t)r] >> 4) != 0;     // clipped_reads
            pair_state[(size_t)r] = state;
        }
        st[0] += (double)n_pair_reads;
        st[7] += (double)n_bad_mate;
        st[8] += (double)paired.size();
        st[12] += pairs_ms;
        h->pairs_given += n_pair_reads;
        ++h->pairs_given_adds;
        h->pair_status = std::move(pair_state);
    } else {
        h->pair_status.assign((size_t)n_reads, kPairNone);
    }
    for (int64_t k = 0; k < n_split; ++k) {
        const uint32_t c = split_counts[(size_t)k];
        split_status[(size_t)split_list[(size_t)k]] = split_state[(size_t)k];
        h->stats[11] += split_state[(size_t)k] == kSplitBadSa;
        h->stats[12] += split_state[(size_t)k] == kSplitTooMany;
        h->stats[13] += (double)(c & 255u);
        h->stats[14] += (double)(c >> 8 & 255u);
        h->stats[15] += (double)(c >> 16 & 255u);
        h->stats[16] += (double)(c >> 24);
    }
    h->stats[10] += (double)n_split;
    h->stats[17] += (double)joined.size();
    h->stats[18] += split_ms;
    h->split_status = std::move(split_status);
    h->status = std::move(status);
    h->counting_given += n_list;
    h->last_hi = hi;
    h->stats[0] += (double)n_reads;
    h->stats[1] += (double)n_belonging;
    h->stats[2] += (double)n_list;
    h->stats[3] += (double)n_walk;
    h->stats[4] += (double)n_seen;
    h->stats[5] += (double)found.size();
    h->stats[7] += cover_ms;
    h->stats[8] += reads_ms;
}

int hello_sv_add(hello_sv* h, const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                 const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends, const uint8_t* mapq,
                 const uint16_t* flags, const uint64_t* name_hash, const uint8_t* hp, int64_t n_reads, int64_t lo, int64_t hi) try {
    sv_add(h, bases, quals, read_offsets, cigars, cigar_offsets, ref_starts, ref_ends, mapq, flags, name_hash, hp, nullptr, nullptr, 0,
           n_reads, lo, hi);
    return HELLO_OK;
} HS_ENTRY_END("hello_sv_add")

int hello_sv_add_split(hello_sv* h, const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                       const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends, const uint8_t* mapq,
                       const uint16_t* flags, const uint64_t* name_hash, const uint8_t* hp, const uint8_t* sa_bytes,
                       const int64_t* sa_offsets, int64_t n_sa_bytes, int64_t n_reads, int64_t lo, int64_t hi) try {
    if (!sa_offsets) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    sv_add(h, bases, quals, read_offsets, cigars, cigar_offsets, ref_starts, ref_ends, mapq, flags, name_hash, hp, sa_bytes, sa_offsets,
           n_sa_bytes, n_reads, lo, hi);
    return HELLO_OK;
} HS_ENTRY_END("hello_sv_add_split")

int hello_sv_add_pairs(hello_sv* h, const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                       const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends, const uint8_t* mapq,
                       const uint16_t* flags, const uint64_t* name_hash, const uint8_t* hp, const uint8_t* sa_bytes,
                       const int64_t* sa_offsets, int64_t n_sa_bytes, const int32_t* mate_tid, const int64_t* mate_pos, int64_t n_reads,
                       int64_t lo, int64_t hi) try {
    if (!sa_offsets || !mate_tid || !mate_pos) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    sv_add(h, bases, quals, read_offsets, cigars, cigar_offsets, ref_starts, ref_ends, mapq, flags, name_hash, hp, sa_bytes, sa_offsets,
           n_sa_bytes, n_reads, lo, hi, mate_tid, mate_pos);
    return HELLO_OK;
} HS_ENTRY_END("hello_sv_add_pairs")

int hello_sv_library(hello_sv* h, int32_t median, int32_t lo, int32_t hi) try {
    using namespace hello;
    if (!h) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (h->has_library) return set_last_error(HELLO_ERR_ARG, "hello_sv_library twice: the handle has its insert sizes");
    if (lo > median || median > hi) return set_last_error(HELLO_ERR_ARG, "library (%d, %d, %d): lo <= median <= hi", median, lo, hi);
    h->library.median = median;
    h->library.lo = lo;
    h->library.hi = hi;
    h->has_library = true;
    return HELLO_OK;
} HS_ENTRY_END("hello_sv_library")

int hello_sv_clip_min(hello_sv* h, int32_t clip_min) try {
    using namespace hello;
    if (!h) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (clip_min < 1) return set_last_error(HELLO_ERR_ARG, "clip_min %d: at least 1", clip_min);
    if (h->pairs_given_adds) return set_last_error(HELLO_ERR_ARG, "hello_sv_clip_min after hello_sv_add_pairs: clips were counted already");
    h->clip_min = clip_min;
    return HELLO_OK;
} HS_ENTRY_END("hello_sv_clip_min")

int hello_sv_contigs(hello_sv* h, const char* const* names, int64_t n, int64_t own) try {
    using namespace hello;
    if (!h || !names) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (n < 1 || n > INT32_MAX) return set_last_error(HELLO_ERR_ARG, "%lld contigs: at least 1", (long long)n);
    if (own < 0 || own >= n) return set_last_error(HELLO_ERR_ARG, "own contig %lld of %lld", (long long)own, (long long)n);
    if (!h->contigs.empty()) return set_last_error(HELLO_ERR_ARG, "hello_sv_contigs twice: the handle has its contig names");
    std::vector<std::pair<uint64_t, std::string>> seen;
    std::vector<uint64_t> hashes;
    for (int64_t i = 0; i < n; ++i) {
        if (!names[i]) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
        seen.emplace_back(sv_name_hash(names[i]), names[i]);
        hashes.push_back(seen.back().first);
    }
    std::sort(seen.begin(), seen.end());
    for (size_t i = 1; i < seen.size(); ++i) {
        if (seen[i].first != seen[i - 1].first) continue;
        if (seen[i].second == seen[i - 1].second) return set_last_error(HELLO_ERR_ARG, "contig '%s' twice", seen[i].second.c_str());
        return set_last_error(HELLO_ERR_ARG, "contigs '%s' and '%s' have one FNV-1a hash", seen[i - 1].second.c_str(), seen[i].second.c_str());
    }
    h->contigs.swap(hashes);
    h->own = (int32_t)own;
    return HELLO_OK;
} HS_ENTRY_END("hello_sv_contigs")

static int sv_check_clustering(int64_t cluster_gap, int32_t len_ratio_percent, int32_t min_support) {
    using namespace hello;
    if (cluster_gap < 0) return set_last_error(HELLO_ERR_ARG, "cluster_gap %lld: 0 or more", (long long)cluster_gap);
    if (len_ratio_percent < 1 || len_ratio_percent > 100)
        return set_last_error(HELLO_ERR_ARG, "len_ratio_percent %d: 1 to 100", len_ratio_percent);
    if (min_support < 1) return set_last_error(HELLO_ERR_ARG, "min_support %d: at least 1", min_support);
    return HELLO_OK;
}

// hello_sv_cluster (types below 2, 13 columns) and hello_sv_cluster_split (types below kSvClustered, SR as the 14th).
static int sv_cluster_rows(const int64_t* signatures, int64_t n, int64_t cluster_gap, int32_t len_ratio_percent, int32_t min_support,
                           int64_t* out, int64_t* n_out, int n_types, int columns) {
    using namespace hello;
    if (!n_out || (n > 0 && (!signatures || !out))) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (n < 0) return set_last_error(HELLO_ERR_ARG, "negative count");
    if (int rc = sv_check_clustering(cluster_gap, len_ratio_percent, min_support)) return rc;
    std::vector<SvSig> sigs((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t* g = signatures + i * kSvSigColumns;
        if (g[0] < 0 || g[0] >= n_types || g[2] < 1 || g[2] > INT32_MAX || g[6] < 0 || g[6] > 1 || g[7] < 0 || g[7] > 255)
            return set_last_error(HELLO_ERR_ARG, "signature %lld: type %lld, len %lld, strand %lld, hp %lld", (long long)i,
                                  (long long)g[0], (long long)g[2], (long long)g[6], (long long)g[7]);
        sigs[(size_t)i] = SvSig{g[1], g[4], g[5], (int32_t)g[2], (int32_t)g[3], (uint8_t)g[0], (uint8_t)g[6], (uint8_t)g[7], 0};
    }
    sv_sort(sigs);
    const std::vector<SvCandidate> found = sv_cluster(sigs, cluster_gap, len_ratio_percent, min_support);
    for (size_t i = 0; i < found.size(); ++i) {
        const SvCandidate& c = found[i];
        const int64_t row[HELLO_SV_CLUSTER_SPLIT_COLUMNS] = {c.type, c.pos, c.len, c.dv, c.dv_fwd, c.dv_rev, c.hp[0], c.hp[1], c.hp[2],
                                                             c.pos_min, c.pos_max, c.len_min, c.len_max, c.sr};
        std::copy(row, row + columns, out + i * columns);
    }
    *n_out = (int64_t)found.size();
    return HELLO_OK;
}

int hello_sv_cluster(const int64_t* signatures, int64_t n, int64_t cluster_gap, int32_t len_ratio_percent, int32_t min_support,
                     int64_t* out, int64_t* n_out) try {
    return sv_cluster_rows(signatures, n, cluster_gap, len_ratio_percent, min_support, out, n_out, 2, HELLO_SV_CLUSTER_COLUMNS);
} HS_ENTRY_END("hello_sv_cluster")

int hello_sv_cluster_split(const int64_t* signatures, int64_t n, int64_t cluster_gap, int32_t len_ratio_percent, int32_t min_support,
                           int64_t* out, int64_t* n_out) try {
    return sv_cluster_rows(signatures, n, cluster_gap, len_ratio_percent, min_support, out, n_out, hello::kSvClustered,
                           HELLO_SV_CLUSTER_SPLIT_COLUMNS);
} HS_ENTRY_END("hello_sv_cluster_split")

int hello_sv_finish(hello_sv* h, int64_t cluster_gap, int32_t len_ratio_percent, int32_t min_support) try {
    using namespace hello;
    if (!h) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (h->finished) return set_last_error(HELLO_ERR_ARG, "hello_sv_finish twice: the handle is finished");
    if (int rc = sv_check_clustering(cluster_gap, len_ratio_percent, min_support)) return rc;
    sv_signature_columns(h);
    int64_t n_assigned = 0, n_pair_only = 0;
    std::vector<SvPairCandidate> found;
    if (h->has_library) {
        found = sv_cluster_pairs(h->sigs, cluster_gap, len_ratio_percent, min_support, h->library, h->flank, &n_assigned);
    } else {
        for (const SvCandidate& c : sv_cluster(h->sigs, cluster_gap, len_ratio_percent, min_support)) {
            SvPairCandidate p{};
            static_cast<SvCandidate&>(p) = c;
            p.end = p.end_min = p.end_max = sv_candidate_end(c);
            found.push_back(p);
        }
    }
    const size_t n = found.size();
    std::vector<long long> depth(n, 0), ce(n, 0);
    float ms = 0.0f;
    if (n > 0) {                                     // a candidate has signatures, so an add has built the device side
        HS_HIP(hipSetDevice(h->device));
        DevMem m;
        std::vector<int64_t> pos(n);
        for (size_t i = 0; i < n; ++i) pos[i] = found[i].pos;
        SvSpanArgs a{};
        a.diff = h->diff;
        a.n_diff = h->length + 1;
        a.n_tiles = (a.n_diff + kSvTile - 1) / kSvTile;
        a.tile_sum = m.room<long long>((size_t)a.n_tiles);
        a.pos = m.put(pos.data(), n);
        a.n_candidates = (int64_t)n;
        a.depth = m.room<long long>(n);
        KernelTimer timer;
        timer.start();
        hipLaunchKernelGGL(sv_tile_kernel, dim3((unsigned)a.n_tiles), dim3(kSvThreads), 0, 0, a);
        ms = timer.stop();
        std::vector<long long> sums((size_t)a.n_tiles), before((size_t)a.n_tiles);
        HS_HIP(hipMemcpy(sums.data(), a.tile_sum, sums.size() * sizeof(long long), hipMemcpyDeviceToHost));
        long long running = 0;
        for (size_t t = 0; t < sums.size(); ++t) {
            before[t] = running;
            running += sums[t];
        }
        HS_HIP(hipMemcpy(a.tile_sum, before.data(), before.size() * sizeof(long long), hipMemcpyHostToDevice));
        timer.start();
        hipLaunchKernelGGL(sv_span_kernel, dim3((unsigned)((n + kSvWaves - 1) / kSvWaves)), dim3(kSvThreads), 0, 0, a);
        ms += timer.stop();
        HS_HIP(hipMemcpy(depth.data(), a.depth, n * sizeof(long long), hipMemcpyDeviceToHost));
        if (h->pairs_built) {                        // CE: the clipped ends around both ends of every candidate
            std::vector<int64_t> end(n);
            for (size_t i = 0; i < n; ++i) end[i] = found[i].end;
            SvClipArgs k{h->clip_left, h->clip_right, a.pos, m.put(end.data(), n), (int64_t)n, h->length, h->flank, m.room<long long>(n)};
            timer.start();
            hipLaunchKernelGGL(sv_clips_kernel, dim3((unsigned)((n + kSvWaves - 1) / kSvWaves)), dim3(kSvThreads), 0, 0, k);
            ms += timer.stop();
            HS_HIP(hipMemcpy(ce.data(), k.ce, n * sizeof(long long), hipMemcpyDeviceToHost));
        }
    }
    std::vector<int64_t> cols[kSvCandColumns], sr(n), of_pairs[5];
    for (auto& c : cols) c.resize(n);
    for (auto& c : of_pairs) c.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const SvPairCandidate& c = found[i];
        int64_t g[kSvGenotypeColumns];
        const int64_t dp = (int64_t)depth[i], dr = sv_depth_ref(dp, c.dv, c.sr);
        sv_genotype(c.dv + c.pr, dr, g);             // pair supporters end before the breakpoint: they are not in DP
        const int64_t more[5] = {c.pr, (int64_t)ce[i], c.end_min, c.end_max, c.imprecise};
        for (int k = 0; k < 5; ++k) of_pairs[k][i] = more[k];
        n_pair_only += c.imprecise;
        const int64_t row[kSvCandColumns] = {c.type, c.pos, c.len, c.dv, c.dv_fwd, c.dv_rev, c.hp[0], c.hp[1], c.hp[2], c.pos_min,
                                             c.pos_max, c.len_min, c.len_max, dp, dr, g[0], g[1], g[2], g[3], g[4]};
        for (int k = 0; k < kSvCandColumns; ++k) cols[k][i] = row[k];
        sr[i] = c.sr;
    }
    // ---- nothing can fail from here on
    for (int k = 0; k < kSvCandColumns; ++k) h->cand_cols[k].swap(cols[k]);
    h->cand_sr.swap(sr);
    for (int k = 0; k < 5; ++k) h->cand_pairs[k].swap(of_pairs[k]);
    h->pair_stats[10] = (double)n_assigned;
    h->pair_stats[11] = (double)n_pair_only;
    h->finished = true;
    h->stats[6] = (double)n;
    h->stats[9] += ms;
    return HELLO_OK;
} HS_ENTRY_END("hello_sv_finish")

int hello_sv_array(hello_sv* h, int32_t which, const void** data, int64_t* count) try {
    using namespace hello;
    if (!h || !data || !count) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (which >= HELLO_SV_SIGNATURES_TYPE && which <= HELLO_SV_SIGNATURES_HP) {
        sv_signature_columns(h);
        const std::vector<int64_t>& c = h->sig_cols[which - HELLO_SV_SIGNATURES_TYPE];
        *data = c.data(); *count = (int64_t)c.size();
    } else if (which >= HELLO_SV_CANDIDATES_TYPE && which <= HELLO_SV_CANDIDATES_PL2) {
        if (!h->finished) return set_last_error(HELLO_ERR_ARG, "array selector %d before hello_sv_finish", which);
        const std::vector<int64_t>& c = h->cand_cols[which - HELLO_SV_CANDIDATES_TYPE];
        *data = c.data(); *count = (int64_t)c.size();
    } else if (which == HELLO_SV_CANDIDATES_SR) {
        if (!h->finished) return set_last_error(HELLO_ERR_ARG, "array selector %d before hello_sv_finish", which);
        *data = h->cand_sr.data(); *count = (int64_t)h->cand_sr.size();
    } else if (which == HELLO_SV_SPLIT_STATUS) {
        *data = h->split_status.data(); *count = (int64_t)h->split_status.size();
    } else if (which == HELLO_SV_STATUS) {
        *data = h->status.data(); *count = (int64_t)h->status.size();
    } else {
        return set_last_error(HELLO_ERR_ARG, "array selector %d", which);
    }
    return HELLO_OK;
} HS_ENTRY_END("hello_sv_array")

int hello_sv_pairs_array(hello_sv* h, int32_t which, const void** data, int64_t* count) try {
    using namespace hello;
    if (!h || !data || !count) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (which == HELLO_SV_PAIRS_INNER) {
        h->inner_host.assign(kInnerBins, 0);
        if (h->pairs_built) {
            HS_HIP(hipSetDevice(h->device));
            HS_HIP(hipMemcpy(h->inner_host.data(), h->inner, kInnerBins * sizeof(int64_t), hipMemcpyDeviceToHost));
        }
        *data = h->inner_host.data(); *count = kInnerBins;
    } else if (which == HELLO_SV_PAIRS_CLIP_LEFT || which == HELLO_SV_PAIRS_CLIP_RIGHT) {
        std::vector<int32_t>& c = h->clip_host[which - HELLO_SV_PAIRS_CLIP_LEFT];
        c.assign((size_t)h->length + 1, 0);
        if (h->pairs_built) {
            HS_HIP(hipSetDevice(h->device));
            HS_HIP(hipMemcpy(c.data(), which == HELLO_SV_PAIRS_CLIP_LEFT ? h->clip_left : h->clip_right, c.size() * sizeof(int32_t),
                             hipMemcpyDeviceToHost));
        }
        *data = c.data(); *count = (int64_t)c.size();
    } else if (which == HELLO_SV_PAIRS_STATUS) {
        *data = h->pair_status.data(); *count = (int64_t)h->pair_status.size();
    } else if (which >= HELLO_SV_PAIRS_CANDIDATES_PR && which <= HELLO_SV_PAIRS_CANDIDATES_IMPRECISE) {
        if (!h->finished) return set_last_error(HELLO_ERR_ARG, "array selector %d before hello_sv_finish", which);
        const std::vector<int64_t>& c = h->cand_pairs[which - HELLO_SV_PAIRS_CANDIDATES_PR];
        *data = c.data(); *count = (int64_t)c.size();
    } else {
        return set_last_error(HELLO_ERR_ARG, "array selector %d", which);
    }
    return HELLO_OK;
} HS_ENTRY_END("hello_sv_pairs_array")

int hello_sv_pairs_stats(const hello_sv* h, double* stats) {
    if (!h || !stats) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    std::copy(h->pair_stats, h->pair_stats + hello::kPairStats, stats);
    return HELLO_OK;
}

int hello_sv_library_of(const int64_t* inner, int64_t k, int64_t* out) try {
    using namespace hello;
    if (!inner || !out) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (k < 1) return set_last_error(HELLO_ERR_ARG, "k %lld: at least 1", (long long)k);
    for (int b = 0; b < kInnerBins; ++b)
        if (inner[b] < 0) return set_last_error(HELLO_ERR_ARG, "bin %d counts %lld", b, (long long)inner[b]);
    if (!sv_library_of(inner, k, out)) return set_last_error(HELLO_ERR_ARG, "an empty histogram has no library");
    return HELLO_OK;
} HS_ENTRY_END("hello_sv_library_of")

int hello_sv_cluster_pairs(const int64_t* signatures, int64_t n, int64_t cluster_gap, int32_t len_ratio_percent, int32_t min_support,
                           int32_t median, int32_t lo, int32_t hi, int32_t flank, int64_t* out, int64_t* n_out) try {
    using namespace hello;
    if (!n_out || (n > 0 && (!signatures || !out))) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (n < 0) return set_last_error(HELLO_ERR_ARG, "negative count");
    if (int rc = sv_check_clustering(cluster_gap, len_ratio_percent, min_support)) return rc;
    if (lo > median || median > hi) return set_last_error(HELLO_ERR_ARG, "library (%d, %d, %d): lo <= median <= hi", median, lo, hi);
    if (flank < 1) return set_last_error(HELLO_ERR_ARG, "flank %d: at least 1", flank);
    std::vector<SvSig> sigs((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t* g = signatures + i * kSvSigColumns;
        const bool pair = g[5] == kPairOp;
        if (g[0] < 0 || g[0] > kSvBnd || g[2] < (g[0] == kSvBnd ? 0 : 1) || g[2] > INT32_MAX || g[3] < (pair ? 0 : INT32_MIN) || g[3] > INT32_MAX
            || g[6] < 0 || g[6] > 1 || g[7] < 0 || g[7] > 255)
            return set_last_error(HELLO_ERR_ARG, "signature %lld: type %lld, len %lld, shift %lld, strand %lld, hp %lld", (long long)i,
                                  (long long)g[0], (long long)g[2], (long long)g[3], (long long)g[6], (long long)g[7]);
        sigs[(size_t)i] = SvSig{g[1], g[4], g[5], (int32_t)g[2], (int32_t)g[3], (uint8_t)g[0], (uint8_t)g[6], (uint8_t)g[7], 0};
    }
    sv_sort(sigs);
    int64_t n_assigned = 0;
    SvLibrary lib;
    lib.median = median; lib.lo = lo; lib.hi = hi;
    const std::vector<SvPairCandidate> found = sv_cluster_pairs(sigs, cluster_gap, len_ratio_percent, min_support, lib, flank, &n_assigned);
    for (size_t i = 0; i < found.size(); ++i) {
        const SvPairCandidate& c = found[i];
        const int64_t row[HELLO_SV_CLUSTER_PAIRS_COLUMNS] = {c.type, c.pos, c.len, c.dv, c.dv_fwd, c.dv_rev, c.hp[0], c.hp[1], c.hp[2],
                                                             c.pos_min, c.pos_max, c.len_min, c.len_max, c.sr, c.pr, c.end_min, c.end_max,
                                                             c.imprecise};
        std::copy(row, row + HELLO_SV_CLUSTER_PAIRS_COLUMNS, out + i * HELLO_SV_CLUSTER_PAIRS_COLUMNS);
    }
    *n_out = (int64_t)found.size();
    return HELLO_OK;
} HS_ENTRY_END("hello_sv_cluster_pairs")

int hello_sv_stats(const hello_sv* h, double* stats) {
    if (!h || !stats) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    return h->copy_stats(stats);
}

void hello_sv_free(hello_sv* h) { delete h; }

int hello_sv_genotype(const int64_t* dv, const int64_t* dr, int64_t n, int64_t* out) try {
    using namespace hello;
    if (!out || (n > 0 && (!dv || !dr))) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (n < 0) return set_last_error(HELLO_ERR_ARG, "negative count");
    for (int64_t i = 0; i < n; ++i)
        if (dv[i] < 0 || dr[i] < 0) return set_last_error(HELLO_ERR_ARG, "candidate %lld: count %lld", (long long)i, (long long)std::min(dv[i], dr[i]));
    for (int64_t i = 0; i < n; ++i) sv_genotype(dv[i], dr[i], out + i * kSvGenotypeColumns);
    return HELLO_OK;
} HS_ENTRY_END("hello_sv_genotype")

}  // extern "C"
