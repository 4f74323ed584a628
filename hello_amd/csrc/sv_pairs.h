// The rules of the discordant read pairs and the clipped ends: what one record's own and mate fields become
// (sv_pair_classify), which clips of a read count (sv_clips), the library from the histogram of inner distances, and at finish the
// assignment of pair rows to the clusters of 7p / 7q and the clusters of pair rows alone.  Plain C++17, the per-read part marked
// __host__ __device__ under HIP: the same text runs in sv_pairs_kernel (sv.hip) and in a stand-alone host program
// (tests/abi/sv_pairs_check.cpp).  hello_amd/sv.py restates it in Python (pair_rows_of, library_of, assigned, clustered_pairs),
// integer for integer.
#pragma once
#include <cstdint>
#include <vector>

#include "cigar.h"
#include "sv_split.h"

namespace hello {
namespace {

constexpr int64_t kPairOp = -16;                 // the OP column of a pair row: no CIGAR operation, no junction of a tag
constexpr int kInnerBins = 4096, kInnerZero = 1024;      // INNER[clamp(ms - e + 1024, 0, 4095)]
constexpr int64_t kMateMaxPos = 2147483647;
constexpr int32_t kLibraryUnsetLo = INT32_MIN, kLibraryUnsetHi = INT32_MAX;
// PAIR_STATUS, per read of the last add
constexpr uint8_t kPairNone = 0, kPairBadMate = 1, kPairRight = 2, kPairNormal = 3, kPairShort = 4, kPairSmall = 5, kPairUnplaced = 6,
                  kPairRow = 7, kPairBndRow = 8;
// what the host hands the kernel per read
constexpr uint8_t kPairClassify = 1, kPairClips = 2;
constexpr int kPairStats = 13;

constexpr uint16_t kPairRefused = 0x4 | 0x8 | 0x100 | 0x800 | 0x400 | 0x200;
SVS_HD inline bool pair_counted(uint16_t flag, int mapq, int mapq_threshold) {
    return (flag & 0x1) && !(flag & kPairRefused) && mapq >= mapq_threshold;          // 0x2 is not consulted
}

// A pair-counted read's mate fields: what a rule may compute with.
SVS_HD inline bool mate_valid(int64_t mate_tid, int64_t mate_pos, int32_t own, int64_t length) {
    return mate_pos >= 0 && mate_pos <= kMateMaxPos && (mate_tid != own || mate_pos <= length);
}

struct SvLibrary {
    int32_t median = 0, lo = kLibraryUnsetLo, hi = kLibraryUnsetHi;
};

struct SvPairOutcome {
    uint8_t status = kPairNone;
    bool inner = false;                          // adds 1 to INNER[bin]
    int32_t bin = 0;
    int32_t type = 0;                            // of the row, with status kPairRow or kPairBndRow
    int64_t pos = 0, len = 0, shift = 0;
};

// One belonging, pair-counted record with valid mate fields: [s, e) on chromosome `own`, the mate at ms on mt.
SVS_HD inline SvPairOutcome sv_pair_classify(uint16_t flag, int64_t s, int64_t e, int32_t own, int64_t mt, int64_t ms, int64_t n_contigs,
                                             SvLibrary lib, int64_t min_size) {
    SvPairOutcome o;
    const bool rev = flag & 0x10, mrev = flag & 0x20;
    if (mt != own) {
        if (mt < 0 || mt >= n_contigs) { o.status = kPairUnplaced; return o; }
        o.status = kPairBndRow;
        o.type = kSvBnd;
        o.pos = rev ? s : e;
        o.len = mt;
        o.shift = ms;
        return o;
    }
    if (!(s < ms || (s == ms && (flag & 0x40)))) { o.status = kPairRight; return o; }
    o.shift = ms;
    if (!rev && mrev) {                          // FR
        const int64_t g = ms - e, at = g + kInnerZero;
        o.inner = true;
        o.bin = (int32_t)(at < 0 ? 0 : at > kInnerBins - 1 ? kInnerBins - 1 : at);
        if (g > lib.hi) {
            o.type = kSvDel;
            o.pos = e;
            o.len = g - lib.median;
        } else {
            o.status = g < lib.lo ? kPairShort : kPairNormal;
            return o;
        }
    } else if (rev && !mrev) {                   // RF
        o.type = kSvDup;
        o.pos = s;
        o.len = ms - s;
        if (ms < e) { o.status = kPairSmall; return o; }          // the mates overlap: a read-through pair
    } else {                                     // FF, RR
        o.type = rev ? kSvInv5 : kSvInv3;
        o.pos = rev ? s : e;
        o.len = ms < o.pos ? o.pos - ms : ms - o.pos;
    }
    o.status = o.len >= min_size && o.len <= kMateMaxPos ? kPairRow : kPairSmall;
    return o;
}

// The soft clips that count: bit 0 the leading one (the first operation, or the second behind an H), bit 1 the trailing one.
SVS_HD inline int sv_clips(const uint32_t* cigar, int64_t n_ops, int64_t clip_min) {
    if (n_ops < 1) return 0;
    int found = 0;
    int64_t i = (cigar[0] & 15) == BAM_CHARD_CLIP ? 1 : 0;
    int64_t j = (cigar[n_ops - 1] & 15) == BAM_CHARD_CLIP ? n_ops - 2 : n_ops - 1;
    if (i < n_ops && (cigar[i] & 15) == BAM_CSOFT_CLIP && (int64_t)(cigar[i] >> 4) >= clip_min) found |= 1;
    if (j > i && (cigar[j] & 15) == BAM_CSOFT_CLIP && (int64_t)(cigar[j] >> 4) >= clip_min) found |= 2;
    return found;
}

// ---- the host side --------------------------------------------------------------------------------------------------------------
// What the host decides per read of one add before any launch (hello_sv_add_pairs; tests/abi/sv_pairs_check.cpp runs the same
// text): which reads sv_pairs_kernel may classify, whose clips it may count, the BAD_MATE reads and the pair ordinals.  `kind` is
// sv_walk's (kPileBelongs | kPileCounted), which has validated every counted read; a pair-counted read that is not counted is
// walked here in the same way (exact_walk_on_reference: refusals are thrown), since s and e come from its CIGAR too.  A read whose
// end lies beyond the chromosome is never marked: the kernel indexes CLIP_LEFT [length + 1] with it.
struct SvPairMarks {
    std::vector<uint8_t> todo, state;            // per read: kPairClassify | kPairClips; kPairNone or kPairBadMate
    std::vector<int64_t> ordinal;                // per read: of a pair-counted one, its index among the handle's
    int64_t n_pair_reads = 0, n_bad_mate = 0, n_classify = 0, n_work = 0;
};
inline SvPairMarks sv_pairs_mark(const ReadsView& in, const std::vector<uint8_t>& kind, const int64_t* sa_offsets, const int32_t* mate_tid,
                                 const int64_t* mate_pos, int32_t own, int64_t length, int mapq_threshold, int64_t pairs_given) {
    SvPairMarks m;
    m.todo.assign((size_t)in.n, 0);
    m.state.assign((size_t)in.n, kPairNone);
    m.ordinal.assign((size_t)in.n, 0);
    for (int64_t r = 0; r < in.n; ++r) {
        if (!(kind[(size_t)r] & kPileBelongs)) continue;
        const bool is_counted = kind[(size_t)r] & kPileCounted;
        if (pair_counted(in.flags[r], in.mapq[r], mapq_threshold)) {
            if (!is_counted) exact_walk_on_reference(in, r, INT32_MAX);
            m.ordinal[(size_t)r] = pairs_given + m.n_pair_reads++;
            if (in.ref_end[r] <= length && mate_valid(mate_tid[r], mate_pos[r], own, length)) {
                m.todo[(size_t)r] |= kPairClassify;
                ++m.n_classify;
            } else {
                m.state[(size_t)r] = kPairBadMate;
                ++m.n_bad_mate;
            }
        }
        if (is_counted && sa_offsets[r + 1] == sa_offsets[r] && in.ref_end[r] <= length &&
            sv_clips(in.cigars + in.cigar_off[r], in.cigar_off[r + 1] - in.cigar_off[r], 1))          // a soft clip of any size at an end
            m.todo[(size_t)r] |= kPairClips;
        m.n_work += m.todo[(size_t)r] != 0;
    }
    return m;
}

// The lower median of the values a histogram counts; -1 for an empty one.
inline int64_t sv_histogram_median(const std::vector<int64_t>& h) {
    int64_t total = 0;
    for (int64_t c : h) total += c;
    if (total == 0) return -1;
    int64_t seen = 0;
    for (size_t v = 0; v < h.size(); ++v) {
        seen += h[v];
        if (seen > (total - 1) / 2) return (int64_t)v;
    }
    return -1;
}

// INNER -> (median, lo, hi); false for an empty histogram.
inline bool sv_library_of(const int64_t* inner, int64_t k, int64_t out[3]) {
    std::vector<int64_t> h(inner, inner + kInnerBins);
    const int64_t at = sv_histogram_median(h);
    if (at < 0) return false;
    std::vector<int64_t> dev(kInnerBins, 0);
    for (int v = 1; v < kInnerBins - 1; ++v) dev[(size_t)(v > at ? v - at : at - v)] += h[(size_t)v];      // without the clamped bins
    const int64_t mad = std::max<int64_t>(sv_histogram_median(dev), 1);
    out[0] = at - kInnerZero;
    out[1] = out[0] - k * mad;
    out[2] = out[0] + k * mad;
    return true;
}

struct SvPairCandidate : SvCandidate {
    int64_t pr = 0, end_min = 0, end_max = 0, imprecise = 0, end = 0;
};

inline int64_t sv_candidate_end(const SvCandidate& c) { return c.type == kSvIns ? c.pos : c.pos + c.len; }

// Whether the pair row (type, a = pos, b = shift) supports the cluster c of its type.
inline bool sv_pair_supports(const SvSig& g, const SvCandidate& c, SvLibrary lib, int64_t slack) {
    if (g.type != c.type) return false;
    const int64_t a = g.pos, b = g.shift, P = c.pos, L = c.len;
    if (g.type == kSvDel) return a - slack <= P && P + L <= b + slack && (b - a) - L >= lib.lo && (b - a) - L <= lib.hi;
    const int64_t da = a < P ? P - a : a - P, db = b < P + L ? P + L - b : b - (P + L);
    return da <= lib.hi && db <= lib.hi;
}

inline int64_t sv_lower_median(std::vector<int64_t> v) {
    std::sort(v.begin(), v.end());
    return v[(v.size() - 1) / 2];
}

// One group of unassigned pair rows of one type -> a candidate when it has at least min_support rows.
inline void sv_pair_group(const SvSig* g, size_t m, int64_t min_support, std::vector<SvPairCandidate>& out) {
    if ((int64_t)m < min_support) return;
    std::vector<int64_t> a(m), b(m), len(m);
    for (size_t i = 0; i < m; ++i) { a[i] = g[i].pos; b[i] = g[i].shift; len[i] = g[i].len; }
    SvPairCandidate c{};
    c.type = g[0].type;
    c.len = sv_lower_median(len);
    c.pos_min = *std::min_element(a.begin(), a.end());
    c.pos_max = *std::max_element(a.begin(), a.end());
    c.end_min = *std::min_element(b.begin(), b.end());
    c.end_max = *std::max_element(b.begin(), b.end());
    c.len_min = *std::min_element(len.begin(), len.end());
    c.len_max = *std::max_element(len.begin(), len.end());
    c.pos = c.type == kSvDel ? c.pos_max : sv_lower_median(a);
    c.end = c.type == kSvDel ? c.end_min : c.pos + c.len;
    c.pr = (int64_t)m;
    c.imprecise = 1;
    out.push_back(c);
}

// `sigs` in sv_sort's order, the rows of all kinds -> the candidates sorted by (pos, type, len, imprecise): the clusters of the
// rows that are no pair rows, as 7p / 7q form them, each with the pair rows it takes, and the clusters of the pair rows left.
// *n_assigned: the pair rows a cluster of step 1 took.
inline std::vector<SvPairCandidate> sv_cluster_pairs(const std::vector<SvSig>& sigs, int64_t cluster_gap, int64_t len_ratio_percent,
                                                     int64_t min_support, SvLibrary lib, int64_t slack, int64_t* n_assigned) {
    std::vector<SvSig> plain, pairs;
    for (const SvSig& g : sigs) (g.op_index == kPairOp ? pairs : plain).push_back(g);
    std::vector<SvPairCandidate> out;
    for (const SvCandidate& c : sv_cluster(plain, cluster_gap, len_ratio_percent, min_support)) {
        SvPairCandidate p{};
        static_cast<SvCandidate&>(p) = c;
        p.end = p.end_min = p.end_max = sv_candidate_end(c);
        out.push_back(p);
    }
    std::vector<SvSig> left;
    *n_assigned = 0;
    for (const SvSig& g : pairs) {
        if (g.type >= kSvClustered) continue;    // a BND
        bool taken = false;
        for (SvPairCandidate& c : out)
            if (sv_pair_supports(g, c, lib, slack)) { ++c.pr; taken = true; break; }
        *n_assigned += taken;
        if (!taken) left.push_back(g);
    }
    std::sort(left.begin(), left.end(), [](const SvSig& x, const SvSig& y) {
        return std::make_tuple(x.type, x.pos, (int64_t)x.shift, x.ordinal) < std::make_tuple(y.type, y.pos, (int64_t)y.shift, y.ordinal);
    });
    const int64_t reach = (int64_t)lib.hi - (int64_t)lib.lo;
    size_t g0 = 0;
    int64_t top = 0, bottom = 0;                 // the intersection of the group so far: [top, bottom]
    for (size_t i = 0; i < left.size(); ++i) {
        const int64_t a = std::min<int64_t>(left[i].pos, left[i].shift), b = std::max<int64_t>(left[i].pos, left[i].shift);
        const bool same_run = i > g0 && left[i].type == left[i - 1].type && left[i].pos - left[i - 1].pos <= reach;
        if (i > g0 && !(same_run && a <= bottom && b >= top)) {
            sv_pair_group(left.data() + g0, i - g0, min_support, out);
            g0 = i;
        }
        if (i == g0) { top = a; bottom = b; }
        else { top = std::max(top, a); bottom = std::min(bottom, b); }
    }
    if (g0 < left.size()) sv_pair_group(left.data() + g0, left.size() - g0, min_support, out);
    std::stable_sort(out.begin(), out.end(), [](const SvPairCandidate& x, const SvPairCandidate& y) {
        return std::make_tuple(x.pos, x.type, x.len, x.imprecise) < std::make_tuple(y.pos, y.type, y.len, y.imprecise);
    });
    return out;
}

// The two windows CE sums CLIP_LEFT + CLIP_RIGHT over, inside [0, length]; the second leaves out what the first holds.
struct SvClipWindows {
    int64_t lo1, hi1, lo2, hi2;                  // inclusive; lo > hi: empty
};
SVS_HD inline SvClipWindows sv_clip_windows(int64_t pos, int64_t end, int64_t flank, int64_t length) {
    SvClipWindows w;
    w.lo1 = pos - flank < 0 ? 0 : pos - flank;
    w.hi1 = pos + flank > length ? length : pos + flank;
    w.lo2 = end - flank < 0 ? 0 : end - flank;
    if (w.lo2 <= w.hi1) w.lo2 = w.hi1 + 1;
    w.hi2 = end + flank > length ? length : end + flank;
    return w;
}

}  // namespace
}  // namespace hello
