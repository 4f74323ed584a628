// The rules of the split alignments: what a segment is, the grammar of one entry of the SA tag, and what the
// junction between two segments that follow each other on the read becomes.  Plain C++17, marked __host__ __device__ under HIP: the
// same text runs in sv_split_kernel (sv.hip), in hello_sv_add_split's host checks and in a stand-alone host program
// (tests/abi/sv_split_check.cpp).  hello_amd/sv.py restates it in Python (segments_of, junctions_of), integer for integer.
//
// Nothing here moves an index by what it reads: every byte index stays inside [begin, end), and garbage only clears `ok`.
#pragma once
#include <cstdint>
#include <string>

#include "sv.h"

#if defined(__HIPCC__)
#define SVS_HD __host__ __device__
#else
#define SVS_HD
#endif

namespace hello {
namespace {

constexpr int kMaxSegments = 8;                  // the primary and at most 7 entries of its SA tag
constexpr int kSvDup = 2, kSvInv3 = 3, kSvInv5 = 4, kSvBnd = 5;
constexpr uint8_t kSplitNone = 0, kSplitParsed = 1, kSplitRow = 2, kSplitBadSa = 3, kSplitTooMany = 4;
constexpr int64_t kSaMaxPos = 2147483647, kSaMaxCount = (int64_t(1) << 28) - 1;
constexpr uint64_t kFnvOffset = 1469598103934665603ull, kFnvPrime = 1099511628211ull;

struct SvSegment {
    int64_t s, e;                                // the reference bases [s, e)
    int64_t a, m, b;                             // the leading clips, the aligned query bases, the trailing clips
    int64_t qs, qe;                              // where the aligned bases lie on the read as it was sequenced
    uint64_t hash;                               // FNV-1a of rname (an entry's alone)
    int32_t tid, mapq, strand, ok;
};

SVS_HD inline void sv_orient(SvSegment& g) {
    g.qs = g.strand ? g.b : g.a;
    g.qe = g.qs + g.m;
}

// 1 to 10 digits at t[i ..) -> v; i stops behind them.  An eleventh digit is an error.
SVS_HD inline bool sa_number(const uint8_t* t, int64_t& i, int64_t end, int64_t& v) {
    int digits = 0;
    v = 0;
    while (i < end && t[i] >= '0' && t[i] <= '9') {
        if (++digits > 10) return false;
        v = v * 10 + (t[i] - '0');
        ++i;
    }
    return digits >= 1;
}

// One CIGAR in text at t[i ..), up to the byte that is neither a digit nor follows a count -> a, m, b and r = e - s.
SVS_HD inline bool sa_cigar(const uint8_t* t, int64_t& i, int64_t end, SvSegment& g, int64_t& r) {
    int phase = 0, n_ops = 0;                    // 0 in the leading clips, 1 in the body, 2 in the trailing clips
    g.a = g.m = g.b = r = 0;
    while (i < end && t[i] >= '0' && t[i] <= '9') {
        int64_t n = 0;
        if (!sa_number(t, i, end, n) || n < 1 || n > kSaMaxCount || i >= end) return false;
        const uint8_t op = t[i++];
        ++n_ops;
        if (op == 'S' || op == 'H') {
            if (phase == 0) g.a += n; else { phase = 2; g.b += n; }
            continue;
        }
        if (phase == 2) return false;            // a clip inside the alignment
        phase = 1;
        if (op == 'M' || op == '=' || op == 'X') { g.m += n; r += n; }
        else if (op == 'I') g.m += n;
        else if (op == 'D' || op == 'N') r += n;
        else if (op != 'P') return false;
    }
    return n_ops >= 1 && g.m >= 1 && r >= 1;
}

// t[begin, end): one entry without its ';' -> the segment; ok = 0 for anything the grammar does not allow.  tid is not filled.
SVS_HD inline SvSegment parse_sa_entry(const uint8_t* t, int64_t begin, int64_t end) {
    SvSegment g{};
    g.tid = -1;
    int64_t i = begin;
    uint64_t hash = kFnvOffset;
    while (i < end && t[i] != ',') {
        hash = (hash ^ t[i]) * kFnvPrime;
        ++i;
    }
    g.hash = hash;
    if (i == begin || i >= end) return g;                                  // no rname, or nothing behind it
    ++i;
    int64_t pos = 0, r = 0, mapq = 0, nm = 0;
    if (!sa_number(t, i, end, pos) || pos < 1 || pos > kSaMaxPos || i >= end || t[i] != ',') return g;
    ++i;
    if (i >= end || (t[i] != '+' && t[i] != '-')) return g;
    g.strand = t[i] == '-' ? 1 : 0;
    ++i;
    if (i >= end || t[i] != ',') return g;
    ++i;
    if (!sa_cigar(t, i, end, g, r) || i >= end || t[i] != ',') return g;
    ++i;
    if (!sa_number(t, i, end, mapq) || mapq > 255 || i >= end || t[i] != ',') return g;
    ++i;
    if (!sa_number(t, i, end, nm) || i != end) return g;
    g.s = pos - 1;
    g.e = g.s + r;
    if (g.e > kSaMaxPos) return g;                                         // a breakpoint is a 32-bit column of the row
    g.mapq = (int32_t)mapq;
    sv_orient(g);
    g.ok = 1;
    return g;
}

// (qs, qe, order of appearance): the primary appears first.
SVS_HD inline bool sv_segment_before(const SvSegment& x, int ix, const SvSegment& y, int iy) {
    if (x.qs != y.qs) return x.qs < y.qs;
    if (x.qe != y.qe) return x.qe < y.qe;
    return ix < iy;
}

constexpr int kJunctionDropped = 0, kJunctionUnplaced = 1, kJunctionSmall = 2, kJunctionRow = 3;

struct SvJunction {
    int32_t outcome, type;
    int64_t pos, len, shift;                     // the row's columns; for a BND len is the mate's tid and shift its breakpoint
    int64_t bound;                               // > 0: a DEL to move to the left while j < bound
};

// A before B on the read, both of a read whose segments on chromosome `own` lie inside [0, length].
SVS_HD inline SvJunction sv_junction(const SvSegment& A, const SvSegment& B, int32_t own, int64_t length, int64_t min_size,
                                     int64_t flank, int32_t mapq_threshold) {
    SvJunction j{};
    j.outcome = kJunctionDropped;
    int64_t g = B.qs - A.qe;
    const int64_t overlap = g < 0 ? -g : 0;
    if (A.mapq < mapq_threshold || B.mapq < mapq_threshold || A.m < flank || B.m - overlap < flank) return j;
    const bool a_own = A.tid == own, b_own = B.tid == own;
    if (!a_own && !b_own) { j.outcome = kJunctionUnplaced; return j; }
    const int64_t x = A.strand ? A.s : A.e;
    int64_t y = B.strand ? B.e : B.s;
    if (a_own != b_own) {
        j.outcome = kJunctionRow;
        j.type = kSvBnd;
        j.pos = a_own ? x : y;
        j.len = a_own ? B.tid : A.tid;
        j.shift = a_own ? y : x;
        return j;
    }
    if (A.strand != B.strand) {
        j.type = A.strand ? kSvInv5 : kSvInv3;
        j.pos = x < y ? x : y;
        j.len = x < y ? y - x : x - y;
        j.outcome = j.len >= min_size ? kJunctionRow : kJunctionSmall;
        return j;
    }
    const bool forward = !A.strand;
    if (overlap) {                               // the overlap leaves B: its entry moves on, the trimmed bases counted as matches
        y += forward ? overlap : -overlap;
        g = 0;
        if (y < 0 || y > length) return j;       // it left the chromosome: dropped
    }
    const int64_t d = forward ? y - x : x - y, net = d - g, lower = x < y ? x : y;
    j.pos = lower;
    if (d <= -min_size) {
        j.type = kSvDup;
        j.len = -d;
    } else if (net >= min_size) {
        j.type = kSvDel;
        j.len = net;
        if (g == 0) {
            const int64_t room = lower - (forward ? A.s : B.s);
            j.bound = room > 0 ? room : 0;
        }
    } else if (net <= -min_size) {
        j.type = kSvIns;
        j.len = -net;
        if (j.len > kSaMaxPos) return j;         // more clipped bases than a 32-bit column holds: dropped
    } else {
        j.outcome = kJunctionSmall;
        return j;
    }
    j.outcome = kJunctionRow;
    return j;
}

// ---- the host side: one read's segments and rows, as sv_split_kernel computes them with a wave ------------------------------------
inline uint64_t sv_name_hash(const std::string& name) {
    uint64_t h = kFnvOffset;
    for (unsigned char c : name) h = (h ^ c) * kFnvPrime;
    return h;
}

struct SvSplitRead {
    uint8_t status = kSplitNone;
    int64_t junctions = 0, dropped = 0, small = 0, unplaced = 0;
    std::vector<SvSig> rows;
};

// The move to the left of 7p for a deletion of n bases at p: the greatest k <= bound with cond(j) for all j < k.
inline int64_t sv_left_shift_host(const uint8_t* ref, int64_t p, int64_t n, int64_t bound) {
    int64_t k = 0;
    while (k < bound && (ref[p - 1 - k] & 0xDF) == (ref[p - 1 - k + n] & 0xDF)) ++k;
    return k;
}

// `primary`: the read's own segment (tid = own); tag[0, n): its SA text, not empty; hashes[n_contigs]: of the contig names.
inline SvSplitRead sv_split_read(SvSegment primary, const uint8_t* tag, int64_t n, const uint64_t* hashes, int64_t n_contigs, int32_t own,
                                 const uint8_t* ref, int64_t length, int64_t min_size, int64_t flank, int32_t mapq_threshold,
                                 int64_t ordinal, uint8_t strand, uint8_t hp) {
    SvSplitRead out;
    out.status = kSplitBadSa;
    int64_t n_semi = 0;
    for (int64_t i = 0; i < n; ++i) n_semi += tag[i] == ';';
    if (n_semi >= kMaxSegments) { out.status = kSplitTooMany; return out; }
    if (n_semi == 0 || tag[n - 1] != ';') return out;
    SvSegment seg[kMaxSegments];
    int n_seg = 1;
    seg[0] = primary;
    const int64_t L = primary.a + primary.m + primary.b;
    if (!primary.ok || primary.e > length) return out;
    for (int64_t begin = 0, i = 0; i < n; ++i) {
        if (tag[i] != ';') continue;
        SvSegment g = parse_sa_entry(tag, begin, i);
        begin = i + 1;
        if (!g.ok || g.a + g.m + g.b != L) return out;
        for (int64_t c = 0; c < n_contigs; ++c)
            if (hashes[c] == g.hash) { g.tid = (int32_t)c; break; }
        if (g.tid == own && g.e > length) return out;
        seg[n_seg++] = g;
    }
    int order[kMaxSegments];
    for (int i = 0; i < n_seg; ++i) {
        int rank = 0;
        for (int k = 0; k < n_seg; ++k) rank += k != i && sv_segment_before(seg[k], k, seg[i], i);
        order[rank] = i;
    }
    out.status = kSplitParsed;
    for (int k = 0; k + 1 < n_seg; ++k) {
        const SvJunction j = sv_junction(seg[order[k]], seg[order[k + 1]], own, length, min_size, flank, mapq_threshold);
        ++out.junctions;
        out.dropped += j.outcome == kJunctionDropped;
        out.small += j.outcome == kJunctionSmall;
        out.unplaced += j.outcome == kJunctionUnplaced;
        if (j.outcome != kJunctionRow) continue;
        const int64_t moved = j.bound > 0 ? sv_left_shift_host(ref, j.pos, j.len, j.bound) : 0;
        SvSig g{};
        g.pos = j.pos - moved;
        g.ordinal = ordinal;
        g.op_index = -(int64_t)(k + 1);
        g.len = (int32_t)j.len;
        g.shift = j.type == kSvBnd ? (int32_t)j.shift : (int32_t)moved;
        g.type = (uint8_t)j.type;
        g.strand = strand;
        g.hp = hp;
        out.rows.push_back(g);
        out.status = kSplitRow;
    }
    return out;
}

}  // namespace
}  // namespace hello
