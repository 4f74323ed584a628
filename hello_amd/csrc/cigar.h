// What the host knows about a set of decoded BAM reads before a kernel may index with them: the CIGAR constants, the read filters
// and the validating walks of the BAM-side stages (strict_walk, counted_walk, and exact_walk under the duplicate marker's, the
// quality metrics', the methylation's, the pileup's and the large events').  Plain C++17 -- no HIP, no kernel -- so the walks also build into a
// stand-alone host program (tests/abi/cigar_check.cpp).  Refusals are thrown as Fail; the entry points turn them into a status.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hello_mi355x.h"

namespace hello {
namespace {

struct Fail {
    int code;
    std::string msg;
};
[[noreturn]] inline void raise(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    throw Fail{code, buf};
}

constexpr int BAM_CMATCH = 0, BAM_CINS = 1, BAM_CDEL = 2, BAM_CREF_SKIP = 3, BAM_CSOFT_CLIP = 4, BAM_CHARD_CLIP = 5, BAM_CPAD = 6,
              BAM_CEQUAL = 7, BAM_CDIFF = 8;

inline bool is_query_op(int op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }
inline bool is_ref_op(int op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }

inline bool usable(uint16_t flag, uint8_t mapq) {                  // is_usable_read, python/PileupContainer.py:33-41
    if (flag & (0x4 | 0x100 | 0x800 | 0x400)) return false;       // unmapped, secondary, supplementary, duplicate
    if ((flag & 0x1) && !(flag & 0x2)) return false;               // paired but not a proper pair
    return mapq > 0;                                               // QC-fail reads stay
}

// The reads the reference blocks and the phasing count: usable, not QC-fail, at or above the mapping-quality threshold.
inline bool counted(uint16_t flag, uint8_t mapq, int mapq_threshold) {
    return usable(flag, mapq) && !(flag & 0x200) && (int)mapq >= mapq_threshold;
}

// The sixteen BAM base codes as a table (byte 0 is none).  Every base of every usable read is checked, which is most of the strict
// walk's time: as a memchr call per base the walk took 85 - 95 ms for 200 k reads of 150 bases, a tenth more or less with the
// registers the surrounding function left the loop; with the table 24 ms.
struct BaseCodes {
    bool is[256] = {};
    constexpr BaseCodes() {
        for (const char* p = "=ACMGRSVTWYHKDBN"; *p; ++p) is[(unsigned char)*p] = true;
    }
};
constexpr BaseCodes kBaseCodes;

// The ten per-read inputs of an entry point.  `flags` == nullptr: a derived set (clipped copies), every read of which is used.
struct ReadsView {
    const uint8_t* bases = nullptr; const uint8_t* quals = nullptr; const int64_t* read_off = nullptr;
    const uint32_t* cigars = nullptr; const int64_t* cigar_off = nullptr; const int64_t* ref_start = nullptr;
    const int64_t* ref_end = nullptr; const uint8_t* mapq = nullptr; const uint16_t* flags = nullptr;
    const uint64_t* name_hash = nullptr;
    int64_t n = 0;
};

// What the strict walk learns about every read as a whole (Read::_get_read_mapping, Read.cpp:4-77).
struct ReadLayout {
    std::vector<int64_t> plant_off, plant, last_pos;    // planting positions (pos - 1) of the I/D operations; last M/D position or -1
    std::vector<uint8_t> pflags;                        // 1 partial_start, 2 partial_stop (Read.cpp:42-49)
    int64_t max_span[2] = {0, 0};                       // the longest reference span of a used read, per read set
};

enum StrictMode {
    kStrictPlain,       // the hotspot stage: a soft clip may sit anywhere
    kStrictRegions,     // the candidate stage: a soft clip between aligned operations would split a region's read bytes
    kStrictClipInput,   // reads about to be clipped: that refusal waits for the clipped CIGARs; what the clip kernels rely on instead
};

// Validation of every usable read (the kernels read within its bases) and its layout.  `origin`: the input read a derived read
// is named by in a refusal.  `source` (one byte per read, below n_sets): the reads of several sets interleaved, each set sorted.
inline void strict_walk(const ReadsView& s, StrictMode mode, ReadLayout& out, const int64_t* origin = nullptr,
                        const uint8_t* source = nullptr, int n_sets = 1) {
    int64_t last_start[2] = {INT64_MIN, INT64_MIN};
    out.max_span[0] = out.max_span[1] = 0;
    out.plant_off.assign((size_t)s.n + 1, 0);
    out.plant.clear();
    out.last_pos.assign((size_t)s.n, -1);
    out.pflags.assign((size_t)s.n, 0);
    for (int64_t r = 0; r < s.n; ++r) {
        out.plant_off[r + 1] = out.plant_off[r];
        if (source && source[r] >= n_sets) raise(HELLO_ERR_ARG, "source[%lld] = %d with %d read set(s)", (long long)r, source[r], n_sets);
        const int set = source ? source[r] : 0;
        if (s.flags && s.ref_start[r] < last_start[set])
            raise(HELLO_ERR_ARG, "read %lld: reads are not coordinate-sorted (the BAM must be)", (long long)r);
        last_start[set] = s.ref_start[r];
        if (s.read_off[r + 1] < s.read_off[r] || s.cigar_off[r + 1] < s.cigar_off[r])
            raise(HELLO_ERR_SHAPE, "read %lld: offsets decrease", (long long)r);
        if (s.flags && !usable(s.flags[r], s.mapq[r])) continue;
        int64_t qlen = 0, rlen = 0;
        const int64_t c0 = s.cigar_off[r], c1 = s.cigar_off[r + 1];
        bool prev = false, aligned = false;
        for (int64_t c = c0; c < c1; ++c) {
            const int op = s.cigars[c] & 15;
            const int64_t len = s.cigars[c] >> 4;
            if (op > 8) raise(HELLO_ERR_ARG, "read %lld: CIGAR operation %d", (long long)r, op);
            if (len == 0) raise(HELLO_ERR_ARG, "read %lld: zero-length CIGAR operation", (long long)r);
            if (op == 1 || op == 2) out.plant.push_back(s.ref_start[r] + rlen - 1);   // rfcounter - 1 (:221,247)
            if (is_query_op(op)) qlen += len;
            if (is_ref_op(op)) rlen += len;
            if (op == 0 || op == 2 || op == 7 || op == 8) { out.last_pos[r] = s.ref_start[r] + rlen - 1; prev = true; aligned = true; }
            else if (op == 3) prev = false;
            else if (op == 1) {
                if (!prev) out.pflags[r] |= 1;
                else if (c == c1 - 1) out.pflags[r] |= 2;
                prev = true;
                aligned = true;
            } else if (op == 4 && aligned && mode == kStrictRegions) {
                for (int64_t k = c + 1; k < c1; ++k)
                    if ((s.cigars[k] & 15) != 4 && (s.cigars[k] & 15) != 5)
                        raise(HELLO_ERR_ARG, "read %lld: a soft clip between aligned operations", (long long)(origin ? origin[r] : r));
            }
        }
        out.plant_off[r + 1] = (int64_t)out.plant.size();
        if (mode == kStrictClipInput && rlen == 0) raise(HELLO_ERR_ARG, "read %lld: no CIGAR operation on the reference", (long long)r);
        if (qlen != s.read_off[r + 1] - s.read_off[r])
            raise(HELLO_ERR_SHAPE, "read %lld: CIGAR query length %lld, %lld bases", (long long)r, (long long)qlen,
                  (long long)(s.read_off[r + 1] - s.read_off[r]));
        if (s.ref_start[r] < 0 || s.ref_end[r] != s.ref_start[r] + std::max<int64_t>(rlen, 1))
            raise(HELLO_ERR_SHAPE, "read %lld: ref_end does not match its CIGAR", (long long)r);
        if (s.flags)
            for (int64_t i = s.read_off[r]; i < s.read_off[r + 1]; ++i)
                if (!kBaseCodes.is[s.bases[i]])
                    raise(HELLO_ERR_ARG, "read %lld: base '%c' is not a BAM base code", (long long)r, s.bases[i]);
        out.max_span[set] = std::max(out.max_span[set], s.ref_end[r] - s.ref_start[r]);
    }
}

// One read of the counted walk: false when the read is not counted; else its query and reference length from the CIGAR, refused
// when the CIGAR consumes more bases than the read has (the kernels read within them).
inline bool counted_walk(const ReadsView& s, int64_t r, int mapq_threshold, int64_t& qlen, int64_t& rlen) {
    if (s.read_off[r + 1] < s.read_off[r] || s.cigar_off[r + 1] < s.cigar_off[r])
        raise(HELLO_ERR_SHAPE, "read %lld: offsets decrease", (long long)r);
    if (!counted(s.flags[r], s.mapq[r], mapq_threshold)) return false;
    qlen = rlen = 0;
    for (int64_t c = s.cigar_off[r]; c < s.cigar_off[r + 1]; ++c) {
        const int op = s.cigars[c] & 15;
        const int64_t len = s.cigars[c] >> 4;
        if (is_query_op(op)) qlen += len;
        if (is_ref_op(op)) rlen += len;
    }
    if (qlen > s.read_off[r + 1] - s.read_off[r])
        raise(HELLO_ERR_ARG, "read %lld: its CIGAR consumes %lld bases, it has %lld", (long long)r, (long long)qlen,
              (long long)(s.read_off[r + 1] - s.read_off[r]));
    return true;
}

// Where a read set begins and how read r follows read r - 1: the offsets start at 0 and do not decrease, and (`sorted`) the reads
// are in coordinate order.
inline void check_read_order(const ReadsView& s, int64_t r, bool sorted) {
    if (r == 0 && (s.read_off[0] != 0 || s.cigar_off[0] != 0)) raise(HELLO_ERR_ARG, "offsets do not start at 0");
    if (s.read_off[r + 1] < s.read_off[r] || s.cigar_off[r + 1] < s.cigar_off[r])
        raise(HELLO_ERR_ARG, "read %lld: offsets decrease", (long long)r);
    if (sorted && r > 0 && s.ref_start[r] < s.ref_start[r - 1])
        raise(HELLO_ERR_ARG, "read %lld: reads are not coordinate-sorted (the BAM must be)", (long long)r);
}

// What a kernel that walks read r's CIGAR over its bases relies on: known operations, a CIGAR that consumes exactly the read's
// bases and ends where ref_end says.  -> the query and reference length and whether an operation is a hard clip.
struct ExactWalk {
    int64_t qlen = 0, rlen = 0;
    bool hard_clipped = false;
};
inline ExactWalk exact_walk(const ReadsView& s, int64_t r) {
    ExactWalk w;
    for (int64_t c = s.cigar_off[r]; c < s.cigar_off[r + 1]; ++c) {
        const int op = s.cigars[c] & 15;
        const int64_t len = s.cigars[c] >> 4;
        if (op > 8) raise(HELLO_ERR_ARG, "read %lld: CIGAR operation %d", (long long)r, op);
        if (op == BAM_CHARD_CLIP) w.hard_clipped = true;
        if (is_query_op(op)) w.qlen += len;
        if (is_ref_op(op)) w.rlen += len;
    }
    if (w.qlen != s.read_off[r + 1] - s.read_off[r])
        raise(HELLO_ERR_ARG, "read %lld: CIGAR query length %lld, %lld bases", (long long)r, (long long)w.qlen,
              (long long)(s.read_off[r + 1] - s.read_off[r]));
    if (s.ref_end[r] != s.ref_start[r] + std::max<int64_t>(w.rlen, 1))
        raise(HELLO_ERR_ARG, "read %lld: ref_end does not match its CIGAR", (long long)r);
    return w;
}

// exact_walk for a read of a span-wise stage, which also needs the read to start on the reference and to have at most
// `max_bases` bases.
inline ExactWalk exact_walk_on_reference(const ReadsView& s, int64_t r, int64_t max_bases) {
    if (s.ref_start[r] < 0) raise(HELLO_ERR_ARG, "read %lld: ref_start %lld", (long long)r, (long long)s.ref_start[r]);
    const ExactWalk w = exact_walk(s, r);
    if (w.qlen > max_bases)
        raise(HELLO_ERR_ARG, "read %lld: %lld bases, at most %lld", (long long)r, (long long)w.qlen, (long long)max_bases);
    return w;
}

// The reads that take part in duplicate marking: mapped, primary, not a duplicate already; mapq, QC-fail and
// the pairing flags do not matter.
inline bool markdup_eligible(uint16_t flag) { return !(flag & (0x4 | 0x100 | 0x800 | 0x400)); }

// The walk of the duplicate marker: every read's offsets and, for an eligible read, what the ends kernel relies on (exact_walk).
// -> the eligible reads, in input order.
inline std::vector<int64_t> markdup_walk(const ReadsView& s) {
    std::vector<int64_t> list;
    for (int64_t r = 0; r < s.n; ++r) {
        check_read_order(s, r, false);
        if (!markdup_eligible(s.flags[r])) continue;
        exact_walk(s, r);
        list.push_back(r);
    }
    return list;
}

// The reads the quality metrics measure: mapped, primary, not a duplicate, not QC-fail; mapq and the pairing
// flags do not matter.
constexpr int kQcNotMeasured = 0x4 | 0x100 | 0x800 | 0x400 | 0x200;
inline bool qc_measured(uint16_t flag) { return !(flag & kQcNotMeasured); }

constexpr uint8_t kQcBelongs = 1, kQcMeasured = 2, kQcCounted = 4;
constexpr int64_t kQcMaxReadBases = (int64_t(1) << 31) / 255;      // a read's qualities sum below 2^31

// The walk of the quality metrics over the reads overlapping a span that starts at `lo`: every read's offsets and order and, for a
// measured or counted read, what the kernels rely on (exact_walk_on_reference; the bound keeps a quality sum inside an int32).
// -> per read kQcBelongs | kQcMeasured | kQcCounted.
inline std::vector<uint8_t> qc_walk(const ReadsView& s, int64_t lo, int mapq_threshold) {
    std::vector<uint8_t> kind((size_t)s.n, 0);
    for (int64_t r = 0; r < s.n; ++r) {
        check_read_order(s, r, true);
        uint8_t k = s.ref_start[r] >= lo ? kQcBelongs : 0;
        if (qc_measured(s.flags[r])) k |= kQcMeasured;
        if (counted(s.flags[r], s.mapq[r], mapq_threshold)) k |= kQcCounted;
        kind[(size_t)r] = k;
        if (k & (kQcMeasured | kQcCounted)) exact_walk_on_reference(s, r, kQcMaxReadBases);
    }
    return kind;
}

constexpr uint8_t kMethBelongs = 1, kMethCounted = 2, kMethHardClipped = 4;
constexpr int64_t kMethMaxReads = (int64_t(1) << 31) / 255;        // counting reads of one handle: its 32-bit sums stay below 2^31

// The walk of the methylation stage over the reads overlapping a span that starts at `lo`: every read's
// offsets and order and, for a counted read, what the kernels rely on (exact_walk_on_reference).  -> per read kMethBelongs |
// kMethCounted | kMethHardClipped.
inline std::vector<uint8_t> meth_walk(const ReadsView& s, int64_t lo, int mapq_threshold) {
    std::vector<uint8_t> kind((size_t)s.n, 0);
    for (int64_t r = 0; r < s.n; ++r) {
        check_read_order(s, r, true);
        uint8_t k = s.ref_start[r] >= lo ? kMethBelongs : 0;
        if (counted(s.flags[r], s.mapq[r], mapq_threshold))
            k |= kMethCounted | (exact_walk_on_reference(s, r, INT32_MAX).hard_clipped ? kMethHardClipped : 0);
        kind[(size_t)r] = k;
    }
    return kind;
}

constexpr uint8_t kPileBelongs = kMethBelongs, kPileCounted = kMethCounted;
constexpr int64_t kPileMaxReads = INT32_MAX;                       // counting reads of one handle: a read adds at most 1 to a counter

// The walk of the pileup at sites: what meth_walk checks and refuses, in its words -- the kernels rely on
// the same things.  A hard clip consumes nothing and is no cause to leave a read out.  -> per read kPileBelongs | kPileCounted.
inline std::vector<uint8_t> pileup_walk(const ReadsView& s, int64_t lo, int mapq_threshold) {
    std::vector<uint8_t> kind = meth_walk(s, lo, mapq_threshold);
    for (uint8_t& k : kind) k &= kPileBelongs | kPileCounted;
    return kind;
}

// The walk of the large deletions and insertions: pileup_walk's classes and refusals, unchanged, and on top
// of them the walk list -- the counting, belonging reads with an I or D operation of at least `min_size` bases, in input order --
// and the count of those operations, which no count of signatures exceeds: the kernel's output buffer is sized with it.
struct SvWalk {
    std::vector<uint8_t> kind;       // per read kPileBelongs | kPileCounted
    std::vector<int64_t> walk;
    int64_t n_ops = 0;
};
inline SvWalk sv_walk(const ReadsView& s, int64_t lo, int mapq_threshold, int64_t min_size) {
    SvWalk w;
    w.kind = pileup_walk(s, lo, mapq_threshold);
    for (int64_t r = 0; r < s.n; ++r) {
        if (w.kind[(size_t)r] != (kPileBelongs | kPileCounted)) continue;
        int64_t n = 0;
        for (int64_t c = s.cigar_off[r]; c < s.cigar_off[r + 1]; ++c) {
            const int op = s.cigars[c] & 15;
            if ((op == BAM_CINS || op == BAM_CDEL) && (int64_t)(s.cigars[c] >> 4) >= min_size) ++n;
        }
        if (n) w.walk.push_back(r);
        w.n_ops += n;
    }
    return w;
}

}  // namespace
}  // namespace hello
