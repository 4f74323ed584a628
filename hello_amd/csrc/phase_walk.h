// What one read shows at the records of one round: the walk both the phasing stage (phase.hip) and the
// haplotag stage (haplotag.hip) run, in one copy.  The lanes of a wave hold up to 64 candidate records of ONE read; the walk over
// the CIGAR is wave-uniform (one operation at a time, the same for all lanes, ended once every lane's record lies behind the
// cursor), and a lane only has work where an operation meets its own span -- it compares the bases it would append with both
// alleles as it goes, so no string is stored.
#pragma once
#include <hip/hip_runtime.h>

#include "cigar.h"

namespace hello {
namespace {

struct PhWalkRead {              // one counted read, validated on the host: its CIGAR stays within its bases
    const uint8_t* bases;
    const uint8_t* quals;
    const uint32_t* cigars;
    int64_t n_ops;
    int64_t ref_start, ref_end;  // ref_end from the CIGAR (the host's counted walk)
};

struct PhWalkTable {             // the records of one chromosome
    const int64_t* rec_start;    // [records], sorted
    const int64_t* rec_end;
    const uint8_t* alleles;      // allele a then allele b of every record, upper case
    const int64_t* allele_off;   // [2 records + 1]
};

// -1, 0 (allele a) or 1 (allele b): what the read shows at record `t`; `mine` false: the lane holds no record and returns -1.
// Holds a wave-wide vote: EVERY lane of the wave calls it, with the same read, whatever `mine` says.
__device__ inline int phase_walk_observe(const PhWalkRead& rd, const PhWalkTable& tb, int64_t t, bool mine, int q_threshold) {
    int64_t A = 0, B = 0, la = 0, lb = 0;
    const uint8_t* al_a = tb.alleles;
    const uint8_t* al_b = tb.alleles;
    if (mine) {
        A = tb.rec_start[t];
        B = tb.rec_end[t];
        const int64_t o0 = tb.allele_off[2 * t], o1 = tb.allele_off[2 * t + 1], o2 = tb.allele_off[2 * t + 2];
        al_a += o0;
        al_b += o1;
        la = o1 - o0;
        lb = o2 - o1;
    }
    bool dead = !mine || !(B < rd.ref_end);                               // the base behind the span must be aligned
    bool ma = true, mb = true;
    int64_t len = 0;
    int minq = 255;
    auto append = [&](int64_t i) {
        const unsigned char c = rd.bases[i] & 0xDF;
        const int q = rd.quals[i];
        ma = ma && len < la && al_a[len] == c;
        mb = mb && len < lb && al_b[len] == c;
        minq = q < minq ? q : minq;
        ++len;
    };
    int64_t rf = rd.ref_start, rp = 0;
    for (int64_t ci = 0; ci < rd.n_ops; ++ci) {
        if (!__any(!dead && rf <= B)) break;                              // every lane's span lies behind the cursor
        const unsigned c = rd.cigars[ci];
        const int op = c & 15u;
        const int64_t n = c >> 4;
        if (op == BAM_CMATCH || op == BAM_CEQUAL || op == BAM_CDIFF) {
            if (!dead) {
                const int64_t j0 = A > rf ? A - rf : 0, j1 = B - rf < n ? B - rf : n;
                for (int64_t i = j0; i < j1 && (ma || mb); ++i) append(rp + i);
            }
            rf += n;
            rp += n;
        } else if (op == BAM_CINS) {
            if (!dead && rf - 1 >= A && rf - 1 < B)
                for (int64_t i = 0; i < n && (ma || mb); ++i) append(rp + i);
            rp += n;
        } else if (op == BAM_CDEL) {
            rf += n;
        } else if (op == BAM_CREF_SKIP) {
            if (rf < B && rf + n > A) dead = true;
            rf += n;
        } else if (op == BAM_CSOFT_CLIP) {
            rp += n;
        }
    }
    int o = -1;
    if (!dead && minq >= q_threshold) {
        if (ma && len == la) o = 0;
        else if (mb && len == lb) o = 1;
    }
    return o;
}

}  // namespace
}  // namespace hello
