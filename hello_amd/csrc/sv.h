// The host rules of the large deletions and insertions: what a signature is as a record, the order the
// SIGNATURES arrays are handed out in, the clusters and the genotype.  Plain C++17 -- no HIP, no kernel -- so the rules also build
// into a stand-alone host program (tests/abi/sv_check.cpp).  hello_amd/sv.py restates them in Python, integer for integer.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <tuple>
#include <vector>

namespace hello {
namespace {

constexpr int kSvDel = 0, kSvIns = 1;
constexpr int kSvClustered = 5;      // the types below it are clustered: DEL, INS and the three of the split alignments (sv_split.h)

struct SvSig {                       // one I or D operation of a read, left-aligned: what sv_reads_kernel writes
    int64_t pos, ordinal, op_index;
    int32_t len, shift;
    uint8_t type, strand, hp, pad;
};

inline auto sv_key(const SvSig& s) { return std::make_tuple(s.type, s.pos, s.len, s.ordinal, s.op_index); }

// (type, pos, len, ordinal, operation index): a read's operation has one key, so the order is total.
inline void sv_sort(std::vector<SvSig>& sigs) {
    std::sort(sigs.begin(), sigs.end(), [](const SvSig& a, const SvSig& b) { return sv_key(a) < sv_key(b); });
}

constexpr int kSvCandidateColumns = 13;
struct SvCandidate {
    int64_t type, pos, len, dv, dv_fwd, dv_rev, hp[3], pos_min, pos_max, len_min, len_max;
    int64_t sr;                      // the distinct reads with a row of a split alignment (operation index below 0): section 7q
};

// One group of signatures, ordered by (len, pos, ordinal, operation index) -> a candidate when its distinct reads number at least
// min_support.  A read's strand and hp are the same in all its signatures, so the first of each ordinal stands for the read.
inline void sv_group(const SvSig* g, size_t m, int64_t min_support, std::vector<SvCandidate>& out) {
    std::vector<int64_t> pos(m);
    std::vector<std::tuple<int64_t, int, int, int>> reads(m);    // a read's split rows sort before its others
    for (size_t i = 0; i < m; ++i) {
        pos[i] = g[i].pos;
        reads[i] = std::make_tuple(g[i].ordinal, g[i].op_index < 0 ? 0 : 1, (int)g[i].strand, g[i].hp == 1 || g[i].hp == 2 ? (int)g[i].hp : 0);
    }
    std::sort(reads.begin(), reads.end());
    std::sort(pos.begin(), pos.end());
    SvCandidate c{};
    for (size_t i = 0; i < m; ++i) {
        if (i > 0 && std::get<0>(reads[i]) == std::get<0>(reads[i - 1])) continue;
        ++c.dv;
        c.sr += std::get<1>(reads[i]) == 0;
        ++(std::get<2>(reads[i]) ? c.dv_rev : c.dv_fwd);
        ++c.hp[std::get<3>(reads[i])];
    }
    if (c.dv < min_support) return;
    c.type = g[0].type;
    c.pos = pos[(m - 1) / 2];
    c.len = g[(m - 1) / 2].len;              // the group is ordered by len first
    c.pos_min = pos.front();
    c.pos_max = pos.back();
    c.len_min = g[0].len;
    c.len_max = g[m - 1].len;
    out.push_back(c);
}

// `sigs` in sv_sort's order -> the candidates, sorted by (pos, type, len).
inline std::vector<SvCandidate> sv_cluster(const std::vector<SvSig>& sigs, int64_t cluster_gap, int64_t len_ratio_percent,
                                           int64_t min_support) {
    std::vector<SvCandidate> out;
    std::vector<SvSig> run;
    size_t i = 0;
    while (i < sigs.size() && sigs[i].type < kSvClustered) {
        size_t j = i + 1;
        while (j < sigs.size() && sigs[j].type == sigs[i].type && sigs[j].pos - sigs[j - 1].pos <= cluster_gap) ++j;
        run.assign(sigs.begin() + (ptrdiff_t)i, sigs.begin() + (ptrdiff_t)j);
        std::sort(run.begin(), run.end(), [](const SvSig& a, const SvSig& b) {
            return std::make_tuple(a.len, a.pos, a.ordinal, a.op_index) < std::make_tuple(b.len, b.pos, b.ordinal, b.op_index);
        });
        size_t g0 = 0;
        for (size_t k = 0; k < run.size(); ++k) {
            if (k + 1 == run.size() || 100 * (int64_t)run[k].len < len_ratio_percent * (int64_t)run[k + 1].len) {
                sv_group(run.data() + g0, k + 1 - g0, min_support, out);
                g0 = k + 1;
            }
        }
        i = j;
    }
    std::sort(out.begin(), out.end(), [](const SvCandidate& a, const SvCandidate& b) {
        return std::make_tuple(a.pos, a.type, a.len) < std::make_tuple(b.pos, b.type, b.len);
    });
    return out;
}

constexpr int kSvGenotypeColumns = 5;       // GT (0, 1, 2 for 0/0, 0/1, 1/1), GQ, PL of 0/0, 0/1, 1/1
constexpr double kSvEpsilon = 0.05;

// A supporter with a split row ends at the breakpoint and is not among the spanning reads (section 7q); with sr = 0 this is 7p's.
inline int64_t sv_depth_ref(int64_t dp, int64_t dv, int64_t sr = 0) { return std::max<int64_t>(0, dp - (dv - sr)); }

// DV reads that show the event and DR that span it without -> out[kSvGenotypeColumns].
inline void sv_genotype(int64_t dv, int64_t dr, int64_t* out) {
    const double f[3] = {kSvEpsilon, 0.5, 1.0 - kSvEpsilon};
    double l[3];
    int best = 0;
    for (int g = 0; g < 3; ++g) {
        l[g] = (double)dv * std::log10(f[g]) + (double)dr * std::log10(1.0 - f[g]);
        if (l[g] > l[best]) best = g;        // the first greatest
    }
    int64_t pl[3];
    for (int g = 0; g < 3; ++g) pl[g] = (int64_t)std::floor(-10.0 * (l[g] - l[best]) + 0.5);
    int64_t sorted[3] = {pl[0], pl[1], pl[2]};
    std::sort(sorted, sorted + 3);
    out[0] = best;
    out[1] = std::min<int64_t>(sorted[1], 99);
    out[2] = pl[0];
    out[3] = pl[1];
    out[4] = pl[2];
}

}  // namespace
}  // namespace hello
