// The contamination stage's host code (hello_amd/csrc/cigar.h: pileup_walk; contam.h: the error rate, the likelihood grid, the
// interval and the LOD) over good, malformed and degenerate inputs, as a stand-alone host program in the style of mods_check.cpp:
// built by tests/test_contamination.py with -fsanitize=address,undefined and run directly.  Every input is an exactly sized heap
// array, so a walk or a sum that leaves it is caught.  Exits non-zero on the first mismatch.
#include <cmath>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../hello_amd/csrc/cigar.h"
#include "../../hello_amd/csrc/contam.h"

using namespace hello;

namespace {

int failures = 0;
#define EXPECT(cond)                                                                        \
    do {                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

struct Set {
    std::vector<uint8_t> quals, mapq;
    std::vector<int64_t> read_off{0}, cigar_off{0}, ref_start, ref_end;
    std::vector<uint32_t> cigars;
    std::vector<uint16_t> flags;
    void add(int64_t start, const std::vector<std::pair<int, int>>& cigar, uint16_t flag = 0, int mq = 60, int64_t n_bases = -1,
             int64_t end_shift = 0) {
        int64_t q = 0, r = 0;
        for (const auto& c : cigar) {
            cigars.push_back((uint32_t)c.first << 4 | (uint32_t)c.second);
            if (is_query_op(c.second)) q += c.first;
            if (is_ref_op(c.second)) r += c.first;
        }
        if (n_bases < 0) n_bases = q;
        quals.insert(quals.end(), (size_t)n_bases, 30);
        read_off.push_back((int64_t)quals.size());
        cigar_off.push_back((int64_t)cigars.size());
        ref_start.push_back(start);
        ref_end.push_back(start + (r > 0 ? r : 1) + end_shift);
        flags.push_back(flag);
        mapq.push_back((uint8_t)mq);
    }
    ReadsView view() const {
        return ReadsView{nullptr, quals.data(), read_off.data(), cigars.data(), cigar_off.data(), ref_start.data(), ref_end.data(),
                         mapq.data(), flags.data(), nullptr, (int64_t)ref_start.size()};
    }
};

struct Walk { std::string refusal; std::vector<uint8_t> kind; };
Walk walk(const Set& s, int64_t lo = 0, int mapq_threshold = 10) {
    Walk w;
    try { w.kind = pileup_walk(s.view(), lo, mapq_threshold); } catch (const Fail& f) { w.refusal = std::to_string(f.code) + " " + f.msg; }
    return w;
}

const std::string kArg = std::to_string(HELLO_ERR_ARG) + " ";
constexpr int M = 0, I = 1, D = 2, S = 4, H = 5;
constexpr uint8_t B = kPileBelongs, C = kPileCounted;

using Counts = std::vector<int64_t>;

struct Estimate { double e; int k, lo, hi; std::vector<double> ll; bool finite; };
Estimate estimate(const Counts& r, const Counts& a, const Counts& o, const std::vector<double>& af, int threads = 0) {
    std::vector<double> out(HELLO_CONTAM_OUT, -1.0);                       // exactly sized
    contam_estimate(r.data(), a.data(), o.data(), af.data(), (int64_t)r.size(), out.data(), threads);
    Estimate got{out[0], (int)out[1], (int)out[2], (int)out[3], std::vector<double>(out.begin() + 4, out.end()), true};
    for (double v : out) got.finite = got.finite && std::isfinite(v);
    return got;
}

}  // namespace

int main() {
    // ---- pileup_walk: the classes, and the refusals in meth_walk's words
    {
        Set s;
        s.add(5, {{10, M}});                                         // starts below lo = 8
        s.add(8, {{10, M}});
        s.add(9, {{10, M}}, 0x400);
        s.add(10, {{10, M}}, 0, 9);                                  // below the threshold
        s.add(11, {{10, M}}, 0x41);                                  // paired, not proper
        s.add(12, {{2, H}, {3, S}, {4, M}, {1, I}, {2, D}, {2, M}, {1, S}});      // a hard clip is no cause to leave a read out
        s.add(13, {{5, 9}}, 0x100);                                  // not counted: its CIGAR may say anything
        s.add(14, {});                                               // no CIGAR
        const Walk w = walk(s, 8);
        EXPECT(w.refusal == "");
        EXPECT((w.kind == std::vector<uint8_t>{C, (uint8_t)(B | C), B, B, B, (uint8_t)(B | C), B, (uint8_t)(B | C)}));
        Set t;
        t.add(0, {{5, M}}, 0, 60, 4);
        EXPECT(walk(t).refusal == kArg + "read 0: CIGAR query length 5, 4 bases");
        t = Set();
        t.add(0, {{5, M}}, 0, 60, 6);
        EXPECT(walk(t).refusal == kArg + "read 0: CIGAR query length 5, 6 bases");
        t = Set();
        t.add(0, {{3, M}, {2, 9}});
        EXPECT(walk(t).refusal == kArg + "read 0: CIGAR operation 9");
        t = Set();
        t.add(0, {{4, M}}, 0, 60, -1, 1);
        EXPECT(walk(t).refusal == kArg + "read 0: ref_end does not match its CIGAR");
        t = Set();
        t.add(-1, {{4, M}});
        EXPECT(walk(t, -4).refusal == kArg + "read 0: ref_start -1");
        t = Set();
        t.add(7, {{4, M}});
        t.add(6, {{4, M}});
        EXPECT(walk(t).refusal == kArg + "read 1: reads are not coordinate-sorted (the BAM must be)");
        t = Set();
        t.add(0, {{4, M}});
        t.add(1, {{4, M}});
        Set u = t;
        u.read_off[2] = 3;
        EXPECT(walk(u).refusal == kArg + "read 1: offsets decrease");
        u = t;
        u.cigar_off[0] = 1;
        EXPECT(walk(u).refusal == kArg + "offsets do not start at 0");
        EXPECT(walk(Set()).refusal == "" && walk(Set()).kind.empty());
    }
    // ---- the error rate
    {
        const Counts none;
        EXPECT(contam_error_rate(none.data(), none.data(), none.data(), 0) == 1e-4);
        const Counts zero{0, 0};
        EXPECT(contam_error_rate(zero.data(), zero.data(), zero.data(), 2) == 1e-4);
        const Counts r{90, 0}, a{0, 90}, o{10, 10};                  // 1.5 * 20 / 200 = 0.15: clamped
        EXPECT(contam_error_rate(r.data(), a.data(), o.data(), 2) == 0.1);
        const Counts o2{1, 1};                                       // 1.5 * 2 / 182
        EXPECT(contam_error_rate(r.data(), a.data(), o2.data(), 2) == 1.5 * 2.0 / 182.0);
    }
    // ---- the grid, the interval and the LOD on the degenerate inputs: all finite
    {
        Estimate e = estimate({}, {}, {}, {});                       // no sites: a flat curve
        EXPECT(e.finite && e.e == 1e-4 && e.k == 0 && e.lo == 0 && e.hi == 500 && e.ll[0] == 0.0 && e.ll[500] == 0.0);
        e = estimate({0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0.1, 0.5, 0.9});       // all counts zero
        EXPECT(e.finite && e.k == 0 && e.lo == 0 && e.hi == 500 && e.ll[250] == 0.0);
        e = estimate({30}, {0}, {0}, {0.3});                         // one site
        EXPECT(e.finite && e.lo <= e.k && e.k <= e.hi && e.ll[e.k] < 0.0);
        const int64_t big = 2147483647;
        e = estimate({big, 0, big}, {0, big, big}, {0, 0, 7}, {0.5, 0.5, 0.5});   // a count of 2^31 - 1
        EXPECT(e.finite && e.lo <= e.k && e.k <= e.hi);
        e = estimate({30, 0, 12}, {0, 30, 14}, {0, 1, 0}, {1e-6, 1.0 - 1e-6, 0.5});     // AF at both ends
        EXPECT(e.finite && e.lo <= e.k && e.k <= e.hi);
        // a mixture of a fifth at depth 30: homozygous sites beside a contaminant of 0, 1 and 2 other copies, and heterozygous
        // ones.  The curve peaks at k = 200 inside the grid, the same for every thread count
        const int pattern[8][2] = {{30, 0}, {27, 3}, {24, 6}, {15, 15}, {0, 30}, {3, 27}, {6, 24}, {15, 15}};
        Counts r, a, o;
        std::vector<double> af;
        for (int i = 0; i < 40; ++i) {
            r.push_back(pattern[i % 8][0]); a.push_back(pattern[i % 8][1]); o.push_back(0); af.push_back(0.5);
        }
        const Estimate one = estimate(r, a, o, af, 1), four = estimate(r, a, o, af, 4), many = estimate(r, a, o, af, 7);
        EXPECT(one.finite && one.k == 200 && one.lo > 100 && one.lo < one.k && one.k < one.hi && one.hi < 300);
        EXPECT(one.ll == four.ll && one.ll == many.ll && one.k == four.k && one.lo == many.lo && one.hi == many.hi);
    }
    {
        std::vector<double> out(2, -1.0);
        const Counts none;
        const std::vector<double> no_af;
        contam_identity(none.data(), none.data(), none.data(), none.data(), none.data(), none.data(), no_af.data(), 0, out.data());
        EXPECT(out[0] == 0.0 && out[1] == 0.0);
        const Counts z{0, 0}, r{30, 0}, a{0, 30};
        const std::vector<double> af{0.3, 0.3};
        contam_identity(r.data(), a.data(), z.data(), z.data(), z.data(), z.data(), af.data(), 2, out.data());      // nothing in BAM 2
        EXPECT(out[0] == 0.0 && out[1] == 0.0);
        contam_identity(r.data(), a.data(), z.data(), r.data(), a.data(), z.data(), af.data(), 2, out.data());      // the same genotypes
        EXPECT(std::isfinite(out[0]) && out[0] > 0.0 && out[1] == 2.0);
        contam_identity(r.data(), a.data(), z.data(), a.data(), r.data(), z.data(), af.data(), 2, out.data());      // opposite ones
        EXPECT(std::isfinite(out[0]) && out[0] < 0.0 && out[1] == 2.0);
        const int64_t big = 2147483647;
        const Counts rb{big}, ab{big}, ob{0};
        const std::vector<double> edge{1e-6};
        contam_identity(rb.data(), ab.data(), ob.data(), rb.data(), ab.data(), ob.data(), edge.data(), 1, out.data());
        EXPECT(std::isfinite(out[0]) && out[1] == 1.0);
        const std::vector<double> other{1.0 - 1e-6};
        contam_identity(rb.data(), ob.data(), ob.data(), ob.data(), ab.data(), ob.data(), other.data(), 1, out.data());
        EXPECT(std::isfinite(out[0]) && out[0] < 0.0);
    }
    if (failures) {
        std::fprintf(stderr, "%d mismatches\n", failures);
        return 1;
    }
    std::puts("contam_check: ok");
    return 0;
}
