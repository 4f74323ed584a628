// The quality metrics' host walk (hello_amd/csrc/cigar.h: qc_walk) over hand-made read sets, as a stand-alone host program in the
// style of markdup_check.cpp: built by tests/test_qc.py with -fsanitize=address,undefined and run directly.  The arrays are exactly
// sized, so a walk that leaves them is caught.  Exits non-zero on the first mismatch.
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../hello_amd/csrc/cigar.h"

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

    // n_bases < 0: as many as the CIGAR consumes; ref_end from the CIGAR plus end_shift
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
    ReadsView view() const {                     // bases, qualities' values and name_hash are not read by the walk
        return ReadsView{nullptr, quals.data(), read_off.data(), cigars.data(), cigar_off.data(), ref_start.data(), ref_end.data(),
                         mapq.data(), flags.data(), nullptr, (int64_t)ref_start.size()};
    }
};

struct Walk { std::string refusal; std::vector<uint8_t> kind; };
Walk walk(const Set& s, int64_t lo = 0, int mapq_threshold = 10) {
    Walk w;
    try {
        w.kind = qc_walk(s.view(), lo, mapq_threshold);
    } catch (const Fail& f) {
        w.refusal = std::to_string(f.code) + " " + f.msg;
    }
    return w;
}

const std::string kArg = std::to_string(HELLO_ERR_ARG) + " ";
constexpr int M = 0, I = 1, D = 2, N = 3, S = 4, H = 5, P = 6;
constexpr uint8_t B = kQcBelongs, ME = kQcMeasured, C = kQcCounted;

}  // namespace

int main() {
    {   // the three classes: belonging by the start, measured by the flags, counted by the gVCF's rule
        Set s;
        s.add(5, {{10, M}});                                         // starts below lo = 8
        s.add(8, {{10, M}});
        s.add(9, {{10, M}}, 0x400);
        s.add(9, {{10, M}}, 0x200);                                  // QC-fail: neither measured nor counted
        s.add(10, {{10, M}}, 0, 9);                                  // below the threshold: measured only
        s.add(10, {{10, M}}, 0, 0);
        s.add(11, {{10, M}}, 0x41);                                  // paired, not proper: measured only
        s.add(11, {{10, M}}, 0x63);
        s.add(12, {{2, H}, {3, S}, {4, M}, {1, I}, {1, P}, {2, D}, {3, N}, {2, M}, {1, S}});
        s.add(13, {{10, M}}, 0x4);
        s.add(13, {{10, M}}, 0x100);
        s.add(13, {{10, M}}, 0x800);
        const Walk w = walk(s, 8);
        EXPECT(w.refusal == "");
        EXPECT((w.kind == std::vector<uint8_t>{(uint8_t)(ME | C), (uint8_t)(B | ME | C), B, B, (uint8_t)(B | ME), (uint8_t)(B | ME),
                                               (uint8_t)(B | ME), (uint8_t)(B | ME | C), (uint8_t)(B | ME | C), B, B, B}));
        EXPECT(qc_measured(0) && qc_measured(0x63) && !qc_measured(0x200) && !qc_measured(0x400) && !qc_measured(0x904));
        EXPECT(walk(s, 8, 0).kind[4] == (B | ME | C) && walk(s, 8, 0).kind[5] == (B | ME));      // mapq 0 is never counted
    }
    {   // a read that is neither measured nor counted is not looked at: its CIGAR may say anything
        Set s;
        s.add(0, {{5, M}}, 0x400, 60, 4, 3);
        s.add(0, {{5, 9}}, 0x100);
        s.add(-3, {{5, M}}, 0x4);
        EXPECT(walk(s).refusal == kArg + "read 2: reads are not coordinate-sorted (the BAM must be)");      // the order is everyone's
        Set t;
        t.add(-3, {{5, M}}, 0x4);
        t.add(0, {{5, M}}, 0x400, 60, 4, 3);
        t.add(0, {{5, 9}}, 0x100);
        EXPECT(walk(t, -5).refusal == "" && (walk(t, -5).kind == std::vector<uint8_t>{B, B, B}));
    }
    {
        Set s;
        s.add(0, {{5, M}}, 0, 60, 4);
        EXPECT(walk(s).refusal == kArg + "read 0: CIGAR query length 5, 4 bases");
    }
    {
        Set s;
        s.add(0, {{5, M}}, 0, 60, 6);                                // more bases than the CIGAR consumes: refused too
        EXPECT(walk(s).refusal == kArg + "read 0: CIGAR query length 5, 6 bases");
    }
    {   // measured but not counted, and the other way round, are both walked
        Set s;
        s.add(0, {{5, M}}, 0, 0, 4);
        EXPECT(walk(s).refusal == kArg + "read 0: CIGAR query length 5, 4 bases");
    }
    {
        Set s;
        s.add(0, {{3, M}, {2, 9}});
        EXPECT(walk(s).refusal == kArg + "read 0: CIGAR operation 9");
    }
    {
        Set s;
        s.add(0, {{4, M}});
        s.add(3, {{4, M}}, 0x10, 60, -1, 1);
        EXPECT(walk(s).refusal == kArg + "read 1: ref_end does not match its CIGAR");
    }
    {
        Set s;
        s.add(-1, {{4, M}});
        EXPECT(walk(s, -4).refusal == kArg + "read 0: ref_start -1");
    }
    {
        Set s;
        s.add(7, {{4, M}});
        s.add(6, {{4, M}});
        EXPECT(walk(s).refusal == kArg + "read 1: reads are not coordinate-sorted (the BAM must be)");
    }
    {   // offsets: the walk refuses before it indexes with them
        Set s;
        s.add(0, {{4, M}});
        s.add(1, {{4, M}});
        Set t = s;
        t.read_off[2] = 3;
        EXPECT(walk(t).refusal == kArg + "read 1: offsets decrease");
        t = s;
        t.cigar_off[2] = 0;
        EXPECT(walk(t).refusal == kArg + "read 1: offsets decrease");
        t = s;
        t.read_off[0] = 1;
        EXPECT(walk(t).refusal == kArg + "offsets do not start at 0");
        t = s;
        t.cigar_off[0] = -1;
        EXPECT(walk(t).refusal == kArg + "offsets do not start at 0");
    }
    {   // a read without a CIGAR and without bases: ref_end is ref_start + 1
        Set s;
        s.add(7, {});
        EXPECT(walk(s).refusal == "" && walk(s).kind.size() == 1 && walk(s).kind[0] == (B | ME | C));
    }
    {   // zero reads
        Set s;
        EXPECT(walk(s).refusal == "" && walk(s).kind.empty());
    }
    if (failures) {
        std::fprintf(stderr, "%d mismatches\n", failures);
        return 1;
    }
    std::puts("qc_check: ok");
    return 0;
}
