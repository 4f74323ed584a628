// The duplicate marker's host walk (hello_amd/csrc/cigar.h: markdup_walk) over hand-made read sets, as a stand-alone host program
// in the style of cigar_check.cpp: built by tests/test_markdup.py with -fsanitize=address,undefined and run directly.  The arrays
// are exactly sized, so a walk that leaves them is caught.  Exits non-zero on the first mismatch.
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
    std::vector<uint8_t> quals;
    std::vector<int64_t> read_off{0}, cigar_off{0}, ref_start, ref_end;
    std::vector<uint32_t> cigars;
    std::vector<uint16_t> flags;

    // n_bases < 0: as many as the CIGAR consumes; ref_end from the CIGAR plus end_shift
    void add(int64_t start, const std::vector<std::pair<int, int>>& cigar, uint16_t flag = 0, int64_t n_bases = -1, int64_t end_shift = 0) {
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
    }
    ReadsView view() const {                     // bases, mapq and name_hash are not read by the walk
        return ReadsView{nullptr, quals.data(), read_off.data(), cigars.data(), cigar_off.data(), ref_start.data(), ref_end.data(),
                         nullptr, flags.data(), nullptr, (int64_t)ref_start.size()};
    }
};

struct Walk { std::string refusal; std::vector<int64_t> list; };
Walk walk(const Set& s) {
    Walk w;
    try {
        w.list = markdup_walk(s.view());
    } catch (const Fail& f) {
        w.refusal = std::to_string(f.code) + " " + f.msg;
    }
    return w;
}

const std::string kArg = std::to_string(HELLO_ERR_ARG) + " ";
constexpr int M = 0, I = 1, D = 2, S = 4, H = 5;

}  // namespace

int main() {
    {   // who takes part: flags alone
        Set s;
        s.add(10, {{10, M}});
        s.add(10, {{10, M}}, 0x400);
        s.add(10, {{10, M}}, 0x4);
        s.add(10, {{10, M}}, 0x100);
        s.add(10, {{10, M}}, 0x800);
        s.add(10, {{10, M}}, 0x200 | 0x63);                          // QC-fail and paired: eligible
        s.add(12, {{2, H}, {3, S}, {4, M}, {1, I}, {2, D}, {2, M}, {1, S}});
        const Walk w = walk(s);
        EXPECT(w.refusal == "" && (w.list == std::vector<int64_t>{0, 5, 6}));
        EXPECT(markdup_eligible(0) && markdup_eligible(0x200) && !markdup_eligible(0x400) && !markdup_eligible(0x904));
    }
    {   // a read that takes no part is not looked at: its CIGAR may say anything
        Set s;
        s.add(0, {{5, M}}, 0x400, 4, 3);
        s.add(0, {{5, 9}}, 0x100);
        EXPECT(walk(s).refusal == "" && walk(s).list.empty());
    }
    {
        Set s;
        s.add(0, {{5, M}}, 0, 4);
        EXPECT(walk(s).refusal == kArg + "read 0: CIGAR query length 5, 4 bases");
    }
    {
        Set s;
        s.add(0, {{5, M}}, 0, 6);                                    // more bases than the CIGAR consumes: refused too
        EXPECT(walk(s).refusal == kArg + "read 0: CIGAR query length 5, 6 bases");
    }
    {
        Set s;
        s.add(0, {{3, M}, {2, 9}});
        EXPECT(walk(s).refusal == kArg + "read 0: CIGAR operation 9");
    }
    {
        Set s;
        s.add(0, {{4, M}});
        s.add(3, {{4, M}}, 0x10, -1, 1);
        EXPECT(walk(s).refusal == kArg + "read 1: ref_end does not match its CIGAR");
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
        EXPECT(walk(s).refusal == "" && walk(s).list.size() == 1);
    }
    {   // zero reads
        Set s;
        EXPECT(walk(s).refusal == "" && walk(s).list.empty());
    }
    if (failures) {
        std::fprintf(stderr, "%d mismatches\n", failures);
        return 1;
    }
    std::puts("markdup_check: ok");
    return 0;
}
