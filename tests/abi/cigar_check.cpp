// The strict, counted and exact host read walks of hello_amd/csrc/cigar.h over hand-made read sets, as a stand-alone host program: built by
// tests/test_stage_host.py with -fsanitize=address,undefined and run directly.  Exits non-zero on the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
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

using Cigar = std::initializer_list<std::pair<int, char>>;

struct Set {                                    // exactly sized arrays, so that a walk that leaves them is caught
    std::vector<uint8_t> bases, quals, mapq;
    std::vector<int64_t> read_off{0}, cigar_off{0}, ref_start, ref_end;
    std::vector<uint32_t> cigars;
    std::vector<uint16_t> flags;
    std::vector<uint64_t> name_hash;

    // bases < 0: as many as the CIGAR consumes; ref_end from the CIGAR plus end_shift
    void add(int64_t start, Cigar cigar, uint16_t flag = 0, uint8_t mq = 60, int64_t n_bases = -1, int64_t end_shift = 0) {
        int64_t q = 0, r = 0;
        for (const auto& c : cigar) {
            const int op = (int)std::string("MIDNSHP=X9").find(c.second);
            cigars.push_back((uint32_t)c.first << 4 | (uint32_t)op);
            if (is_query_op(op)) q += c.first;
            if (is_ref_op(op)) r += c.first;
        }
        if (n_bases < 0) n_bases = q;
        bases.insert(bases.end(), (size_t)n_bases, 'A');
        quals.insert(quals.end(), (size_t)n_bases, 30);
        read_off.push_back((int64_t)bases.size());
        cigar_off.push_back((int64_t)cigars.size());
        ref_start.push_back(start);
        ref_end.push_back(start + (r > 0 ? r : 1) + end_shift);
        flags.push_back(flag);
        mapq.push_back(mq);
        name_hash.push_back(ref_start.size());
    }
    ReadsView view() const {
        return ReadsView{bases.data(), quals.data(), read_off.data(), cigars.data(), cigar_off.data(), ref_start.data(),
                         ref_end.data(), mapq.data(), flags.data(), name_hash.data(), (int64_t)ref_start.size()};
    }
};

// "" when the walk accepts the set, else "<code> <message>"
std::string strict(const Set& s, StrictMode mode, ReadLayout& out) {
    try {
        strict_walk(s.view(), mode, out);
    } catch (const Fail& f) {
        return std::to_string(f.code) + " " + f.msg;
    }
    return "";
}
std::string strict(const Set& s, StrictMode mode = kStrictRegions) {
    ReadLayout out;
    return strict(s, mode, out);
}

struct Counted { std::string refusal; std::vector<int64_t> reads, qlen, rlen; };
Counted counted_all(const Set& s, int mapq_threshold) {
    Counted c;
    const ReadsView v = s.view();
    try {
        for (int64_t r = 0; r < v.n; ++r) {
            int64_t q = -1, l = -1;
            if (!counted_walk(v, r, mapq_threshold, q, l)) continue;
            c.reads.push_back(r);
            c.qlen.push_back(q);
            c.rlen.push_back(l);
        }
    } catch (const Fail& f) {
        c.refusal = std::to_string(f.code) + " " + f.msg;
    }
    return c;
}

// exact_walk of read r (on the reference with `max_bases` when it is given): (the refusal or "", what it returns)
std::pair<std::string, ExactWalk> exact(const Set& s, int64_t r, int64_t max_bases = -1) {
    try {
        return {"", max_bases < 0 ? exact_walk(s.view(), r) : exact_walk_on_reference(s.view(), r, max_bases)};
    } catch (const Fail& f) {
        return {std::to_string(f.code) + " " + f.msg, ExactWalk{}};
    }
}
std::string order(const Set& s, int64_t r, bool sorted) {
    try {
        check_read_order(s.view(), r, sorted);
    } catch (const Fail& f) {
        return std::to_string(f.code) + " " + f.msg;
    }
    return "";
}

const std::string kArg =std::to_string(HELLO_ERR_ARG) + " ", kShape = std::to_string(HELLO_ERR_SHAPE) + " ";

}  // namespace

int main() {
    {   // the worked read: 3M2I4M1D5M at 10
        Set s;
        s.add(10, {{3, 'M'}, {2, 'I'}, {4, 'M'}, {1, 'D'}, {5, 'M'}});
        ReadLayout out;
        EXPECT(strict(s, kStrictRegions, out) == "");
        EXPECT((out.plant_off == std::vector<int64_t>{0, 2}));
        EXPECT((out.plant == std::vector<int64_t>{12, 16}));
        EXPECT((out.last_pos == std::vector<int64_t>{22}));
        EXPECT((out.pflags == std::vector<uint8_t>{0}));
        EXPECT(out.max_span[0] == 13);
        ReadLayout plain;                                            // the hotspot stage's mode: the same planting positions and span
        EXPECT(strict(s, kStrictPlain, plain) == "" && plain.plant == out.plant && plain.max_span[0] == 13);
        const Counted c = counted_all(s, 10);
        EXPECT(c.refusal == "" && c.reads.size() == 1 && c.qlen[0] == 14 && c.rlen[0] == 13);
    }
    {   // partial insertions
        Set s;
        s.add(5, {{2, 'I'}, {5, 'M'}});
        s.add(6, {{5, 'M'}, {2, 'I'}});
        s.add(7, {{3, 'M'}, {2, 'N'}, {1, 'I'}, {3, 'M'}});          // an insertion behind N starts anew
        ReadLayout out;
        EXPECT(strict(s, kStrictRegions, out) == "");
        EXPECT((out.pflags == std::vector<uint8_t>{1, 2, 1}));
        EXPECT((out.plant == std::vector<int64_t>{4, 10, 11}));
        EXPECT((out.last_pos == std::vector<int64_t>{9, 10, 14}));
    }
    {   // strict refusals
        Set s;
        s.add(0, {{5, 'M'}}, 0, 60, 4);
        EXPECT(strict(s) == kShape + "read 0: CIGAR query length 5, 4 bases");
    }
    {
        Set s;
        s.add(0, {{3, 'M'}, {0, 'I'}, {3, 'M'}});
        EXPECT(strict(s) == kArg + "read 0: zero-length CIGAR operation");
    }
    {
        Set s;
        s.add(0, {{3, 'M'}, {2, '9'}});
        EXPECT(strict(s) == kArg + "read 0: CIGAR operation 9");
    }
    {
        Set s;
        s.add(0, {{4, 'M'}});
        s.add(3, {{4, 'M'}}, 0, 60, -1, 1);
        EXPECT(strict(s) == kShape + "read 1: ref_end does not match its CIGAR");
    }
    {
        Set s;
        s.add(0, {{4, 'M'}});
        s.bases[2] = 'Z';
        EXPECT(strict(s) == kArg + "read 0: base 'Z' is not a BAM base code");
        s.bases[2] = 0;                                              // strchr finds the terminator: refused all the same, and
        EXPECT(strict(s) == kArg + "read 0: base '");                // the message ends at the byte it prints
    }
    {
        Set s;
        s.add(9, {{4, 'M'}});
        s.add(8, {{4, 'M'}});
        EXPECT(strict(s) == kArg + "read 1: reads are not coordinate-sorted (the BAM must be)");
        EXPECT(strict(s, kStrictPlain) == kArg + "read 1: reads are not coordinate-sorted (the BAM must be)");
    }
    {
        Set s;
        s.add(0, {{3, 'M'}, {2, 'S'}, {3, 'M'}});
        EXPECT(strict(s, kStrictRegions) == kArg + "read 0: a soft clip between aligned operations");
        EXPECT(strict(s, kStrictClipInput) == "");
        EXPECT(strict(s, kStrictPlain) == "");
    }
    {   // an unusable read is not looked at
        Set s;
        s.add(0, {{5, 'M'}}, 0x4, 60, 4);
        EXPECT(strict(s) == "");
    }
    {   // counted walk
        Set s;
        s.add(0, {{5, 'M'}}, 0, 60, 4);
        EXPECT(counted_all(s, 10).refusal == kArg + "read 0: its CIGAR consumes 5 bases, it has 4");
    }
    {
        Set s;
        s.add(0, {{5, 'M'}}, 0x200, 60, 4);                          // QC-fail: skipped before its CIGAR is read
        s.add(1, {{5, 'M'}}, 0, 9, 4);                               // below the threshold: likewise
        s.add(2, {{2, 'S'}, {3, 'M'}, {4, 'N'}, {2, 'M'}});
        const Counted c = counted_all(s, 10);
        EXPECT(c.refusal == "" && (c.reads == std::vector<int64_t>{2}) && c.qlen[0] == 7 && c.rlen[0] == 9);
        EXPECT(counted(0, 10, 10) && !counted(0, 9, 10) && !counted(0x200, 60, 10) && !counted(0x400, 60, 10) && !counted(0, 0, 0));
    }
    {   // zero reads
        Set s;
        ReadLayout out;
        EXPECT(strict(s, kStrictRegions, out) == "" && (out.plant_off == std::vector<int64_t>{0}) && out.plant.empty());
        EXPECT(counted_all(s, 10).refusal == "" && counted_all(s, 10).reads.empty());
    }
    {   // exact walk: the lengths of the worked read, and a hard clip seen but consuming nothing
        Set s;
        s.add(10, {{3, 'M'}, {2, 'I'}, {4, 'M'}, {1, 'D'}, {5, 'M'}});
        s.add(11, {{2, 'H'}, {1, 'S'}, {3, '='}, {2, 'N'}, {1, 'P'}, {2, 'X'}, {3, 'H'}});
        const ExactWalk a = exact(s, 0).second, b = exact(s, 1).second;
        EXPECT(exact(s, 0).first == "" && a.qlen == 14 && a.rlen == 13 && !a.hard_clipped);
        EXPECT(exact(s, 1).first == "" && b.qlen == 6 && b.rlen == 7 && b.hard_clipped);
    }
    {   // exact walk: an empty CIGAR belongs to a read without bases that ends one past its start
        Set s;
        s.add(4, {});
        const auto e = exact(s, 0);
        EXPECT(e.first == "" && e.second.qlen == 0 && e.second.rlen == 0 && !e.second.hard_clipped);
        Set with_bases;
        with_bases.add(4, {}, 0, 60, 3);
        EXPECT(exact(with_bases, 0).first == kArg + "read 0: CIGAR query length 0, 3 bases");
    }
    {   // exact walk: each refusal once, with HELLO_ERR_ARG; the unknown operation comes before the lengths
        Set s;
        s.add(0, {{3, 'M'}, {2, '9'}}, 0, 60, 7);
        s.add(1, {{5, 'M'}}, 0, 60, 4);
        s.add(2, {{5, 'M'}}, 0, 60, 6);
        s.add(3, {{4, 'M'}}, 0, 60, -1, 1);
        s.add(4, {{4, 'M'}}, 0, 60, -1, -1);
        EXPECT(exact(s, 0).first == kArg + "read 0: CIGAR operation 9");
        EXPECT(exact(s, 1).first == kArg + "read 1: CIGAR query length 5, 4 bases");
        EXPECT(exact(s, 2).first == kArg + "read 2: CIGAR query length 5, 6 bases");
        EXPECT(exact(s, 3).first == kArg + "read 3: ref_end does not match its CIGAR");
        EXPECT(exact(s, 4).first == kArg + "read 4: ref_end does not match its CIGAR");
    }
    {   // exact walk on the reference: a start below 0 and the bound on the bases
        Set s;
        s.add(-1, {{4, 'M'}});
        s.add(3, {{4, 'M'}});
        EXPECT(exact(s, 0, 100).first == kArg + "read 0: ref_start -1");
        EXPECT(exact(s, 1, 4).first == "" && exact(s, 1, 3).first == kArg + "read 1: 4 bases, at most 3");
    }
    {   // the order of a read set
        Set s;
        s.add(9, {{4, 'M'}});
        s.add(8, {{4, 'M'}});
        EXPECT(order(s, 0, true) == "" && order(s, 1, false) == "");
        EXPECT(order(s, 1, true) == kArg + "read 1: reads are not coordinate-sorted (the BAM must be)");
        s.read_off[2] = 3;
        EXPECT(order(s, 1, false) == kArg + "read 1: offsets decrease");
        s.read_off[0] = 1;
        EXPECT(order(s, 0, false) == kArg + "offsets do not start at 0");
    }
    if (failures) {
        std::fprintf(stderr, "%d mismatches\n", failures);
        return 1;
    }
    std::puts("cigar_check: ok");
    return 0;
}
