// The host rules of the large deletions and insertions -- sv_walk of hello_amd/csrc/cigar.h and the sort, the clusters and the genotype
// of hello_amd/csrc/sv.h -- over hand-made inputs, as a stand-alone host program: built by tests/test_sv.py with
// -fsanitize=address,undefined and run directly.  Exits non-zero on the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "../../hello_amd/csrc/cigar.h"
#include "../../hello_amd/csrc/sv.h"

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

    void add(int64_t start, Cigar cigar, uint16_t flag = 0, uint8_t mq = 60, int64_t n_bases = -1) {
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
        ref_end.push_back(start + (r > 0 ? r : 1));
        flags.push_back(flag);
        mapq.push_back(mq);
        name_hash.push_back(ref_start.size());
    }
    ReadsView view() const {
        return ReadsView{bases.data(), quals.data(), read_off.data(), cigars.data(), cigar_off.data(), ref_start.data(),
                         ref_end.data(), mapq.data(), flags.data(), name_hash.data(), (int64_t)ref_start.size()};
    }
};

std::string walked(const Set& s, int64_t lo, int64_t min_size, SvWalk& out) {
    try {
        out = sv_walk(s.view(), lo, 10, min_size);
    } catch (const Fail& f) {
        return std::to_string(f.code) + " " + f.msg;
    }
    return "";
}

SvSig sig(int type, int64_t pos, int len, int64_t ordinal, int64_t op, int strand = 0, int hp = 0, int shift = 0) {
    return SvSig{pos, ordinal, op, len, shift, (uint8_t)type, (uint8_t)strand, (uint8_t)hp, 0};
}

bool same(const SvCandidate& c, std::initializer_list<int64_t> want) {
    const int64_t got[kSvCandidateColumns] = {c.type, c.pos, c.len, c.dv, c.dv_fwd, c.dv_rev, c.hp[0], c.hp[1], c.hp[2], c.pos_min,
                                              c.pos_max, c.len_min, c.len_max};
    return want.size() == (size_t)kSvCandidateColumns && std::equal(want.begin(), want.end(), got);
}

const std::string kArg = std::to_string(HELLO_ERR_ARG) + " ";

}  // namespace

int main() {
    {   // the walk list and the count of operations: min_size 5, the span begins at 10
        Set s;
        s.add(8, {{8, 'M'}, {5, 'D'}, {8, 'M'}});                        // starts below the span: does not belong
        s.add(10, {{8, 'M'}, {5, 'D'}, {3, 'M'}, {6, 'I'}, {8, 'M'}});   // two operations
        s.add(11, {{8, 'M'}, {4, 'D'}, {8, 'M'}, {4, 'I'}, {2, 'M'}});   // none of five bases
        s.add(12, {{8, 'M'}, {5, 'N'}, {8, 'M'}});                       // N is no event
        s.add(13, {{5, 'D'}, {8, 'M'}});                                 // a leading one is walked all the same: the kernel decides
        s.add(14, {{8, 'M'}, {5, 'D'}, {8, 'M'}}, 0, 9);                 // below the mapq threshold
        s.add(15, {{8, 'M'}, {5, 'D'}, {8, 'M'}}, 0x400);                // a duplicate
        s.add(16, {{2, 'H'}, {3, 'S'}, {7, 'I'}, {8, '='}, {9, 'D'}, {1, 'X'}});
        s.add(17, {});
        SvWalk w;
        EXPECT(walked(s, 10, 5, w) == "");
        EXPECT((w.walk == std::vector<int64_t>{1, 4, 7}));
        EXPECT(w.n_ops == 5);
        EXPECT((w.kind == std::vector<uint8_t>{kPileCounted, 3, 3, 3, 3, kPileBelongs, kPileBelongs, 3, 3}));
        EXPECT(walked(s, 10, 1, w) == "" && w.n_ops == 7 && w.walk.size() == 4);
        EXPECT(walked(s, 10, 10, w) == "" && w.n_ops == 0 && w.walk.empty());
    }
    {   // the refusals are pileup_walk's, in its words
        Set s;
        s.add(0, {{5, 'M'}}, 0, 60, 4);
        SvWalk w;
        EXPECT(walked(s, 0, 5, w) == kArg + "read 0: CIGAR query length 5, 4 bases");
        Set order;
        order.add(9, {{4, 'M'}});
        order.add(8, {{4, 'M'}});
        EXPECT(walked(order, 0, 5, w) == kArg + "read 1: reads are not coordinate-sorted (the BAM must be)");
        Set op;
        op.add(0, {{3, 'M'}, {2, '9'}}, 0, 60, 5);
        EXPECT(walked(op, 0, 5, w) == kArg + "read 0: CIGAR operation 9");
        Set start;
        start.add(-1, {{4, 'M'}});
        EXPECT(walked(start, -5, 5, w) == kArg + "read 0: ref_start -1");
        Set unread;                                                       // a read that does not count is not looked at
        unread.add(0, {{5, 'M'}}, 0x4, 60, 4);
        EXPECT(walked(unread, 0, 5, w) == "" && w.walk.empty());
        Set none;
        EXPECT(walked(none, 0, 5, w) == "" && w.kind.empty() && w.walk.empty() && w.n_ops == 0);
    }
    {   // the order of the SIGNATURES arrays: (type, pos, len, ordinal, operation index)
        std::vector<SvSig> g = {sig(kSvIns, 5, 9, 0, 1), sig(kSvDel, 9, 9, 0, 1), sig(kSvDel, 7, 12, 3, 1), sig(kSvDel, 7, 9, 4, 1),
                                sig(kSvDel, 7, 9, 2, 5), sig(kSvDel, 7, 9, 2, 3)};
        sv_sort(g);
        const int64_t ordinals[6] = {2, 2, 4, 3, 0, 0}, ops[6] = {3, 5, 1, 1, 1, 1};
        for (int i = 0; i < 6; ++i) EXPECT(g[(size_t)i].ordinal == ordinals[i] && g[(size_t)i].op_index == ops[i]);
        EXPECT(g[4].type == kSvDel && g[5].type == kSvIns);
    }
    {   // a gap of exactly cluster_gap joins, one more parts
        std::vector<SvSig> g = {sig(kSvDel, 100, 20, 0, 1), sig(kSvDel, 110, 20, 1, 1, 1, 1), sig(kSvDel, 121, 20, 2, 1),
                                sig(kSvDel, 121, 20, 3, 1, 0, 2)};
        sv_sort(g);
        const std::vector<SvCandidate> c = sv_cluster(g, 10, 70, 2);
        EXPECT(c.size() == 2 && same(c[0], {kSvDel, 100, 20, 2, 1, 1, 1, 1, 0, 100, 110, 20, 20}) &&
               same(c[1], {kSvDel, 121, 20, 2, 2, 0, 1, 0, 1, 121, 121, 20, 20}));
        EXPECT(sv_cluster(g, 11, 70, 2).size() == 1 && sv_cluster(g, 10, 70, 3).empty() && sv_cluster(g, 0, 70, 2).size() == 1);
    }
    {   // a ratio exactly at the threshold joins, just under parts
        std::vector<SvSig> g = {sig(kSvIns, 50, 14, 0, 1), sig(kSvIns, 50, 20, 1, 1), sig(kSvIns, 50, 29, 2, 1), sig(kSvIns, 50, 29, 3, 1)};
        sv_sort(g);
        const std::vector<SvCandidate> c = sv_cluster(g, 10, 70, 2);
        EXPECT(c.size() == 2 && same(c[0], {kSvIns, 50, 14, 2, 2, 0, 2, 0, 0, 50, 50, 14, 20}) &&
               same(c[1], {kSvIns, 50, 29, 2, 2, 0, 2, 0, 0, 50, 50, 29, 29}));
        EXPECT(sv_cluster(g, 10, 71, 2).size() == 1);                     // 14 and 20 part: the two of 29 alone stay
        EXPECT(sv_cluster(g, 10, 68, 1).size() == 1);                     // 20 and 29 join too
    }
    {   // one read twice in a group counts once; a deletion and an insertion at one position; the lower medians of three
        std::vector<SvSig> twice = {sig(kSvDel, 10, 8, 7, 1, 1, 2), sig(kSvDel, 15, 8, 7, 3, 1, 2)};
        sv_sort(twice);
        EXPECT(sv_cluster(twice, 10, 70, 2).empty());
        const std::vector<SvCandidate> once = sv_cluster(twice, 10, 70, 1);
        EXPECT(once.size() == 1 && same(once[0], {kSvDel, 10, 8, 1, 0, 1, 0, 0, 1, 10, 15, 8, 8}));
        std::vector<SvSig> g = {sig(kSvIns, 30, 9, 0, 1, 0, 1), sig(kSvIns, 30, 9, 1, 1, 0, 1), sig(kSvDel, 30, 9, 0, 3, 0, 1),
                                sig(kSvDel, 31, 10, 1, 3, 0, 1), sig(kSvDel, 29, 11, 2, 1, 1, 3)};
        sv_sort(g);
        const std::vector<SvCandidate> c = sv_cluster(g, 10, 70, 2);
        EXPECT(c.size() == 2 && same(c[0], {kSvDel, 30, 10, 3, 2, 1, 1, 2, 0, 29, 31, 9, 11}) &&
               same(c[1], {kSvIns, 30, 9, 2, 2, 0, 0, 2, 0, 30, 30, 9, 9}));
        EXPECT(sv_cluster(std::vector<SvSig>{}, 10, 70, 1).empty());
    }
    {   // the genotype: 3 with and 2 without; 2 with and none without; none with; ties go to the first
        int64_t g[kSvGenotypeColumns];
        sv_genotype(3, 2, g);
        EXPECT(g[0] == 1 && g[1] == 12 && g[2] == 24 && g[3] == 0 && g[4] == 12);
        sv_genotype(2, 0, g);
        EXPECT(g[0] == 2 && g[1] == 6 && g[2] == 26 && g[3] == 6 && g[4] == 0);
        sv_genotype(0, 0, g);
        EXPECT(g[0] == 0 && g[1] == 0 && g[2] == 0 && g[3] == 0 && g[4] == 0);
        sv_genotype(0, 40, g);
        EXPECT(g[0] == 0 && g[1] == 99 && g[2] == 0);
        sv_genotype(1000000, 1000000, g);
        EXPECT(g[0] == 1 && g[1] == 99 && g[3] == 0 && g[2] == g[4] && g[2] > 1000000);
        EXPECT(sv_depth_ref(5, 3) == 2 && sv_depth_ref(1, 2) == 0);
    }
    if (failures) {
        std::fprintf(stderr, "%d mismatches\n", failures);
        return 1;
    }
    std::puts("sv_check: ok");
    return 0;
}
