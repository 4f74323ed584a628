// The methylation stage's host code (hello_amd/csrc/mods.h: parse_mods, find_mods, mods_walk; cigar.h: meth_walk) over good and
// malformed inputs, as a stand-alone host program in the style of qc_check.cpp: built by tests/test_methylation.py with
// -fsanitize=address,undefined and run directly.  Every input is an exactly sized heap array, so a parser or a walk that leaves
// it is caught.  Exits non-zero on the first mismatch.
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../hello_amd/csrc/mods.h"

using namespace hello;

namespace {

int failures = 0;
#define EXPECT(cond)                                                                        \
    do {                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

using Deltas = std::vector<int32_t>;
using Probs = std::vector<uint8_t>;

// the text and the bytes as exactly sized vectors (no NUL behind the text)
ModsOfRead parse(const std::string& mm, const Probs& ml, bool has_ml = true) {
    const std::vector<uint8_t> text(mm.begin(), mm.end());
    const std::vector<uint8_t> bytes(ml);
    ModsOfRead out;
    parse_mods(text.data(), text.size(), has_ml, bytes.data(), bytes.size(), out);
    return out;
}

bool is(const ModsOfRead& m, int state, const Deltas& deltas = {}, const Probs& probs = {}, int mode = 0) {
    return m.state == state && m.deltas == deltas && m.probs == probs && m.mode == mode;
}

void put32(std::vector<uint8_t>& v, uint32_t x) { for (int i = 0; i < 4; ++i) v.push_back((uint8_t)(x >> (8 * i))); }

std::vector<uint8_t> z_field(const char* tag, const std::string& text, char type = 'Z') {
    std::vector<uint8_t> v{(uint8_t)tag[0], (uint8_t)tag[1], (uint8_t)type};
    v.insert(v.end(), text.begin(), text.end());
    v.push_back(0);
    return v;
}

std::vector<uint8_t> b_field(const char* tag, char sub, const Probs& values, int width = 1) {
    std::vector<uint8_t> v{(uint8_t)tag[0], (uint8_t)tag[1], 'B', (uint8_t)sub};
    put32(v, (uint32_t)values.size());
    for (uint8_t x : values) { v.push_back(x); for (int i = 1; i < width; ++i) v.push_back(0); }
    return v;
}

ModsOfRead found(const std::vector<std::vector<uint8_t>>& fields, size_t cut = SIZE_MAX) {
    std::vector<uint8_t> aux;
    for (const auto& f : fields) aux.insert(aux.end(), f.begin(), f.end());
    if (cut < aux.size()) aux.resize(cut);
    ModsOfRead out;
    find_mods(aux.data(), aux.data() + aux.size(), out);
    return out;
}

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
    try { w.kind = meth_walk(s.view(), lo, mapq_threshold); } catch (const Fail& f) { w.refusal = std::to_string(f.code) + " " + f.msg; }
    return w;
}

struct ModSet {
    Deltas deltas; Probs probs; std::vector<int64_t> off{0}; std::vector<uint8_t> mode, state;
    void add(const Deltas& d, int m = 0, int s = 1) {
        deltas.insert(deltas.end(), d.begin(), d.end());
        probs.insert(probs.end(), d.size(), 9);
        off.push_back((int64_t)deltas.size());
        mode.push_back((uint8_t)m);
        state.push_back((uint8_t)s);
    }
    std::string walk() const {
        try {
            mods_walk(ModsView{deltas.data(), probs.data(), off.data(), mode.data(), state.data(), (int64_t)deltas.size(),
                               (int64_t)probs.size()}, (int64_t)mode.size());
        } catch (const Fail& f) { return std::to_string(f.code) + " " + f.msg; }
        return "";
    }
};

const std::string kArg = std::to_string(HELLO_ERR_ARG) + " ";
constexpr int M = 0, I = 1, D = 2, S = 4, H = 5;
constexpr uint8_t B = kMethBelongs, C = kMethCounted, HC = kMethHardClipped;

}  // namespace

int main() {
    // ---- parse_mods: the grammar
    {
        ModsOfRead none;
        parse_mods(nullptr, 0, false, nullptr, 0, none);
        EXPECT(is(none, kModsNone));
        EXPECT(is(parse("", {}), kModsNone));
        EXPECT(is(parse("C+m,5,2;", {7, 8}), kModsUsable, {5, 2}, {7, 8}));
        EXPECT(is(parse("C+m.,5;", {7}), kModsUsable, {5}, {7}, 0));
        EXPECT(is(parse("C+m?,5;", {7}), kModsUsable, {5}, {7}, 1));
        EXPECT(is(parse("C+m;", {}), kModsUsable));
        EXPECT(is(parse("C+m?;", {}), kModsUsable, {}, {}, 1));
        EXPECT(is(parse("C+mh,5,2;", {1, 2, 3, 4}), kModsUsable, {5, 2}, {1, 3}));          // delta-major: m5 h5 m2 h2
        EXPECT(is(parse("C+hm,5,2;", {1, 2, 3, 4}), kModsUsable, {5, 2}, {2, 4}));
        EXPECT(is(parse("C+h,0,1;C+m,3;", {1, 2, 9}), kModsUsable, {3}, {9}));              // the group before takes its bytes
        EXPECT(is(parse("C+m,3;C+h,0,1;", {9, 1, 2}), kModsUsable, {3}, {9}));
        EXPECT(is(parse("G-m,0;C+76792,1;N+n?,2;C+m,4;A+a.;", {1, 2, 3, 200}), kModsUsable, {4}, {200}));
        EXPECT(is(parse("C+m,2147483647;", {1}), kModsUsable, {2147483647}, {1}));
        EXPECT(is(parse("C+m,0007;", {1}), kModsUsable, {7}, {1}));
        EXPECT(is(parse("C+h,0;", {1}), kModsNone));                                        // no C+m group: ML is not looked at
        EXPECT(is(parse("C-m,0;G+m,1;T+m;U+m;", {}), kModsNone));
        EXPECT(is(parse("C+109,0;", {1}), kModsNone));                                      // 'm' as a number is another code
    }
    // ---- parse_mods: every bad case
    for (const char* broken : {"C+m,0", "C+m", "C", "C+", "C+;", "C+,0;", "X+m,0;", "c+m,0;", "C*m,0;", "C+m,;", "C+m,a;", "C+m,-1;",
                               "C+m,0,;", "C+m,0;;", ";", "C+m,0; ", "C+M,0;", "C+m!,0;", "C+m.?,0;", "C+m 0;", "C+1m,0;", "C+m1,0;",
                               "C+m,0;C+", "C+m,2147483648;", "C+m,99999999999999999999999;", "C+h,2147483648;C+m,0;"})
        EXPECT(is(parse(broken, {1}), kModsBad));
    EXPECT(is(parse("C+m,0;C+m,1;", {1, 2}), kModsBad));                                    // two groups match
    EXPECT(is(parse("C+m,0;C+hm,1;", {1, 2, 3}), kModsBad));
    EXPECT(is(parse("C+m,0;", {}, false), kModsBad));                                       // ML missing
    EXPECT(is(parse("C+m;", {}, false), kModsBad));
    EXPECT(is(parse("C+m,0;", {}), kModsBad));                                              // ML of another length
    EXPECT(is(parse("C+m,0;", {1, 2}), kModsBad));
    EXPECT(is(parse("C+h,0;C+m,0;", {1}), kModsBad));
    // ---- find_mods: the auxiliary fields of a record
    {
        const auto hp = std::vector<uint8_t>{'H', 'P', 'C', 2};
        const auto mm = z_field("MM", "C+m,1,0;"), ml = b_field("ML", 'C', {200, 30});
        EXPECT(is(found({hp, mm, ml}), kModsUsable, {1, 0}, {200, 30}));
        EXPECT(is(found({ml, z_field("XX", "text"), mm, hp}), kModsUsable, {1, 0}, {200, 30}));          // in any order
        EXPECT(is(found({hp}), kModsNone));
        EXPECT(is(found({}), kModsNone));
        EXPECT(is(found({mm}), kModsBad));                                                   // no ML
        EXPECT(is(found({mm, b_field("ML", 'S', {200, 30}, 2)}), kModsBad));                 // ML of type B:S
        EXPECT(is(found({mm, b_field("ML", 'c', {1, 30})}), kModsBad));
        EXPECT(is(found({z_field("MM", "C+m,1,0;", 'H'), ml}), kModsBad));                   // MM that is no text
        EXPECT(is(found({{'M', 'M', 'C', 7}, ml}), kModsBad));
        EXPECT(is(found({z_field("Mm", "C+m,1,0;"), b_field("Ml", 'C', {200, 30})}), kModsNone));        // the tags before the standard
        EXPECT(is(found({z_field("MM", "C+h,1;"), b_field("ML", 'C', {4})}), kModsNone));
        // fields that cannot be walked: what was found before the break is used, and nothing is read behind the end
        std::vector<uint8_t> all;
        for (const auto& f : {hp, mm, ml}) all.insert(all.end(), f.begin(), f.end());
        for (size_t cut = 0; cut <= all.size(); ++cut) {
            const ModsOfRead got = found({hp, mm, ml}, cut);
            EXPECT(got.state == (cut == all.size() ? kModsUsable : cut >= hp.size() + mm.size() ? kModsBad : kModsNone));
        }
        auto huge = b_field("ML", 'C', {1, 2});
        huge[4] = huge[5] = huge[6] = huge[7] = 0xFF;                                         // a count the record does not hold
        EXPECT(is(found({mm, huge}), kModsBad));
        EXPECT(is(found({{'X', 'Y', 'q', 1}, mm, ml}), kModsNone));                           // an unknown type ends the walk
    }
    // ---- mods_walk
    {
        ModSet good;
        good.add({0, 5});
        good.add({}, 1, 0);
        good.add({3}, 0, 2);
        EXPECT(good.walk() == "");
        EXPECT(ModSet().walk() == "");
        ModSet m = good;
        m.off[0] = 1;
        EXPECT(m.walk() == kArg + "modification offsets do not start at 0");
        m = good;
        m.off[2] = 1;
        EXPECT(m.walk() == kArg + "read 1: modification offsets decrease");
        m = good;
        m.off[3] = 2;
        EXPECT(m.walk() == kArg + "modification offsets end at 2, 3 deltas");
        m = good;
        m.probs.pop_back();
        EXPECT(m.walk() == kArg + "2 probabilities for 3 deltas");
        m = good;
        m.deltas[1] = -5;
        EXPECT(m.walk() == kArg + "read 0: delta -5");
        m = good;
        m.state[1] = 3;
        EXPECT(m.walk() == kArg + "read 1: modification state 3");
        m = good;
        m.mode[2] = 2;
        EXPECT(m.walk() == kArg + "read 2: modification mode 2");
    }
    // ---- meth_walk
    {
        Set s;
        s.add(5, {{10, M}});                                         // starts below lo = 8
        s.add(8, {{10, M}});
        s.add(9, {{10, M}}, 0x400);
        s.add(10, {{10, M}}, 0, 9);                                  // below the threshold
        s.add(11, {{10, M}}, 0x41);                                  // paired, not proper
        s.add(12, {{2, H}, {3, S}, {4, M}, {1, I}, {2, D}, {2, M}, {1, S}});
        s.add(13, {{5, 9}}, 0x100);                                  // not counted: its CIGAR may say anything
        const Walk w = walk(s, 8);
        EXPECT(w.refusal == "");
        EXPECT((w.kind == std::vector<uint8_t>{C, (uint8_t)(B | C), B, B, B, (uint8_t)(B | C | HC), B}));
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
    if (failures) {
        std::fprintf(stderr, "%d mismatches\n", failures);
        return 1;
    }
    std::puts("mods_check: ok");
    return 0;
}
