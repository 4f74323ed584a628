// Base modifications of a BAM record (SAM tags MM:Z and ML:B:C) as the methylation stage reads them: the
// parser the BAM decoder runs per record, and the validation of the arrays hello_meth_add is given.  Plain C++17 -- no HIP, no
// kernel -- so both also build into a stand-alone host program (tests/abi/mods_check.cpp).  hello_amd/methylation.py: parse_mm
// restates the parser.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "cigar.h"

namespace hello {
namespace {

constexpr uint8_t kModsNone = 0, kModsUsable = 1, kModsBad = 2;

// One record's 5mC calls: per listed base the delta (bases of its kind skipped before it) and the probability byte.
struct ModsOfRead {
    std::vector<int32_t> deltas;
    std::vector<uint8_t> probs;
    uint8_t mode = 0;      // 0 implicit ('.' or absent): a base that is not listed is unmodified; 1 unknown ('?'): it says nothing
    uint8_t state = kModsNone;
};

// mm[0 .. mm_len): the text of MM without its NUL, or nullptr when the record has none.  ml[0 .. ml_len): the bytes of ML;
// has_ml: the record has an ML of type B:C (it may be empty).  The group used is C+ with letter codes containing 'm'; every other
// group is skipped and still takes its bytes of ML.
inline void parse_mods(const uint8_t* mm, size_t mm_len, bool has_ml, const uint8_t* ml, size_t ml_len, ModsOfRead& out) {
    out.deltas.clear();
    out.probs.clear();
    out.mode = 0;
    out.state = kModsNone;
    if (!mm) return;
    auto bad = [&]() { out.deltas.clear(); out.probs.clear(); out.mode = 0; out.state = kModsBad; };
    size_t i = 0, total = 0, offset = 0, n_codes_used = 0, index_m = 0;
    bool found = false;
    uint8_t mode = 0;
    std::vector<int32_t> deltas;
    while (i < mm_len) {
        const uint8_t base = mm[i++];
        if (!(base == 'A' || base == 'C' || base == 'G' || base == 'T' || base == 'U' || base == 'N')) return bad();
        if (i >= mm_len || (mm[i] != '+' && mm[i] != '-')) return bad();
        const uint8_t strand = mm[i++];
        size_t n_codes = 0, at_m = SIZE_MAX;
        if (i < mm_len && mm[i] >= '0' && mm[i] <= '9') {
            while (i < mm_len && mm[i] >= '0' && mm[i] <= '9') ++i;                 // one numeric code, whatever its value
            n_codes = 1;
        } else {
            while (i < mm_len && mm[i] >= 'a' && mm[i] <= 'z') {
                if (mm[i] == 'm' && at_m == SIZE_MAX) at_m = n_codes;
                ++n_codes;
                ++i;
            }
        }
        if (n_codes == 0) return bad();
        uint8_t group_mode = 0;
        if (i < mm_len && (mm[i] == '.' || mm[i] == '?')) group_mode = mm[i++] == '?' ? 1 : 0;
        const bool mine = base == 'C' && strand == '+' && at_m != SIZE_MAX;
        if (mine && found) return bad();                                            // two groups match
        size_t n_deltas = 0;
        while (i < mm_len && mm[i] == ',') {
            ++i;
            if (i >= mm_len || mm[i] < '0' || mm[i] > '9') return bad();
            int64_t v = 0;
            while (i < mm_len && mm[i] >= '0' && mm[i] <= '9') {
                v = v * 10 + (mm[i++] - '0');
                if (v > INT32_MAX) return bad();                                    // a delta that does not fit an int32
            }
            if (mine) deltas.push_back((int32_t)v);
            ++n_deltas;
        }
        if (i >= mm_len || mm[i] != ';') return bad();
        ++i;
        if (mine) {
            found = true;
            offset = total;
            n_codes_used = n_codes;
            index_m = at_m;
            mode = group_mode;
        }
        total += n_deltas * n_codes;
    }
    if (!found) return;                                                             // no C+m group: no modifications
    if (!has_ml || ml_len != total) return bad();
    out.deltas = std::move(deltas);
    out.probs.resize(out.deltas.size());
    for (size_t k = 0; k < out.deltas.size(); ++k) out.probs[k] = ml[offset + k * n_codes_used + index_m];
    out.mode = mode;
    out.state = kModsUsable;
}

// The MM and ML fields among a record's auxiliary fields [aux, end) -> parse_mods.  Fields that cannot be walked are nobody
// else's concern (as for HP): what was found before the break is used.  An MM of another type than Z is broken syntax.
inline void find_mods(const uint8_t* aux, const uint8_t* end, ModsOfRead& out) {
    auto scalar = [](uint8_t t) -> int {
        switch (t) {
            case 'A': case 'c': case 'C': return 1;
            case 's': case 'S': return 2;
            case 'i': case 'I': case 'f': return 4;
            default: return 0;
        }
    };
    auto le32 = [](const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); };
    const uint8_t* mm = nullptr; const uint8_t* ml = nullptr;
    size_t mm_len = 0, ml_len = 0;
    bool mm_seen = false;
    while (end - aux >= 3) {
        const uint8_t t0 = aux[0], t1 = aux[1], type = aux[2];
        const bool is_mm = t0 == 'M' && t1 == 'M', is_ml = t0 == 'M' && t1 == 'L';
        aux += 3;
        if (type == 'Z' || type == 'H') {
            const uint8_t* z = (const uint8_t*)memchr(aux, 0, (size_t)(end - aux));
            if (!z) break;
            if (is_mm && !mm_seen) { mm_seen = true; if (type == 'Z') { mm = aux; mm_len = (size_t)(z - aux); } }
            aux = z + 1;
        } else if (type == 'B') {
            if (end - aux < 5) break;
            const int w = scalar(aux[0]);
            const uint32_t n = le32(aux + 1);
            if (!w || (uint64_t)n * w > (uint64_t)(end - aux - 5)) break;
            if (is_ml && !ml && aux[0] == 'C') { ml = aux + 5; ml_len = n; }
            if (is_mm) mm_seen = true;
            aux += 5 + (size_t)n * w;
        } else {
            const int w = scalar(type);
            if (!w || end - aux < w) break;
            if (is_mm) mm_seen = true;
            aux += w;
        }
    }
    if (mm_seen && !mm) {                                                           // MM of a type that holds no text
        out.deltas.clear(); out.probs.clear(); out.mode = 0; out.state = kModsBad;
        return;
    }
    parse_mods(mm, mm_len, ml != nullptr, ml, ml_len, out);
}

// The modification arrays of a read set as hello_meth_add takes them: offsets [n + 1] into deltas / probs, mode and state per read.
struct ModsView {
    const int32_t* deltas = nullptr; const uint8_t* probs = nullptr; const int64_t* off = nullptr;
    const uint8_t* mode = nullptr; const uint8_t* state = nullptr;
    int64_t n_deltas = 0, n_probs = 0;
};

// What the kernels rely on: offsets that start at 0, do not decrease and end at the arrays' length; as many probabilities as
// deltas; no negative delta (the targets then increase strictly, the kernel searches them); known states and modes.
inline void mods_walk(const ModsView& m, int64_t n) {
    if (m.n_deltas < 0 || m.n_probs != m.n_deltas)
        raise(HELLO_ERR_ARG, "%lld probabilities for %lld deltas", (long long)m.n_probs, (long long)m.n_deltas);
    if (m.off[0] != 0) raise(HELLO_ERR_ARG, "modification offsets do not start at 0");
    for (int64_t r = 0; r < n; ++r) {
        if (m.off[r + 1] < m.off[r]) raise(HELLO_ERR_ARG, "read %lld: modification offsets decrease", (long long)r);
        if (m.state[r] > kModsBad) raise(HELLO_ERR_ARG, "read %lld: modification state %d", (long long)r, m.state[r]);
        if (m.mode[r] > 1) raise(HELLO_ERR_ARG, "read %lld: modification mode %d", (long long)r, m.mode[r]);
    }
    if (m.off[n] != m.n_deltas)
        raise(HELLO_ERR_ARG, "modification offsets end at %lld, %lld deltas", (long long)m.off[n], (long long)m.n_deltas);
    for (int64_t r = 0; r < n; ++r)
        for (int64_t k = m.off[r]; k < m.off[r + 1]; ++k)
            if (m.deltas[k] < 0) raise(HELLO_ERR_ARG, "read %lld: delta %d", (long long)r, m.deltas[k]);
}

}  // namespace
}  // namespace hello
