// The host walks of hello_amd/csrc/cigar.h over whole generated corpora (tests/read_fuzz.py), as a stand-alone host program in the
// style of qc_check.cpp: built by tests/test_read_fuzz.py with -fsanitize=address,undefined and run directly.  Every argument is a
// flat dump of one read set: int64 n_reads, n_bases, n_cigars, then read_off [n + 1], cigar_off [n + 1], ref_start [n], ref_end [n]
// (int64), cigars (uint32), flags (uint16), mapq, bases, quals (uint8).  The arrays are sized exactly, so a walk that leaves them is
// caught.  Per read it prints what the walks found; the test holds that against what it derives from the rows.
#include <cstdio>
#include <string>
#include <vector>

#include "../../hello_amd/csrc/cigar.h"

using namespace hello;

namespace {

template <class T>
std::vector<T> take(std::FILE* f, int64_t n) {
    std::vector<T> v((size_t)n);
    if (n > 0 && std::fread(v.data(), sizeof(T), (size_t)n, f) != (size_t)n) raise(HELLO_ERR_ARG, "short dump");
    return v;
}

int walk(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "%s: cannot open\n", path); return 1; }
    const std::vector<int64_t> head = take<int64_t>(f, 3);
    const int64_t n = head[0];
    const auto read_off = take<int64_t>(f, n + 1), cigar_off = take<int64_t>(f, n + 1), ref_start = take<int64_t>(f, n),
               ref_end = take<int64_t>(f, n);
    const auto cigars = take<uint32_t>(f, head[2]);
    const auto flags = take<uint16_t>(f, n);
    const auto mapq = take<uint8_t>(f, n), bases = take<uint8_t>(f, head[1]), quals = take<uint8_t>(f, head[1]);
    std::fclose(f);
    const ReadsView s{bases.data(), quals.data(), read_off.data(), cigars.data(), cigar_off.data(), ref_start.data(), ref_end.data(),
                      mapq.data(), flags.data(), nullptr, n};
    ReadLayout layout;
    strict_walk(s, kStrictPlain, layout);
    const std::vector<int64_t> eligible = markdup_walk(s);
    const std::vector<uint8_t> kind = qc_walk(s, 0, 10);
    std::vector<uint8_t> is_eligible((size_t)n, 0);
    for (int64_t r : eligible) is_eligible[(size_t)r] = 1;
    std::printf("corpus %s reads %lld span %lld\n", path, (long long)n, (long long)layout.max_span[0]);
    for (int64_t r = 0; r < n; ++r) {
        int64_t qlen = -1, rlen = -1;
        const bool is_counted = counted_walk(s, r, 10, qlen, rlen);
        std::printf("%lld %d %lld %lld %d %d %lld\n", (long long)r, is_counted ? 1 : 0, (long long)(is_counted ? qlen : -1),
                    (long long)(is_counted ? rlen : -1), (int)is_eligible[(size_t)r], (int)kind[(size_t)r], (long long)layout.last_pos[(size_t)r]);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    for (int k = 1; k < argc; ++k) {
        try {
            if (walk(argv[k])) return 1;
        } catch (const Fail& fail) {
            std::printf("refused %s: %d %s\n", argv[k], fail.code, fail.msg.c_str());
            return 1;
        }
    }
    std::puts("walk_corpus: ok");
    return 0;
}
