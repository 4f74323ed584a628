// PCR duplicates (include/hello_mi355x.h: hello_markdup_*): the aligned reads of one chromosome of one BAM -> per read its packed
// 5' end, its score, its mate, its kind (pair, single, unresolved) and whether it is a duplicate.  Not in the reference; DESIGN.md
// section 7j states the rules and hello_amd/markdup.py restates them in Python, integer for integer.
//
// Host: the eligibility filter (flags alone) and the validation of every eligible read (cigar.h: markdup_walk; the ends kernel
// reads within its qualities and its CIGAR).  Device, per hello_markdup_add one kernel over the eligible reads of the span:
//   ends: a wave per eligible read.  The lanes stride the quality bytes, each adds those >= 15 with a saturating add, and the wave
//     reduces with shuffles.  Lane 0 sums the leading (forward read) or trailing (reverse read) run of S / H operations and
//     writes e = 2 end5 + strand and the score: one writer per output.
// and per hello_markdup_find, over the eligible reads of ALL spans, indexed c = 0..n-1 in the order given:
//   pair (two kernels): the mate join of section 7i, phase_pair.h, which phase.hip includes too; `source` is 0 for every read.
//   key: a second open-addressing table of 2^k >= 2 inserts slots, a thread per eligible read.  An entry is END(e) or PAIR(lo, hi)
//     and is claimed with atomicCAS on an int32 owner: INT32_MIN empty, c >= 0 for END(e[c]), -1 - c for PAIR of c and its mate.
//     Keys are compared in the input arrays, so no key value is reserved.  Every joined read ORs `paired` into END(e); every
//     single does atomicMax on END(e).best; the smaller-index mate of every pair does atomicMax on PAIR(lo, hi).best, where
//     best = score << 32 | (0xFFFFFFFF - representative index) is unique per contender: the winner does not depend on arrival
//     order (which read owns an entry does, and nothing reads the owner but the probe).
//   mark: a launch of its own, so the atomics of the key launch are complete.  A thread per eligible read finds its entry again
//     and writes its own kind and duplicate (both mates of a pair compute the same answer); the statistics take one atomicAdd
//     per wave and counter, from a ballot.
// Integers only, and every output has one writer: two runs give the same bytes.
#include <memory>

#include "phase_pair.h"
#include "stage_host.h"

namespace hello {
namespace {

constexpr int kMdThreads = 256;
constexpr int kMdWaves = kMdThreads / 64;
constexpr int kMdMinQuality = 15;
constexpr int32_t kMdMaxScore = (1 << 30) - 1;
constexpr int32_t kMdEmpty = INT32_MIN;

struct MdEndsArgs {
    const uint8_t* quals;
    const int64_t* read_off;
    const uint32_t* cigars;
    const int64_t* cigar_off;
    const int64_t* ref_start;
    const int64_t* ref_end;
    const uint16_t* flags;
    const int64_t* list;         // the eligible reads of the span, in input order
    int64_t* e;                  // [eligible]
    int32_t* score;
    int64_t n_eligible;
};

__global__ __launch_bounds__(kMdThreads) void markdup_ends_kernel(MdEndsArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * kMdWaves + (threadIdx.x >> 6);
    if (k >= a.n_eligible) return;                                        // the whole wave
    const int64_t r = a.list[k], q0 = a.read_off[r], q1 = a.read_off[r + 1];
    int32_t s = 0;
    for (int64_t i = q0 + lane; i < q1; i += 64) {
        const int32_t q = a.quals[i];
        if (q >= kMdMinQuality) s = min(s + q, kMdMaxScore);
    }
    for (int d = 32; d >= 1; d >>= 1) s = min(s + __shfl_down(s, d, 64), kMdMaxScore);      // two terms <= 2^30 - 1 fit an int32
    if (lane != 0) return;
    const int64_t c0 = a.cigar_off[r], c1 = a.cigar_off[r + 1];
    const bool reverse = (a.flags[r] & 0x10) != 0;
    int64_t clip = 0;
    if (!reverse) {
        for (int64_t c = c0; c < c1 && ((a.cigars[c] & 15) == 4 || (a.cigars[c] & 15) == 5); ++c) clip += a.cigars[c] >> 4;
    } else {
        for (int64_t c = c1 - 1; c >= c0 && ((a.cigars[c] & 15) == 4 || (a.cigars[c] & 15) == 5); --c) clip += a.cigars[c] >> 4;
    }
    const int64_t end5 = reverse ? a.ref_end[r] - 1 + clip : a.ref_start[r] - clip;
    a.e[k] = 2 * end5 + (reverse ? 1 : 0);
    a.score[k] = s;
}

struct MdKeyArgs {
    const int64_t* e;            // [n]: the eligible reads of all spans
    const int32_t* score;
    const uint16_t* flags;
    const int32_t* mate;         // the join's answer
    int32_t* owner;              // [mask + 1]: kMdEmpty, c (END of e[c]) or -1 - c (PAIR of c and mate[c])
    uint32_t* paired;            // END entries: a joined read has this end
    unsigned long long* best;    // score << 32 | (0xFFFFFFFF - representative index), 0 without a contender
    uint8_t* kind;               // [n]
    uint8_t* duplicate;
    int32_t* totals;             // singles, unresolved, duplicate_pairs, duplicate_singles
    int64_t n;
    uint32_t mask;
};

struct MdKey { int64_t a, b; uint32_t pair; };     // END: (e, 0, 0); PAIR: (lo, hi, 1)

// The first slot probed for a key (markdup.key_table_slot restates it): every bit of both ends reaches the slot.
__host__ __device__ inline uint32_t key_slot(const MdKey& k, uint32_t mask) {
    uint64_t x = (uint64_t)k.a;
    x ^= x >> 29;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 32;
    x += (uint64_t)k.b + k.pair;
    x ^= x >> 29;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 32;
    return (uint32_t)x & mask;
}

__device__ inline bool is_single(int f) { return !(f & 0x1) || (f & 0x8); }

__device__ inline MdKey end_key(const MdKeyArgs& a, int32_t c) { return MdKey{a.e[c], 0, 0}; }

__device__ inline MdKey pair_key(const MdKeyArgs& a, int32_t c) {
    const int64_t x = a.e[c], y = a.e[a.mate[c]];
    return MdKey{x < y ? x : y, x < y ? y : x, 1};
}

// The slot of the entry with key k.  claim: an empty slot on the way becomes c's entry of that kind.  The table holds at least
// twice the inserts, so a probe ends at an empty slot or at its entry before it has come round; it wraps at the table's end.
template <bool claim> __device__ inline uint32_t key_probe(const MdKeyArgs& a, const MdKey& k, int32_t c) {
    const int32_t mine = k.pair ? -1 - c : c;
    uint32_t slot = key_slot(k, a.mask);
    for (uint32_t tried = 0; tried <= a.mask; ++tried) {
        const int32_t o = claim ? atomicCAS(&a.owner[slot], kMdEmpty, mine) : a.owner[slot];
        if (o == kMdEmpty || o == mine) break;                            // claimed just now (or, looking up, not there: never)
        if ((o < 0) == (k.pair != 0)) {                                   // an entry of the same kind: its owner's key, in the arrays
            const MdKey other = o < 0 ? pair_key(a, -1 - o) : end_key(a, o);
            if (other.a == k.a && other.b == k.b) break;
        }
        slot = (slot + 1) & a.mask;
    }
    return slot;
}

__device__ inline unsigned long long contender(int64_t score, int32_t representative) {
    return ((unsigned long long)score << 32) | (0xFFFFFFFFu - (uint32_t)representative);
}

__global__ __launch_bounds__(kMdThreads) void markdup_key_kernel(MdKeyArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kMdThreads + threadIdx.x;
    if (i >= a.n) return;
    const int32_t c = (int32_t)i, m = a.mate[c];
    if (m >= 0) {
        atomicOr(&a.paired[key_probe<true>(a, end_key(a, c), c)], 1u);
        if (c < m) atomicMax(&a.best[key_probe<true>(a, pair_key(a, c), c)], contender((int64_t)a.score[c] + a.score[m], c));
    } else if (is_single(a.flags[c])) {
        atomicMax(&a.best[key_probe<true>(a, end_key(a, c), c)], contender(a.score[c], c));
    }
}

__global__ __launch_bounds__(kMdThreads) void markdup_mark_kernel(MdKeyArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kMdThreads + threadIdx.x;
    bool single = false, unresolved = false, dup_pair = false, dup_single = false;
    if (i < a.n) {
        const int32_t c = (int32_t)i, m = a.mate[c];
        bool dup = false;
        if (m >= 0) {
            const int32_t rep = c < m ? c : m;
            const uint32_t slot = key_probe<false>(a, pair_key(a, c), rep);
            dup = (int32_t)(0xFFFFFFFFu - (uint32_t)a.best[slot]) != rep;
            dup_pair = dup && c == rep;                                   // a pair is counted once, at its smaller index
        } else if (is_single(a.flags[c])) {
            const uint32_t slot = key_probe<false>(a, end_key(a, c), c);
            dup = a.paired[slot] != 0 || (int32_t)(0xFFFFFFFFu - (uint32_t)a.best[slot]) != c;
            single = true;
            dup_single = dup;
        } else {
            unresolved = true;
        }
        a.kind[c] = m >= 0 ? 1 : single ? 2 : 3;
        a.duplicate[c] = dup ? 1 : 0;
    }
    // one add per wave and counter: every lane reaches the ballots
    const unsigned long long b0 = __ballot(single), b1 = __ballot(unresolved), b2 = __ballot(dup_pair), b3 = __ballot(dup_single);
    if ((threadIdx.x & 63) == 0) {
        if (b0) atomicAdd(&a.totals[0], __popcll(b0));
        if (b1) atomicAdd(&a.totals[1], __popcll(b1));
        if (b2) atomicAdd(&a.totals[2], __popcll(b2));
        if (b3) atomicAdd(&a.totals[3], __popcll(b3));
    }
}

struct MdBatch {                 // the eligible reads of one hello_markdup_add, on the device
    uint64_t* name = nullptr;
    uint16_t* flags = nullptr;
    int64_t* e = nullptr;
    int32_t* score = nullptr;
    int64_t n = 0;
    void free() { (void)hipFree(name); (void)hipFree(flags); (void)hipFree(e); (void)hipFree(score); }
};

}  // namespace
}  // namespace hello

struct hello_markdup {
    int device = 0;
    bool found = false;
    int64_t n_reads = 0;
    std::vector<hello::MdBatch> batches;
    std::vector<int64_t> eligible;               // the read of c, in the order given
    std::vector<uint16_t> flags;                 // of the eligible reads
    std::vector<int64_t> e, mate;                // aligned with the reads given
    std::vector<int32_t> score;
    std::vector<uint8_t> kind, duplicate;
    double stats[HELLO_MARKDUP_STATS] = {0};
    ~hello_markdup() {
        for (auto& b : batches) b.free();
    }
};

extern "C" {

int hello_markdup_add(const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                      const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends, const uint8_t* mapq,
                      const uint16_t* flags, const uint64_t* name_hash, const uint8_t* source, int64_t n_reads, int32_t device,
                      hello_markdup** handle) try {
    using namespace hello;
    (void)bases; (void)mapq; (void)source;                                 // neither decides a duplicate
    if (!handle || !read_offsets || !cigar_offsets || (n_reads > 0 && (!quals || !cigars || !ref_starts || !ref_ends || !flags ||
        !name_hash)))
        return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (n_reads < 0) return set_last_error(HELLO_ERR_ARG, "negative count");
    hello_markdup* h = *handle;
    if (h && h->found) return set_last_error(HELLO_ERR_ARG, "reads cannot be added after hello_markdup_find");
    if (h && device != h->device) return set_last_error(HELLO_ERR_ARG, "a further call names another device than the first");
    const ReadsView in{bases, quals, read_offsets, cigars, cigar_offsets, ref_starts, ref_ends, mapq, flags, name_hash, n_reads};
    const std::vector<int64_t> list = markdup_walk(in);                    // validated (cigar.h): the kernel indexes with these alone
    std::vector<uint64_t> name;
    std::vector<uint16_t> fl;
    for (int64_t r : list) {
        name.push_back(name_hash[r]);
        fl.push_back(flags[r]);
    }
    const int64_t n = (int64_t)list.size();
    if ((h ? (int64_t)h->eligible.size() : 0) + n > INT32_MAX)
        return set_last_error(HELLO_ERR_ARG, "more than %d eligible reads in one handle", INT32_MAX);
    std::unique_ptr<hello_markdup> own;
    if (!h) {
        open_device(device);
        own.reset(new hello_markdup());
        h = own.get();
        h->device = device;
    } else {
        HS_HIP(hipSetDevice(h->device));
    }

    std::vector<int64_t> e((size_t)n);
    std::vector<int32_t> score((size_t)n);
    float ends_ms = 0.0f;
    if (n > 0) {
        DevMem m;
        const size_t nr = (size_t)n_reads;
        MdEndsArgs a{};
        a.quals = m.put(quals, (size_t)read_offsets[nr]);
        a.read_off = m.put(read_offsets, nr + 1);
        a.cigars = m.put(cigars, (size_t)cigar_offsets[nr]);
        a.cigar_off = m.put(cigar_offsets, nr + 1);
        a.ref_start = m.put(ref_starts, nr);
        a.ref_end = m.put(ref_ends, nr);
        a.flags = m.put(flags, nr);
        a.list = m.put(list.data(), list.size());
        a.e = m.room<int64_t>((size_t)n);
        a.score = m.room<int32_t>((size_t)n);
        a.n_eligible = n;
        uint64_t* d_name = m.put(name.data(), name.size());
        uint16_t* d_flags = m.put(fl.data(), fl.size());
        KernelTimer timer;
        timer.start();
        hipLaunchKernelGGL(markdup_ends_kernel, dim3(blocks_for(n, kMdWaves)), dim3(kMdThreads), 0, 0, a);
        ends_ms = timer.stop();
        HS_HIP(hipMemcpy(e.data(), a.e, e.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
        HS_HIP(hipMemcpy(score.data(), a.score, score.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        h->batches.reserve(h->batches.size() + 1);
        MdBatch b;                                                          // what hello_markdup_find reads stays on the device
        b.name = m.release(d_name);
        b.flags = m.release(d_flags);
        b.e = m.release(a.e);
        b.score = m.release(a.score);
        b.n = n;
        h->batches.push_back(b);
    }
    // ---- the host's view, aligned with the reads given so far
    h->e.resize((size_t)(h->n_reads + n_reads), 0);
    h->score.resize((size_t)(h->n_reads + n_reads), 0);
    for (int64_t k = 0; k < n; ++k) {
        h->e[(size_t)(h->n_reads + list[k])] = e[k];
        h->score[(size_t)(h->n_reads + list[k])] = score[k];
        h->eligible.push_back(h->n_reads + list[k]);
    }
    h->flags.insert(h->flags.end(), fl.begin(), fl.end());
    h->n_reads += n_reads;
    h->stats[0] = (double)h->n_reads;
    h->stats[1] = (double)h->eligible.size();
    h->stats[8] += ends_ms;
    if (own) *handle = own.release();
    return HELLO_OK;
} HS_ENTRY_END("hello_markdup_add")

int hello_markdup_find(hello_markdup* h) try {
    using namespace hello;
    if (!h) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (h->found) return set_last_error(HELLO_ERR_ARG, "hello_markdup_find is called once, after the last hello_markdup_add");
    const int64_t n = (int64_t)h->eligible.size();
    if (n > kPairMaxReads) return set_last_error(HELLO_ERR_ARG, "%lld eligible reads in one chromosome", (long long)n);
    std::vector<int32_t> mate((size_t)n, -1);
    std::vector<uint8_t> kind((size_t)n), duplicate((size_t)n);
    int32_t joined[2] = {0, 0}, totals[4] = {0, 0, 0, 0};
    float pair_ms = 0.0f, key_ms = 0.0f, mark_ms = 0.0f;
    if (n > 0) {
        HS_HIP(hipSetDevice(h->device));
        DevMem m;
        uint64_t* name = m.room<uint64_t>((size_t)n);                       // the spans' arrays stay on the device: joined there
        uint16_t* flags = m.room<uint16_t>((size_t)n);
        int64_t* e = m.room<int64_t>((size_t)n);
        int32_t* score = m.room<int32_t>((size_t)n);
        int64_t at = 0;
        for (const MdBatch& b : h->batches) {
            HS_HIP(hipMemcpy(name + at, b.name, (size_t)b.n * sizeof(uint64_t), hipMemcpyDeviceToDevice));
            HS_HIP(hipMemcpy(flags + at, b.flags, (size_t)b.n * sizeof(uint16_t), hipMemcpyDeviceToDevice));
            HS_HIP(hipMemcpy(e + at, b.e, (size_t)b.n * sizeof(int64_t), hipMemcpyDeviceToDevice));
            HS_HIP(hipMemcpy(score + at, b.score, (size_t)b.n * sizeof(int32_t), hipMemcpyDeviceToDevice));
            at += b.n;
        }
        if (at != n) raise(HELLO_ERR_SHAPE, "the batches hold %lld eligible reads, the handle %lld", (long long)at, (long long)n);
        int32_t* d_mate = m.room<int32_t>((size_t)n);
        pair_ms = pair_join(m, name, flags, m.zeros<uint8_t>((size_t)n), n, d_mate, joined);
        HS_HIP(hipMemcpy(mate.data(), d_mate, mate.size() * sizeof(int32_t), hipMemcpyDeviceToHost));

        // ---- the key table: an END insert per joined read and per single, a PAIR insert per pair
        int64_t inserts = 3 * (int64_t)joined[0];
        for (int64_t c = 0; c < n; ++c)
            if (mate[c] < 0 && (!(h->flags[c] & 0x1) || (h->flags[c] & 0x8))) ++inserts;
        uint32_t table = 2;
        while ((int64_t)table < 2 * inserts) table <<= 1;                  // inserts <= 1.5 n <= 3 * 2^28: the table fits 32 bits
        MdKeyArgs a{};
        a.e = e;
        a.score = score;
        a.flags = flags;
        a.mate = d_mate;
        a.owner = m.room<int32_t>(table);
        HS_HIP(hipMemsetD32((hipDeviceptr_t)a.owner, kMdEmpty, table));
        a.paired = m.zeros<uint32_t>(table);
        a.best = m.zeros<unsigned long long>(table);
        a.kind = m.room<uint8_t>((size_t)n);
        a.duplicate = m.room<uint8_t>((size_t)n);
        a.totals = m.zeros<int32_t>(4);
        a.n = n;
        a.mask = table - 1;
        KernelTimer timer;
        timer.start();
        hipLaunchKernelGGL(markdup_key_kernel, dim3(blocks_for(n, kMdThreads)), dim3(kMdThreads), 0, 0, a);
        key_ms = timer.stop();
        timer.start();
        hipLaunchKernelGGL(markdup_mark_kernel, dim3(blocks_for(n, kMdThreads)), dim3(kMdThreads), 0, 0, a);
        mark_ms = timer.stop();
        HS_HIP(hipMemcpy(kind.data(), a.kind, (size_t)n, hipMemcpyDeviceToHost));
        HS_HIP(hipMemcpy(duplicate.data(), a.duplicate, (size_t)n, hipMemcpyDeviceToHost));
        HS_HIP(hipMemcpy(totals, a.totals, sizeof(totals), hipMemcpyDeviceToHost));
    }
    h->mate.assign((size_t)h->n_reads, -1);
    h->kind.assign((size_t)h->n_reads, 0);
    h->duplicate.assign((size_t)h->n_reads, 0);
    for (int64_t c = 0; c < n; ++c) {
        const size_t r = (size_t)h->eligible[c];
        if (mate[c] >= 0) h->mate[r] = h->eligible[mate[c]];
        h->kind[r] = kind[c];
        h->duplicate[r] = duplicate[c];
    }
    for (auto& b : h->batches) b.free();                                    // nothing reads them again
    h->batches.clear();
    h->stats[2] = (double)joined[0];
    h->stats[3] = (double)totals[0];
    h->stats[4] = (double)totals[1];
    h->stats[5] = (double)joined[1];
    h->stats[6] = (double)totals[2];
    h->stats[7] = (double)totals[3];
    h->stats[9] = pair_ms;
    h->stats[10] = key_ms;
    h->stats[11] = mark_ms;
    h->found = true;
    return HELLO_OK;
} HS_ENTRY_END("hello_markdup_find")

int hello_markdup_array(const hello_markdup* h, int32_t which, const void** data, int64_t* count) {
    if (!h || !data || !count) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    switch (which) {
        case HELLO_MARKDUP_E: *data = h->e.data(); *count = (int64_t)h->e.size(); break;
        case HELLO_MARKDUP_SCORE: *data = h->score.data(); *count = (int64_t)h->score.size(); break;
        case HELLO_MARKDUP_MATE: *data = h->mate.data(); *count = (int64_t)h->mate.size(); break;
        case HELLO_MARKDUP_KIND: *data = h->kind.data(); *count = (int64_t)h->kind.size(); break;
        case HELLO_MARKDUP_DUPLICATE: *data = h->duplicate.data(); *count = (int64_t)h->duplicate.size(); break;
        default: return hello::set_last_error(HELLO_ERR_ARG, "array selector %d", which);
    }
    return HELLO_OK;
}

int hello_markdup_stats(const hello_markdup* h, double* stats) {
    if (!h || !stats) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    std::copy(h->stats, h->stats + HELLO_MARKDUP_STATS, stats);
    return HELLO_OK;
}

void hello_markdup_free(hello_markdup* h) {
    if (h) (void)hipSetDevice(h->device);
    delete h;
}

}  // extern "C"
