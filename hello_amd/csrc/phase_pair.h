// The mate join of DESIGN.md section 7i, in one copy: the phasing stage (phase.hip, hello_phase_fragments) and the duplicate
// marker (markdup.hip, hello_markdup_find) both group reads by (name_hash, source) with it.  An open-addressing table of
// 2^k >= 2 n slots in global memory, two kernels with a thread per read, c = 0..n-1:
//   insert: claims the slot of c's (name_hash, source) with atomicCAS on an int32 owner (-1 empty, else the claiming read) or
//     finds the slot whose owner has its key -- keys are compared in the input arrays, so no key value is reserved -- and counts
//     itself into the slot: reads, first mates, second mates, the smallest index of each kind (atomicAdd / atomicMin, the result
//     does not depend on arrival order; which read owns a slot does, and nothing reads the owner but the probe).
//   look-up: finds the slot again and writes mate[c]; the slot's owner counts the group into pairs / groups_refused.
#pragma once
#include <climits>

#include "stage_host.h"

namespace hello {
namespace {

constexpr int kPairThreads = 256;

struct PhPairArgs {
    const uint64_t* name;        // [n]: name_hash, flags and source of the reads to join, gathered on the host
    const uint16_t* flags;
    const uint8_t* source;
    int32_t* owner;              // [mask + 1]: -1 empty, else the read that claimed the slot
    int32_t* count;              // reads of the slot's group
    int32_t* n_first;            // those with flag 0x1 and flag & 0xC0 == 0x40
    int32_t* n_second;           // ... == 0x80
    int32_t* min_first;          // the smallest index of each kind
    int32_t* min_second;
    int32_t* mate;               // [n]
    int32_t* totals;             // pairs, groups_refused
    int64_t n_counted;
    uint32_t mask;
};

// The first slot probed for a key (phase.pair_table_slot restates it): every bit of the name reaches the slot.
__host__ __device__ inline uint32_t pair_slot(uint64_t name, uint32_t source, uint32_t mask) {
    uint64_t x = name ^ (name >> 29);
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 32;
    return ((uint32_t)x + source) & mask;
}

// The slot of c's group.  claim: an empty slot on the way becomes c's.  The table holds at least twice the reads, so a
// probe ends at an empty slot or at its group's before it has come round; it wraps at the table's end.
template <bool claim> __device__ inline uint32_t pair_probe(const PhPairArgs& a, int32_t c) {
    const uint64_t name = a.name[c];
    const uint32_t source = a.source[c];
    uint32_t slot = pair_slot(name, source, a.mask);
    for (uint32_t tried = 0; tried <= a.mask; ++tried) {
        const int32_t o = claim ? atomicCAS(&a.owner[slot], -1, c) : a.owner[slot];
        if (o < 0 || o == c) break;                                       // claimed just now (or, looking up, not there: never)
        if (a.name[o] == name && a.source[o] == source) break;
        slot = (slot + 1) & a.mask;
    }
    return slot;
}

__global__ __launch_bounds__(kPairThreads) void phase_pair_insert_kernel(PhPairArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kPairThreads + threadIdx.x;
    if (i >= a.n_counted) return;
    const int32_t c = (int32_t)i;
    const uint32_t slot = pair_probe<true>(a, c);
    atomicAdd(&a.count[slot], 1);
    const int f = a.flags[c];
    if ((f & 0x1) && (f & 0xC0) == 0x40) { atomicAdd(&a.n_first[slot], 1); atomicMin(&a.min_first[slot], c); }
    if ((f & 0x1) && (f & 0xC0) == 0x80) { atomicAdd(&a.n_second[slot], 1); atomicMin(&a.min_second[slot], c); }
}

__global__ __launch_bounds__(kPairThreads) void phase_pair_lookup_kernel(PhPairArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kPairThreads + threadIdx.x;
    bool joined = false, refused = false;                                               // of the group this thread owns
    if (i < a.n_counted) {
        const int32_t c = (int32_t)i;
        const uint32_t slot = pair_probe<false>(a, c);
        const int n = a.count[slot];
        const bool pair = n == 2 && a.n_first[slot] == 1 && a.n_second[slot] == 1;
        a.mate[c] = !pair ? -1 : a.min_first[slot] == c ? a.min_second[slot] : a.min_first[slot];
        joined = a.owner[slot] == c && pair;                                            // a group is counted once, by its owner
        refused = a.owner[slot] == c && !pair && n >= 2;
    }
    // one add per wave and counter instead of one per group: every lane reaches the ballots
    const unsigned long long j = __ballot(joined), r = __ballot(refused);
    if ((threadIdx.x & 63) == 0) {
        if (j) atomicAdd(&a.totals[0], __popcll(j));
        if (r) atomicAdd(&a.totals[1], __popcll(r));
    }
}

constexpr int64_t kPairMaxReads = 1 << 29;          // a table of 2^k >= 2 n slots is indexed with 32 bits

unsigned blocks_for(int64_t items, int per_block) {
    const int64_t n = (items + per_block - 1) / per_block;
    if (n > INT32_MAX) raise(HELLO_ERR_ARG, "%lld items in one launch", (long long)items);
    return (unsigned)n;
}

// The join of n >= 1 reads whose name / flags / source are on the device: the table lives in `m`, the two launches run on the
// default stream, mate[c] (device, [n]) is written in full.  -> the kernel time; totals: pairs, groups_refused.
float pair_join(DevMem& m, const uint64_t* name, const uint16_t* flags, const uint8_t* source, int64_t n, int32_t* mate,
                int32_t totals[2]) {
    uint32_t table = 2;
    while ((int64_t)table < 2 * n) table <<= 1;
    PhPairArgs p{};
    p.name = name;
    p.flags = flags;
    p.source = source;
    p.owner = m.room<int32_t>(table);
    HS_HIP(hipMemset(p.owner, 0xFF, (size_t)table * sizeof(int32_t)));
    p.count = m.zeros<int32_t>(table);
    p.n_first = m.zeros<int32_t>(table);
    p.n_second = m.zeros<int32_t>(table);
    p.min_first = m.room<int32_t>(table);
    p.min_second = m.room<int32_t>(table);
    HS_HIP(hipMemset(p.min_first, 0x7F, (size_t)table * sizeof(int32_t)));      // above every index
    HS_HIP(hipMemset(p.min_second, 0x7F, (size_t)table * sizeof(int32_t)));
    p.mate = mate;
    p.totals = m.zeros<int32_t>(2);
    p.n_counted = n;
    p.mask = table - 1;
    KernelTimer timer;
    timer.start();
    hipLaunchKernelGGL(phase_pair_insert_kernel, dim3(blocks_for(n, kPairThreads)), dim3(kPairThreads), 0, 0, p);
    hipLaunchKernelGGL(phase_pair_lookup_kernel, dim3(blocks_for(n, kPairThreads)), dim3(kPairThreads), 0, 0, p);
    const float ms = timer.stop();
    HS_HIP(hipMemcpy(totals, p.totals, 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return ms;
}

}  // namespace
}  // namespace hello
