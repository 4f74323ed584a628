// The ranked bit vector of a chromosome's sites, once for the stages that count at sites (methylation.hip, pileup.hip): a bit per
// position in 64-position words, and before[w], the sites below word w.  The rank of the site at p -- its index in the ascending
// list of sites -- is before[p >> 6] + popcount(bits[p >> 6] & below(p)).  How the bits come to be set is the stage's own kernel;
// the scan over the words' popcounts and its launch are here.
#pragma once
#include "stage_host.h"

namespace hello {
namespace {

struct SiteBits {
    const unsigned long long* bits;      // [n_words]
    const int* before;                   // [n_words + 1]
    int64_t length, n_words;             // positions of the chromosome; (length + 63) / 64

    __device__ __forceinline__ unsigned long long word(int64_t p) const { return bits[p >> 6]; }
    __device__ __forceinline__ static bool has(unsigned long long word, int64_t p) { return (word >> (p & 63)) & 1ull; }
    __device__ __forceinline__ bool has(int64_t p) const { return has(word(p), p); }
    __device__ __forceinline__ int rank(unsigned long long word, int64_t p) const {      // word: word(p), already loaded
        return before[p >> 6] + __popcll(word & ((1ull << (p & 63)) - 1ull));
    }
    __device__ __forceinline__ int rank(int64_t p) const { return rank(word(p), p); }
    // Whether [s, e) holds a site; e <= length, so every word exists.
    __device__ __forceinline__ bool any_in(int64_t s, int64_t e) const {
        if (s >= e) return false;
        const int64_t w0 = s >> 6, w1 = (e - 1) >> 6;
        unsigned long long any = 0;
        for (int64_t w = w0; w <= w1; ++w) {
            unsigned long long b = bits[w];
            if (w == w0) b &= ~0ull << (s & 63);
            if (w == w1 && ((e & 63) != 0)) b &= (1ull << (e & 63)) - 1ull;
            any |= b;
        }
        return any != 0;
    }
};

constexpr int kSiteScanThreads = 1024;

// One workgroup walks the words' popcounts kSiteScanThreads at a time with a carry: before[w] for every word and, in
// before[n_words], the number of sites (below 2^31: a chromosome has fewer positions).
__global__ __launch_bounds__(kSiteScanThreads) void site_scan_kernel(const unsigned long long* bits, int* before, int64_t n_words) {
    __shared__ int wave_sum[kSiteScanThreads / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int carry = 0;
    for (int64_t base = 0; base < n_words; base += kSiteScanThreads) {      // block-uniform
        const int64_t i = base + tid;
        const int v = i < n_words ? __popcll(bits[i]) : 0;
        int s = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(s, d, 64);
            if (lane >= d) s += t;
        }
        if (lane == 63) wave_sum[wave] = s;
        __syncthreads();
        int pre = 0, total = 0;
        for (int k = 0; k < kSiteScanThreads / 64; ++k) {
            if (k < wave) pre += wave_sum[k];
            total += wave_sum[k];
        }
        if (i < n_words) before[i] = carry + pre + s - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) before[n_words] = carry;
}

// Behind the stage's kernel that set `bits`, launched under `timer`: the scan, the end of the timing (added to ms) -> the sites.
int build_scan(KernelTimer& timer, const unsigned long long* bits, int* before, int64_t n_words, float& ms) {
    hipLaunchKernelGGL(site_scan_kernel, dim3(1), dim3(kSiteScanThreads), 0, 0, bits, before, n_words);
    ms += timer.stop();
    int n_sites = 0;
    HS_HIP(hipMemcpy(&n_sites, before + n_words, sizeof(int), hipMemcpyDeviceToHost));
    return n_sites;
}

}  // namespace
}  // namespace hello
