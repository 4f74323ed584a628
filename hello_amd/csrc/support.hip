// Per-allele read support (include/hello_mi355x.h: hello_engine_allele_support): how many reads stand behind every allele of
// a launch, how many of them on the forward strand, and the sums of their mapping qualities and squared mapping qualities --
// what the record stage turns into DP / AD / ADF / ADR / MQ.  The reference writes none of these; its users went back to the
// BAM for them.  The per-read arrays are the featurizer's own (on the resident route they exist only in device memory).
//
// One wave per allele, four alleles per workgroup.  The 64 lanes stride the allele's reads (byte loads of mapq and
// orientation and 8-byte loads of the CIGAR offsets, all coalesced), the wave adds up with shuffles and lane 0 writes the
// four int64 values: integers written by index, no atomics, no LDS -- two runs give the same bytes.  HBM-side glue:
// 10 distinct bytes per read (a lane loads both ends of its read's CIGAR range; the neighbour's end comes from the cache),
// 8 in and 32 out per allele.
#include "kernels.h"

namespace hello {

__global__ __launch_bounds__(256) void allele_support_kernel(SupportArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long allele = (long long)blockIdx.x * 4 + wave;
    if (allele >= a.n_alleles) return;                       // wave-uniform
    // device-side guard (host callers are validated): offsets outside [0, n_reads] read nothing
    long long lo = a.allele_off[allele], hi = a.allele_off[allele + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > a.n_reads ? a.n_reads : hi;
    long long n = 0, forward = 0, sum = 0, squares = 0;
    for (long long r = lo + lane; r < hi; r += 64) {
        if (a.cigar_off[r + 1] > a.cigar_off[r]) {           // a read without operations is the dummy row: it supports nothing
            const long long q = a.mapq[r];
            n += 1;
            forward += a.orientation[r] > 0 ? 1 : 0;
            sum += q;
            squares += q * q;
        }
    }
    for (int step = 32; step > 0; step >>= 1) {
        n += __shfl_down(n, step, 64);
        forward += __shfl_down(forward, step, 64);
        sum += __shfl_down(sum, step, 64);
        squares += __shfl_down(squares, step, 64);
    }
    if (lane == 0) {
        long long* o = a.out + allele * 4;
        o[0] = n;
        o[1] = forward;
        o[2] = sum;
        o[3] = squares;
    }
}

hipError_t launch_allele_support(const SupportArgs& a, hipStream_t stream) {
    if (a.n_alleles <= 0) return hipSuccess;
    const long long groups = (a.n_alleles + 3) / 4;
    if (groups > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(allele_support_kernel, dim3((unsigned)groups), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace hello
