// Per-allele base-level read evidence (include/hello_mi355x.h: hello_engine_allele_evidence): for every allele of a launch, how
// good the bases are that its reads put inside the site's span and how close to a read end they sit, and how its reads split
// over the two haplotags -- what the record stage turns into MBQ / MPOS / AH1 / AH2.  The reference writes none of these.  The
// per-read arrays are the featurizer's own (on the resident route they exist only in device memory); nothing else reads a base
// quality after the featurizer has folded it into a pileup byte.
//
// The walk of one read r over the span [s, e) of its site, n = the read's bases, p = ref_start[r], i = 0, operation by operation:
//   M = X (0 7 8), L   base i+j sits at p+j and BELONGS iff s <= p+j < e;  p += L, i += L
//   I (1), L           all L bases belong iff s <= p <= e (the insertion joins the base on its left, as in the candidate stage:
//                      one right behind the last span base counts, and so does one at an empty span s == e);  i += L
//   S (4)              i += L, never belongs          D N (2 3)   p += L          H P (5 6) and codes >= 9   nothing
// The walk STOPS in front of the first reference-consuming operation (M = X D N) that begins at p >= e: nothing behind it can
// belong, and it is not examined.  GUARD: an operation of the walk that would move i past n ends it; the read is then counted in
// column 5 and in no other column, and no byte outside [read_off[r], read_off[r+1]) is read.  A site_of_read outside [0, S)
// does the same.  A read with zero operations is the dummy row of an unsupported allele and contributes nothing at all.
// Per read with a belonging base: qmin = its lowest belonging quality, d = min(i0, n-1-i1) with i0 / i1 the first / last
// belonging read index (soft-clipped bases are read bases).  Per allele: [reads with a belonging base, sum qmin, sum d, reads
// with hp == 1, reads with hp == 2, guarded reads].
//
// One wave per allele, four alleles per workgroup, as allele_support_kernel: the 64 lanes stride the allele's reads, each lane
// walks its own read (a short-read CIGAR is one to three operations, and only the span's bases -- a few -- are loaded), the wave
// adds up with shuffles and lane 0 writes six int64 values: integers written by index, no atomics, no LDS -- two runs give
// the same bytes.
#include "kernels.h"

namespace hello {

__global__ __launch_bounds__(256) void allele_evidence_kernel(EvidenceArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long allele = (long long)blockIdx.x * 4 + wave;
    if (allele >= a.n_alleles) return;                       // wave-uniform
    // device-side guard (host callers are validated): offsets outside [0, n_reads] read nothing
    long long lo = a.allele_off[allele], hi = a.allele_off[allele + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > a.n_reads ? a.n_reads : hi;
    long long nq = 0, sum_q = 0, sum_d = 0, hp1 = 0, hp2 = 0, guarded = 0;
    for (long long r = lo + lane; r < hi; r += 64) {
        const long long c0 = a.cigar_off[r], c1 = a.cigar_off[r + 1];
        if (c1 <= c0) continue;                              // the dummy row
        const long long site = a.site_of_read[r];
        bool bad = site < 0 || site >= a.n_sites;
        const long long b0 = a.read_off[r], n = a.read_off[r + 1] - b0;
        int qmin = 256;
        long long i0 = -1, i1 = -1;
        if (!bad) {
            const long long s = a.asm_start[site], e = a.asm_stop[site];
            const uint8_t* q = a.quals + b0;
            long long p = a.ref_start[r], i = 0;
            for (long long c = c0; c < c1; ++c) {
                const uint32_t word = a.cigars[c];
                const int op = word & 15u;
                const long long len = word >> 4;
                const bool aligned = op == 0 || op == 7 || op == 8;
                if ((aligned || op == 2 || op == 3) && p >= e) break;
                if (aligned || op == 1 || op == 4) {
                    if (len > n - i) { bad = true; break; }  // i <= n always: n - i cannot overflow
                    long long j0 = 0, j1 = 0;                // the belonging bases of this operation: read indices [i+j0, i+j1)
                    if (aligned) {
                        j0 = s > p ? s - p : 0;
                        j1 = e - p < len ? e - p : len;
                        p += len;
                    } else if (op == 1 && s <= p && p <= e) {
                        j1 = len;
                    }
                    if (j1 > j0) {
                        for (long long j = j0; j < j1; ++j) {
                            const int v = q[i + j];
                            qmin = v < qmin ? v : qmin;
                        }
                        if (i0 < 0) i0 = i + j0;
                        i1 = i + j1 - 1;
                    }
                    i += len;
                } else if (op == 2 || op == 3) {
                    p += len;
                }
            }
        }
        if (bad) {
            guarded += 1;
            continue;
        }
        const int hp = a.hp[r];
        hp1 += hp == 1 ? 1 : 0;
        hp2 += hp == 2 ? 1 : 0;
        if (i0 >= 0) {
            const long long tail = n - 1 - i1;
            nq += 1;
            sum_q += qmin;
            sum_d += i0 < tail ? i0 : tail;
        }
    }
    for (int step = 32; step > 0; step >>= 1) {
        nq += __shfl_down(nq, step, 64);
        sum_q += __shfl_down(sum_q, step, 64);
        sum_d += __shfl_down(sum_d, step, 64);
        hp1 += __shfl_down(hp1, step, 64);
        hp2 += __shfl_down(hp2, step, 64);
        guarded += __shfl_down(guarded, step, 64);
    }
    if (lane == 0) {
        long long* o = a.out + allele * 6;
        o[0] = nq;
        o[1] = sum_q;
        o[2] = sum_d;
        o[3] = hp1;
        o[4] = hp2;
        o[5] = guarded;
    }
}

hipError_t launch_allele_evidence(const EvidenceArgs& a, hipStream_t stream) {
    if (a.n_alleles <= 0) return hipSuccess;
    const long long groups = (a.n_alleles + 3) / 4;
    if (groups > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(allele_evidence_kernel, dim3((unsigned)groups), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace hello
