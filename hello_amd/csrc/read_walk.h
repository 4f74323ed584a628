// One CIGAR operation as the kernels that walk a read's bases see it (qc.hip, methylation.hip, pileup.hip): its code, its length,
// whether it is M / = / X, and whether it consumes bases of the read.  Each of those kernels keeps its own wave-uniform loop over the operations,
// and the two kernels that walk a tile's reads (refblocks_kernel, qc_depth_kernel) are as they were: a shared loop that handed
// each operation to a callable cost registers and time.
#pragma once
#include <hip/hip_runtime.h>

#include "cigar.h"

namespace hello {
namespace {

struct CigarOp {
    int op, n;                   // n < 2^28
    bool m;                      // M, = or X: the operation's bases lie on reference positions
    __device__ __forceinline__ bool on_read() const { return m || op == BAM_CINS || op == BAM_CSOFT_CLIP; }    // it has bases of the read
};

__device__ __forceinline__ CigarOp decode_op(unsigned c) {
    const int op = (int)(c & 15u);
    return CigarOp{op, (int)(c >> 4), op == BAM_CMATCH || op == BAM_CEQUAL || op == BAM_CDIFF};
}

}  // namespace
}  // namespace hello
