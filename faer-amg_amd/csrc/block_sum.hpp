// block_sum.hpp -- the fixed reduction tree of the deterministic dots.
//
// Shared by blas1.hip (vec_dot) and pcg.hip (the column dots of the block solve
// drivers): both sum a 256-thread block through this one function, so a column
// dot of the block drivers is vec_dot of that column bit for bit.
#pragma once

#include <hip/hip_runtime.h>

namespace famg {

// Sum of v over the block: the xor butterfly inside each wave, then thread 0 adds
// the waves' sums in wave order.  sh: one double per wave.  The result is valid
// in thread 0 only.
__device__ __forceinline__ double block_sum(double v, double *sh) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int k = 0; k < (int)(blockDim.x >> 6); k++) t += sh[k];
    return t;
}

}  // namespace famg
