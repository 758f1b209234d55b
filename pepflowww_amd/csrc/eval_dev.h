// Device helpers shared by the evaluation kernels (tm_score.hip, tm_align.hip, violations.hip, sasa.hip, torsions.hip): only what is
// the same computation in each of them.  The arithmetic that follows an oracle's operation order stays in its own file.  So do
// tm_score.hip's tm_point and the seed-length rule of tm_score.hip and of tm_align.hip: with load3d, or with either file's form of
// the rule in both, hipcc schedules tm_search_kernel or tm_align_kernel differently (profiles/r08/README.md), and the kernels'
// machine code is what was validated.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// three floats widened to double
__device__ __forceinline__ void load3d(const float* p, double v[3]) {
    v[0] = p[0];
    v[1] = p[1];
    v[2] = p[2];
}

// row of a [21, .] per-type table: the package's residue types 0..19 and 20, and 20 for anything outside
__device__ __forceinline__ int type_row(int64_t t) { return (t < 0 || t > 20) ? 20 : (int)t; }

// sum over a block of NT threads in a fixed order (tree over thread ids); red holds NT doubles; every thread gets the result
template <int NT>
__device__ __forceinline__ double block_sum(double v, double* red, int tid) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    return red[0];
}

// (score, candidate) total order of the TM searches: the higher score, of equal scores the first candidate (c smaller)
__device__ __forceinline__ bool cand_better(double s, long long c, double s2, long long c2) {
    return s > s2 || (s == s2 && c < c2);
}

// the wave's best (score, candidate): a maximum under a total order, so the result does not depend on the butterfly's pairing
__device__ __forceinline__ void wave_best(double& s, long long& c) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double s2 = __shfl_xor(s, m);
        const long long c2 = __shfl_xor(c, m);
        if (cand_better(s2, c2, s, c)) { s = s2; c = c2; }
    }
}
