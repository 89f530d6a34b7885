// k_appearance_dev.hpp — the summation of the appearance score as ONE text: the five binary64 sums Sa, Sp, Saa, Spp, Sap of
// two [nt][kpad] bf16 matrices over their first `cols` columns, in a FIXED order of additions, and the similarity they give.
// Shared by the score launch of the appearance check (k_appearance.hip) and the score launch of the peak arbitration
// (k_arbitrate.hip); both files are compiled with -ffp-contract=off, so equal rows give equal bits in both.
//
// The order: a lane adds its elements i = lane, lane + 256, ... of the chunk's (rows x cols) in ascending i; the 64 lanes of a
// wave as an xor butterfly 32, 16, 8, 4, 2, 1; the 4 waves in index order; the chunk partials go to global memory and the
// last-arriving workgroup (a ticket per summed pair) adds them in chunk order. No floating-point atomics.
#pragma once
#include "vt_common.hpp"

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// Every thread of a 256-thread workgroup calls this: the chunk's partial sums of rows [r0, r1) of A and P (both point at row
// r0). wsum: 20 doubles of LDS. Thread 0 returns with out[0..5) set; the other threads' out is unspecified.
__device__ __forceinline__ void appear_chunk_sums(const bf16_t* __restrict__ A, const bf16_t* __restrict__ P, int rows, int cols,
                                                  int kpad, double (*wsum)[5], double* out) {
    const int cnt = rows * cols;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const int rr = i / cols, c = i - rr * cols;
        const size_t o = (size_t)rr * kpad + c;
        const double x = (double)bf16_to_f32(A[o]), y = (double)bf16_to_f32(P[o]);
        s[0] = s[0] + x;
        s[1] = s[1] + y;
        s[2] = s[2] + x * x;
        s[3] = s[3] + y * y;
        s[4] = s[4] + x * y;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) s[k] = wave_sum_f64(s[k]);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < 5; ++k) wsum[wave][k] = s[k];
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 0; k < 5; ++k) out[k] = ((wsum[0][k] + wsum[1][k]) + wsum[2][k]) + wsum[3][k];
}

// the last arriver (one thread): the nch chunk partials [nch][5] in index order into t
__device__ __forceinline__ void appear_add_chunks(const double* all, int nch, double* t) {
#pragma unroll
    for (int k = 0; k < 5; ++k) t[k] = 0.0;
    for (int c = 0; c < nch; ++c)
#pragma unroll
        for (int k = 0; k < 5; ++k)
            t[k] = t[k] + __hip_atomic_load(all + (size_t)c * 5 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the five sums -> the similarity, clamped to [-1, 1] and rounded once to binary32; false (similarity 0) where a variance is
// not positive
__device__ __forceinline__ bool appear_similarity(const double* t, int nt, int cols, float* similarity) {
    const double n = (double)nt * (double)cols;
    const double cov = t[4] - t[0] * t[1] / n;
    const double va = t[2] - t[0] * t[0] / n;
    const double vp = t[3] - t[1] * t[1] / n;
    const bool ok = va > 0.0 && vp > 0.0;
    double sim = ok ? cov / sqrt(va * vp) : 0.0;
    sim = sim > 1.0 ? 1.0 : (sim < -1.0 ? -1.0 : sim);
    *similarity = (float)sim;
    return ok;
}
