// k_misc.hpp — launchers of the LayerNorm, row-term, fold and range kernels (k_misc.hip).
#pragma once
#include "vt_common.hpp"

// y[r] (bf16) = LN(x[in_row(r)]) ; in_row(r) = (r / group) * in_stride + in_off + r % group
hipError_t launch_layernorm(const float* x, const float* gamma, const float* beta, bf16_t* y,
                            int rows, int D, int group, int in_stride, int in_off, float eps,
                            hipStream_t st);
// the same on the split residual stream: x = xh + xl * lo_q (3-byte pair, lo_q = 2^-s)
hipError_t launch_layernorm_split(const bf16_t* xh, const uint8_t* xl, const float* gamma, const float* beta,
                                  bf16_t* y, int rows, int D, int group, int in_stride, int in_off,
                                  float eps, float lo_q, hipStream_t st);
// Range report of a stored pair (k_misc.hip, off the hot path): out[0] = max |x| as the bit pattern of a non-negative
// float, out[1] = n(|lo8| == 127), out[1 + k] = n(|x| >= 2^k), k = 1..9, accumulated into out (zero it first) over
// rows [0, rows) of xh / xl (contiguous rows of length D, D % 8 == 0), for `stages` copies of the pair that lie
// stage_stride bytes apart in BOTH planes (the tap slots), into out[stage][VT_XRANGE_WORDS]
#define VT_XRANGE_WORDS 11
hipError_t launch_xrange(const bf16_t* xh, const uint8_t* xl, unsigned* out, int rows, int D, float lo_q, int stages,
                         size_t stage_stride, hipStream_t st);
// rowstat[m] = (rstd, -mean * rstd) from the chunk partials of an X-epilogue (D = 32 * nchunk columns)
hipError_t launch_rowstat_finalize(const float2* cstat, float2* rowstat, int M, int nchunk, float eps,
                                   hipStream_t st);
// LayerNorm folded into the weights of the GEMM that consumes it (once, at engine creation):
// Wf[n][k] = bf16(gamma[k] * W[n][k]); colsum[n] = sum_k Wf[n][k]; cvec[n] = sum_k beta[k] W[n][k] + bias[n]
hipError_t launch_fold_layernorm(const bf16_t* W, const float* gamma, const float* beta, const float* bias,
                                 bf16_t* Wf, float* colsum, float* cvec, int N, int K, hipStream_t st);
