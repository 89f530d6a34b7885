// k_attn.hpp — the attention launch API (k_attn.hip) and the permuted Vt key order its QKV producers share.
#pragma once
#include "vt_common.hpp"

// out[M][D] bf16 = softmax(q k^T) v, q/k rows in qk[M][2D], v transposed in vt[B*H][64][npad]
hipError_t launch_attention(const bf16_t* qk, const bf16_t* vt, bf16_t* out, int B, int tokens,
                            int H, int npad, hipStream_t st);

// Which attention kernel launch_attention() will run for this shape,
// and whether it wants Vt with the permuted key order (mode 3). The QKV GEMM that feeds it must be
// given the same vt_perm.
int attention_pick_mode(int tokens, int npad);
inline int attention_vt_perm(int mode) { return mode >= 3 ? 1 : 0; }
// position of key t inside its group of 16 in the permuted Vt layout: bits 2 and 3 swapped
__host__ __device__ inline int attn_perm16(int t) { return (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1); }

hipError_t attention_prepare();   // once per device, before the first launch / any stream capture
hipError_t launch_attention_mode(const bf16_t* qk, const bf16_t* vt, bf16_t* out, int B, int tokens,
                                 int H, int npad, int mode, hipStream_t st);

// mode 3 (tokens % 4 == 0, npad % 64 == 0) on the queries q0 .. q0 + nq - 1 of every stream only, keys and values all
// `tokens`: out is compact, [B * nq][H * 64], row b * nq + (q - q0). Same bits as those rows of launch_attention_mode(3)
// while every query's scores stay inside the kernel's +-32 window (k_attn.hip, attention_dma_q_kernel)
hipError_t launch_attention_queries(const bf16_t* qk, const bf16_t* vt, bf16_t* out, int B, int tokens, int H, int npad,
                                    int q0, int nq, hipStream_t st);
