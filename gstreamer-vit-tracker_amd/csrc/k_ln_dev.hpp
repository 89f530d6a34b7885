// k_ln_dev.hpp — device only: one LayerNorm row by half a wave and the 3-byte residual pair's encode / decode.
#pragma once
#include "vt_common.hpp"
#include "k_gemm.hpp"

// ---- one LayerNorm row by half a wave (D = 256 * NCH) -------------------------------------------
// Lane l32 of the half-wave owns the 8-float chunks c = l32 + 32 j, j < NCH. Two-pass variance; the sums run
// over a lane's chunks in ascending order, then over the 32 lanes as an xor butterfly (16, 8, 4, 2, 1). The ONE
// definition of this arithmetic: the LayerNorm kernel (k_misc.hip) and the head's first layer, which normalises
// its band's rows itself (k_head.hip), produce the same bits by construction.
// Sum over the 32 lanes of a half-wave, every lane gets the total: the xor butterfly 16, 8, 4, 2, 1 in registers -
// v_permlane16_swap (odd 16-lane rows of one operand <-> even rows of the other: both copies of v, so a lane ends up
// holding its own and its xor-16 partner's value), row_ror:8, two masked row shifts by 4 (DPP has no xor-4 pattern:
// banks 0 / 2 of a row take lane + 4, banks 1 / 3 lane - 4), two quad_perms. Same partners in the same order as
// "for (off = 16; off >= 1; off >>= 1) v += __shfl_xor(v, off)" and therefore the same bits (tools/dpp_xor_check.hip), without
// that form's five dependent LDS round trips (ds_bpermute) per sum.
// PRECONDITION - FULL EXEC: every lane of the wave must be active at the call. A DPP / permlane source lane that is
// masked off reads as 0 (bound_ctrl) or keeps the old value, so under divergence (`if (r < rows) ln_row(...)`) the sums
// would silently miss terms. All callers keep the wave uniform: rows past the end are CLAMPED to the last row and only
// the stores are guarded (k_misc.hip layernorm kernels, k_head.hip LNC path). The same holds for quad_sum / row16_sum /
// row8_sum of k_gemm_util.hpp and k_head.hip. The s_nop counts inside the asm are the gfx950 wait states (VALU write ->
// permlane read: 2; permlane write -> VALU read: 2) the compiler cannot check there; tools/dpp_xor_check.hip (run by
// tests/test_gpu_ops.py on the box, built with the box's ROCm) guards both the workaround and those counts.
__device__ __forceinline__ float half_wave_sum(float v) {
    // inline asm, not __builtin_amdgcn_permlane16_swap: on float operands hipcc (ROCm 7.2) adds the swap's FIRST result to
    // itself (the integer form compiles correctly; tools/dpp_xor_check.hip caught it). s_nop: VALU write -> permlane read
    // and permlane write -> VALU read wait states, which the compiler cannot see inside the asm.
    float lo, hi;
    asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %2\n\ts_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1"
                 : "=&v"(lo), "=&v"(hi) : "v"(v));
    v = lo + hi;
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x128, 0xF, 0xF, true));       // row_ror:8
    int t = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x104, 0xF, 0x5, false);                       // row_shl:4 -> banks 0, 2
    t = __builtin_amdgcn_update_dpp(t, __builtin_bit_cast(int, v), 0x114, 0xF, 0xA, false);                           // row_shr:4 -> banks 1, 3
    v += __builtin_bit_cast(float, t);
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));        // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));        // quad_perm [1,0,3,2]
    return v;
}

template <int NCH>
struct LnCoef { f32x4_t g[NCH][2], b[NCH][2]; };

template <int NCH>
__device__ __forceinline__ void ln_load_coef(const float* gamma, const float* beta, int l32, LnCoef<NCH>& k) {
    const f32x4_t* g4 = reinterpret_cast<const f32x4_t*>(gamma);
    const f32x4_t* b4 = reinterpret_cast<const f32x4_t*>(beta);
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c = l32 + 32 * j;
        k.g[j][0] = g4[2 * c]; k.g[j][1] = g4[2 * c + 1];
        k.b[j][0] = b4[2 * c]; k.b[j][1] = b4[2 * c + 1];
    }
    // hipcc otherwise sinks these loads behind the row's reductions: pin the values here, all loads issued
#pragma unroll
    for (int j = 0; j < NCH; ++j)
        asm volatile("" : "+v"(k.g[j][0]), "+v"(k.g[j][1]), "+v"(k.b[j][0]), "+v"(k.b[j][1]) : : "memory");
}

// ---- the 3-byte residual pair (specification v3, top of k_gemm.hpp) ------------------------------------------------
// decode: element k of a lane's 8 consecutive columns = bf16 half k of h (16 B) + signed byte k of l (8 B) * q, q = 2^-s
__device__ __forceinline__ float lo8_f32(uint32_t w, int byte) {
    return (float)((int)(w << (24 - 8 * byte)) >> 24);          // sign-extended byte (v_bfe_i32 / SDWA sext) -> float
}
__device__ __forceinline__ void x_join8(const u32x4_t& hi, const u32x2_t& lo, float q, float (&x)[8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t lw = lo[e >> 1];
        x[2 * e] = __builtin_fmaf(lo8_f32(lw, (2 * e) & 3), q, __uint_as_float(hi[e] << 16));
        x[2 * e + 1] = __builtin_fmaf(lo8_f32(lw, (2 * e + 1) & 3), q, __uint_as_float(hi[e] & 0xffff0000u));
    }
}
// encode: hi = bf16(x) (round to nearest even); d = x - hi (exact); lo8 = rint(clamp(d, +-127 q) / q) by the float add of
// magic = 1.5 * 2^(23 - s): the sum's ulp is q = 2^-s, the add rounds to nearest even, and the low byte of the sum's bit
// pattern (at s = 12: 0x45400000 + n) is the two's-complement lo8 - for every s in 6..14 alike. The clamp and the magic
// are wave-uniform (LoQuant): v_med3_f32 takes the one SGPR as -lo_max and lo_max (a source modifier, one constant-bus
// read), the SDWA add its magic from a register as before. The add is issued in its SDWA form with dst_sel:BYTE_k, which writes that
// low byte straight into byte k of the destination dword - no extraction, no packing: 2 vector operations per element
// (v_med3_f32 + v_add_f32_sdwa) where clamp + add + v_perm gathering took 2.75 (same-box A/B in profiles/r06_lo8_residual.txt:
// + 0.5 % of the whole frame; without the clamp another + 0.2 %, not taken: a value beyond the range must saturate, not wrap).
__device__ __forceinline__ void x_split8(const float (&x)[8], const LoQuant& lq, u32x4_t& hi, u32x2_t& lo) {
    uint32_t h[4];
    float c[8];
    const float lo_max = lq.lo_max;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        h[e] = pack_bf16x2(x[2 * e], x[2 * e + 1]);
        c[2 * e] = __builtin_amdgcn_fmed3f(x[2 * e] - __uint_as_float(h[e] << 16), -lo_max, lo_max);
        c[2 * e + 1] = __builtin_amdgcn_fmed3f(x[2 * e + 1] - __uint_as_float(h[e] & 0xffff0000u), -lo_max, lo_max);
    }
    hi = u32x4_t{h[0], h[1], h[2], h[3]};
    const float magic = lq.magic;           // SDWA takes no literal: a register
    uint32_t w0, w1;
#define VT_LO8_BYTE(W, K, UNUSED, C) asm("v_add_f32_sdwa %0, %1, %2 dst_sel:BYTE_" #K " dst_unused:" #UNUSED " src0_sel:DWORD src1_sel:DWORD" : W : "v"(C), "v"(magic))
    VT_LO8_BYTE("=v"(w0), 0, UNUSED_PAD, c[0]); VT_LO8_BYTE("+v"(w0), 1, UNUSED_PRESERVE, c[1]);
    VT_LO8_BYTE("+v"(w0), 2, UNUSED_PRESERVE, c[2]); VT_LO8_BYTE("+v"(w0), 3, UNUSED_PRESERVE, c[3]);
    VT_LO8_BYTE("=v"(w1), 0, UNUSED_PAD, c[4]); VT_LO8_BYTE("+v"(w1), 1, UNUSED_PRESERVE, c[5]);
    VT_LO8_BYTE("+v"(w1), 2, UNUSED_PRESERVE, c[6]); VT_LO8_BYTE("+v"(w1), 3, UNUSED_PRESERVE, c[7]);
#undef VT_LO8_BYTE
    lo = u32x2_t{w0, w1};
}
// the LayerNorm readers' form: 8 values of a chunk as two float4
__device__ __forceinline__ void ln_unpack_split(const u32x4_t h, const u32x2_t l, float q, f32x4_t (&v)[2]) {
    float x[8];
    x_join8(h, l, q, x);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e >> 2][e & 3] = x[e];
}

// v: the row's values of this lane (overwritten); o[j]: the normalised chunk l32 + 32 j as 8 bf16
template <int NCH>
__device__ __forceinline__ void ln_row(f32x4_t (&v)[NCH][2], const LnCoef<NCH>& k, int D, float eps, uint4 (&o)[NCH]) {
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) sum += v[j][0][e] + v[j][1][e];
    sum = half_wave_sum(sum);
    const float mean = sum / (float)D;
    float sq = 0.0f;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[j][h][e] -= mean;
                sq += v[j][h][e] * v[j][h][e];
            }
    sq = half_wave_sum(sq);
    const float rstd = 1.0f / sqrtf(sq / (float)D + eps);
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const f32x4_t g0 = k.g[j][0], g1 = k.g[j][1], b0 = k.b[j][0], b1 = k.b[j][1];
        o[j].x = pack_bf16x2((v[j][0][0] * rstd) * g0[0] + b0[0], (v[j][0][1] * rstd) * g0[1] + b0[1]);
        o[j].y = pack_bf16x2((v[j][0][2] * rstd) * g0[2] + b0[2], (v[j][0][3] * rstd) * g0[3] + b0[3]);
        o[j].z = pack_bf16x2((v[j][1][0] * rstd) * g1[0] + b1[0], (v[j][1][1] * rstd) * g1[1] + b1[1]);
        o[j].w = pack_bf16x2((v[j][1][2] * rstd) * g1[2] + b1[2], (v[j][1][3] * rstd) * g1[3] + b1[3]);
    }
}
