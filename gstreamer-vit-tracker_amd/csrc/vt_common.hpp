// vt_common.hpp — the core every translation unit shares, the math kernels included: vector types, vt_launch, bf16 helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

typedef uint16_t bf16_t;  // bfloat16 bit pattern
typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(4))) short bf16x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;

// ---- kernel launches -----------------------------------------------------------------------------
// Every kernel of the library is launched through vt_launch. It is hipLaunchKernelGGL, except while the engine's
// instrumented pass (vt_group_profile_device) has armed a probe on the calling thread: the first launch behind the arming
// then goes through hipExtLaunchKernelGGL with the probe's two HIP events, which receive the begin and end timestamps of
// THAT dispatch - the duration rocprofv3's kernel trace reports - instead of the time between two marker packets around
// it (which adds the dispatch and marker latency, ~4 us per launch on this stack).
struct LaunchProbe { hipEvent_t start, stop; int launches; };
extern thread_local LaunchProbe* vt_launch_probe;
template <typename F, typename... Args>
inline void vt_launch(F kernel, const dim3& grid, const dim3& block, size_t smem, hipStream_t st, Args... args) {
    LaunchProbe* pr = vt_launch_probe;
    if (pr && pr->launches++ == 0) hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)smem, st, pr->start, pr->stop, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, smem, st, args...);
}

// ---- small device helpers ---------------------------------------------------------------------

__device__ __forceinline__ float bf16_to_f32(bf16_t b) {
    return __uint_as_float(((uint32_t)b) << 16);
}
// f32 -> bf16, round to nearest even, NaN kept a NaN: one v_cvt_pk_bf16_f32 (gfx950). Same
// result as the integer rounding (u + 0x7fff + ((u >> 16) & 1)) >> 16 of the oracle for every
// finite input. Observed on the MI355X through the ReLU, GELU and QKV epilogues of configurations 2, 3, 18
// and 19 (tests/test_gpu_epilogue_edges.py): every normal bf16 pattern, both tie directions at every
// exponent, the band that rounds to infinity and 4 * 10^5 ordinary values come back as the oracle's bits;
// so do the subnormal inputs (bf16 subnormal patterns, their ties, a subnormal q = y * QK_SCALE) - none is
// flushed to zero, in the scalar or in the packed form (profiles/epilogue_edges.txt).
typedef __bf16 bf16v2_t __attribute__((ext_vector_type(2)));
typedef float f32v2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ bf16_t f32_to_bf16(float f) {
    return __builtin_bit_cast(bf16_t, (__bf16)f);
}
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    const f32v2_t v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16v2_t));
}
