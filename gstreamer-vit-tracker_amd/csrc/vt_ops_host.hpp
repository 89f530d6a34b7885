// vt_ops_host.hpp — the host arithmetic of the operator entry points (vt_ops.hip): number formats, operand generators
// and argument rules. Pure C++17 - no HIP, nothing of vt_engine.hpp - so tests/ops_host_main.cpp runs all of it on the CPU.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

// float32 <-> bf16 bit pattern (round to nearest even)
static inline uint16_t host_bf16(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
static inline float host_f32(uint16_t b) {
    const uint32_t u = ((uint32_t)b) << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static inline void widen_bf16(const uint16_t* in, size_t n, float* out) {     // bit copies: a NaN keeps its payload
    for (size_t i = 0; i < n; ++i) { const uint32_t u = ((uint32_t)in[i]) << 16; memcpy(out + i, &u, 4); }
}

// the 3-byte pair of the residual stream (specification v3, k_gemm.hpp): hi = bf16(x),
// lo8 = clamp(rint((x - hi) * 2^s), -127, 127); its value is hi + lo8 * q with the quantum q = 2^-s
static inline void pair_pack(const float* x, size_t n, int s, uint16_t* hi, int8_t* lo) {
    for (size_t i = 0; i < n; ++i) {
        hi[i] = host_bf16(x[i]);
        const float r = nearbyintf((x[i] - host_f32(hi[i])) * (float)(1 << s));
        lo[i] = (int8_t)(r < -127.0f ? -127.0f : r > 127.0f ? 127.0f : r);
    }
}
static inline void pair_value(const uint16_t* hi, const int8_t* lo, size_t n, float q, float* x) {
    for (size_t i = 0; i < n; ++i) x[i] = host_f32(hi[i]) + (float)lo[i] * q;
}
constexpr int kLoShiftMin = 6, kLoShiftMax = 14;        // VT_LO_SHIFT_MIN / _MAX (vt_ops_util.hpp asserts it)
static inline bool lo_shift_ok(int s) { return s >= kLoShiftMin && s <= kLoShiftMax; }

// operands of the timing hooks: bf16 values of magnitude 1 .. 2 with a random sign, from a linear congruential generator;
// returns the seed to go on with, so one sequence can fill several arrays
static inline uint32_t fill_lcg_bf16(uint16_t* out, size_t n, uint32_t seed) {
    for (size_t i = 0; i < n; ++i) {
        seed = seed * 1664525u + 1013904223u;
        out[i] = (uint16_t)(0x3c00u + ((seed >> 9) & 0x3ffu) + ((seed >> 3) & 0x8000u));
    }
    return seed;
}
// ... and random bytes (xorshift32) for the pixel timers
static inline void fill_xorshift_u8(uint8_t* out, size_t n, uint32_t seed = 2463534242u) {
    for (size_t i = 0; i < n; ++i) { seed ^= seed << 13; seed ^= seed >> 17; seed ^= seed << 5; out[i] = (uint8_t)seed; }
}

// a hook's `cfg` argument: < 0 the launcher's own choice; else the tile configuration in bits 0-7 and, in bits 8-9, the
// order in which an XCD's run of workgroups covers the tile grid (0 the launcher's rule, 1 rows, 2 columns)
struct TileCfg { int cfg, order; };
static inline TileCfg split_cfg(int cfg) {
    return cfg < 0 ? TileCfg{cfg, 0} : TileCfg{cfg & 0xff, (cfg >> 8) & 3};
}
