// k_preproc_dev.hpp — what the crop kernels of k_preproc.hip, the template refresh of k_refresh.hip and the target chips of
// k_chip.hip share besides the kernel bodies of k_preproc_body.inc: the pixel fetch, the tile constants and the tap
// rectangle of a crop.
#pragma once
#include "vt_common.hpp"
#include "vt_frame.hpp"

// /root/reference/src/nv12_convert.rs:24-29 (table entries) and :124-131 (per pixel)
__device__ __forceinline__ void yuv_to_rgb(int y, int u, int v, int& r, int& g, int& b) {
    const int yv = 298 * (y - 16);
    r = yv + 409 * (v - 128) + 128;
    g = yv - 100 * (u - 128) - 208 * (v - 128) + 128;
    b = yv + 516 * (u - 128) + 128;
    // clamp_u8(x >> 8) written as clamp first, shift second (same value: the arithmetic shift is
    // monotonic). The shift-then-clamp form is pattern-matched by hipcc (ROCm 7.2) into
    // v_ashr_pk_u8_i32, whose upper 16 result bits are not zero on MI355X although the
    // compiler ORs the result as if they were — measured: wrong bytes 2/3 of every packed dword.
    r = min(max(r, 0), 0xffff) >> 8;
    g = min(max(g, 0), 0xffff) >> 8;
    b = min(max(b, 0), 0xffff) >> 8;
}

// The coefficient table of the colour codes (vt_frame.hpp: pix_color_code; vittrack_hip.h: vt_color_matrix), the ONE copy
// the kernels have: row c = matrix * 2 + range holds YO, CY, CRV, CGU, CGV, CBU, each rint(256 * exact) (DESIGN.md section 3
// "Colorimetry"). Row 0 is yuv_to_rgb's; rows 6 and 7 repeat it so that any three bits index inside the table.
struct YuvCoef { int yo, cy, crv, cgu, cgv, cbu; };
// the row of a layout word's code (bits 28..30 of FrameDesc.lay, set by to_desc). The word is uniform per slot - a pass's
// slots may carry different codes - so the row is read with scalar loads, not per pixel.
__device__ __forceinline__ YuvCoef yuv_coef(int lay) {
    static constexpr YuvCoef table[8] = {
        {16, 298, 409, -100, -208, 516}, {0, 256, 359, -88, -183, 454},
        {16, 298, 459, -55, -136, 541},  {0, 256, 403, -48, -120, 475},
        {16, 298, 430, -48, -167, 548},  {0, 256, 377, -42, -146, 482},
        {16, 298, 409, -100, -208, 516}, {16, 298, 409, -100, -208, 516}};
    return table[(lay >> PIXL_CODE_SHIFT) & PIXL_CODE_MASK];
}
// yuv_to_rgb with the coefficients of a code: the same form - clamp first, shift second (see above); the sums reach 140946
__device__ __forceinline__ void yuv_to_rgb_code(const YuvCoef& k, int y, int u, int v, int& r, int& g, int& b) {
    const int yv = k.cy * (y - k.yo);
    r = yv + k.crv * (v - 128) + 128;
    g = yv + k.cgu * (u - 128) + k.cgv * (v - 128) + 128;
    b = yv + k.cbu * (u - 128) + 128;
    r = min(max(r, 0), 0xffff) >> 8;
    g = min(max(g, 0), 0xffff) >> 8;
    b = min(max(b, 0), 0xffff) >> 8;
}
// the conversion of a kernel of level ANY: levels 0..2 never see a frame with a code and keep yuv_to_rgb's constants and
// instructions; level 3 converts with the frame's row
template <int ANY>
__device__ __forceinline__ void yuv_to_rgb_lay(int lay, int y, int u, int v, int& r, int& g, int& b) {
    if constexpr (ANY >= 3) yuv_to_rgb_code(yuv_coef(lay), y, u, v, r, g, b);
    else yuv_to_rgb(y, u, v, r, g, b);
}

// frame pixel (px,py) as float RGB; outside the frame -> 0 (zero padding).
// ANY = 0: the kernels of RGB8, NV12 and YUY2 (the layouts that define the families, with their byte offsets as
// constants); ANY = 1: every vt_pixfmt, each its family read through the byte offsets of f.lay (vt_frame.hpp); ANY = 2:
// every vt_pixfmt2 as well, through the whole layout word. The engine launches the kernels of the lowest level that reads
// every format of the pass (pix_level): reading the offsets at run time costs the crop kernels 3-19 SGPRs, the planar,
// 16-bit and grey layouts another 6 and 23 spilled (kernel-resource-usage; profiles/planar_formats_cfg3.txt), and the
// kernels of the formats that were there before keep their budgets and their instructions. ANY = 3: every layout of level
// 2, converted with the frame's colour code (bits 28..30 of f.lay) instead of the BT.601 limited-range constants.
template <int ANY>
__device__ __forceinline__ void fetch_rgb(const FrameDesc& f, int px, int py, float* rgb, int& miss) {
    if (px < 0 || py < 0 || px >= f.w || py >= f.h) {
        rgb[0] = rgb[1] = rgb[2] = 0.0f;
        return;
    }
    int r, g, b;
    const int sx = px - f.x0, sy = py - f.y0;   // position inside the stored window
    // inside the frame but outside what the caller stored (a window narrower than the crop): black,
    // never an out-of-bounds read. The library's own window planner always covers the crop.
    if ((unsigned)sx >= (unsigned)f.ww || (unsigned)sy >= (unsigned)f.wh) {
        rgb[0] = rgb[1] = rgb[2] = 0.0f;
        miss = 1;
        return;
    }
    if constexpr (ANY >= 2) {    // the masks keep every offset inside its pixel / pair / sample: no other byte is read
        const int lay = f.lay;
        if (f.fmt == PIXF_RGB) {            // RGB8 .. BGRX, XRGB, XBGR, GRAY8: the colour bytes at their offsets in the pixel
            const uint8_t* p = f.p0 + (size_t)sy * f.s0 + (size_t)sx * (unsigned)(lay >> 24);
            r = p[lay & 3]; g = p[(lay >> 8) & 3]; b = p[(lay >> 16) & 3];
        } else if (f.fmt == PIXF_420SP) {   // NV12, NV21, I420, YV12, P010, NV16; x0 (and y0, but NV16's) even
            const int ss = (lay >> 20) & 1, hb = (lay >> 22) & 1;       // 16-bit samples: the shift and the byte read
            const int y = f.p0[(size_t)sy * f.s0 + ((size_t)sx << ss) + hb];
            int u, v;
            if (lay & PIXL_PLANAR) {        // the second chroma plane lies behind the first one's stored rows
                const uint8_t* c = f.p1 + (size_t)(sy >> 1) * f.s1 + (sx >> 1);
                const size_t second = (size_t)f.s1 * (size_t)((((lay & PIXL_FULLH) ? f.h : f.wh) + 1) >> 1);
                u = c[(lay & 1) ? second : 0];
                v = c[(lay & 0x100) ? second : 0];
            } else {
                const uint8_t* uv = f.p1 + (size_t)(sy >> (((lay >> 24) & 1) ^ 1)) * f.s1 + ((size_t)(sx & ~1) << ss) + hb;
                u = uv[(lay & 1) << ss];
                v = uv[((lay >> 8) & 1) << ss];
            }
            yuv_to_rgb_lay<ANY>(lay, y, u, v, r, g, b);
        } else {                            // YUY2 (Y0 U Y1 V), UYVY (U Y0 V Y1) per pixel pair
            const uint8_t* p = f.p0 + (size_t)sy * f.s0 + (size_t)(sx & ~1) * 2;
            yuv_to_rgb_lay<ANY>(lay, p[(sx & 1) ? (lay >> 16) & 3 : lay & 3], p[(lay >> 8) & 3], p[(lay >> 24) & 3], r, g, b);
        }
    } else if constexpr (ANY == 1) {    // the masks keep every offset inside its pixel / pair
        const int lay = f.lay;
        if (f.fmt == PIXF_RGB) {            // RGB8, BGR8, RGBX, BGRX: colour bytes 0-2, permuted by the offsets
            const uint8_t* p = f.p0 + (size_t)sy * f.s0 + (size_t)sx * (unsigned)(lay >> 24);
            const uint32_t c = __builtin_amdgcn_perm(0u, (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16),
                                                     ((uint32_t)lay & 0x00ffffffu) | 0x0c000000u);
            r = c & 255; g = (c >> 8) & 255; b = c >> 16;
        } else if (f.fmt == PIXF_420SP) {   // NV12, NV21
            const int y = f.p0[(size_t)sy * f.s0 + sx];
            const uint8_t* uv = f.p1 + (size_t)(sy >> 1) * f.s1 + (sx & ~1);   // x0, y0 even
            const uint32_t c = __builtin_amdgcn_perm(0u, (uint32_t)uv[0] | ((uint32_t)uv[1] << 8), ((uint32_t)lay & 0xffffu) | 0x0c0c0000u);
            yuv_to_rgb(y, c & 255, c >> 8, r, g, b);
        } else {                            // YUY2 (Y0 U Y1 V), UYVY (U Y0 V Y1) per pixel pair
            const uint8_t* p = f.p0 + (size_t)sy * f.s0 + (size_t)(sx & ~1) * 2;
            yuv_to_rgb(p[(sx & 1) ? (lay >> 16) & 3 : lay & 3], p[(lay >> 8) & 3], p[(lay >> 24) & 3], r, g, b);
        }
    } else if (f.fmt == VT_PIX_RGB8) {
        const uint8_t* p = f.p0 + (size_t)sy * f.s0 + (size_t)sx * 3;
        r = p[0]; g = p[1]; b = p[2];
    } else if (f.fmt == VT_PIX_NV12) {
        const int y = f.p0[(size_t)sy * f.s0 + sx];
        const uint8_t* uv = f.p1 + (size_t)(sy >> 1) * f.s1 + (sx & ~1);   // x0, y0 even
        yuv_to_rgb(y, uv[0], uv[1], r, g, b);
    } else {  // YUY2: Y0 U Y1 V per pixel pair
        const uint8_t* p = f.p0 + (size_t)sy * f.s0 + (size_t)(sx & ~1) * 2;
        yuv_to_rgb(p[(sx & 1) * 2], p[1], p[3], r, g, b);
    }
    rgb[0] = (float)r; rgb[1] = (float)g; rgb[2] = (float)b;
}

// output tile of the tile body and its smallest LDS buffer in source pixels (k_preproc.hip: the tiers)
#define PRE_TILE_W 64
#define PRE_TILE_H 32
#define PRE_TILE_LDS 4096       // source pixels (16 KiB): tier 0, the benchmark's 64-px targets

// tap rectangle of a crop along one axis: the source pixels its first and last output pixel touch - the expressions of
// the tile body's sx_lo / sx_hi (k_preproc_body.inc) for the whole crop (the geometry rules of k_refresh.hip, k_chip.hip)
__device__ __forceinline__ void tap_range(float scale, float x0m, int size, int& lo, int& hi) {
    lo = (int)floorf(((float)0 + 0.5f) * scale + x0m);
    hi = (int)floorf(((float)(size - 1) + 0.5f) * scale + x0m) + 1;
}
