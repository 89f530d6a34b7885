// k_overlay.hip — the reference's overlay drawing on the NV12 luma plane, on the GPU.
//
// The reference draws into the mapped frame on the CPU right after tracking
// (/root/reference/src/pipeline.rs:125-174): draw_background_nv12, draw_text_nv12,
// draw_rect_nv12, draw_crosshair_nv12 (src/nv12_convert.rs:172-343) and draw_cursor /
// draw_selection (src/drawing.rs:5-50). With the frame resident in HBM the same commands are
// applied here by one launch: one lane per luma pixel walks the command list IN ORDER and applies
// every command that covers its pixel — identical to applying the commands one after another,
// because each command's effect on a pixel depends only on that pixel. The coverage predicates are
// the closed forms of the reference's loops, including its usize wrap-around quirks (a rectangle
// whose right edge x + w is negative extends to the last column). Bit-exact with
// oracle/vt_oracle.c's line-by-line restatements.
#include "k_overlay.hpp"
#include "k_overlay_dev.hpp"     // covers, covers_rgb, glyph_bit and the glyph table

__global__ __launch_bounds__(256) void overlay_kernel(uint8_t* __restrict__ yplane, int width,
                                                      int height, int stride,
                                                      const vt_draw_cmd* __restrict__ cmds, int n) {
    const int px = blockIdx.x * 64 + (threadIdx.x & 63);
    const int py = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (px >= width || py >= height) return;
    uint8_t v = 0;
    bool loaded = false;
    for (int i = 0; i < n; ++i) {
        const vt_draw_cmd& c = cmds[i];
        if (!covers(c, (u64)px, (u64)py, (u64)width, (u64)height)) continue;
        if (!loaded) { v = yplane[(size_t)py * stride + px]; loaded = true; }
        if (c.type == VT_DRAW_BACKGROUND)
            v = (uint8_t)(((unsigned)v * (unsigned)(255 - (c.value & 255))) / 255u);
        else
            v = (c.type == VT_DRAW_CURSOR || c.type == VT_DRAW_SELECTION) ? 255 : (uint8_t)c.value;
    }
    if (loaded) yplane[(size_t)py * stride + px] = v;
}

hipError_t launch_overlay(uint8_t* yplane, int width, int height, int stride, const vt_draw_cmd* d_cmds,
                          int n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    dim3 grid((width + 63) / 64, (height + 3) / 4);
    vt_launch(overlay_kernel, grid, dim3(256), 0, st, yplane, width, height, stride, d_cmds, n);
    return hipGetLastError();
}

// ---- packed RGB8 surface (src/drawing_rgb.rs:4-129): the same scheme with covers_rgb -------------------------------------
__global__ __launch_bounds__(256) void overlay_rgb_kernel(uint8_t* __restrict__ rgb, int width, int height,
                                                          int stride, const vt_draw_cmd* __restrict__ cmds,
                                                          int n) {
    const int px = blockIdx.x * 64 + (threadIdx.x & 63);
    const int py = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (px >= width || py >= height) return;
    int r = 0, g = 0, b = 0;
    bool hit = false;
    for (int i = 0; i < n; ++i) {
        const vt_draw_cmd& c = cmds[i];
        if (!covers_rgb(c, px, py, width, height)) continue;
        hit = true;
        switch (c.type) {
            case VT_DRAW_BACKGROUND: r = g = b = 30; break;
            case VT_DRAW_TEXT: r = g = b = c.value & 255; break;
            case VT_DRAW_CURSOR: r = 0; g = 255; b = 0; break;
            case VT_DRAW_SELECTION: r = 255; g = 255; b = 0; break;
            default: r = (c.value >> 16) & 255; g = (c.value >> 8) & 255; b = c.value & 255; break;
        }
    }
    if (hit) {
        uint8_t* p = rgb + (size_t)py * stride + (size_t)px * 3;
        p[0] = (uint8_t)r; p[1] = (uint8_t)g; p[2] = (uint8_t)b;
    }
}

hipError_t launch_overlay_rgb(uint8_t* rgb, int width, int height, int stride, const vt_draw_cmd* d_cmds, int n,
                              hipStream_t st) {
    if (n <= 0) return hipSuccess;
    dim3 grid((width + 63) / 64, (height + 3) / 4);
    vt_launch(overlay_rgb_kernel, grid, dim3(256), 0, st, rgb, width, height, stride, d_cmds, n);
    return hipGetLastError();
}
