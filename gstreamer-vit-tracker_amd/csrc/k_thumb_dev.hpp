// k_thumb_dev.hpp — the cell of the uint16 frame thumbnails (k_camera_motion.hip, k_health.hip): sixteen fetch_rgb taps at
// (i * c + u * (c / 4) + c / 8, j * c + v * (c / 4) + c / 8), u, v = 0..3, an integer luma (77 r + 150 g + 29 b + 128) >> 8
// each, summed: 0..4080. Every tap lies inside a frame of at least (i + 1) * c x (j + 1) * c pixels.
#pragma once
#include "k_preproc_dev.hpp"

template <int ANY>
__device__ __forceinline__ int thumb_cell(const FrameDesc& f, int i, int j, int c) {
    const int step = c >> 2, half = c >> 3;
    int sum = 0, miss = 0;
#pragma unroll 1
    for (int v = 0; v < 4; ++v) {
        const int py = j * c + v * step + half;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int px = i * c + u * step + half;
            float rgb[3];
            fetch_rgb<ANY>(f, px, py, rgb, miss);       // integers 0..255
            sum += (77 * (int)rgb[0] + 150 * (int)rgb[1] + 29 * (int)rgb[2] + 128) >> 8;
        }
    }
    return sum;
}
