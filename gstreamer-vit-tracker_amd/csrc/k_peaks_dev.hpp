// k_peaks_dev.hpp — the iteration of the response peaks as ONE text: vto_decode (oracle/vt_oracle.c) iterated under a
// suppression square, by one workgroup of 256 threads. Shared by the response-peaks launch (k_peaks.hip) and the list launch
// of the peak arbitration (k_arbitrate.hip); both files are compiled with k_head.hip's flags (one IEEE operation per source
// operation), so both list the same bits.
//
// The definition: peak k is the decode of the slot's logits with the score logit of every cell inside the (2R + 1)^2 squares
// around peaks 0..k-1 set to -inf. sigmoid(-inf) is exactly 0, so a suppressed cell has response 0: it is never listed and
// enters a later 3x3 window with weight 0 - its terms are computed, not skipped (0 * NaN of a NaN offset logit is NaN there
// as in the specification).
//
// The arithmetic restates k_head.hip's decode (hc_sigmoid, hc_better, hc_decoded_cell, the window terms and the box /
// clamp sequence of decode_box) operation for operation.
#pragma once
#include "vt_common.hpp"

__device__ __forceinline__ float pk_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
// candidate a = (response, cell) beats b: the larger response, the lower cell on a tie; a NaN never compares greater
__device__ __forceinline__ bool pk_better(float ra, int ia, float rb, int ib) { return ra > rb || (ra == rb && ia < ib); }
#define PK_NO_CELL 0x7fffffff

// the LDS of one iteration beside the response plane ([ns] floats, dynamic)
struct PeaksLds {
    float wb[4];
    int wi[4];
    float win[48];              // 9 x 5 window terms + [45] the peak cell's score logit
};
// what the rounds need of the stream's state: it does not change from round to round
struct PeaksGeo { float geo0, geo1, side, W, Hh; };

// Every thread of the 256 calls this with the same arguments. ho: the slot's logits [ns][8]; plane: [ns] floats of LDS;
// peaks: room for K records of 8 dwords in LDS, zeroed by the caller - a listed peak k leaves the words of a vt_peak at
// peaks + 8 * k (thread 0 stores them; visible to every thread on return). Returns the number of peaks listed, 1..K.
__device__ __forceinline__ int peaks_iterate(const float* ho, const float* hann, float* plane, PeaksLds& l, uint32_t* peaks, int ns,
                                             int grid, int K, int R, float min_resp, const PeaksGeo& g) {
    const int tid = threadIdx.x;
    for (int i = tid; i < ns; i += 256) plane[i] = pk_sigmoid(ho[(size_t)i * 8]) * hann[i];
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    int n = 0;
    for (int k = 0; k < K; ++k) {
        float best = -1.0f;
        int bidx = PK_NO_CELL;
        for (int i = tid; i < ns; i += 256) {
            const float r = plane[i];
            if (pk_better(r, i, best, bidx)) { best = r; bidx = i; }
        }
        // no thread's candidate is a NaN (a NaN never replaces the start value), so the order is total and every lane
        // of the butterfly ends with the same pair
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ob = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bidx, off, 64);
            if (pk_better(ob, oi, best, bidx)) { best = ob; bidx = oi; }
        }
        if (lane == 0) { l.wb[wave] = best; l.wi[wave] = bidx; }
        __syncthreads();
        best = l.wb[0]; bidx = l.wi[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (pk_better(l.wb[w], l.wi[w], best, bidx)) { best = l.wb[w]; bidx = l.wi[w]; }
        const int idx = bidx == PK_NO_CELL ? 0 : bidx;     // nothing compared: cell 0, vto_decode's initial `best`
        const float resp = plane[idx];
        // peak 0 is the update's own decode and always listed; a later one needs a positive response of at least
        // min_resp (a NaN fails both). Responses do not increase from round to round: the first failure ends the list.
        if (k >= 1 && !(resp > 0.0f && resp >= min_resp)) break;
        const int bx = idx % grid, by = idx / grid;
        if (tid < 9) {
            const int ix = bx + tid % 3 - 1, iy = by + tid / 3 - 1;
            float t[5] = {-1.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (ix >= 0 && iy >= 0 && ix < grid && iy < grid) {
                const int c = iy * grid + ix;
                float o[5];
#pragma unroll
                for (int j = 0; j < 5; ++j) o[j] = ho[(size_t)c * 8 + j];
                const float r = plane[c];                   // the suppression-aware response
                const float w = r * r;
                const float offx = 3.0f * pk_sigmoid(o[1]) - 1.0f;
                const float offy = 3.0f * pk_sigmoid(o[2]) - 1.0f;
                const float cxj = ((float)ix + offx) / (float)grid;
                const float cyj = ((float)iy + offy) / (float)grid;
                t[0] = w; t[1] = w * cxj; t[2] = w * cyj; t[3] = w * pk_sigmoid(o[3]); t[4] = w * pk_sigmoid(o[4]);
                if (tid == 4) l.win[45] = o[0];
            }
#pragma unroll
            for (int j = 0; j < 5; ++j) l.win[tid * 5 + j] = t[j];
        }
        __syncthreads();
        if (tid == 0) {
            const float score = pk_sigmoid(l.win[45]);
            float sw = 0.0f, scx = 0.0f, scy = 0.0f, sbw = 0.0f, sbh = 0.0f;
            for (int j = 0; j < 9; ++j) {
                if (l.win[j * 5] < 0.0f) continue;
                sw = sw + l.win[j * 5];
                scx = scx + l.win[j * 5 + 1];
                scy = scy + l.win[j * 5 + 2];
                sbw = sbw + l.win[j * 5 + 3];
                sbh = sbh + l.win[j * 5 + 4];
            }
            const float cxn = scx / sw, cyn = scy / sw, wn = sbw / sw, hn = sbh / sw;
            const float cx = (g.geo0 + 0.5f) + cxn * g.side;
            const float cy = (g.geo1 + 0.5f) + cyn * g.side;
            float bw = wn * g.side, bh = hn * g.side;
            float x1 = cx - 0.5f * bw, y1 = cy - 0.5f * bh;
            float x2 = x1 + bw, y2 = y1 + bh;
            const float margin = 10.0f;
            x1 = fminf(fmaxf(0.0f, x1), g.W - margin);
            y1 = fminf(fmaxf(0.0f, y1), g.Hh - margin);
            x2 = fminf(fmaxf(margin, x2), g.W);
            y2 = fminf(fmaxf(margin, y2), g.Hh);
            bw = fmaxf(margin, x2 - x1);
            bh = fmaxf(margin, y2 - y1);
            uint32_t* p = peaks + k * 8;
            p[0] = __float_as_uint(score); p[1] = __float_as_uint(resp);     // = score * hann[idx]: the plane's value of an unsuppressed cell
            p[2] = __float_as_uint(x1); p[3] = __float_as_uint(y1); p[4] = __float_as_uint(bw); p[5] = __float_as_uint(bh);
            p[6] = (uint32_t)idx; p[7] = 0u;
        }
        n = k + 1;
        // the square around the peak, clipped at the map's borders: (2R + 1)^2 <= 81 cells
        const int sq = 2 * R + 1;
        if (tid < sq * sq) {
            const int ix = bx + tid % sq - R, iy = by + tid / sq - R;
            if (ix >= 0 && iy >= 0 && ix < grid && iy < grid) plane[iy * grid + ix] = 0.0f;
        }
        __syncthreads();
    }
    return n;
}
