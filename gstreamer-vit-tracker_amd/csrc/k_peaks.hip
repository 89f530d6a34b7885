// k_peaks.hip — response peaks: up to VT_PEAKS_MAX maxima of a slot's Hann-weighted score map with their decoded boxes,
// found behind the decode of the pass (DESIGN.md section 3 "Response peaks").
//
// The definition is vto_decode (oracle/vt_oracle.c) iterated: peak k is the decode of the slot's logits with the score
// logit of every cell inside the (2R + 1)^2 squares around peaks 0..k-1 set to -inf. sigmoid(-inf) is exactly 0, so a
// suppressed cell has response 0: it is never listed and enters a later 3x3 window with weight 0 - its terms are
// computed, not skipped (0 * NaN of a NaN offset logit is NaN there as in the specification).
//
// One workgroup of 256 threads per slot. The response plane sigmoid(score logit) * hann goes to LDS once (ns floats);
// a round is: the block argmax under hc_better (a 6-step wave butterfly + one step over the four waves' candidates),
// the window by nine threads, thread 0's sums and box into the record (LDS), the square's cells set to 0 in the plane.
// The finished record leaves as 68 dwords to the device array and to the pass's pinned host array. Nothing else is
// written: no word of StreamState, no result; no atomics, no tickets.
//
// The arithmetic restates k_head.hip's decode (hc_sigmoid, hc_better, hc_decoded_cell, the window terms and the box /
// clamp sequence of decode_box) operation for operation; this file is compiled with k_head.hip's flags (one IEEE
// operation per source operation). tests/test_gpu_response_peaks.py holds peak 0 to the decode's bits.
#include "vt_common.hpp"

static_assert(sizeof(vt_peak) == 32 && sizeof(vt_peaks) == 272, "vt_peaks layout");
static_assert(sizeof(PeaksPolicy) == 16, "PeaksPolicy layout");
static constexpr int kRecWords = sizeof(vt_peaks) / 4;

__device__ __forceinline__ float pk_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
// candidate a = (response, cell) beats b: the larger response, the lower cell on a tie; a NaN never compares greater
__device__ __forceinline__ bool pk_better(float ra, int ia, float rb, int ib) { return ra > rb || (ra == rb && ia < ib); }
#define PK_NO_CELL 0x7fffffff

__global__ __launch_bounds__(256) void response_peaks_kernel(PeaksArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_plane[];    // [ns] responses; 0 where suppressed
    __shared__ float s_wb[4];
    __shared__ int s_wi[4];
    __shared__ float s_win[48];                 // 9 x 5 window terms + [45] the peak cell's score logit
    __shared__ uint32_t s_rec[kRecWords];       // the record as it will be stored
    const int b = blockIdx.x, tid = threadIdx.x;
    // the gate: wave-uniform loads (everything is indexed by the block)
    const int sb = a.slot_stream ? a.slot_stream[b] : b;
    const PeaksPolicy pol = a.policy[sb];
    const bool listed = pol.max_peaks > 0 && (!a.winner || a.winner[b] == b);
    const PassOut po = *a.out;
    if (!listed) {
        if (tid == 0) {
            a.records[b].n = 0;
            if (po.host_peaks) po.host_peaks[b].n = 0;
            __threadfence_system();
        }
        return;
    }
    const int ns = a.ns, grid = a.grid;
    const int K = min(pol.max_peaks, VT_PEAKS_MAX), R = pol.radius;
    const float* ho = a.head_out + (size_t)b * ns * 8;
    // what the rounds need of the stream's state does not change from round to round: fetched once, wave-uniform
    const StreamState& s = a.states[sb];
    const float geo0 = s.geo[0], geo1 = s.geo[1], side = s.geo[3];
    const float W = (float)s.frame_w, Hh = (float)s.frame_h;
    const int frames_done = s.frames_done;
    for (int i = tid; i < ns; i += 256) s_plane[i] = pk_sigmoid(ho[(size_t)i * 8]) * a.hann[i];
    if (tid < kRecWords) s_rec[tid] = 0u;
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    int n = 0;
    for (int k = 0; k < K; ++k) {
        float best = -1.0f;
        int bidx = PK_NO_CELL;
        for (int i = tid; i < ns; i += 256) {
            const float r = s_plane[i];
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
        if (lane == 0) { s_wb[wave] = best; s_wi[wave] = bidx; }
        __syncthreads();
        best = s_wb[0]; bidx = s_wi[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (pk_better(s_wb[w], s_wi[w], best, bidx)) { best = s_wb[w]; bidx = s_wi[w]; }
        const int idx = bidx == PK_NO_CELL ? 0 : bidx;     // nothing compared: cell 0, vto_decode's initial `best`
        const float resp = s_plane[idx];
        // peak 0 is the update's own decode and always listed; a later one needs a positive response of at least
        // min_resp (a NaN fails both). Responses do not increase from round to round: the first failure ends the list.
        if (k >= 1 && !(resp > 0.0f && resp >= pol.min_resp)) break;
        const int bx = idx % grid, by = idx / grid;
        if (tid < 9) {
            const int ix = bx + tid % 3 - 1, iy = by + tid / 3 - 1;
            float t[5] = {-1.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (ix >= 0 && iy >= 0 && ix < grid && iy < grid) {
                const int c = iy * grid + ix;
                float o[5];
#pragma unroll
                for (int j = 0; j < 5; ++j) o[j] = ho[(size_t)c * 8 + j];
                const float r = s_plane[c];                 // the suppression-aware response
                const float w = r * r;
                const float offx = 3.0f * pk_sigmoid(o[1]) - 1.0f;
                const float offy = 3.0f * pk_sigmoid(o[2]) - 1.0f;
                const float cxj = ((float)ix + offx) / (float)grid;
                const float cyj = ((float)iy + offy) / (float)grid;
                t[0] = w; t[1] = w * cxj; t[2] = w * cyj; t[3] = w * pk_sigmoid(o[3]); t[4] = w * pk_sigmoid(o[4]);
                if (tid == 4) s_win[45] = o[0];
            }
#pragma unroll
            for (int j = 0; j < 5; ++j) s_win[tid * 5 + j] = t[j];
        }
        __syncthreads();
        if (tid == 0) {
            const float score = pk_sigmoid(s_win[45]);
            float sw = 0.0f, scx = 0.0f, scy = 0.0f, sbw = 0.0f, sbh = 0.0f;
            for (int j = 0; j < 9; ++j) {
                if (s_win[j * 5] < 0.0f) continue;
                sw = sw + s_win[j * 5];
                scx = scx + s_win[j * 5 + 1];
                scy = scy + s_win[j * 5 + 2];
                sbw = sbw + s_win[j * 5 + 3];
                sbh = sbh + s_win[j * 5 + 4];
            }
            const float cxn = scx / sw, cyn = scy / sw, wn = sbw / sw, hn = sbh / sw;
            const float cx = (geo0 + 0.5f) + cxn * side;
            const float cy = (geo1 + 0.5f) + cyn * side;
            float bw = wn * side, bh = hn * side;
            float x1 = cx - 0.5f * bw, y1 = cy - 0.5f * bh;
            float x2 = x1 + bw, y2 = y1 + bh;
            const float margin = 10.0f;
            x1 = fminf(fmaxf(0.0f, x1), W - margin);
            y1 = fminf(fmaxf(0.0f, y1), Hh - margin);
            x2 = fminf(fmaxf(margin, x2), W);
            y2 = fminf(fmaxf(margin, y2), Hh);
            bw = fmaxf(margin, x2 - x1);
            bh = fmaxf(margin, y2 - y1);
            uint32_t* p = s_rec + 4 + k * 8;
            p[0] = __float_as_uint(score); p[1] = __float_as_uint(resp);     // = score * hann[idx]: the plane's value of an unsuppressed cell
            p[2] = __float_as_uint(x1); p[3] = __float_as_uint(y1); p[4] = __float_as_uint(bw); p[5] = __float_as_uint(bh);
            p[6] = (uint32_t)idx; p[7] = 0u;
        }
        n = k + 1;
        // the square around the peak, clipped at the map's borders: (2R + 1)^2 <= 81 cells
        const int sq = 2 * R + 1;
        if (tid < sq * sq) {
            const int ix = bx + tid % sq - R, iy = by + tid / sq - R;
            if (ix >= 0 && iy >= 0 && ix < grid && iy < grid) s_plane[iy * grid + ix] = 0.0f;
        }
        __syncthreads();
    }
    if (tid == 0) {
        s_rec[0] = (uint32_t)n; s_rec[1] = (uint32_t)sb;
        s_rec[2] = (uint32_t)frames_done; s_rec[3] = (uint32_t)R;
    }
    __syncthreads();
    if (tid < kRecWords) {
        const uint32_t v = s_rec[tid];
        reinterpret_cast<uint32_t*>(a.records + b)[tid] = v;
        if (po.host_peaks) reinterpret_cast<uint32_t*>(po.host_peaks + b)[tid] = v;
        __threadfence_system();     // the host's copy is visible once the pass's event or the stream synchronises
    }
}

hipError_t launch_response_peaks(const PeaksArgs& a, hipStream_t st) {
    if (a.n < 1 || a.grid < 1 || a.ns != a.grid * a.grid || !a.head_out || !a.hann || !a.states || !a.policy || !a.records ||
        !a.out)
        return hipErrorInvalidValue;
    const size_t lds = (size_t)a.ns * sizeof(float);
    if (lds > 48 * 1024) return hipErrorInvalidValue;      // a map of more than 110^2 cells: no model has one
    vt_launch(response_peaks_kernel, dim3(a.n), dim3(256), lds, st, a);
    return hipGetLastError();
}
