// k_peaks.hip — response peaks: up to VT_PEAKS_MAX maxima of a slot's Hann-weighted score map with their decoded boxes,
// found behind the decode of the pass (DESIGN.md section 3 "Response peaks").
//
// The definition is vto_decode (oracle/vt_oracle.c) iterated; its text is k_peaks_dev.hpp's peaks_iterate, which the list
// launch of the peak arbitration (k_arbitrate.hip) shares.
//
// One workgroup of 256 threads per slot. The response plane sigmoid(score logit) * hann goes to LDS once (ns floats);
// a round is: the block argmax under hc_better (a 6-step wave butterfly + one step over the four waves' candidates),
// the window by nine threads, thread 0's sums and box into the record (LDS), the square's cells set to 0 in the plane.
// The finished record leaves as 68 dwords to the device array and to the pass's pinned host array. Nothing else is
// written: no word of StreamState, no result; no atomics, no tickets.
//
// This file is compiled with k_head.hip's flags (one IEEE operation per source operation).
// tests/test_gpu_response_peaks.py holds peak 0 to the decode's bits.
#include "k_peaks.hpp"
#include "k_peaks_dev.hpp"

static_assert(sizeof(vt_peak) == 32 && sizeof(vt_peaks) == 272, "vt_peaks layout");
static_assert(sizeof(PeaksPolicy) == 16, "PeaksPolicy layout");
static constexpr int kRecWords = sizeof(vt_peaks) / 4;

__global__ __launch_bounds__(256) void response_peaks_kernel(PeaksArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_plane[];    // [ns] responses; 0 where suppressed
    __shared__ PeaksLds s_it;
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
    const int K = min(pol.max_peaks, VT_PEAKS_MAX), R = pol.radius;
    // what the rounds need of the stream's state does not change from round to round: fetched once, wave-uniform
    const StreamState& s = a.states[sb];
    const PeaksGeo g{s.geo[0], s.geo[1], s.geo[3], (float)s.frame_w, (float)s.frame_h};
    const int frames_done = s.frames_done;
    if (tid < kRecWords) s_rec[tid] = 0u;
    const int n = peaks_iterate(a.head_out + (size_t)b * a.ns * 8, a.hann, s_plane, s_it, s_rec + 4, a.ns, a.grid, K, R, pol.min_resp, g);
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
