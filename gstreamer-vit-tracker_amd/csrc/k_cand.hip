// k_cand.hip — the two kernels of a candidate pass (vt_group_update_*_candidates): several slots may work for one
// stream, each an independent update around a box of its own; the device picks the stream's best slot and commits
// only that one.
//
//   fill    ahead of the crop: slot i's candidate state = its stream's state as it is ON THE DEVICE now, with the box
//           replaced where the slot brings one. Crop, band and decode kernels then run unchanged on the candidate
//           states (one StreamState per slot, identity slot map): nothing of a losing slot reaches a stream's state.
//   commit  behind the decode: per listed stream the winner among its slots, the stream's state, the winner table
//           and the host's copies.
#include "k_cand.hpp"

static_assert(sizeof(vt_candidate) == 24, "vt_candidate layout");
static_assert(sizeof(StreamState) == 88, "StreamState layout");
static constexpr int kStateWords = sizeof(StreamState) / 4;

// one thread per 32-bit word of a candidate state: words 0..3 are the box
__global__ __launch_bounds__(256) void cand_fill_kernel(CandArgs a) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n * kStateWords) return;
    const int slot = t / kStateWords, w = t - slot * kStateWords;
    const vt_candidate c = a.cands[slot];
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.states + c.stream);
    uint32_t v = src[w];
    if (c.has_box && w < 4) v = __float_as_uint(c.box[w]);
    reinterpret_cast<uint32_t*>(a.cand_states + slot)[w] = v;
}

// slot a = (score, index) beats slot b: the greater score; a NaN loses to any number; equal scores (or two NaNs): the
// lower slot. The tie rule of hc_better (k_head.hip), with NaN given a place so that the order is total.
__device__ __forceinline__ bool cand_better(float sa, int ia, float sb, int ib) {
    const bool na = sa != sa, nb = sb != sb;
    if (na != nb) return nb;
    if (!na && sa != sb) return sa > sb;
    return ia < ib;
}

// One workgroup, one pass over the n <= VT_MAX_STREAMS slots: streams and scores into LDS, then every slot scans the
// slots of its own stream. The slot that finds itself the winner commits the stream - exactly one does, so no two
// threads write one state and no atomics are needed.
__global__ __launch_bounds__(1024) void cand_commit_kernel(CandArgs a) {
    __shared__ int32_t s_stream[VT_MAX_STREAMS];
    __shared__ float s_score[VT_MAX_STREAMS];
    const int n = a.n;
    for (int i = threadIdx.x; i < n; i += 1024) {
        s_stream[i] = a.cands[i].stream;
        s_score[i] = a.results[i].score;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 1024) {
        const int s = s_stream[i];
        int best = -1;
        for (int j = 0; j < n; ++j)
            if (s_stream[j] == s && (best < 0 || cand_better(s_score[j], j, s_score[best], best))) best = j;
        a.winner[i] = best;
        if (a.host_winner) a.host_winner[i] = best;
        if (best != i) continue;
        // the winner's candidate state IS the stream's next state (the decode advanced frames_done by one and
        // success_count by the slot's success, from the values the fill copied) - but a winner that failed leaves the
        // stream's box what it was before the pass, never the candidate's
        StreamState w = a.cand_states[i];
        if (!a.results[i].success) {
            const StreamState& old = a.states[s];
#pragma unroll
            for (int k = 0; k < 4; ++k) w.box[k] = old.box[k];
        }
        a.states[s] = w;
        if (a.host_states) a.host_states[s] = w;
    }
    __threadfence_system();     // the host's copies are visible once the stream synchronises
}

hipError_t launch_cand_fill(const CandArgs& a, hipStream_t st) {
    if (a.n < 1 || a.n > VT_MAX_STREAMS || !a.cands || !a.states || !a.cand_states) return hipErrorInvalidValue;
    vt_launch(cand_fill_kernel, dim3((a.n * kStateWords + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_cand_commit(const CandArgs& a, hipStream_t st) {
    if (a.n < 1 || a.n > VT_MAX_STREAMS || !a.cands || !a.states || !a.cand_states || !a.results || !a.winner)
        return hipErrorInvalidValue;
    vt_launch(cand_commit_kernel, dim3(1), dim3(1024), 0, st, a);
    return hipGetLastError();
}
