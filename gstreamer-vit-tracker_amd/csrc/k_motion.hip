// k_motion.hip — the two launches of the motion prior (DESIGN.md section 3 "Motion prior"; include/vittrack_hip.h above
// the "motion_*" keys): a per-stream velocity estimate that places the next search window where the target is heading,
// and keeps it moving through a few failed updates.
//
//   place   the first launch of a pass, ahead of every crop and of cand_fill: per listed, initialised stream the record's
//           prior = the state box, and the box moves by v where the engine flag is on and the moved centre stays inside
//           the frame. Everything downstream reads the state as it always did.
//   settle  behind the decode (candidate pass: behind the commit): the velocity update on a success, the coast or the
//           restore on a failure, then the final box and the record to the device and to the pinned mirrors.
//
// One workgroup, one lane per slot, n <= VT_MAX_STREAMS. Binary32 throughout, one IEEE operation per source operation:
// this file is built like the decode, with -ffp-contract=off and correctly rounded division and square root (build.py),
// and says so itself with the pragma below.
// Plain vector stores, no atomics: exactly one lane works for a stream.
#include "k_motion.hpp"

#pragma clang fp contract(off)

static_assert(VT_MAX_STREAMS <= 1024, "one workgroup covers every slot");

// the one lane that works for slot i's stream in the place launch: the first slot that names it (a candidate pass may
// name a stream in several slots; every other pass names it once)
__device__ __forceinline__ bool mo_first_of_stream(const int32_t* s_stream, int i) {
    const int s = s_stream[i];
    for (int j = 0; j < i; ++j)
        if (s_stream[j] == s) return false;
    return true;
}

__global__ __launch_bounds__(1024) void motion_place_kernel(MotionArgs a) {
    __shared__ int32_t s_stream[VT_MAX_STREAMS];
    const int i = threadIdx.x, n = a.n;
    if (i < n) s_stream[i] = a.slot_stream ? a.slot_stream[i] : i;
    __syncthreads();
    if (i >= n) return;
    if (a.slot_stream && !mo_first_of_stream(s_stream, i)) return;
    const int s = s_stream[i];
    StreamState* st = a.states + s;
    if (!st->initialized) return;
    const MotionPolicy pol = *a.policy;
    MotionRec r = a.recs[s];
    const float b[4] = {st->box[0], st->box[1], st->box[2], st->box[3]};
    float nb[4];
    const bool tried = pol.on && !(r.v[0] == 0.0f && r.v[1] == 0.0f);
    const bool moved = motion_predict(pol.on, b, r.v, st->frame_w, st->frame_h, nb);
#pragma unroll
    for (int k = 0; k < 4; ++k) r.prior[k] = b[k];
    r.shift[0] = 0.0f; r.shift[1] = 0.0f;
    if (moved) {
        r.shift[0] = r.v[0]; r.shift[1] = r.v[1];
        r.n_shift += 1;
        st->box[0] = nb[0]; st->box[1] = nb[1];
    } else if (tried) {         // the moved centre would leave the frame: the estimate is dropped, the box stays
        r.v[0] = 0.0f; r.v[1] = 0.0f;
        r.live = 0;
    }
    a.recs[s] = r;
}

__global__ __launch_bounds__(1024) void motion_settle_kernel(MotionArgs a) {
    const int i = threadIdx.x;
    if (i >= a.n) return;
    if (a.winner && a.winner[i] != i) return;      // a candidate pass: the winning slot speaks for its stream
    const int s = a.slot_stream ? a.slot_stream[i] : i;
    StreamState* st = a.states + s;
    if (!st->initialized) return;
    const MotionPolicy pol = *a.policy;
    MotionRec r = a.recs[s];
    float b[4] = {st->box[0], st->box[1], st->box[2], st->box[3]};
    if (pol.on) {
        const vt_result res = a.results[i];
        const bool placed = a.cands && a.cands[i].has_box != 0;    // the caller placed the winning slot: no motion
        if (res.success && !placed) {
            const float cox = r.prior[0] + 0.5f * r.prior[2], coy = r.prior[1] + 0.5f * r.prior[3];
            const float cnx = b[0] + 0.5f * b[2], cny = b[1] + 0.5f * b[3];
            const float d[2] = {cnx - cox, cny - coy};
            const float g = (float)pol.gain_pct / 100.0f;
            const float area = b[2] * b[3];
            const float lim = ((float)pol.max_pct / 100.0f) * sqrtf(area);     // correctly rounded, as the crop's side is
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float e = d[k] - r.v[k];
                const float ge = g * e;
                float v = r.v[k] + ge;              // three operations, three roundings
                // fminf(fmaxf(v, -lim), lim) as two comparisons: the sign of a zero result (lim == 0) does not depend
                // on how a minimum orders -0 and +0
                v = v < -lim ? -lim : v;
                r.v[k] = v > lim ? lim : v;
            }
            r.live = pol.coast;
        } else if (res.success) {
            r.v[0] = 0.0f; r.v[1] = 0.0f;
            r.live = pol.coast;
        } else if (r.live > 0) {    // the box stays where the place launch put it: it coasts
            r.live -= 1;
            if (r.shift[0] != 0.0f || r.shift[1] != 0.0f) r.n_coast += 1;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) b[k] = r.prior[k];
            r.v[0] = 0.0f; r.v[1] = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) st->box[k] = b[k];
        }
        a.recs[s] = r;
    }
    StreamState* hs = a.host_states ? a.host_states : (a.out ? a.out->host_states : nullptr);
    MotionRec* hm = a.out ? a.out->host_motion : nullptr;
    if (hs) {
#pragma unroll
        for (int k = 0; k < 4; ++k) hs[s].box[k] = b[k];
    }
    if (hm) hm[s] = r;
    __threadfence_system();     // the host's copies are visible once the stream synchronises
}

static bool motion_args_ok(const MotionArgs& a) {
    return a.n >= 1 && a.n <= VT_MAX_STREAMS && a.states && a.recs && a.policy;
}

hipError_t launch_motion_place(const MotionArgs& a, hipStream_t st) {
    if (!motion_args_ok(a)) return hipErrorInvalidValue;
    vt_launch(motion_place_kernel, dim3(1), dim3(1024), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_motion_settle(const MotionArgs& a, hipStream_t st) {
    if (!motion_args_ok(a) || !a.results) return hipErrorInvalidValue;
    vt_launch(motion_settle_kernel, dim3(1), dim3(1024), 0, st, a);
    return hipGetLastError();
}
