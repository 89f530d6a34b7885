// k_conflicts.hip — the one launch of the stream conflicts (DESIGN.md section 3 "Stream conflicts"; include/vittrack_hip.h
// above the "conflicts*" keys): per stream of a pass, which other streams of the SAME pass and the same scene overlap its new
// box, and by how much.
//
//   check   behind the decode (candidate pass: behind the commit) and motion_settle, ahead of everything that cuts or draws:
//           per stream the eligibility, the IoU with every other eligible stream of its scene, the count of those at or over
//           tau and the four largest of them by (iou descending, stream index ascending), then the record to the device and
//           to the pinned mirror and the stream's counters. Refresh rule 9 (k_refresh.hip) reads the record.
//
// One workgroup, one lane per slot, n <= VT_MAX_STREAMS. Streams, scenes (0 for a slot nobody is compared with) and boxes are
// staged in LDS once; every working lane then walks the n entries - all lanes read entry j at the same time, so the reads
// are broadcasts - and keeps its four best in registers (constant indices only: nothing goes to scratch).
// Binary32 throughout, one IEEE operation per source operation: this file is built like k_motion.hip, with
// -ffp-contract=off and correctly rounded division (build.py), and says so itself with the pragma below.
// Plain vector stores, no atomics: exactly one lane works for a stream. Streams that are not in the pass are never read.
#include "k_conflicts.hpp"

#pragma clang fp contract(off)

static_assert(VT_MAX_STREAMS <= 1024, "one workgroup covers every slot");
static_assert(VT_CONFLICT_MAX == 4, "the insertion below is written for four entries");

// the IoU of two boxes (x, y, w, h), or 0 where they do not overlap; iou(s, t) and iou(t, s) are the same bits. Without a
// branch: the quotient of a pair that does not overlap is computed and dropped (no floating-point operation traps here)
__device__ __forceinline__ float cf_iou(const float4 s, const float4 t) {
    const float ix = fminf(s.x + s.z, t.x + t.z) - fmaxf(s.x, t.x);
    const float iy = fminf(s.y + s.w, t.y + t.w) - fmaxf(s.y, t.y);
    const float inter = ix * iy;
    const float as = s.z * s.w, at = t.z * t.w;
    const float uni = (as + at) - inter;
    const float q = inter / uni;
    return ix > 0.0f && iy > 0.0f ? q : 0.0f;
}

__global__ __launch_bounds__(1024) void conflicts_check_kernel(ConflictArgs a) {
    const ConflictPolicy pol = *a.policy;
    if (pol.on == 0) return;            // the whole workgroup: nothing is written
    __shared__ float4 s_box[VT_MAX_STREAMS];
    __shared__ int32_t s_stream[VT_MAX_STREAMS];
    __shared__ int2 s_key[VT_MAX_STREAMS];          // x: the scene, 0 where the slot is nobody's partner; y: the stream
    const int i = threadIdx.x, n = a.n;
    int s = 0;
    if (i < n) { s = a.slot_stream ? a.slot_stream[i] : i; s_stream[i] = s; }
    __syncthreads();
    // the one lane that works for a stream: the winning slot of a candidate pass, else the first (the only) slot that names it
    bool work = i < n;
    if (work && a.winner) work = a.winner[i] == i;
    else if (work && a.slot_stream)
        for (int j = 0; j < i; ++j)
            if (s_stream[j] == s) { work = false; break; }
    int scene = 0, frames_done = 0;
    float4 box = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (work) {
        const StreamState* st = a.states + s;
        frames_done = st->frames_done;
        const int sc = a.scenes[s];
        if (sc != 0 && st->initialized != 0 && a.results[i].success != 0 && st->window_miss != frames_done) {
            scene = sc;
            box = make_float4(st->box[0], st->box[1], st->box[2], st->box[3]);
        }
    }
    if (i < n) { s_key[i] = make_int2(scene, s); s_box[i] = box; }
    __syncthreads();
    if (!work) return;
    ConflictRec r;
    r.status = 3; r.frames_done = frames_done; r.n_over = 0; r.reserved = 0;
    float v[VT_CONFLICT_MAX];
    int p[VT_CONFLICT_MAX];
#pragma unroll
    for (int k = 0; k < VT_CONFLICT_MAX; ++k) { v[k] = 0.0f; p[k] = -1; }
    if (scene != 0) {
        const float tau = pol.tau;
        int n_over = 0;
        // entry j: both reads ahead of every test, a few entries at a time, so that the walk waits for LDS once per batch
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const int2 key = s_key[j];
            const float iou = cf_iou(box, s_box[j]);
            if (!(key.x == scene && j != i && iou > 0.0f && iou >= tau)) continue;      // a pair that does not overlap is never listed
            n_over += 1;
            const int t = key.y;
            // entry k takes the candidate where it is better than entry k and not better than entry k - 1, and entry
            // k - 1's old value where it is better than that one too (the list is sorted: better than k - 1 implies better than k)
#pragma unroll
            for (int k = VT_CONFLICT_MAX - 1; k >= 0; --k) {
                const int m = k > 0 ? k - 1 : 0;      // a constant once unrolled
                const bool bk = iou > v[k] || (iou == v[k] && t < p[k]);
                const bool bm = k > 0 && (iou > v[m] || (iou == v[m] && t < p[m]));
                v[k] = bm ? v[m] : bk ? iou : v[k];
                p[k] = bm ? p[m] : bk ? t : p[k];
            }
        }
        r.status = n_over > 0 ? 2 : 1;
        r.n_over = n_over;
        ConflictCount c = a.counts[s];
        c.evaluated += 1;
        c.conflicting += n_over > 0 ? 1 : 0;
        a.counts[s] = c;
    }
#pragma unroll
    for (int k = 0; k < VT_CONFLICT_MAX; ++k) { r.partner[k] = p[k]; r.iou[k] = v[k]; }
    a.recs[s] = r;
    ConflictRec* hc = a.out ? a.out->host_conflicts : nullptr;
    if (hc) hc[s] = r;
    __threadfence_system();     // the host's copy is visible once the stream synchronises
}

hipError_t launch_conflicts_check(const ConflictArgs& a, hipStream_t st) {
    if (a.n < 1 || a.n > VT_MAX_STREAMS || !a.states || !a.results || !a.policy || !a.scenes || !a.recs || !a.counts)
        return hipErrorInvalidValue;
    vt_launch(conflicts_check_kernel, dim3(1), dim3(1024), 0, st, a);
    return hipGetLastError();
}
