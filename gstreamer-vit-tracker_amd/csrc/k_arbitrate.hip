// k_arbitrate.hip — peak arbitration ("Peak arbitration"): commit the runner-up of the response map
// that matches the stream's anchor where the Hann-weighted argmax no longer does. The rule is stated to the bit in
// include/vittrack_hip_ops.h (vt_op_arbitrate). Nothing new is computed here; three existing texts are combined:
//
// arbitrate_list, one workgroup per slot: peaks_iterate (k_peaks_dev.hpp: the response-peaks launch's iteration) under the
// policy's K, R and min_resp; then one thread decides whether the slot is due and which peaks are eligible - the model's
// success threshold on the score, refresh rules 6 and 7 (k_refresh_dev.hpp: the refresh kernel's text) on a copy of the
// state whose box is the peak's integer box - and writes the stream's record: final for status 0, 3, 4, 5, "due" (status 1,
// the peaks to cut marked 1) otherwise. Nothing of the state is written but the window-miss mark of a rule-7 failure.
//
// arbitrate_probe, grid (template tiles, slot x peak): for the marked peaks of due slots the text of the crop kernels
// (k_refresh_crop.inc around k_preproc_body.inc, is_template = 1) at the peak's integer box into probe[stream][peak]: the
// bits vt_group_init_*(stream, this frame, that box) would write as template rows.
//
// arbitrate_score, grid (row chunks, slot x peak): the appearance score's five binary64 sums in its fixed order
// (k_appearance_dev.hpp) of anchor[stream] and probe[stream][peak]; the (slot, peak)'s last-arriving workgroup - a ticket
// of its own per (slot, peak) - adds the chunk partials in index order and writes the peak's similarity. No floating-point
// atomics: the record is a function of the inputs alone.
//
// arbitrate_commit, one thread per slot: the switch rule on the similarities, the final record and, on a switch, exactly the
// words decode_box (k_head.hip) would have written had the chosen peak been the argmax.
//
// Compiled like k_refresh.hip (-ffp-contract=off, correctly rounded divide and sqrt): one IEEE operation per source operation.
#include "k_arbitrate.hpp"
#include "k_refresh_dev.hpp"
#include "k_peaks_dev.hpp"
#include "k_appearance_dev.hpp"

static_assert(VT_ARB_MAX <= VT_PEAKS_MAX, "the list is a prefix of the response peaks'");

__device__ __forceinline__ float arb_threshold(int32_t pm) { return (float)pm / 1000.0f; }      // the text of vtkeys::tau_of

// the stream's record, on the device and - final records only - in the pinned mirror
__device__ __forceinline__ void arb_store(const ArbArgs& a, int stream, const ArbRec& rec, bool mirror) {
    a.recs[stream] = rec;
    if (!mirror) return;
    ArbRec* h = a.host_recs ? a.host_recs : (a.out ? a.out->host_arbitrate : nullptr);
    if (h) { h[stream] = rec; __threadfence_system(); }
}

__device__ __forceinline__ void arb_int_box(const float* fbox, float* ibox) {        // as decode_box rounds
#pragma unroll
    for (int j = 0; j < 4; ++j) ibox[j] = (float)(int32_t)floorf(fbox[j] + 0.5f);
}

__global__ __launch_bounds__(256) void arbitrate_list_kernel(ArbArgs a, int size, int ssize) {
    extern __shared__ __attribute__((aligned(16))) float s_plane[];    // [ns] responses; 0 where suppressed
    __shared__ PeaksLds s_it;
    __shared__ uint32_t s_peaks[VT_ARB_MAX * 8];
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int stream = a.slot_stream ? a.slot_stream[slot] : slot;
    if (a.winner && a.winner[slot] != slot) return;                 // a stream's record is its winning slot's
    const ArbPolicy pol = *a.policy;
    const vt_result r = a.results[slot];
    const StreamState st = a.states[stream];                        // a copy
    ArbRec rec{};
    rec.frames_done = st.frames_done;
    // ---- the part of the due rule that needs no list ----
    if (pol.on == 0 || a.winner || r.success == 0 || st.window_miss == st.frames_done) {
        rec.status = pol.on != 0 && a.winner ? 3 : 0;
        if (tid == 0) arb_store(a, stream, rec, true);
        return;
    }
    const int K = min(max(pol.max_peaks, 1), VT_ARB_MAX);
    const PeaksGeo g{st.geo[0], st.geo[1], st.geo[3], (float)st.frame_w, (float)st.frame_h};
    if (tid < VT_ARB_MAX * 8) s_peaks[tid] = 0u;
    const int n = peaks_iterate(a.head_out + (size_t)slot * a.ns * 8, a.hann, s_plane, s_it, s_peaks, a.ns, a.grid, K, pol.radius,
                                arb_threshold(pol.min_resp_pm), g);
    if (tid != 0) return;
    // ---- eligibility, the geometry, the record ----
    rec.n = n;
    const FrameDesc fw = a.frames[slot];
    int status = 0, eligible = 0;
    for (int k = 0; k < n; ++k) {
        const uint32_t* p = s_peaks + k * 8;
        ArbPeak& pk = rec.peak[k];
        pk.score = __uint_as_float(p[0]); pk.resp = __uint_as_float(p[1]);
#pragma unroll
        for (int j = 0; j < 4; ++j) pk.box[j] = __uint_as_float(p[2 + j]);
        pk.cell = (int32_t)p[6];
    }
    for (int k = 0; k < n && status == 0; ++k) {
        ArbPeak& pk = rec.peak[k];
        if (k >= 1 && !(pk.score >= a.success_threshold)) continue;         // a NaN score fails
        StreamState at = st;
        arb_int_box(pk.box, at.box);
        const int rule = template_taps_rule(at, fw, size, ssize);
        if (rule == 7) status = 5;
        else if (rule == 6) { if (k == 0) status = 4; else pk.status = 2; }
        else { pk.status = 1; eligible += k >= 1; }
    }
    if (status == 0 && eligible > 0) {      // due: the probe, score and commit launches complete the record
        rec.status = 1;
        arb_store(a, stream, rec, false);
        return;
    }
    // final: nothing is cut, so no peak stays marked "cut"
    for (int k = 0; k < n; ++k)
        if (rec.peak[k].status == 1) rec.peak[k].status = 0;
    rec.status = status;
    if (status == 5)    // the host redoes the pass with an exact window; the redo arbitrates
        mark_window_miss(a.states, a.host_states ? a.host_states : (a.out ? a.out->host_states : nullptr), stream, st.frames_done);
    arb_store(a, stream, rec, true);
}

hipError_t launch_arbitrate_list(const ArbArgs& a, const ModelDims& d, hipStream_t st) {
    if (a.n < 1 || a.grid < 1 || a.ns != a.grid * a.grid || !a.head_out || !a.hann || !a.frames || !a.states || !a.results ||
        !a.policy || !a.recs)
        return hipErrorInvalidValue;
    const size_t lds = (size_t)a.ns * sizeof(float);
    if (lds > 48 * 1024) return hipErrorInvalidValue;      // as the response-peaks launch
    vt_launch(arbitrate_list_kernel, dim3(a.n), dim3(256), lds, st, a, d.T, d.S);
    return hipGetLastError();
}

// (slot, peak) of a workgroup of the probe and score launches, and whether it has work: the slot is due and the peak marked
struct ArbWork { int slot, k, stream; bool due; };
__device__ __forceinline__ ArbWork arb_work(const ArbArgs& a, int y) {
    ArbWork w;
    w.slot = y / VT_ARB_MAX; w.k = y % VT_ARB_MAX;
    w.stream = a.slot_stream ? a.slot_stream[w.slot] : w.slot;
    w.due = false;
    if (a.winner) return w;                                         // a candidate pass: the list launch said so (status 3)
    const ArbRec* rec = a.recs + w.stream;
    w.due = rec->status == 1 && w.k < rec->n && rec->peak[w.k].status == 1;
    return w;
}

template <int MODE, int ANY>
__global__ __launch_bounds__(256) void arbitrate_probe_kernel(ArbArgs a, int size, int patch, int kpad, int tpl_elems, float na0,
                                                              float na1, float na2, float nb0, float nb1, float nb2) {
    constexpr int LDSPX = VT_TEMPLATE_CROP_LDSPX(MODE);
    __shared__ uint32_t src[MODE <= 2 ? LDSPX : 1];
    const ArbWork w = arb_work(a, blockIdx.y);
    if (!w.due) return;
    const int slot = w.slot;
    StreamState st = a.states[w.stream];                            // a copy whose box is the peak's integer box
    {
        const ArbPeak& pk = a.recs[w.stream].peak[w.k];
        const float fbox[4] = {pk.box[0], pk.box[1], pk.box[2], pk.box[3]};
        arb_int_box(fbox, st.box);
    }
    bf16_t* const crop_rows = a.probe + ((size_t)w.stream * VT_ARB_MAX + w.k) * tpl_elems;
#include "k_refresh_crop.inc"
}

template <int ANY>
static void launch_arb_probe_t(const ArbArgs& a, const ModelDims& d, int tier, hipStream_t st) {
    const int size = d.T, tpl_elems = d.nt * d.kpad;
#define ARB_KERNEL(MODE) arbitrate_probe_kernel<MODE, ANY>
    VT_TEMPLATE_CROP_LAUNCH(ARB_KERNEL, d, tier, a.n * VT_ARB_MAX, st, a, size, d.patch, d.kpad, tpl_elems, d.norm_a[0], d.norm_a[1],
                            d.norm_a[2], d.norm_b[0], d.norm_b[1], d.norm_b[2]);
#undef ARB_KERNEL
}

hipError_t launch_arbitrate_probe(const ArbArgs& a, const ModelDims& d, int tier, int any_layout, hipStream_t st) {
    if (a.n < 1 || a.n * VT_ARB_MAX > 65535 || !a.frames || !a.states || !a.recs || !a.probe) return hipErrorInvalidValue;
    if (any_layout >= 3) launch_arb_probe_t<3>(a, d, tier, st);
    else if (any_layout == 2) launch_arb_probe_t<2>(a, d, tier, st);
    else if (any_layout == 1) launch_arb_probe_t<1>(a, d, tier, st);
    else launch_arb_probe_t<0>(a, d, tier, st);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void arbitrate_score_kernel(ArbArgs a, int nt, int cols, int kpad) {
    __shared__ double wsum[4][5];
    const int pair = blockIdx.y, chunk = blockIdx.x, nch = gridDim.x;
    // "cut" by this pass's list launch. The peak's final status is written behind the pair's last ticket, and every workgroup
    // reads it in front of its own: all of them decide alike.
    const ArbWork w = arb_work(a, pair);
    if (!w.due) return;
    const int r0 = chunk * VT_APPEAR_CHUNK_ROWS, r1 = min(nt, r0 + VT_APPEAR_CHUNK_ROWS);
    const bf16_t* __restrict__ A = a.anchor + (size_t)w.stream * nt * kpad + (size_t)r0 * kpad;
    const bf16_t* __restrict__ P = a.probe + ((size_t)w.stream * VT_ARB_MAX + w.k) * nt * kpad + (size_t)r0 * kpad;
    double part_sums[5];
    appear_chunk_sums(A, P, r1 - r0, cols, kpad, wsum, part_sums);      // k_appearance_dev.hpp: the fixed order
    if (threadIdx.x != 0) return;
    double* part = a.partials + ((size_t)pair * nch + chunk) * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) part[k] = part_sums[k];
    const unsigned arrived = __hip_atomic_fetch_add(a.tickets + pair, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (arrived != (unsigned)nch - 1) return;
    // ---- the pair's last workgroup: the chunks in index order, the similarity into the peak's two words ----
    double t[5];
    appear_add_chunks(a.partials + (size_t)pair * nch * 5, nch, t);
    float sim;
    const bool ok = appear_similarity(t, nt, cols, &sim);
    ArbPeak* pk = a.recs[w.stream].peak + w.k;
    pk->similarity = sim;
    pk->status = ok ? 1 : 3;
    __hip_atomic_store(a.tickets + pair, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

hipError_t launch_arbitrate_score(const ArbArgs& a, int nt, int cols, int kpad, hipStream_t st) {
    if (a.n < 1 || a.n * VT_ARB_MAX > 65535 || nt < 1 || cols < 1 || kpad < cols || !a.recs || !a.tickets || !a.partials || !a.anchor ||
        !a.probe)
        return hipErrorInvalidValue;
    vt_launch(arbitrate_score_kernel, dim3(appear_chunks(nt), a.n * VT_ARB_MAX), dim3(256), 0, st, a, nt, cols, kpad);
    return hipGetLastError();
}

__global__ __launch_bounds__(64) void arbitrate_commit_kernel(ArbArgs a) {
    const int slot = blockIdx.x * 64 + threadIdx.x;
    if (slot >= a.n || a.winner) return;
    const int stream = a.slot_stream ? a.slot_stream[slot] : slot;
    ArbRec rec = a.recs[stream];
    if (rec.status != 1) return;                                    // final since the list launch
    const ArbPolicy pol = *a.policy;
    const float low = arb_threshold(pol.low_pm), high = arb_threshold(pol.high_pm);
    int chosen = 0;
    // low 0 challenges nobody, whatever the sign of the similarity: the option is inert there, like a gate of 0 elsewhere
    if (rec.peak[0].status == 1 && low > 0.0f && rec.peak[0].similarity < low) {
        float best = 0.0f;
        for (int k = 1; k < rec.n; ++k) {
            const ArbPeak& pk = rec.peak[k];
            if (pk.status != 1 || !(pk.similarity >= high)) continue;
            if (chosen == 0 || pk.similarity > best) { chosen = k; best = pk.similarity; }      // a tie: the lowest k
        }
    }
    rec.status = chosen ? 2 : 1;
    rec.chosen = chosen;
    if (a.counts) {
        a.counts[stream].evaluated += 1;
        if (chosen) a.counts[stream].switched += 1;
    }
    if (chosen) {
        // what decode_box would have written had the chosen peak been the argmax; frames_done and success_count stay
        const ArbPeak& pk = rec.peak[chosen];
        float ibox[4];
        arb_int_box(pk.box, ibox);
        vt_result r;
        r.success = 1;
        r.score = pk.score;
        r.bbox.x = (int32_t)ibox[0]; r.bbox.y = (int32_t)ibox[1]; r.bbox.width = (int32_t)ibox[2]; r.bbox.height = (int32_t)ibox[3];
        a.results[slot] = r;
        StreamState* hs = a.host_states ? a.host_states : (a.out ? a.out->host_states : nullptr);
        vt_result* hr = a.out ? a.out->host_results : nullptr;
        if (hr) hr[slot] = r;
        StreamState* const both[2] = {a.states + stream, hs ? hs + stream : nullptr};
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            StreamState* s = both[m];
            if (!s) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) { s->last_fbox[j] = pk.box[j]; s->box[j] = ibox[j]; }
            s->last_score = pk.score;
            s->last_idx = pk.cell;
        }
        __threadfence_system();
    }
    arb_store(a, stream, rec, true);
}

hipError_t launch_arbitrate_commit(const ArbArgs& a, hipStream_t st) {
    if (a.n < 1 || !a.states || !a.results || !a.policy || !a.recs) return hipErrorInvalidValue;
    vt_launch(arbitrate_commit_kernel, dim3((a.n + 63) / 64), dim3(64), 0, st, a);
    return hipGetLastError();
}
