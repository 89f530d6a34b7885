// k_appearance.hip — the appearance check ("Appearance check").
//
// Two launches behind the decode of every pass of an engine that enabled the check (behind the candidate commit and
// motion_settle; ahead of the refresh, chip, peaks and overlay launches, so the probe is cut from undrawn pixels):
//
// appearance_probe, grid (template tiles, slots): every workgroup evaluates its slot's due rule from wave-uniform loads
// - the engine's policy, the result, the stream's state as the pass left it, the stream's refresh policy - and leaves at
// once when the slot is not due. A due slot applies refresh rules 6 and 7 (k_refresh_dev.hpp: the refresh kernel's text)
// and, where both hold, crops the template from ITS frame of THIS pass at the committed box into probe[stream]: the
// text of the crop kernels (k_refresh_crop.inc around k_preproc_body.inc, is_template = 1), so the rows are the bits
// vt_group_init_*(stream, this frame, result.bbox) would write as template rows. One thread writes the stream's record:
// final for status 0 and 2, "cut" (status 1, similarity 0) where the crop runs. Nothing of the state is written but the
// window-miss mark of a rule-7 failure.
//
// appearance_score, grid (row chunks, slots): for slots whose record says "cut", the five sums Sa, Sp, Saa, Spp, Sap of
// anchor[stream] and probe[stream] over the first `cols` columns of the nt rows, every value the exact binary64 of its
// bf16 (products of two bf16 values are exact in binary64). The order of the additions is FIXED: a lane adds its
// elements i = lane, lane + 256, ... of the chunk's (rows x cols) in ascending i; the 64 lanes of a wave as an xor
// butterfly 32, 16, 8, 4, 2, 1; the 4 waves in index order; the chunk partials go to global memory and the slot's
// last-arriving workgroup (the ticket pattern of k_refresh.hip) adds them in chunk order. No floating-point atomics: the
// record is a function of the inputs alone, whichever workgroup arrives last - pipelined == synchronous, bit for bit.
// Pad columns (cols..kpad) are never read. The summation's text is k_appearance_dev.hpp's, which the score launch of the peak
// arbitration (k_arbitrate.hip) shares.
//
// Compiled like k_refresh.hip (-ffp-contract=off): one IEEE operation per source operation.
#include "k_appearance.hpp"
#include "k_refresh_dev.hpp"
#include "k_appearance_dev.hpp"

// the stream's record, on the device and - final records only - in the pinned mirror of the pass
__device__ __forceinline__ void appear_store(const AppearArgs& a, int stream, const AppearRec& rec, bool mirror) {
    a.recs[stream] = rec;
    if (mirror && a.out) {
        AppearRec* h = a.out->host_appearance;
        if (h) { h[stream] = rec; __threadfence_system(); }
    }
}

template <int MODE, int ANY>
__global__ __launch_bounds__(256) void appearance_probe_kernel(AppearArgs a, int size, int ssize, int patch, int kpad,
                                                               int tpl_elems, float na0, float na1, float na2, float nb0,
                                                               float nb1, float nb2) {
    constexpr int LDSPX = VT_TEMPLATE_CROP_LDSPX(MODE);
    __shared__ uint32_t src[MODE <= 2 ? LDSPX : 1];
    const int slot = blockIdx.y;
    const int stream = a.slot_stream ? a.slot_stream[slot] : slot;
    if (a.winner && a.winner[slot] != slot) return;                 // (b) a stream's record is its winning slot's
    const AppearPolicy pol = *a.policy;
    const vt_result r = a.results[slot];
    StreamState st = a.states[stream];                              // a copy, as in the refresh kernel
    // ---- due: (a), (c), (d), (e) ----
    bool due = pol.on != 0 && r.success != 0 && st.window_miss != st.frames_done;
    if (due) {
        bool e = st.frames_done % max(pol.period, 1) == 0;
        if (!e && pol.tau > 0.0f && a.refresh) {                    // a refresh that rule 8 will judge in this pass
            const RefreshPolicy rp = a.refresh[stream];
            e = refresh_rule1(rp) && refresh_rule3(rp, r) && refresh_rule4(rp, st);
        }
        due = e;
    }
    // ---- refresh rules 6 and 7, unchanged ----
    const int rule = due ? template_taps_rule(st, a.frames[slot], size, ssize) : 0;
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
    if (!due || rule != 0) {
        if (lead) {
            if (rule == 7)      // the host redoes the pass with an exact window; the redo evaluates
                mark_window_miss(a.states, a.host_states ? a.host_states : (a.out ? a.out->host_states : nullptr), stream,
                                 st.frames_done);
            appear_store(a, stream, AppearRec{rule == 6 ? 2 : 0, st.frames_done, 0.0f, {st.box[0], st.box[1], st.box[2], st.box[3]}, 0},
                         true);
        }
        return;
    }
    if (lead)   // cut: the score launch completes the record
        appear_store(a, stream, AppearRec{1, st.frames_done, 0.0f, {st.box[0], st.box[1], st.box[2], st.box[3]}, 0}, false);
    // ---- the crop ----
    bf16_t* const crop_rows = a.probe + (size_t)stream * tpl_elems;
#include "k_refresh_crop.inc"
}

template <int ANY>
static void launch_probe_t(const AppearArgs& a, const ModelDims& d, int tier, hipStream_t st) {
    const int size = d.T, tpl_elems = d.nt * d.kpad;
#define AP_KERNEL(MODE) appearance_probe_kernel<MODE, ANY>
    VT_TEMPLATE_CROP_LAUNCH(AP_KERNEL, d, tier, a.n, st, a, size, d.S, d.patch, d.kpad, tpl_elems, d.norm_a[0], d.norm_a[1],
                            d.norm_a[2], d.norm_b[0], d.norm_b[1], d.norm_b[2]);
#undef AP_KERNEL
}

hipError_t launch_appearance_probe(const AppearArgs& a, const ModelDims& d, int tier, int any_layout, hipStream_t st) {
    if (a.n < 1 || !a.frames || !a.states || !a.results || !a.policy || !a.recs || !a.probe) return hipErrorInvalidValue;
    if (any_layout >= 3) launch_probe_t<3>(a, d, tier, st);
    else if (any_layout == 2) launch_probe_t<2>(a, d, tier, st);
    else if (any_layout == 1) launch_probe_t<1>(a, d, tier, st);
    else launch_probe_t<0>(a, d, tier, st);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void appearance_score_kernel(AppearArgs a, int nt, int cols, int kpad) {
    __shared__ double wsum[4][5];
    const int slot = blockIdx.y, chunk = blockIdx.x, nch = gridDim.x;
    const int stream = a.slot_stream ? a.slot_stream[slot] : slot;
    if (a.winner && a.winner[slot] != slot) return;
    // "cut" by this pass's probe launch. The final record is written behind the slot's last ticket, and every workgroup
    // reads the status in front of its own: all of them decide alike.
    if (a.recs[stream].status != 1) return;
    const int r0 = chunk * VT_APPEAR_CHUNK_ROWS, r1 = min(nt, r0 + VT_APPEAR_CHUNK_ROWS);
    const bf16_t* __restrict__ A = a.anchor + (size_t)stream * nt * kpad + (size_t)r0 * kpad;
    const bf16_t* __restrict__ P = a.probe + (size_t)stream * nt * kpad + (size_t)r0 * kpad;
    double part_sums[5];
    appear_chunk_sums(A, P, r1 - r0, cols, kpad, wsum, part_sums);      // k_appearance_dev.hpp: the fixed order
    if (threadIdx.x != 0) return;
    double* part = a.partials + ((size_t)slot * nch + chunk) * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) part[k] = part_sums[k];
    const unsigned arrived = __hip_atomic_fetch_add(a.tickets + slot, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (arrived != (unsigned)nch - 1) return;
    // ---- the slot's last workgroup: the chunks in index order, the similarity, the record ----
    double t[5];
    appear_add_chunks(a.partials + (size_t)slot * nch * 5, nch, t);
    AppearRec rec = a.recs[stream];
    rec.status = appear_similarity(t, nt, cols, &rec.similarity) ? 1 : 3;
    if (a.counts) a.counts[stream].evaluated += 1;
    if (a.sums)
#pragma unroll
        for (int k = 0; k < 5; ++k) a.sums[(size_t)slot * 5 + k] = t[k];
    appear_store(a, stream, rec, true);
    __hip_atomic_store(a.tickets + slot, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

hipError_t launch_appearance_score(const AppearArgs& a, int nt, int cols, int kpad, hipStream_t st) {
    if (a.n < 1 || nt < 1 || cols < 1 || kpad < cols || !a.policy || !a.recs || !a.tickets || !a.partials || !a.anchor || !a.probe)
        return hipErrorInvalidValue;
    vt_launch(appearance_score_kernel, dim3(appear_chunks(nt), a.n), dim3(256), 0, st, a, nt, cols, kpad);
    return hipGetLastError();
}
