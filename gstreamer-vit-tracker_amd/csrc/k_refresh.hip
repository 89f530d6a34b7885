// k_refresh.hip — device-side template refresh ("Template refresh").
//
// One launch behind the decode of every pass of an engine that enabled a refresh policy: grid (template tiles, slots).
// Every workgroup evaluates its slot's gate from wave-uniform loads - policy, result, the stream's state as the pass left
// it - and leaves at once when it does not fire, which is (period - 1) / period of the passes. A firing slot crops the
// template from ITS frame of THIS pass at the committed box into the stream's non-current buffer of the two-buffer store
// and then bumps the state's tpl_gen / tpl_frame, on the device and in the host's copy of the state.
//
// The crop is the text of the crop kernels (k_preproc_body.inc, with is_template = 1): the rows are the bits
// vt_group_init_*(stream, this frame, result.bbox) writes. This file is compiled like k_preproc.hip (-ffp-contract=off).
// The policy's rules, the geometry (rules 6 and 7), the crop's text and the launch table are shared with the appearance
// probe (k_appearance.hip): k_refresh_dev.hpp, k_refresh_crop.inc.
//
// Hand-over inside the launch: ONE word per slot, the ticket. Every workgroup of a firing slot takes a ticket after all
// its waves have read the state (the barrier in front of the ticket); the last to arrive writes the two words, so no
// workgroup can see the bumped state and decide otherwise than its neighbours. The rows themselves are read by later
// launches only. The last arrival puts the ticket back to zero; the engine also zeroes the tickets wherever a pass may
// have been abandoned (Engine::reset_refresh_tickets).
#include "k_refresh.hpp"
#include "k_appearance.hpp"     // rules 8, 9 and 10 read the three features' policies, counters and records
#include "k_conflicts.hpp"
#include "k_health.hpp"
#include "k_refresh_dev.hpp"

// What the kernels take of RefreshArgs: the members every engine sets, in their order, and - LAST in the argument block, so
// that the kernels of engines without the appearance check read the arguments they always read where they always lay -
// rule 8's three pointers, rule 8's and rule 9's (a null rule-8 policy: an engine without the appearance check), those and
// rule 10's, or nothing.
struct RefreshCore {
    const FrameDesc* frames; StreamState* states; const vt_result* results; const int32_t* slot_stream; const int32_t* winner;
    RefreshPolicy* policy; unsigned* tickets; bf16_t* tpl; const PassOut* out; StreamState* host_states; int n;
};
template <int GATE> struct RefreshGate {};
template <> struct RefreshGate<1> { const AppearPolicy* policy; AppearCount* counts; const AppearRec* recs; };
template <> struct RefreshGate<2> : RefreshGate<1> { const ConflictPolicy* cf_policy; ConflictCount* cf_counts; const ConflictRec* cf_recs; };
template <> struct RefreshGate<3> : RefreshGate<2> { const HealthPolicy* hl_policy; HealthCount* hl_counts; const HealthRec* hl_recs; };

// MODE: which crop body (k_refresh_dev.hpp, VT_TEMPLATE_CROP_LAUNCH). GATE: 3 on health-capable engines - rule 10, and rules 9
// and 8 where the engine has those features too (a null policy: off) -, 2 on conflicts-capable engines - rule 9, and
// rule 8 where the engine is appearance-capable too -, 1 on engines that are appearance-capable only - rule 8 -, 0 everywhere
// else: the kernels without the rules
template <int MODE, int ANY, int GATE>
__global__ __launch_bounds__(256) void template_refresh_kernel(RefreshCore a, int size, int ssize, int patch, int kpad,
                                                               int tpl_elems, float na0, float na1, float na2, float nb0,
                                                               float nb1, float nb2, RefreshGate<GATE> gate) {
    constexpr int LDSPX = VT_TEMPLATE_CROP_LDSPX(MODE);
    __shared__ uint32_t src[MODE <= 2 ? LDSPX : 1];
    const int slot = blockIdx.y;
    const int stream = a.slot_stream ? a.slot_stream[slot] : slot;
    // ---- the gate: rules 1-5 ----
    const RefreshPolicy pol = a.policy[stream];
    if (!refresh_rule1(pol)) return;
    if (a.winner && a.winner[slot] != slot) return;                 // a candidate pass refreshes at the committed slot only
    const vt_result r = a.results[slot];
    if (!refresh_rule3(pol, r)) return;
    StreamState st = a.states[stream];                              // a copy: the crop below never sees the bump
    if (!refresh_rule4(pol, st)) return;
    if (st.window_miss == st.frames_done) return;                   // this pass's search crop missed its window: the redo refreshes
    // ---- rule 9: no other stream of the stream's scene sits on the same pixels (k_conflicts.hip) ----
    // ahead of the geometry: a gated refresh counts no geometry skip and sets no window-miss mark
    if constexpr (GATE >= 2) {
        const ConflictPolicy cp = GATE == 2 || gate.cf_policy ? *gate.cf_policy : ConflictPolicy{};    // GATE 3 without the check: off
        if (cp.on != 0 && cp.gate != 0) {                             // "conflicts" 0 switches the gate off with the check
            const ConflictRec rec = gate.cf_recs[stream];
            if (rec.status == 2 && rec.frames_done == st.frames_done) {     // this pass's record
                if (blockIdx.x == 0 && threadIdx.x == 0) gate.cf_counts[stream].gated += 1;
                return;
            }
        }
    }
    // ---- rule 10: the picture itself is no good - frozen, flat or cut (k_health.hip). Behind rule 9: a refresh rule 9 refused
    // is not counted here; ahead of the geometry, like rule 9 ----
    if constexpr (GATE == 3) {
        const HealthPolicy hp = *gate.hl_policy;
        if (hp.on != 0 && hp.gate != 0) {                             // "health" 0 switches the gate off with the measures
            const HealthRec rec = gate.hl_recs[stream];
            if (rec.flags != 0 && rec.frames_done == st.frames_done) {      // this pass's record
                if (blockIdx.x == 0 && threadIdx.x == 0) gate.hl_counts[stream].gated += 1;
                return;
            }
        }
    }
    // ---- rules 6 and 7: the geometry (k_refresh_dev.hpp) ----
    {
        const int rule = template_taps_rule(st, a.frames[slot], size, ssize);
        if (rule == 6) {
            if (blockIdx.x == 0 && threadIdx.x == 0) a.policy[stream].skipped_geometry = pol.skipped_geometry + 1;
            return;
        }
        if (rule == 7) {
            if (blockIdx.x == 0 && threadIdx.x == 0)
                mark_window_miss(a.states, a.host_states ? a.host_states : a.out->host_states, stream, st.frames_done);
            return;
        }
    }
    // ---- rule 8: what the box holds still looks like what the stream was started from (k_appearance.hip) ----
    if constexpr (GATE != 0) {
        const AppearPolicy ap = GATE == 1 || gate.policy ? *gate.policy : AppearPolicy{0, 1, 0, 0.0f};    // GATE 2, 3 without the check: off
        const float tau = ap.tau;
        if (ap.on != 0 && tau > 0.0f) {                               // "appearance" 0 switches the gate off with the check
            const AppearRec rec = gate.recs[stream];
            if (!(rec.status == 1 && rec.frames_done == st.frames_done && rec.similarity >= tau)) {
                if (blockIdx.x == 0 && threadIdx.x == 0) gate.counts[stream].gated += 1;
                return;
            }
        }
    }
    // ---- the crop ----
    bf16_t* const crop_rows = a.tpl + ((size_t)stream * 2 + ((st.tpl_gen + 1) & 1)) * tpl_elems;
#include "k_refresh_crop.inc"
    // ---- commit: the last workgroup of the slot to arrive writes the two words ----
    __syncthreads();                                                 // every wave of this workgroup has read the state
    if (threadIdx.x != 0) return;
    const unsigned arrived = __hip_atomic_fetch_add(a.tickets + slot, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (arrived != gridDim.x - 1) return;
    const int gen = st.tpl_gen + 1, at = st.frames_done;
    a.states[stream].tpl_gen = gen;
    a.states[stream].tpl_frame = at;
    StreamState* hs = a.host_states ? a.host_states : a.out->host_states;
    if (hs) { hs[stream].tpl_gen = gen; hs[stream].tpl_frame = at; }
    __threadfence_system();                                          // as decode_box: the host's copy is visible at the pass's end
    __hip_atomic_store(a.tickets + slot, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int ANY, int GATE>
static void launch_refresh_t(const RefreshArgs& ra, const ModelDims& d, int tier, hipStream_t st) {
    const int size = d.T, tpl_elems = d.nt * d.kpad;
    const RefreshCore a{ra.frames, ra.states, ra.results, ra.slot_stream, ra.winner, ra.policy, ra.tickets, ra.tpl, ra.out,
                        ra.host_states, ra.n};
    RefreshGate<GATE> gate;
    if constexpr (GATE != 0) { gate.policy = ra.ap_policy; gate.counts = ra.ap_counts; gate.recs = ra.ap_recs; }
    if constexpr (GATE >= 2) { gate.cf_policy = ra.cf_policy; gate.cf_counts = ra.cf_counts; gate.cf_recs = ra.cf_recs; }
    if constexpr (GATE == 3) { gate.hl_policy = ra.hl_policy; gate.hl_counts = ra.hl_counts; gate.hl_recs = ra.hl_recs; }
#define RF_KERNEL(MODE) template_refresh_kernel<MODE, ANY, GATE>
    VT_TEMPLATE_CROP_LAUNCH(RF_KERNEL, d, tier, a.n, st, a, size, d.S, d.patch, d.kpad, tpl_elems, d.norm_a[0], d.norm_a[1],
                            d.norm_a[2], d.norm_b[0], d.norm_b[1], d.norm_b[2], gate);
#undef RF_KERNEL
}

template <int GATE>
static void launch_refresh_g(const RefreshArgs& a, const ModelDims& d, int tier, int any_layout, hipStream_t st) {
    if (any_layout >= 3) launch_refresh_t<3, GATE>(a, d, tier, st);
    else if (any_layout == 2) launch_refresh_t<2, GATE>(a, d, tier, st);
    else if (any_layout == 1) launch_refresh_t<1, GATE>(a, d, tier, st);
    else launch_refresh_t<0, GATE>(a, d, tier, st);
}

hipError_t launch_template_refresh(const RefreshArgs& a, const ModelDims& d, int tier, int any_layout, hipStream_t st) {
    if (a.n < 1 || !a.frames || !a.states || !a.results || !a.policy || !a.tickets || !a.tpl || !a.out)
        return hipErrorInvalidValue;
    const bool gate = a.ap_policy != nullptr;
    if (gate && (!a.ap_counts || !a.ap_recs)) return hipErrorInvalidValue;
    if (a.cf_policy && (!a.cf_counts || !a.cf_recs)) return hipErrorInvalidValue;
    if (a.hl_policy && (!a.hl_counts || !a.hl_recs)) return hipErrorInvalidValue;
    if (a.hl_policy) launch_refresh_g<3>(a, d, tier, any_layout, st);
    else if (a.cf_policy) launch_refresh_g<2>(a, d, tier, any_layout, st);
    else if (gate) launch_refresh_g<1>(a, d, tier, any_layout, st);
    else launch_refresh_g<0>(a, d, tier, any_layout, st);
    return hipGetLastError();
}
