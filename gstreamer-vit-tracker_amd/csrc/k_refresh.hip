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
//
// Hand-over inside the launch: ONE word per slot, the ticket. Every workgroup of a firing slot takes a ticket after all
// its waves have read the state (the barrier in front of the ticket); the last to arrive writes the two words, so no
// workgroup can see the bumped state and decide otherwise than its neighbours. The rows themselves are read by later
// launches only. The last arrival puts the ticket back to zero; the engine also zeroes the tickets wherever a pass may
// have been abandoned (Engine::reset_refresh_tickets).
#include "vt_common.hpp"
#include "k_preproc_dev.hpp"

// MODE: which crop body, as launch_preproc picks it for the template - 0, 1, 2: the tile body with 16 / 32 / 64 KiB of
// LDS (the pass's tier; a tile that does not fit takes the body's per-pixel path), 3: wide stores of 8 pixels, 4: of 2
// pixels (patch 14), 5: one lane per pixel
template <int MODE, int ANY>
__global__ __launch_bounds__(256) void template_refresh_kernel(RefreshArgs a, int size, int ssize, int patch, int kpad,
                                                               int tpl_elems, float na0, float na1, float na2, float nb0,
                                                               float nb1, float nb2) {
    constexpr int LDSPX = MODE == 0 ? PRE_TILE_LDS : (MODE == 1 ? 2 * PRE_TILE_LDS : 4 * PRE_TILE_LDS);
    __shared__ uint32_t src[MODE <= 2 ? LDSPX : 1];
    const int slot = blockIdx.y;
    const int stream = a.slot_stream ? a.slot_stream[slot] : slot;
    // ---- the gate: rules 1-5 ----
    const RefreshPolicy pol = a.policy[stream];
    if (pol.period < 2) return;
    if (a.winner && a.winner[slot] != slot) return;                 // a candidate pass refreshes at the committed slot only
    const vt_result r = a.results[slot];
    if (!r.success || !(r.score >= pol.min_score)) return;          // a NaN score fails
    StreamState st = a.states[stream];                              // a copy: the crop below never sees the bump
    if (st.frames_done - st.tpl_frame < pol.period) return;
    if (st.window_miss == st.frames_done) return;                   // this pass's search crop missed its window: the redo refreshes
    // ---- rule 6: the template crop's taps at the new box lie inside the taps of the search crop this pass sampled ----
    {
        const float area = st.box[2] * st.box[3];
        const float side = 2.0f * sqrtf(area);
        const float scale = side / (float)size;
        const float half = 0.5f * side;
        const float x0t = ((st.box[0] + 0.5f * st.box[2]) - half) - 0.5f;
        const float y0t = ((st.box[1] + 0.5f * st.box[3]) - half) - 0.5f;
        int tx0, tx1, ty0, ty1, sx0, sx1, sy0, sy1;
        tap_range(scale, x0t, size, tx0, tx1);
        tap_range(scale, y0t, size, ty0, ty1);
        tap_range(st.geo[2], st.geo[0], ssize, sx0, sx1);
        tap_range(st.geo[2], st.geo[1], ssize, sy0, sy1);
        if (tx0 < sx0 || tx1 > sx1 || ty0 < sy0 || ty1 > sy1) {
            if (blockIdx.x == 0 && threadIdx.x == 0) a.policy[stream].skipped_geometry = pol.skipped_geometry + 1;
            return;
        }
        // ---- rule 7: the in-frame part of the template's taps lies inside the window the caller stored ----
        // A window the library cut for THIS box (synchronous passes, redone passes) holds the search crop's rectangle
        // and 4 pixels around it, whole frames hold everything: the term cannot fail there. A SPECULATIVE window
        // (pipelined passes: cut around the previous box) can end inside the search rectangle without a miss - where the
        // rectangle hangs over the frame edge its first tapped in-frame column may lie up to `scale` pixels inside the
        // frame, and at scales above 2 the search crop steps over columns the denser template crop taps. Such a pass
        // is reported as a window miss instead of refreshed from black taps: the host redoes it with an exact window,
        // as for any other miss, and the redo refreshes - pipelined == synchronous holds here too.
        const FrameDesc& fw = a.frames[slot];
        const int cx0 = max(tx0, 0), cx1 = min(tx1, fw.w - 1), cy0 = max(ty0, 0), cy1 = min(ty1, fw.h - 1);
        if (cx0 <= cx1 && cy0 <= cy1 &&
            (cx0 < fw.x0 || cx1 >= fw.x0 + fw.ww || cy0 < fw.y0 || cy1 >= fw.y0 + fw.wh)) {
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                a.states[stream].window_miss = st.frames_done;
                StreamState* hs = a.host_states ? a.host_states : a.out->host_states;
                if (hs) hs[stream].window_miss = st.frames_done;
                __threadfence_system();
            }
            return;
        }
    }
    // ---- the crop: the names the body's text expects ----
    {
        const FrameDesc f = a.frames[slot];
        StreamState& s = st;
        bf16_t* __restrict__ patches = a.tpl + ((size_t)stream * 2 + ((st.tpl_gen + 1) & 1)) * tpl_elems;
        const int b = 0, ntok = 0, row_off = 0, is_template = 1;    // rows [0, nt) of `patches`
        const float factor = 2.0f;
        auto crop = [&]() {                                          // a body may return: from here
            if constexpr (MODE <= 2) {
                constexpr int PX = 8;
#define PRE_BODY 3
#include "k_preproc_body.inc"
            } else if constexpr (MODE <= 4) {
                constexpr int PX = MODE == 3 ? 8 : 2;
#define PRE_BODY 2
#include "k_preproc_body.inc"
            } else {
#define PRE_BODY 1
#include "k_preproc_body.inc"
            }
        };
        crop();
    }
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

template <int ANY>
static void launch_refresh_t(const RefreshArgs& a, const ModelDims& d, int tier, hipStream_t st) {
    const int size = d.T, tpl_elems = d.nt * d.kpad;
#define RF_ARGS a, size, d.S, d.patch, d.kpad, tpl_elems, d.norm_a[0], d.norm_a[1], d.norm_a[2], d.norm_b[0], d.norm_b[1], d.norm_b[2]
    // the branches of launch_preproc_t (k_preproc.hip) for the template crop
    if (d.patch % 8 == 0 && d.kpad % 8 == 0 && size % PRE_TILE_W == 0 && size % PRE_TILE_H == 0) {
        const dim3 grid((size / PRE_TILE_W) * (size / PRE_TILE_H), a.n);
        if (tier <= 0) vt_launch(template_refresh_kernel<0, ANY>, grid, dim3(256), 0, st, RF_ARGS);
        else if (tier == 1) vt_launch(template_refresh_kernel<1, ANY>, grid, dim3(256), 0, st, RF_ARGS);
        else vt_launch(template_refresh_kernel<2, ANY>, grid, dim3(256), 0, st, RF_ARGS);
    } else if (d.patch % 8 == 0 && d.kpad % 8 == 0) {
        vt_launch(template_refresh_kernel<3, ANY>, dim3((size * size / 8 + 255) / 256, a.n), dim3(256), 0, st, RF_ARGS);
    } else if (d.patch % 2 == 0 && d.kpad % 2 == 0) {
        vt_launch(template_refresh_kernel<4, ANY>, dim3((size * size / 2 + 255) / 256, a.n), dim3(256), 0, st, RF_ARGS);
    } else {
        vt_launch(template_refresh_kernel<5, ANY>, dim3((size * size + 255) / 256, a.n), dim3(256), 0, st, RF_ARGS);
    }
#undef RF_ARGS
}

hipError_t launch_template_refresh(const RefreshArgs& a, const ModelDims& d, int tier, int any_layout, hipStream_t st) {
    if (a.n < 1 || !a.frames || !a.states || !a.results || !a.policy || !a.tickets || !a.tpl || !a.out)
        return hipErrorInvalidValue;
    if (any_layout >= 2) launch_refresh_t<2>(a, d, tier, st);
    else if (any_layout == 1) launch_refresh_t<1>(a, d, tier, st);
    else launch_refresh_t<0>(a, d, tier, st);
    return hipGetLastError();
}
