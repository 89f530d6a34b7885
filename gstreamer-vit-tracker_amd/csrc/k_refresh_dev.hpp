// k_refresh_dev.hpp — what the launches that cut a template-sized crop at a box of the pass share: the template refresh
// (k_refresh.hip), the appearance probe (k_appearance.hip) and the peak arbitration (k_arbitrate.hip: rules 6 and 7 in its list
// launch, the launch table in its probe launch). The ONE text of refresh rules 1, 3, 4 (the policy's part of
// the gate), of rules 6 and 7 (the geometry: DESIGN.md section 3, "Template refresh"), of the window-miss mark a rule-7
// failure leaves, and of the launch table that picks a crop body as launch_preproc picks it for the template. The crop
// itself is the text of k_refresh_crop.inc around the crop kernels' bodies (k_preproc_body.inc).
#pragma once
#include "k_refresh.hpp"
#include "k_preproc_dev.hpp"

// rule 1: the stream has a policy; rule 3: the update succeeded with at least the policy's score (a NaN score fails);
// rule 4: the policy's period has passed since the stream's last refresh
__device__ __forceinline__ bool refresh_rule1(const RefreshPolicy& pol) { return pol.period >= 2; }
__device__ __forceinline__ bool refresh_rule3(const RefreshPolicy& pol, const vt_result& r) {
    if (!r.success || !(r.score >= pol.min_score)) return false;
    return true;
}
__device__ __forceinline__ bool refresh_rule4(const RefreshPolicy& pol, const StreamState& st) {
    return st.frames_done - st.tpl_frame >= pol.period;
}

// Rules 6 and 7 for a template crop (factor 2, side `size`) at st.box, against the search crop this pass sampled (st.geo,
// side `ssize`) and the window the caller stored of the slot's frame. 0: both hold; 6 / 7: the first that fails.
// rule 6: the template crop's taps at the new box lie inside the taps of the search crop this pass sampled
// rule 7: the in-frame part of the template's taps lies inside the window the caller stored.
// A window the library cut for THIS box (synchronous passes, redone passes) holds the search crop's rectangle
// and 4 pixels around it, whole frames hold everything: the term cannot fail there. A SPECULATIVE window
// (pipelined passes: cut around the previous box) can end inside the search rectangle without a miss - where the
// rectangle hangs over the frame edge its first tapped in-frame column may lie up to `scale` pixels inside the
// frame, and at scales above 2 the search crop steps over columns the denser template crop taps. Such a pass
// is reported as a window miss instead of cut from black taps: the host redoes it with an exact window,
// as for any other miss, and the redo cuts - pipelined == synchronous holds here too.
__device__ __forceinline__ int template_taps_rule(const StreamState& st, const FrameDesc& fw, int size, int ssize) {
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
    if (tx0 < sx0 || tx1 > sx1 || ty0 < sy0 || ty1 > sy1) return 6;
    const int cx0 = max(tx0, 0), cx1 = min(tx1, fw.w - 1), cy0 = max(ty0, 0), cy1 = min(ty1, fw.h - 1);
    if (cx0 <= cx1 && cy0 <= cy1 &&
        (cx0 < fw.x0 || cx1 >= fw.x0 + fw.ww || cy0 < fw.y0 || cy1 >= fw.y0 + fw.wh))
        return 7;
    return 0;
}

// what a rule-7 failure leaves (one thread): this pass counts as a window miss, on the device and in the host's copy
__device__ __forceinline__ void mark_window_miss(StreamState* states, StreamState* host_states, int stream, int frames_done) {
    states[stream].window_miss = frames_done;
    if (host_states) host_states[stream].window_miss = frames_done;
    __threadfence_system();
}

// The branches of launch_preproc_t (k_preproc.hip) for the template crop: K(MODE) names the kernel instance of a crop
// body - MODE 0, 1, 2: the tile body with 16 / 32 / 64 KiB of LDS (the pass's tier; a tile that does not fit takes the
// body's per-pixel path), 3: wide stores of 8 pixels, 4: of 2 pixels (patch 14), 5: one lane per pixel. Grid
// (template tiles or pixel groups, slots).
#define VT_TEMPLATE_CROP_LAUNCH(K, d, tier, slots, st, ...)                                                              \
    do {                                                                                                                 \
        const int size_ = (d).T;                                                                                         \
        if ((d).patch % 8 == 0 && (d).kpad % 8 == 0 && size_ % PRE_TILE_W == 0 && size_ % PRE_TILE_H == 0) {              \
            const dim3 grid_((size_ / PRE_TILE_W) * (size_ / PRE_TILE_H), (slots));                                      \
            if ((tier) <= 0) vt_launch(K(0), grid_, dim3(256), 0, st, __VA_ARGS__);                                      \
            else if ((tier) == 1) vt_launch(K(1), grid_, dim3(256), 0, st, __VA_ARGS__);                                 \
            else vt_launch(K(2), grid_, dim3(256), 0, st, __VA_ARGS__);                                                  \
        } else if ((d).patch % 8 == 0 && (d).kpad % 8 == 0) {                                                            \
            vt_launch(K(3), dim3((size_ * size_ / 8 + 255) / 256, (slots)), dim3(256), 0, st, __VA_ARGS__);              \
        } else if ((d).patch % 2 == 0 && (d).kpad % 2 == 0) {                                                            \
            vt_launch(K(4), dim3((size_ * size_ / 2 + 255) / 256, (slots)), dim3(256), 0, st, __VA_ARGS__);              \
        } else {                                                                                                         \
            vt_launch(K(5), dim3((size_ * size_ + 255) / 256, (slots)), dim3(256), 0, st, __VA_ARGS__);                  \
        }                                                                                                                \
    } while (0)
// LDS pixels of a MODE's tile body
#define VT_TEMPLATE_CROP_LDSPX(MODE) ((MODE) == 0 ? PRE_TILE_LDS : ((MODE) == 1 ? 2 * PRE_TILE_LDS : 4 * PRE_TILE_LDS))
