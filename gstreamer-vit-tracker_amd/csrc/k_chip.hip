// k_chip.hip — target chips ("Target chips"): a resized crop of each stream's new box, cut inside the pass.
//
// One launch behind the decode (behind cand_commit and the refresh launch where the pass has them) of every pass of an
// engine that enabled chips: grid (chip tiles, slots). Every workgroup evaluates its slot's gate from wave-uniform loads -
// policy, the stream's state as the pass left it - and leaves at once when it does not fire, as template_refresh_kernel
// does. A firing slot crops ITS frame of THIS pass at the committed box into the stream's chip buffer. Thread 0 of the
// slot's first workgroup writes the stream's vt_chip_info, fired or not; nothing in the state is bumped, so the launch
// needs no ticket. The one word of state it may write is window_miss (rule 5), as the refresh launch does.
//
// The crop is the text of the crop kernels (k_preproc_body.inc) with patch := C, kpad := 3 C^2, ntok = row_off = b = 0 and
// is_template = 1: the body's own store then writes the planar [3][C][C] bf16 chip, and vto_preproc with the same
// arguments is its oracle. The u8 kind keeps the bilinear value v of the same text (PRE_OUT) and stores packed RGB bytes
// (PRE_STORE_RGB8). This file is compiled like k_preproc.hip (-ffp-contract=off).
#include "k_chip.hpp"
#include "k_preproc_dev.hpp"

// a lane's run of 8 pixels as packed RGB: 24 bytes at a 24-byte stride (8-byte aligned: C is a multiple of 8), stored as
// three 8-byte pieces. A wave's three store instructions together cover whole lines (192 contiguous bytes per tile row,
// 1,536 in the wide body). Handing the tile over through LDS for 16-byte stores of whole rows measured 0.1 us (1 %) apart
// in the pass and cannot serve the wide body; not kept (profiles/target_chips.txt).
__device__ __forceinline__ void chip_pack_run(const bf16_t (&o)[3][8], uint32_t (&w)[6]) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int byte = 4 * j + i;
            v |= (uint32_t)o[byte % 3][byte / 3] << (8 * i);
        }
        w[j] = v;
    }
}
__device__ __forceinline__ void chip_store_run(const bf16_t (&o)[3][8], uint8_t* dst) {
    uint32_t w[6];
    chip_pack_run(o, w);
    uint2* d = reinterpret_cast<uint2*>(dst);
    d[0] = make_uint2(w[0], w[1]);
    d[1] = make_uint2(w[2], w[3]);
    d[2] = make_uint2(w[4], w[5]);
}

// MODE: which crop body - 0, 1, 2: the tile body with 16 / 32 / 64 KiB of LDS (the pass's tier; a tile that does not fit
// takes the body's per-pixel path), 3: wide stores of 8 pixels. KIND: vt_chip_kind
template <int MODE, int ANY, int KIND>
__global__ __launch_bounds__(256) void target_chip_kernel(ChipArgs a, int size, int ssize, int chip_bytes, float na0, float na1,
                                                          float na2, float nb0, float nb1, float nb2) {
    constexpr int LDSPX = MODE == 0 ? PRE_TILE_LDS : (MODE == 1 ? 2 * PRE_TILE_LDS : 4 * PRE_TILE_LDS);
    __shared__ uint32_t src[MODE <= 2 ? LDSPX : 1];
    const int slot = blockIdx.y;
    const int stream = a.slot_stream ? a.slot_stream[slot] : slot;
    // ---- the gate ----
    const ChipPolicy pol = a.policy[stream];
    if (!(pol.factor > 0.0f)) return;                               // off: the stream's record stays untouched
    if (a.winner && a.winner[slot] != slot) return;                 // a candidate pass cuts at the committed slot only
    StreamState st = a.states[stream];
    const float factor = pol.factor;
    // the chip crop's geometry at the new box: the operations of the bodies below, in their order
    const float area = st.box[2] * st.box[3];
    const float side = factor * sqrtf(area);
    const float scale = side / (float)size;
    const float half = 0.5f * side;
    const float x0c = ((st.box[0] + 0.5f * st.box[2]) - half) - 0.5f;
    const float y0c = ((st.box[1] + 0.5f * st.box[3]) - half) - 0.5f;
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    auto info = [&](int status) {
        if (!writer) return;
        const vt_result r = a.results[slot];
        vt_chip_info ci;
        ci.status = status;
        ci.frames_done = st.frames_done;
        ci.success = r.success;
        ci.score = r.score;
#pragma unroll
        for (int k = 0; k < 4; ++k) ci.box[k] = (int32_t)st.box[k];
        ci.geo[0] = x0c; ci.geo[1] = y0c; ci.geo[2] = scale;
        ci.reserved[0] = 0;
        a.infos[stream] = ci;
    };
    if (st.frames_done % pol.period != pol.phase) { info(0); return; }     // rule 1: not due
    if (st.window_miss == st.frames_done) { info(0); return; }      // rule 3: this pass is redone, and the redo cuts
    {
        // ---- rule 4: the chip's taps at the new box lie inside the taps of the search crop this pass sampled ----
        int tx0, tx1, ty0, ty1, sx0, sx1, sy0, sy1;
        tap_range(scale, x0c, size, tx0, tx1);
        tap_range(scale, y0c, size, ty0, ty1);
        tap_range(st.geo[2], st.geo[0], ssize, sx0, sx1);
        tap_range(st.geo[2], st.geo[1], ssize, sy0, sy1);
        if (tx0 < sx0 || tx1 > sx1 || ty0 < sy0 || ty1 > sy1) { info(2); return; }
        // ---- rule 5: the in-frame part of the chip's taps lies inside the window the caller stored (k_refresh.hip, rule 7)
        const FrameDesc& fw = a.frames[slot];
        const int cx0 = max(tx0, 0), cx1 = min(tx1, fw.w - 1), cy0 = max(ty0, 0), cy1 = min(ty1, fw.h - 1);
        if (cx0 <= cx1 && cy0 <= cy1 &&
            (cx0 < fw.x0 || cx1 >= fw.x0 + fw.ww || cy0 < fw.y0 || cy1 >= fw.y0 + fw.wh)) {
            if (writer) {
                a.states[stream].window_miss = st.frames_done;
                StreamState* hs = a.host_states ? a.host_states : a.out->host_states;
                if (hs) hs[stream].window_miss = st.frames_done;
                __threadfence_system();
            }
            info(0);
            return;
        }
    }
    info(1);
    // ---- the crop: the names the body's text expects ----
    const FrameDesc f = a.frames[slot];
    StreamState& s = st;
    uint8_t* const chip8 = a.chips + (size_t)stream * chip_bytes;
    bf16_t* __restrict__ patches = reinterpret_cast<bf16_t*>(chip8);
    const int patch = size, kpad = 3 * size * size;                 // one token: its row is the planar chip
    const int b = 0, ntok = 0, row_off = 0, is_template = 1;
    if constexpr (KIND == VT_CHIP_NORM_BF16) {
        if constexpr (MODE <= 2) {
            constexpr int PX = 8;
#define PRE_BODY 3
#include "k_preproc_body.inc"
        } else {
            constexpr int PX = 8;
#define PRE_BODY 2
#include "k_preproc_body.inc"
        }
    } else {
#define PRE_OUT(v, c) ((void)na, (void)nb, (bf16_t)fminf(fmaxf(rintf(v), 0.0f), 255.0f))    // the norms are not this kind's
#define PRE_STORE_RGB8
        if constexpr (MODE <= 2) {
            constexpr int PX = 8;
#define PRE_STORE_RGB8_RUN(o, dst) chip_store_run(o, dst)
#define PRE_BODY 3
#include "k_preproc_body.inc"
#undef PRE_STORE_RGB8_RUN
        } else {
            constexpr int PX = 8;
#define PRE_STORE_RGB8_RUN(o, dst) chip_store_run(o, dst)
#define PRE_BODY 2
#include "k_preproc_body.inc"
#undef PRE_STORE_RGB8_RUN
        }
#undef PRE_STORE_RGB8
#undef PRE_OUT
    }
}

template <int ANY, int KIND>
static void launch_chips_t(const ChipArgs& a, int C, int chip_bytes, const float* na, const float* nb, int ssize, int tier,
                           hipStream_t st) {
#define CH_ARGS a, C, ssize, chip_bytes, na[0], na[1], na[2], nb[0], nb[1], nb[2]
    if (C % PRE_TILE_W == 0) {      // PRE_TILE_H divides PRE_TILE_W
        const dim3 grid((C / PRE_TILE_W) * (C / PRE_TILE_H), a.n);
        if (tier <= 0) vt_launch(target_chip_kernel<0, ANY, KIND>, grid, dim3(256), 0, st, CH_ARGS);
        else if (tier == 1) vt_launch(target_chip_kernel<1, ANY, KIND>, grid, dim3(256), 0, st, CH_ARGS);
        else vt_launch(target_chip_kernel<2, ANY, KIND>, grid, dim3(256), 0, st, CH_ARGS);
    } else {
        vt_launch(target_chip_kernel<3, ANY, KIND>, dim3((C * C / 8 + 255) / 256, a.n), dim3(256), 0, st, CH_ARGS);
    }
#undef CH_ARGS
}

hipError_t launch_target_chips(const ChipArgs& a, int C, int kind, const float* na, const float* nb, int search_size,
                               int tier, int any_layout, hipStream_t st) {
    if (a.n < 1 || !a.frames || !a.states || !a.results || !a.policy || !a.chips || !a.infos || !a.out || !na || !nb ||
        C < 32 || C > 512 || C % 8 != 0 || (kind != VT_CHIP_NORM_BF16 && kind != VT_CHIP_RGB8))
        return hipErrorInvalidValue;
    const int chip_bytes = C * C * (kind == VT_CHIP_NORM_BF16 ? 6 : 3);
    if (kind == VT_CHIP_NORM_BF16) {
        if (any_layout >= 3) launch_chips_t<3, VT_CHIP_NORM_BF16>(a, C, chip_bytes, na, nb, search_size, tier, st);
        else if (any_layout == 2) launch_chips_t<2, VT_CHIP_NORM_BF16>(a, C, chip_bytes, na, nb, search_size, tier, st);
        else if (any_layout == 1) launch_chips_t<1, VT_CHIP_NORM_BF16>(a, C, chip_bytes, na, nb, search_size, tier, st);
        else launch_chips_t<0, VT_CHIP_NORM_BF16>(a, C, chip_bytes, na, nb, search_size, tier, st);
    } else {
        if (any_layout >= 3) launch_chips_t<3, VT_CHIP_RGB8>(a, C, chip_bytes, na, nb, search_size, tier, st);
        else if (any_layout == 2) launch_chips_t<2, VT_CHIP_RGB8>(a, C, chip_bytes, na, nb, search_size, tier, st);
        else if (any_layout == 1) launch_chips_t<1, VT_CHIP_RGB8>(a, C, chip_bytes, na, nb, search_size, tier, st);
        else launch_chips_t<0, VT_CHIP_RGB8>(a, C, chip_bytes, na, nb, search_size, tier, st);
    }
    return hipGetLastError();
}
