// k_result_overlay.hip — the result overlay: each slot's new box drawn into its frame as the LAST launch of the pass
// (DESIGN.md section 3 "Result overlay"). The reference draws right behind its update (src/pipeline.rs:145-172,
// src/pipeline_ir.rs:182-202): a rectangle at the box, a crosshair at its centre, the text "score: N%". Here the box is
// in device memory when the decode has finished, so the join needs no host: the slot's command list
//     flag 1  VT_DRAW_RECT      {b.x, b.y, b.width, b.height, p = thickness}
//     flag 2  VT_DRAW_CROSSHAIR {b.x + b.width / 2, b.y + b.height / 2, p = size}
//     flag 4  VT_DRAW_TEXT      "score: N%" at max(b.x, 0), above the box where that fits, else below it
// is formed from results[slot] by one thread and applied with the coverage predicates k_overlay.hip uses
// (k_overlay_dev.hpp): the frame's bytes are those vt_overlay_nv12_device / vt_overlay_rgb8_device would leave.
//
// Sparse enumeration. One grid for all slots, (VT_RESULT_OVERLAY_TILES, n). A slot's workgroups walk CANDIDATE pixels
// only: up to seven rectangles - the rectangle's four strips, the crosshair's two lines, the label's cell box - taken
// from the closed-form bounds of the predicates themselves (not from the box: the luma rectangle's x range includes
// x + w and wraps when negative), clipped to the stored window. Every candidate lane evaluates the slot's whole ordered
// list and stores the value of the last covering command, so a pixel that two strips share is stored twice with the
// same bytes, and a candidate no command covers (most of the label's cell box) is not stored at all.
//
// Slots on one frame. Slots whose descriptors are equal draw as if their lists were concatenated in slot order: where a
// HIGHER slot of the same frame draws and covers the pixel, this slot leaves it alone - that slot's workgroups store
// it. The descriptor comparison runs once per workgroup (one slot per thread, wave-uniform afterwards); the higher
// slots' lists are formed in LDS, RO_CHUNK slots at a time, only where there are any.
//
// Everything the gate reads - descriptors, results, the slot -> stream and winner tables, the policy, the pass's
// device-frames word - is device memory: a replayed graph needs nothing patched. Stores are plain byte stores from
// vector registers; the counters are bumped with ordinary atomics by one thread per slot. Nothing is read back.
//
// Compiled with k_head.hip's flags (one IEEE operation per source operation: the gate's divide, the label's multiply).
#include "k_result_overlay.hpp"
#include "k_overlay_dev.hpp"

static_assert(sizeof(OverlayPolicy) == 32 && sizeof(OverlayStats) == 32, "overlay record layout");
static_assert(sizeof(vt_draw_cmd) == 64, "vt_draw_cmd layout");

#define RO_REGIONS 7
#define RO_CHUNK 16
#define RO_CMDS 3
struct RoRegion { int x, y, nx, ny; };      // candidate pixels x .. x + nx - 1, y .. y + ny - 1 (frame coordinates)

// what the frame's format lets the overlay write: 0 nothing (P010), 1 a luma byte, 2 three colour bytes
__device__ __forceinline__ int ro_surface(const FrameDesc& f) {
    if (f.fmt == PIXF_RGB) return ((uint32_t)f.lay >> 24) == 1 ? 1 : 2;     // GRAY8 is a luma surface
    if (f.fmt == PIXF_422) return 1;
    if (f.fmt == PIXF_420SP) return (f.lay & PIXL_S16) ? 0 : 1;
    return 0;
}
__device__ __forceinline__ bool ro_same_frame(const FrameDesc& a, const FrameDesc& b) {
    return a.p0 == b.p0 && a.p1 == b.p1 && a.w == b.w && a.h == b.h && a.s0 == b.s0 && a.s1 == b.s1 && a.fmt == b.fmt &&
           a.x0 == b.x0 && a.y0 == b.y0 && a.ww == b.ww && a.wh == b.wh && a.lay == b.lay;
}
__device__ __forceinline__ bool ro_gate(const vt_result& r, float thr) { return r.success != 0 && r.score > thr; }   // a NaN fails
__device__ __forceinline__ int ro_label_n(float score) {
    const float v = rintf(score * 100.0f);      // one binary32 multiply, ties to even
    return v >= 100.0f ? 100 : v > 0.0f ? (int)v : 0;       // clamped to 0..100; a NaN gives 0 (it never passes the gate)
}

// the slot's ordered list, always RO_CMDS entries: a flag that is not set leaves a command of type -1, which covers nothing
__device__ void ro_build_cmds(const vt_result& r, const OverlayPolicy& p, bool rgb, vt_draw_cmd* c) {
    const vt_bbox b = r.bbox;
    for (int k = 0; k < RO_CMDS; ++k) {
        c[k].type = -1; c[k].x = c[k].y = c[k].w = c[k].h = c[k].p = c[k].value = 0;
        for (int i = 0; i < (int)sizeof(c[k].text); ++i) c[k].text[i] = 0;
    }
    const int shape_value = rgb ? p.rgb : p.luma;
    if (p.flags & 1) {
        c[0].type = VT_DRAW_RECT; c[0].x = b.x; c[0].y = b.y; c[0].w = b.width; c[0].h = b.height;
        c[0].p = p.thickness; c[0].value = shape_value;
    }
    if (p.flags & 2) {
        c[1].type = VT_DRAW_CROSSHAIR; c[1].x = b.x + b.width / 2; c[1].y = b.y + b.height / 2;
        c[1].p = p.size; c[1].value = shape_value;
    }
    if (p.flags & 4) {
        const int above = b.y - 7 * p.scale - 4;
        c[2].type = VT_DRAW_TEXT; c[2].x = b.x > 0 ? b.x : 0; c[2].y = above >= 0 ? above : b.y + b.height + 4;
        c[2].p = p.scale; c[2].value = p.luma;
        char* t = c[2].text;
        t[0] = 's'; t[1] = 'c'; t[2] = 'o'; t[3] = 'r'; t[4] = 'e'; t[5] = ':'; t[6] = ' ';
        const int n = ro_label_n(r.score);
        int k = 7;
        if (n >= 100) t[k++] = '1';
        if (n >= 10) t[k++] = (char)('0' + n / 10 % 10);
        t[k++] = (char)('0' + n % 10);
        t[k] = '%';
    }
}

// [xa, xb] x [ya, yb] clipped to [cx0, cx1] x [cy0, cy1]; kept if anything is left
__device__ __forceinline__ void ro_add(RoRegion* reg, int& n, long long xa, long long xb, long long ya, long long yb,
                                       long long cx0, long long cx1, long long cy0, long long cy1) {
    xa = xa > cx0 ? xa : cx0; xb = xb < cx1 ? xb : cx1;
    ya = ya > cy0 ? ya : cy0; yb = yb < cy1 ? yb : cy1;
    if (xa > xb || ya > yb) return;
    reg[n++] = RoRegion{(int)xa, (int)ya, (int)(xb - xa + 1), (int)(yb - ya + 1)};
}
__device__ __forceinline__ long long ro_max0(long long v) { return v > 0 ? v : 0; }
__device__ __forceinline__ long long ro_min(long long a, long long b) { return a < b ? a : b; }

// candidate rectangles of the list c: supersets of what covers / covers_rgb accept, from their closed forms
__device__ int ro_regions(const vt_draw_cmd* c, bool rgb, const FrameDesc& f, RoRegion* reg) {
    const long long W = f.w, H = f.h;
    // the stored window inside the frame: nothing outside it is ever a candidate
    const long long cx0 = f.x0, cy0 = f.y0, cx1 = ro_min((long long)f.x0 + f.ww, W) - 1, cy1 = ro_min((long long)f.y0 + f.wh, H) - 1;
    int n = 0;
    if (c[0].type == VT_DRAW_RECT) {
        const vt_draw_cmd& r = c[0];
        const long long th = r.p;
        if (!rgb) {     // covers(): x1 .. x2 includes x + w; a negative x + w is a huge usize: the last column
            const long long sx = (long long)(r.x + r.w), sy = (long long)(r.y + r.h);
            const long long x1 = ro_max0(r.x), y1 = ro_max0(r.y);
            const long long x2 = sx < 0 ? W - 1 : ro_min(sx, W - 1), y2 = sy < 0 ? H - 1 : ro_min(sy, H - 1);
            ro_add(reg, n, x1, x2, y1, y1 + th - 1, cx0, cx1, cy0, cy1);
            ro_add(reg, n, x1, x2, ro_max0(y2 - th + 1), y2, cx0, cx1, cy0, cy1);
            ro_add(reg, n, x1, x1 + th - 1, y1, y2, cx0, cx1, cy0, cy1);
            ro_add(reg, n, ro_max0(x2 - th + 1), x2, y1, y2, cx0, cx1, cy0, cy1);
        } else {        // covers_rgb(): a strip of th rows at y and at y + h - th for rx in [0, w) - whatever h is -, and of th
                        // columns at x and at x + w - th for ry in [0, h): an empty range adds nothing
            const long long xa = r.x, xb = (long long)r.x + r.w - 1, ya = r.y, yb = (long long)r.y + r.h - 1;
            ro_add(reg, n, xa, xb, ya, ya + th - 1, cx0, cx1, cy0, cy1);
            ro_add(reg, n, xa, xb, yb - th + 1, yb, cx0, cx1, cy0, cy1);
            ro_add(reg, n, xa, xa + th - 1, ya, yb, cx0, cx1, cy0, cy1);
            ro_add(reg, n, xb - th + 1, xb, ya, yb, cx0, cx1, cy0, cy1);
        }
    }
    if (c[1].type == VT_DRAW_CROSSHAIR) {
        const vt_draw_cmd& r = c[1];
        const long long s = r.p;
        if (!rgb) {
            const long long cx = ro_max0(r.x), cy = ro_max0(r.y);
            ro_add(reg, n, ro_max0(cx - s), ro_min(cx + s, W - 1), cy, cy, cx0, cx1, cy0, cy1);
            ro_add(reg, n, cx, cx, ro_max0(cy - s), ro_min(cy + s, H - 1), cx0, cx1, cy0, cy1);
        } else {
            ro_add(reg, n, (long long)r.x - s, (long long)r.x + s, r.y, r.y, cx0, cx1, cy0, cy1);
            ro_add(reg, n, r.x, r.x, (long long)r.y - s, (long long)r.y + s, cx0, cx1, cy0, cy1);
        }
    }
    if (c[2].type == VT_DRAW_TEXT && c[2].p > 0) {
        const vt_draw_cmd& r = c[2];
        long long len = 0;
        while (len < (long long)sizeof(r.text) && r.text[len]) ++len;
        // the luma form takes x and y as usize: a negative one lies beyond every pixel
        if (rgb || (r.x >= 0 && r.y >= 0))
            ro_add(reg, n, r.x, (long long)r.x + 6LL * r.p * len - 1, r.y, (long long)r.y + 7LL * r.p - 1, cx0, cx1, cy0, cy1);
    }
    return n;
}

__global__ __launch_bounds__(256) void result_overlay_kernel(ResultOverlayArgs a) {
    __shared__ vt_draw_cmd s_own[RO_CMDS];
    __shared__ vt_draw_cmd s_oth[RO_CHUNK * RO_CMDS];
    __shared__ RoRegion s_reg[RO_REGIONS];
    __shared__ int s_nreg, s_total, s_nshare;
    __shared__ uint16_t s_list[VT_RESULT_OVERLAY_MAX_SLOTS];
    const int b = blockIdx.y, tid = threadIdx.x;
    // the gate: wave-uniform loads (everything is indexed by the block)
    const OverlayPolicy pol = *a.policy;
    const int devf = *a.device_frames;
    const int sb = a.slot_stream ? a.slot_stream[b] : b;
    const bool won = !a.winner || a.winner[b] == b;
    const vt_result r = a.results[b];
    const FrameDesc f = a.frames[b];
    const float thr = (float)pol.min_score_pct / 100.0f;
    const int surf = ro_surface(f);
    const bool considered = pol.flags != 0 && devf != 0 && won;     // rules 1 - 3
    const bool gate = ro_gate(r, thr);                              // rule 4
    const bool draws = considered && gate && surf != 0;             // rule 5
    if (blockIdx.x == 0 && tid == 0 && won) {       // the stream's record: one thread of the slot that works for it
        OverlayStats* s = a.stats + sb;
        s->drawn_last = draws ? 1 : 0;
        if (draws) {
            atomicAdd(&s->n_drawn, 1);
            if (pol.flags & 4) s->last_n = ro_label_n(r.score);
        } else if (considered && !gate) {
            atomicAdd(&s->n_gated, 1);
        } else if (considered) {
            atomicAdd(&s->n_unsupported, 1);
        }
    }
    if (!draws) return;
    const bool rgb = surf == 2;
    const int W = f.w, H = f.h;
    if (tid == 0) s_nshare = 0;
    __syncthreads();
    // higher slots on the same frame that draw: their pixels are theirs
    for (int j = b + 1 + tid; j < a.n; j += 256) {
        if (a.frames[j].p0 != f.p0) continue;
        const FrameDesc g = a.frames[j];
        if (!ro_same_frame(g, f)) continue;
        if (a.winner && a.winner[j] != j) continue;
        const vt_result rj = a.results[j];
        if (!ro_gate(rj, thr)) continue;
        s_list[atomicAdd(&s_nshare, 1)] = (uint16_t)j;
    }
    if (tid == 0) {
        ro_build_cmds(r, pol, rgb, s_own);
        const int nr = ro_regions(s_own, rgb, f, s_reg);
        int total = 0;
        for (int k = 0; k < nr; ++k) total += s_reg[k].nx * s_reg[k].ny;
        s_nreg = nr; s_total = total;
    }
    __syncthreads();
    const int nreg = s_nreg, total = s_total, nshare = s_nshare;
    const int cr = (pol.rgb >> 16) & 255, cg = (pol.rgb >> 8) & 255, cb = pol.rgb & 255;
    for (int base = blockIdx.x * 256; base < total; base += gridDim.x * 256) {      // uniform: the barriers below are safe
        int i = base + tid;
        bool hit = false, text = false;
        int px = 0, py = 0;
        if (i < total) {
            int k = 0;
            while (k + 1 < nreg && i >= s_reg[k].nx * s_reg[k].ny) { i -= s_reg[k].nx * s_reg[k].ny; ++k; }
            const RoRegion g = s_reg[k];
            px = g.x + i % g.nx; py = g.y + i / g.nx;
            for (int c = 0; c < RO_CMDS; ++c) {     // in order: the last covering command's value stands
                const bool cov = rgb ? covers_rgb(s_own[c], px, py, W, H) : covers(s_own[c], (u64)px, (u64)py, (u64)W, (u64)H);
                if (cov) { hit = true; text = c == 2; }
            }
        }
        for (int c0 = 0; c0 < nshare; c0 += RO_CHUNK) {
            const int cn = min(RO_CHUNK, nshare - c0);
            __syncthreads();        // the previous chunk's readers are done
            if (tid < cn) ro_build_cmds(a.results[s_list[c0 + tid]], pol, rgb, s_oth + RO_CMDS * tid);
            __syncthreads();
            for (int c = 0; hit && c < cn * RO_CMDS; ++c)
                if (rgb ? covers_rgb(s_oth[c], px, py, W, H) : covers(s_oth[c], (u64)px, (u64)py, (u64)W, (u64)H)) hit = false;
        }
        const int qx = px - f.x0, qy = py - f.y0;
        if (!hit || qx < 0 || qy < 0 || qx >= f.ww || qy >= f.wh) continue;    // no store ever leaves the stored window
        uint8_t* row = const_cast<uint8_t*>(f.p0) + (size_t)qy * (size_t)f.s0;
        if (rgb) {
            uint8_t* p = row + (size_t)qx * ((uint32_t)f.lay >> 24);
            p[f.lay & 255] = (uint8_t)(text ? pol.luma : cr);       // the pad byte of a 4-byte pixel is never written
            p[(f.lay >> 8) & 255] = (uint8_t)(text ? pol.luma : cg);
            p[(f.lay >> 16) & 255] = (uint8_t)(text ? pol.luma : cb);
        } else if (f.fmt == PIXF_422) {     // the pixel's Y byte inside its pair: chroma is never touched
            row[(size_t)(qx >> 1) * 4 + ((qx & 1) ? (f.lay >> 16) & 255 : f.lay & 255)] = (uint8_t)pol.luma;
        } else {
            row[qx] = (uint8_t)pol.luma;
        }
    }
}

hipError_t launch_result_overlay(const ResultOverlayArgs& a, hipStream_t st) {
    if (a.n < 1 || a.n > VT_RESULT_OVERLAY_MAX_SLOTS || !a.frames || !a.results || !a.policy || !a.stats || !a.device_frames)
        return hipErrorInvalidValue;
    vt_launch(result_overlay_kernel, dim3(VT_RESULT_OVERLAY_TILES, a.n), dim3(256), 0, st, a);
    return hipGetLastError();
}
