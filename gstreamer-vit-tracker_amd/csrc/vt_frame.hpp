// vt_frame.hpp — pixel-format tables, frame descriptor, stream state, model dimensions and the pass's host sinks.
#pragma once
#include <stdint.h>

#include "../../include/vittrack_hip.h"

// Pixel layout families: every value of vt_frame.format (vt_pixfmt, vt_pixfmt2) is one family plus a layout word
// (FrameDesc.lay). The family codes are the vt_pixfmt values of the formats that defined them, so those formats'
// descriptors are unchanged.
enum PixFamily {
    // packed R,G,B(,x) / x,R,G,B / one grey byte: lay = R | G << 8 | B << 16 (byte offsets inside the pixel, 0..3) |
    // bytes per pixel << 24 (GRAY8: 1, every offset 0)
    PIXF_RGB = VT_PIX_RGB8,
    // a luma plane + chroma at half the horizontal rate. lay = U offset | V offset << 8 (0 or 1: the position in an
    // interleaved pair, or - PIXL_PLANAR - which of the two chroma planes) | the PIXL_* bits below. NV12, NV21, I420,
    // YV12, P010 and NV16 (whose sibling is YUY2: the same luma, the same chroma pair per pixel pair, one row per row)
    PIXF_420SP = VT_PIX_NV12,
    PIXF_422 = VT_PIX_YUY2        // packed pixel pairs: lay = Y0 | U << 8 | Y1 << 16 | V << 24 (byte offsets)
};
// PIXF_420SP layout bits (zero for NV12 / NV21)
#define PIXL_PLANAR (1 << 16)     // U and V in planes of their own: p1 is the first, the second lies s1 * ceil(R / 2) bytes
                                  // behind it, R = the stored rows: wh, or - PIXL_FULLH - h
#define PIXL_S16 (1 << 20)        // 16-bit little-endian samples (strides in bytes), of which ...
#define PIXL_HIBYTE (1 << 22)     // ... byte 1 is read
#define PIXL_ROWS422 (1 << 24)    // one chroma row per luma row (no row shift)
#define PIXL_FULLH (1 << 25)      // set by to_desc: the planes belong to a whole frame (vt_frame.windowed != 1)

// vt_frame.format = pixel format | matrix << 8 | range << 12 (vittrack_hip.h: VT_FRAME_FORMAT). The word is split and checked
// HERE and nowhere else: pix_family refuses (-1) what the boundary refuses, every other helper works on the base format,
// so that the frame checks, the window packing and the drawable rule need no case for colour.
inline int pix_base(int fmt) { return fmt & 0xff; }
// colour code of a word = matrix * 2 + range: the row of the coefficient table (k_preproc_dev.hpp: yuv_to_rgb_code), 0 =
// BT.601 limited, the conversion every format had before the bits existed. Meaningful for a word pix_family accepts.
inline int pix_color_code(int fmt) { return ((fmt >> 8) & 15) * 2 + ((fmt >> 12) & 15); }
// where the code travels to the kernels: bits 28..30 of FrameDesc.lay (to_desc), free in the PIXF_420SP and PIXF_422 layout
// words - every read of those words by a kernel of levels 0..2 is masked below bit 26 - and never set for PIXF_RGB
#define PIXL_CODE_SHIFT 28
#define PIXL_CODE_MASK 7

inline int pix_family_base(int fmt) {
    switch (fmt) {
    case VT_PIX_RGB8: case VT_PIX_BGR8: case VT_PIX_RGBX: case VT_PIX_BGRX:
    case VT_PIX2_GRAY8: case VT_PIX2_XRGB: case VT_PIX2_XBGR: return PIXF_RGB;
    case VT_PIX_NV12: case VT_PIX_NV21:
    case VT_PIX2_I420: case VT_PIX2_YV12: case VT_PIX2_P010: case VT_PIX2_NV16: return PIXF_420SP;
    case VT_PIX_YUY2: case VT_PIX_UYVY: return PIXF_422;
    default: return -1;
    }
}
// family of a format word (-1: refused) and its layout word. Refused: an unknown base format, a bit above 15, a matrix
// above VT_COLOR_BT2020, a range above VT_RANGE_FULL, colour bits on a format without chroma (PIXF_RGB)
inline int pix_family(int fmt) {
    if (fmt < 0 || fmt > 0xffff) return -1;
    const int fam = pix_family_base(pix_base(fmt));
    const int matrix = (fmt >> 8) & 15, range = (fmt >> 12) & 15;
    if (fam < 0 || matrix > VT_COLOR_BT2020 || range > VT_RANGE_FULL) return -1;
    if (fam == PIXF_RGB && (matrix | range) != 0) return -1;
    return fam;
}
inline int32_t pix_layout(int fmt) {
    switch (pix_base(fmt)) {
    case VT_PIX_RGB8: return 0 | 1 << 8 | 2 << 16 | 3 << 24;
    case VT_PIX_BGR8: return 2 | 1 << 8 | 0 << 16 | 3 << 24;
    case VT_PIX_RGBX: return 0 | 1 << 8 | 2 << 16 | 4 << 24;
    case VT_PIX_BGRX: return 2 | 1 << 8 | 0 << 16 | 4 << 24;
    case VT_PIX_NV12: return 0 | 1 << 8;
    case VT_PIX_NV21: return 1 | 0 << 8;
    case VT_PIX_YUY2: return 0 | 1 << 8 | 2 << 16 | 3 << 24;
    case VT_PIX_UYVY: return 1 | 0 << 8 | 3 << 16 | 2 << 24;
    case VT_PIX2_I420: return 0 | 1 << 8 | PIXL_PLANAR;
    case VT_PIX2_YV12: return 1 | 0 << 8 | PIXL_PLANAR;
    case VT_PIX2_P010: return 0 | 1 << 8 | PIXL_S16 | PIXL_HIBYTE;
    case VT_PIX2_NV16: return 0 | 1 << 8 | PIXL_ROWS422;
    case VT_PIX2_GRAY8: return 0 | 0 << 8 | 0 << 16 | 1 << 24;
    case VT_PIX2_XRGB: return 1 | 2 << 8 | 3 << 16 | 4 << 24;
    case VT_PIX2_XBGR: return 3 | 2 << 8 | 1 << 16 | 4 << 24;
    default: return 0;
    }
}
// name of a format (of its base format) for error texts
inline const char* pix_name(int fmt) {
    static const char* const names[] = {"rgb8", "nv12", "yuy2", "bgr8", "rgbx", "bgrx", "nv21", "uyvy"};
    static const char* const names2[] = {"i420", "yv12", "p010", "nv16", "gray8", "xrgb", "xbgr"};
    fmt = fmt < 0 ? -1 : pix_base(fmt);
    return fmt >= 0 && fmt < 8 ? names[fmt] : fmt >= VT_PIX2_I420 && fmt <= VT_PIX2_XBGR ? names2[fmt - VT_PIX2_I420] : "?";
}
// why pix_family refuses a word, for error texts that name the format: null for a word it accepts or whose base format is
// unknown (the caller's "unknown pixel format" text)
inline const char* pix_refusal(int fmt) {
    if (pix_family(fmt) >= 0 || fmt < 0 || pix_family_base(pix_base(fmt)) < 0) return nullptr;
    if (fmt > 0xffff) return "format bits above 15 must be zero";
    if (((fmt >> 8) & 15) > VT_COLOR_BT2020) return "unknown colour matrix";
    if (((fmt >> 12) & 15) > VT_RANGE_FULL) return "unknown colour range";
    return "colour matrix / range bits on a format without chroma";
}
// which crop kernels (k_preproc.hip, fetch_rgb<level>) read this format: 0 those of RGB8, NV12 and YUY2, 1 those that read
// the byte offsets of f.lay (every vt_pixfmt), 2 those that read the whole layout word (every vt_pixfmt2 as well), 3 those
// that also convert with the frame's colour code (every word whose code is not 0). A kernel of a level reads every format
// of the levels below it.
#define PIX_LEVELS 4
inline int pix_level(int fmt) {
    if (pix_family(fmt) >= 0 && pix_color_code(fmt) != 0) return 3;
    return fmt >= VT_PIX2_I420 ? 2 : fmt != VT_PIX_RGB8 && fmt != VT_PIX_NV12 && fmt != VT_PIX_YUY2 ? 1 : 0;
}
// bytes per pixel of plane 0's rows (PIXF_420SP: the luma plane)
inline int pix_row_bpp(int fmt) {
    const int fam = pix_family(fmt);
    return fam == PIXF_RGB ? pix_layout(fmt) >> 24 : fam == PIXF_422 ? 2 : (pix_layout(fmt) & PIXL_S16) ? 2 : 1;
}
// PIXF_420SP: U and V lie in two planes behind each other / chroma rows of `rows` luma rows / window rules of YUY2
// (no rule on rows) instead of NV12's
inline bool pix_planar(int fmt) { return pix_family(fmt) == PIXF_420SP && (pix_layout(fmt) & PIXL_PLANAR); }
inline bool pix_rows422(int fmt) { return pix_family(fmt) == PIXF_420SP && (pix_layout(fmt) & PIXL_ROWS422); }
inline int pix_chroma_rows(int fmt, int rows) { return pix_rows422(fmt) ? rows : (rows + 1) / 2; }
// PIXF_420SP: bytes of a chroma row (of one plane) that belong to `ww` pixels
inline int pix_chroma_row_bytes(int fmt, int ww) {
    return pix_planar(fmt) ? (ww + 1) / 2 : ((ww + 1) & ~1) * pix_row_bpp(fmt);
}

// one device-resident input frame (mirrors vt_frame, 64-bit pointers)
struct FrameDesc {
    const uint8_t* p0;  // packed pixels, or the luma plane of PIXF_420SP
    const uint8_t* p1;  // PIXF_420SP: the interleaved chroma plane, or the first of the two chroma planes
    int32_t w, h, s0, s1;
    int32_t fmt;        // PixFamily
    int32_t x0, y0;     // frame coordinates of the first stored pixel (window upload)
    int32_t ww, wh;     // extent of the stored window in pixels: samples outside it read as black
    int32_t lay;        // byte layout within the family (PixFamily)
};
static_assert(sizeof(FrameDesc) == 56, "FrameDesc layout");

// per tracked stream, lives in HBM; the decode kernel of frame t writes what the preprocessing
// kernel of frame t+1 reads, so a stream of updates never needs the host in between.
struct StreamState {
    float box[4];        // last accepted box, frame pixels: x, y, w, h (top-left + size)
    float geo[4];        // search-crop geometry of the running frame: x0m, y0m, scale, side
    int32_t frame_w, frame_h;
    int32_t initialized;
    int32_t frames_done;     // updates completed since init
    int32_t success_count;   // of which result.success
    int32_t last_idx;        // argmax cell of the last update
    float last_fbox[4];      // unrounded clipped box of the last update
    float last_score;
    // index (= frames_done + 1 at the time) of the last pass in which the crop needed a pixel that
    // lies inside the frame but outside the window the caller stored: such samples read as black, so
    // a host that uploaded a SPECULATIVE window (vt_group_enqueue_host) must redo that pass
    int32_t window_miss;
    // template refresh (k_refresh.hip): refreshes since init - the stream's current template is buffer
    // tpl_gen & 1 of a two-buffer store - and frames_done at the last one. Zero after init. They rewind and commit with
    // the state they are part of.
    int32_t tpl_gen;
    int32_t tpl_frame;
};
static_assert(sizeof(StreamState) == 88, "StreamState layout");

struct ModelDims {
    int patch, T, S, D, H, L, mlp, C, kpad;
    int gt, gs, nt, ns, ntok;   // grids and token counts
    int npad;                   // ntok rounded up to 64 (attention key padding)
    float norm_a[3], norm_b[3];
    float success_threshold, ln_eps;
};

// Where a pass leaves its results for the host: pinned, device-visible host memory the decode kernel
// stores to directly (no device-to-host copy on the stream). Uploaded with the frame descriptors of
// the pass, right behind them in the same buffer.
struct MotionRec;
struct AppearRec;
struct PropRec;
struct ConflictRec;
struct HealthRec;
struct ArbRec;
struct PassOut {
    vt_result* host_results;    // [slots of the pass] or null
    StreamState* host_states;   // [B] (by stream) or null
    vt_peaks* host_peaks;       // [slots of the pass] or null: the response-peaks launch's records (k_peaks.hip)
    MotionRec* host_motion;      // [B] (by stream) or null: the motion records as the settle launch left them (k_motion.hip)
    AppearRec* host_appearance;  // [B] (by stream) or null: the appearance records of the pass's streams (k_appearance.hip)
    PropRec* host_proposals;     // [B] (by stream) or null: the proposal records of the pass's streams (k_proposals.hip)
    ConflictRec* host_conflicts; // [B] (by stream) or null: the conflict records of the pass's streams (k_conflicts.hip)
    HealthRec* host_health;      // [B] (by stream) or null: the frame-health records of the pass's streams (k_health.hip)
    ArbRec* host_arbitrate;      // [B] (by stream) or null: the arbitration records of the pass's streams (k_arbitrate.hip)
};
