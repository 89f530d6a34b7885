// k_result_overlay.hpp — the result overlay's records and launcher (k_result_overlay.hip; DESIGN.md section 3 "Result overlay").
#pragma once
#include "vt_common.hpp"
#include "vt_frame.hpp"

// ONE per engine, device memory, written by the host only (never rewound, not part of a snapshot)
struct OverlayPolicy {
    int32_t flags;              // 1 rectangle | 2 crosshair | 4 score label; 0: off
    int32_t thickness;          // 1..16: the rectangle's
    int32_t size;               // 1..64: the crosshair's half length
    int32_t scale;              // 1..4: the label's glyph scale
    int32_t luma;               // 0..255: every value on a luma surface, the label on every surface
    int32_t rgb;                // 0xRRGGBB: rectangle and crosshair on a packed-RGB surface
    int32_t min_score_pct;      // 0..100: a slot draws iff success and score > (float)pct / 100.0f
    int32_t reserved;
};
#define VT_OVERLAY_DEFAULT_POLICY OverlayPolicy{0, 3, 15, 2, 255, 0x00FF00, 25, 0}
// per stream, device memory: written by the overlay launch (the slot that works for the stream; a candidate pass: its winner)
struct OverlayStats {
    int32_t drawn_last;         // the stream's last pass drew it (0 / 1)
    int32_t n_drawn, n_gated, n_unsupported;    // passes that drew / failed the score gate / met a format that is not drawable
    int32_t last_n;             // N of the last label drawn
    int32_t reserved[3];
};
struct ResultOverlayArgs {
    const FrameDesc* frames;        // [n] by slot: the frames of this pass - WRITTEN, whatever the pointers' type says
    const vt_result* results;       // [n] by slot, as the decode left them
    const int32_t* slot_stream;     // [n] slot -> stream, null: the identity
    const int32_t* winner;          // candidate pass: [n] the winning slot of slot i's stream (only winners draw); else null
    const OverlayPolicy* policy;    // one record
    OverlayStats* stats;            // by stream
    const int32_t* device_frames;   // one word: non-zero when the pass received its frames through a device entry point
    int n;
};
#define VT_RESULT_OVERLAY_TILES 8       // workgroups per slot
#define VT_RESULT_OVERLAY_MAX_SLOTS 1024
// The LAST launch of a pass: per slot the gate of DESIGN.md section 3 "Result overlay" and, where it passes, the slot's
// rectangle / crosshair / score label into its frame. grid = (VT_RESULT_OVERLAY_TILES, n); hipErrorInvalidValue on null
// operands or n outside 1..VT_RESULT_OVERLAY_MAX_SLOTS.
hipError_t launch_result_overlay(const ResultOverlayArgs& a, hipStream_t st);
