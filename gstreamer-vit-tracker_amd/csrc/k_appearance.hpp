// k_appearance.hpp — the appearance check's records and launchers (k_appearance.hip).
#pragma once
#include "vt_common.hpp"
#include "vt_frame.hpp"
#include "k_refresh.hpp"

// ---- appearance check (k_appearance.hip) --------------------------------------------------------------------------------
// DESIGN.md section 3 "Appearance check": the zero-mean normalised correlation of the template-sized crop at each new box
// (the probe) with the rows the stream was started from (the anchor). Per stream, device memory, mirrored to pinned host
// memory beside the states; every pass writes the records of its streams (a redone pass writes them again); no part of
// StreamState or of a snapshot.
struct AppearRec {
    int32_t status;             // 0: not due or not evaluated; 1: evaluated; 2: refresh rule 6 failed at the box; 3: a variance is not positive
    int32_t frames_done;        // the stream's frames_done in the pass that wrote the record
    float similarity;           // [-1, 1]; 0 unless status is 1
    float box[4];               // the box the probe was (or would have been) cut at: the state's box behind the pass
    int32_t reserved;
};
static_assert(sizeof(AppearRec) == 32, "AppearRec layout");
// ONE record per engine, device memory, written by the host only (vt_group_set_tuning "appearance*")
struct AppearPolicy {
    int32_t on;                 // "appearance": 0 / 1
    int32_t period;             // 1..VT_APPEAR_MAX_PERIOD: evaluated when frames_done % period == 0
    int32_t gate_pm;            // 0..1000 per mille; 0: report only
    float tau;                  // (float)gate_pm / 1000.0f, one binary32 divide (the host's)
};
#define VT_APPEAR_MAX_PERIOD 1000000
#define VT_APPEAR_DEFAULT_POLICY AppearPolicy{0, 1, 0, 0.0f}
// per stream, beside the policy: diagnostics, never rewound - a redone pass may count twice (like skipped_geometry)
struct AppearCount {
    int32_t evaluated;          // records written with status 1 or 3
    int32_t gated;              // refreshes that rules 1-7 allowed and rule 8 refused
};
#define VT_APPEAR_CHUNK_ROWS 8  // rows of the [nt][cols] matrices per workgroup of the score launch
inline int appear_chunks(int nt) { return (nt + VT_APPEAR_CHUNK_ROWS - 1) / VT_APPEAR_CHUNK_ROWS; }
struct AppearArgs {
    const FrameDesc* frames;    // [n] by slot: the frames of this pass (probe)
    StreamState* states;        // [B] by stream, as decode / cand_commit / motion_settle left them
    const vt_result* results;   // [n] by slot
    const int32_t* slot_stream; // [n] slot -> stream, null: the identity
    const int32_t* winner;      // candidate pass: [n] the winning slot of slot i's stream (only winners evaluate); else null
    const AppearPolicy* policy; // the engine's record
    AppearCount* counts;        // [B] by stream
    AppearRec* recs;            // [B] by stream
    const RefreshPolicy* refresh;   // [B] by stream or null: refresh rules 1, 3, 4 make a slot due while tau > 0
    unsigned* tickets;          // [n] by slot, zero between launches (score)
    double* partials;           // [n][appear_chunks(nt)][5] by slot (score)
    const bf16_t* anchor;       // [B][nt][kpad] by stream
    bf16_t* probe;              // [B][nt][kpad] by stream
    const PassOut* out;         // device copy of the pass's PassOut: host_states (a window miss), host_appearance; may be null
    StreamState* host_states;   // non-null: used instead of out->host_states (candidate passes: the commit's mirror)
    double* sums;               // null, or [n][5] by slot: Sa, Sp, Saa, Spp, Sap of the slots the score launch evaluated
    int n;
};
// behind the decode (candidate pass: the commit) and motion_settle, ahead of the refresh, chip, peaks and overlay launches:
// per slot the due rule, refresh rules 6 and 7, the record (status 0 / 2, or 1 = cut: the score launch completes it) and,
// where the slot passes, the template crop of this pass's frame at the committed box into probe[stream]
hipError_t launch_appearance_probe(const AppearArgs& a, const ModelDims& d, int tier, int any_layout, hipStream_t st);
// behind the probe launch: per slot whose record says "cut", the five sums over the first `cols` columns of the nt rows of
// anchor[stream] and probe[stream] in binary64, in a FIXED order (per-lane strided partials, wave and workgroup tree,
// chunk partials added in index order by the slot's last workgroup), the similarity and the final record
hipError_t launch_appearance_score(const AppearArgs& a, int nt, int cols, int kpad, hipStream_t st);
