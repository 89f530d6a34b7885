// k_conflicts.hpp — the stream conflicts' records and launcher (k_conflicts.hip).
#pragma once
#include "vt_common.hpp"
#include "vt_frame.hpp"

// ---- stream conflicts (k_conflicts.hip) ---------------------------------------------------------------------------------
// DESIGN.md section 3 "Stream conflicts": per stream of a pass, which other streams of the same pass and the same scene
// overlap its new box, and by how much (IoU). Per stream, device memory, mirrored to pinned host memory beside the states;
// every pass writes the records of its streams whole (a redone pass writes them again); no part of StreamState or of a
// snapshot.
#define VT_CONFLICT_MAX 4       // partners a record lists
struct ConflictRec {
    int32_t status;             // 0: no pass wrote it; 1: evaluated, nobody over tau; 2: evaluated, n_over > 0; 3: not eligible
    int32_t frames_done;        // the stream's frames_done in the pass that wrote the record
    int32_t n_over;             // partners with iou >= tau (may exceed VT_CONFLICT_MAX)
    int32_t reserved;
    int32_t partner[VT_CONFLICT_MAX];   // the over-tau partners' stream indices by (iou descending, stream ascending); unused: -1
    float iou[VT_CONFLICT_MAX];         // theirs; unused: 0
};
static_assert(sizeof(ConflictRec) == 48, "ConflictRec layout");
// ONE record per engine, device memory, written by the host only (vt_group_set_tuning "conflicts*")
struct ConflictPolicy {
    int32_t on;                 // "conflicts": 0 / 1
    int32_t iou_pm;             // 1..1000 per mille
    int32_t gate;               // "conflicts_gate": 0 / 1 - refresh rule 9
    float tau;                  // (float)iou_pm / 1000.0f, one binary32 divide (the host's)
    int32_t reserved[4];
};
#define VT_CONFLICT_DEFAULT_POLICY ConflictPolicy{0, 300, 0, 0.3f, {0, 0, 0, 0}}
#define VT_CONFLICT_MAX_SCENE 65535
// per stream, beside the policy: diagnostics, never rewound - a redone pass may count twice (like skipped_geometry)
struct ConflictCount {
    int32_t evaluated;          // records written with status 1 or 2
    int32_t conflicting;        // of which status 2
    int32_t gated;              // refreshes that rules 1-5 allowed and rule 9 refused
    int32_t reserved;
};
struct ConflictArgs {
    const StreamState* states;  // [B] by stream, as decode / cand_commit / motion_settle left them
    const vt_result* results;   // [n] by slot
    const int32_t* slot_stream; // [n] slot -> stream, null: the identity
    const int32_t* winner;      // candidate pass: [n] the winning slot of slot i's stream (only winners work); else null
    const ConflictPolicy* policy;   // the engine's record
    const int32_t* scenes;      // [B] by stream; 0: compared with nobody
    ConflictRec* recs;          // [B] by stream
    ConflictCount* counts;      // [B] by stream
    const PassOut* out;         // device copy of the pass's PassOut: host_conflicts; may be null
    int n;
};
// behind the decode (candidate pass: the commit) and motion_settle, ahead of the appearance, proposals, refresh, chip, peaks
// and overlay launches: one workgroup, one lane per slot (n <= VT_MAX_STREAMS), the records and counters of the pass's streams
hipError_t launch_conflicts_check(const ConflictArgs& a, hipStream_t st);
