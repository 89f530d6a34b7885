// k_proposals.hpp — the reacquire proposals' records and launchers (k_proposals.hip).
#pragma once
#include "vt_common.hpp"
#include "vt_frame.hpp"

// ---- reacquire proposals (k_proposals.hip) ------------------------------------------------------------------------------
// DESIGN.md section 3 "Reacquire proposals": the stream's own template, pooled to an M x M pattern of int16 cells, slid
// over an int16 thumbnail of the whole frame of the pass; the best places, with boxes, in a record per stream. The rule is
// stated to the bit in include/vittrack_hip.h ("proposals*" keys). Integer sums: no order of additions matters, nothing
// here is a floating-point atomic. Per stream a record, mirrored to pinned host memory like the appearance records;
// per slot the working set (header, pattern, thumbnail, map). No part of StreamState or of a snapshot; nothing of the
// pass's results, states, templates or frames is written.
#define VT_PROP_MAX 8               // proposals a record lists at most
#define VT_PROP_M_MAX 16            // the pattern side: 16, or 14 for templates that 16 does not divide
#define VT_PROP_OUTSIDE (-32768)     // a thumbnail cell with a sub-tap outside the frame: no value clamps to it; never matched
#define VT_PROP_MIN_CELLS 16384
#define VT_PROP_MAX_CELLS 4194304
#define VT_PROP_MAX_PERIOD 1000000
struct PropEntry {
    float sim;                  // [-1, 1]
    float box[4];               // x, y, w, h: the state's size centred on the match window's centre
    int32_t pos;                // py * (Wg - M + 1) + px
};
struct PropRec {
    int32_t status;             // 0: not due; 1: evaluated; 2: geometry (grid too large or smaller than the pattern);
                                // 3: flat pattern; 4: no whole device frame (host-pointer pass or a windowed frame)
    int32_t frames_done;        // the stream's frames_done in the pass that wrote the record
    int32_t n;                  // proposals listed
    float c;                    // the cell side in source pixels (0 unless status is 1, 2 or 3)
    int32_t Wg, Hg;             // the thumbnail's grid
    int32_t reserved[2];
    PropEntry p[VT_PROP_MAX];
};
static_assert(sizeof(PropEntry) == 24 && sizeof(PropRec) == 224, "PropRec layout");
// ONE record per engine, device memory, written by the host only (vt_group_set_tuning "proposals*")
struct PropPolicy {
    int32_t mode;               // "proposals": 0 off, 1 slots whose update failed, 2 every update
    int32_t period;             // 1..VT_PROP_MAX_PERIOD: due when frames_done % period == 0
    int32_t max_n;              // 1..VT_PROP_MAX
    int32_t min_sim_pm;         // 0..1000 per mille
    float tau;                  // (float)min_sim_pm / 1000.0f, one binary32 divide (the host's)
    int32_t max_cells;          // thumbnail cells per slot: fixed by the first enable
    int32_t reserved[2];
};
#define VT_PROP_DEFAULT_POLICY PropPolicy{0, 1, 4, 500, 0.5f, 262144, {0, 0}}
// per slot, written by the prepare launch and obeyed by the three behind it
struct PropHead {
    int32_t status;             // the record's status so far: 1 = the thumbnail, map and listing run
    int32_t frames_done;
    int32_t M, Wg, Hg;
    float c, X0;                // cell side, grid origin (X0 == Y0)
    float box[4];               // the state's box as the pass left it
    int32_t reserved;
    long long Sa, Saa;          // the whole pattern's sums (status 3; a position uses those of its cells inside the frame)
};
static_assert(sizeof(PropHead) == 64, "PropHead layout");
__host__ __device__ inline int prop_pattern_side(int T) { return T % 16 == 0 ? 16 : T % 14 == 0 ? 14 : 0; }
struct PropArgs {
    const FrameDesc* frames;    // [n] by slot: the frames of this pass
    const StreamState* states;  // [B] by stream, as decode / cand_commit / motion_settle left them
    const vt_result* results;   // [n] by slot
    const int32_t* slot_stream; // [n] slot -> stream, null: the identity
    const int32_t* winner;      // candidate pass: [n] the winning slot of slot i's stream (only winners evaluate); else null
    const PropPolicy* policy;   // the engine's record
    const int32_t* devflag;     // 1: the pass came through a device entry point
    const bf16_t* tpl;          // [B][tpl_bufs][nt][kpad] by stream: the template store
    int tpl_bufs;               // 2: a stream's rows are buffer tpl_gen & 1
    PropRec* recs;              // [B] by stream
    int32_t* evaluated;         // [B] by stream: records written with status 1 or 3 (diagnostic, never rewound)
    PropHead* heads;            // [n] by slot
    int16_t* pattern;           // [n][VT_PROP_M_MAX^2] by slot: M x M, row-major
    int16_t* thumb;             // [n][max_cells] by slot: Hg x Wg, row-major
    float* map;                 // [n][max_cells] by slot: (Hg - M + 1) x (Wg - M + 1), row-major
    const PassOut* out;         // device copy of the pass's PassOut: host_proposals; may be null
    int max_cells;              // the stride of thumb and map; fixes the launch dimensions
    int n;
};
// the four launches, in this order, behind decode / commit / motion_settle / appearance and ahead of refresh, chips,
// peaks and overlay (the frame is undrawn): the due rule, geometry and pattern; the thumbnail; the similarity map; the
// listing and the record. Fixed launch dimensions (max_cells): workgroups of slots that are not due leave at once.
hipError_t launch_proposals_prepare(const PropArgs& a, const ModelDims& d, hipStream_t st);
hipError_t launch_proposals_thumb(const PropArgs& a, const ModelDims& d, int any_layout, hipStream_t st);
hipError_t launch_proposals_match(const PropArgs& a, hipStream_t st);
hipError_t launch_proposals_list(const PropArgs& a, hipStream_t st);
