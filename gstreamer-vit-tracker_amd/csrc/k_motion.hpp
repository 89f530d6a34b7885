// k_motion.hpp — the motion prior's records, place rule and launchers (k_motion.hip).
#pragma once
#include "vt_common.hpp"
#include "vt_frame.hpp"

// ---- motion prior (k_motion.hip) ------------------------------------------------------------------------------------------
// DESIGN.md section 3 "Motion prior". Per stream, device memory, mirrored to pinned host memory beside the states; it
// rewinds and commits with the state it belongs to, but is no part of StreamState or of a snapshot.
struct MotionRec {
    float v[2];                 // velocity estimate, pixels per update of this stream
    float prior[4];             // the state box as the place launch of the stream's last pass found it
    float shift[2];             // what that launch added to the box's x, y (0 or v)
    int32_t live;               // failed updates through which the box still advances
    int32_t n_shift;            // passes with a non-zero shift
    int32_t n_coast;            // failed updates that left the box advanced
    int32_t reserved;
};
static_assert(sizeof(MotionRec) == 48, "MotionRec layout");
// ONE record per engine, device memory, written by the host only (vt_group_set_tuning "motion_*")
struct MotionPolicy {
    int32_t on;                 // "motion_prior": 0 / 1
    int32_t gain_pct;           // 1..100
    int32_t coast;              // 0..60
    int32_t max_pct;            // 0..200
};
#define VT_MOTION_DEFAULT_POLICY MotionPolicy{0, 50, 5, 100}
// The place rule on one stream, every operation a binary32 operation of its own (this header's users are built with
// -ffp-contract=off): the box the pass is cut around. Shared by the place kernel and the host's window planning
// (vt_ingest.hip), which must agree to the bit. Returns true where the box moves: out = (x + vx, y + vy, w, h).
__host__ __device__ inline bool motion_predict(int on, const float* box, const float* v, int frame_w, int frame_h, float* out) {
    out[0] = box[0]; out[1] = box[1]; out[2] = box[2]; out[3] = box[3];
    if (!on || (v[0] == 0.0f && v[1] == 0.0f)) return false;
    const float px = box[0] + v[0], py = box[1] + v[1];
    const float hw = 0.5f * box[2], hh = 0.5f * box[3];
    const float cx = px + hw, cy = py + hh;
    if (!(cx >= 0.0f && cx < (float)frame_w && cy >= 0.0f && cy < (float)frame_h)) return false;
    out[0] = px; out[1] = py;
    return true;
}
struct MotionArgs {
    StreamState* states;        // [B] by stream
    MotionRec* recs;            // [B] by stream
    const MotionPolicy* policy; // the engine's record
    const vt_result* results;   // [n] by slot (settle)
    const int32_t* slot_stream; // [n] slot -> stream, null: the identity
    const int32_t* winner;      // candidate pass: [n] the winning slot of slot i's stream (settle: only winners); else null
    const vt_candidate* cands;  // candidate pass: [n] the slots (settle: has_box of the winner); else null
    const PassOut* out;         // device copy of the pass's PassOut: host_states, host_motion (settle); may be null
    StreamState* host_states;   // non-null: used instead of out->host_states (candidate passes: the commit's mirror)
    int n;
};
// the first launch of a pass: per listed, initialised stream (once, however many slots name it) prior = box, and the box
// moves by v where the rule allows it. One lane per slot, n <= VT_MAX_STREAMS.
hipError_t launch_motion_place(const MotionArgs& a, hipStream_t st);
// behind the decode (candidate pass: behind the commit), ahead of the refresh, chip, peaks and overlay launches: the
// velocity update / coast / restore per stream of the pass, the final box and the record to device and pinned mirrors
hipError_t launch_motion_settle(const MotionArgs& a, hipStream_t st);
