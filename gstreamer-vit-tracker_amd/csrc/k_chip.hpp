// k_chip.hpp — the target chips' records and launcher (k_chip.hip).
#pragma once
#include "vt_common.hpp"
#include "vt_frame.hpp"

// ---- target chips (k_chip.hip) ------------------------------------------------------------------------------------------
// per stream, device memory, written by the host only (never rewound)
struct ChipPolicy {
    float factor;               // 0: off, else 0.5..4: the crop side is factor * sqrt(w * h) of the new box
    int32_t period, phase;      // a chip is due when frames_done % period == phase
    int32_t reserved;
};
#define VT_CHIP_MAX_PERIOD 1000000
struct ChipArgs {
    const FrameDesc* frames;    // [n] by slot: the frames of this pass
    StreamState* states;        // [B] by stream, as decode / cand_commit (and the refresh launch) left them
    const vt_result* results;   // [n] by slot
    const int32_t* slot_stream; // [n] slot -> stream, null: the identity
    const int32_t* winner;      // candidate pass: [n] the winning slot of slot i's stream (only winners cut); else null
    const ChipPolicy* policy;   // [B] by stream
    uint8_t* chips;             // the store [B][chip_bytes], one buffer per stream
    vt_chip_info* infos;        // [B] by stream
    const PassOut* out;         // device copy of the pass's PassOut: host_states gets a window miss too
    StreamState* host_states;   // non-null: used instead of out->host_states (candidate passes: the commit's mirror)
    int n;
};
// behind the decode (candidate pass: behind the commit; behind the refresh launch where there is one): per slot the gate
// of DESIGN.md section 3 "Target chips", the stream's info record and, where the gate fires, the chip - a crop of this
// pass's frame at the committed box, side C, kind VT_CHIP_NORM_BF16 (na, nb: the caller's) or VT_CHIP_RGB8
hipError_t launch_target_chips(const ChipArgs& a, int C, int kind, const float* na, const float* nb, int search_size,
                               int tier, int any_layout, hipStream_t st);
