// k_cand.hpp — launchers of the candidate-pass kernels (k_cand.hip), shared with the engine.
#pragma once
#include "vt_common.hpp"
#include "vt_frame.hpp"

// A candidate pass: slot i works for stream cands[i].stream, on a candidate state of its own. Crop and decode run on
// cand_states with the identity slot map; the template gather keeps the slot -> stream map.
struct CandArgs {
    const vt_candidate* cands;  // [n] device: the pass's slots
    StreamState* states;        // [B] by stream
    StreamState* cand_states;   // [n] by slot
    const vt_result* results;   // [n] by slot (device), written by the decode
    int32_t* winner;            // [n] device: the winning slot of slot i's stream
    StreamState* host_states;   // pinned, [B] by stream (only the listed streams' entries are written), or null
    int32_t* host_winner;       // pinned, [n], or null
    int n;
};
hipError_t launch_cand_fill(const CandArgs& a, hipStream_t st);      // cand_states[i] <- states[stream] (+ the slot's box)
hipError_t launch_cand_commit(const CandArgs& a, hipStream_t st);    // winners, the listed streams' states, the host's copies
