// k_peaks.hpp — the response peaks' records and launcher (k_peaks.hip).
#pragma once
#include "vt_common.hpp"
#include "vt_frame.hpp"

// ---- response peaks (k_peaks.hip) ---------------------------------------------------------------------------------------
// per stream, device memory, written by the host only (never rewound, not part of a snapshot)
struct PeaksPolicy {
    int32_t max_peaks;          // 0: off, else 1..VT_PEAKS_MAX
    int32_t radius;             // 1..4: half side of the suppression square
    float min_resp;             // a peak behind the first needs resp > 0 and resp >= min_resp
    int32_t reserved;
};
struct PeaksArgs {
    const float* head_out;      // [n * ns][8] by slot: the logits the decode of this pass read
    const float* hann;          // [ns]
    const StreamState* states;  // [B] by stream, as decode / cand_commit (and the refresh and chip launches) left them
    const int32_t* slot_stream; // [n] slot -> stream, null: the identity
    const int32_t* winner;      // candidate pass: [n] the winning slot of slot i's stream (only winners list); else null
    const PeaksPolicy* policy;  // [B] by stream
    vt_peaks* records;          // [n] by slot (device)
    const PassOut* out;         // device copy of the pass's PassOut: host_peaks [n] by slot, or null
    int n, ns, grid;
};
// behind the decode (candidate pass: behind the commit; behind the refresh and chip launches where there are any): per
// slot up to VT_PEAKS_MAX maxima of the response map with their decoded boxes - DESIGN.md section 3 "Response peaks".
// One workgroup per slot; writes the slot's record (device + pinned host) and nothing else.
hipError_t launch_response_peaks(const PeaksArgs& a, hipStream_t st);
