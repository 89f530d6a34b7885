// k_arbitrate.hpp — the peak arbitration's records and launchers (k_arbitrate.hip).
#pragma once
#include "vt_common.hpp"
#include "vt_frame.hpp"
#include "k_appearance.hpp"     // appear_chunks: the size of ArbArgs.partials

// ---- peak arbitration (k_arbitrate.hip) ---------------------------------------------------------------------------------
// DESIGN.md section 3 "Peak arbitration": where the committed box (peak 0 of the response map) no longer looks like the
// anchor and a runner-up does, the runner-up is committed instead - result, state and mirrors rewritten as the decode would
// have written them had that peak been the argmax. The rule is stated to the bit in include/vittrack_hip_ops.h
// (vt_op_arbitrate) and in include/vittrack_hip.h ("arbitrate*" keys). Four launches: list, probe, score, commit.
// A record is FINAL whenever a launch sequence has ended. Inside one, between the list and the commit launch, record status 1
// also stands for "due" and peak status 1 for "to cut": the list launch rewrites the record of every stream the pass lists
// before the probe and score launches read it, those two look at the slots of the pass only, and the pinned mirror is written
// for final records only - so no reader outside the four launches ever sees the transient meaning.
#define VT_ARB_MAX 4            // peaks examined at most, peak 0 included
struct ArbPeak {
    int32_t cell;               // y * score_grid + x
    int32_t status;             // 0: not cut (a score below the model's success threshold, or a slot that is not due); 1: cut and
                                // scored; 2: refresh rule 6 failed at the integer box; 3: cut, a variance is not positive (similarity 0)
    float score, resp;          // as vt_peak
    float similarity;           // [-1, 1]; 0 unless status is 1
    int32_t reserved;
    float box[4];               // the float clamped box (vt_peak's); the probe is cut at floorf(v + 0.5f) of each
};
struct ArbRec {
    int32_t status;             // 0: not due; 1: kept; 2: switched; 3: candidate pass; 4: refresh rule 6 failed at peak 0;
                                // 5: refresh rule 7 failed (window miss marked)
    int32_t frames_done;        // the stream's frames_done in the pass that wrote the record
    int32_t n;                  // peaks listed (0 where the list launch left before the iteration)
    int32_t chosen;             // status 2: the committed peak, 1..n-1; else 0
    ArbPeak peak[VT_ARB_MAX];   // peak[0..n) in listing order, zeros behind
};
static_assert(sizeof(ArbPeak) == 40 && sizeof(ArbRec) == 176, "ArbRec layout");
// ONE record per caller, device memory, written by the host only. Thresholds are formed in the kernels as
// (float)pm / 1000.0f: one binary32 divide each, no derived words
struct ArbPolicy {
    int32_t on;                 // "arbitrate": 0 / 1
    int32_t max_peaks;          // 2..VT_ARB_MAX
    int32_t radius;             // 1..4
    int32_t min_resp_pm;        // 0..1000: a runner-up needs resp > 0 and resp >= pm / 1000
    int32_t low_pm;             // 0..1000: peak 0 is challenged only while its similarity is below pm / 1000
    int32_t high_pm;            // 0..1000: a runner-up must reach pm / 1000
    int32_t reserved[2];
};
static_assert(sizeof(ArbPolicy) == 32, "ArbPolicy layout");
#define VT_ARB_DEFAULT_POLICY ArbPolicy{0, 3, 2, 50, 300, 500, {0, 0}}
struct ArbCount {
    int32_t evaluated;          // records written with status 1 or 2
    int32_t switched;           // of which status 2
};
struct ArbArgs {
    const float* head_out;      // [n * ns][8] by slot: the logits the decode of this pass read
    const float* hann;          // [ns]
    const FrameDesc* frames;    // [n] by slot: the frames of this pass
    StreamState* states;        // [B] by stream, as decode left them
    vt_result* results;         // [n] by slot (device)
    const int32_t* slot_stream; // [n] slot -> stream, null: the identity
    const int32_t* winner;      // non-null: a candidate pass - nothing is arbitrated, the winning slots' streams get status 3
    const ArbPolicy* policy;    // the caller's record
    ArbRec* recs;               // [B] by stream
    ArbCount* counts;           // [B] by stream, or null
    unsigned* tickets;          // [n * VT_ARB_MAX] by (slot, peak), zero between launches (score)
    double* partials;           // [n * VT_ARB_MAX][appear_chunks(nt)][5] (score)
    const bf16_t* anchor;       // [B][nt][kpad] by stream: the appearance store's
    bf16_t* probe;              // [B][VT_ARB_MAX][nt][kpad] by stream and peak
    const PassOut* out;         // device copy of the pass's PassOut: host_results, host_states; may be null
    StreamState* host_states;   // non-null: used instead of out->host_states
    ArbRec* host_recs;          // non-null: used instead of out->host_arbitrate - the [B] pinned mirror of the records (final records only)
    int n, ns, grid;
    float success_threshold;
};
// behind decode, ahead of motion_settle. list: one workgroup per slot - the iteration of the response peaks under the policy's
// K, R and min_resp, the due rule, eligibility (refresh rules 6 and 7 at each integer box), the record (final unless due)
hipError_t launch_arbitrate_list(const ArbArgs& a, const ModelDims& d, hipStream_t st);
// probe: per due slot and scored peak the template crop of this pass's frame at the peak's integer box into probe[stream][k]
hipError_t launch_arbitrate_probe(const ArbArgs& a, const ModelDims& d, int tier, int any_layout, hipStream_t st);
// score: the five sums of anchor[stream] and probe[stream][k] per due (slot, peak) in the appearance check's fixed order
hipError_t launch_arbitrate_score(const ArbArgs& a, int nt, int cols, int kpad, hipStream_t st);
// commit: one thread per slot - the switch rule, the final record and, on a switch, result, state and mirrors
hipError_t launch_arbitrate_commit(const ArbArgs& a, hipStream_t st);
