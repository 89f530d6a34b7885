// k_refresh.hpp — the template refresh's records and launcher (k_refresh.hip).
#pragma once
#include "vt_common.hpp"
#include "vt_frame.hpp"

// ---- template refresh (k_refresh.hip) ---------------------------------------------------------------------------------
// per stream, device memory, written by the host only (never rewound) - but for the diagnostic counter
struct RefreshPolicy {
    int32_t period;             // 0: off, else 2..VT_REFRESH_MAX_PERIOD updates between refreshes
    float min_score;            // a refresh needs result.score >= min_score
    int32_t skipped_geometry;   // due refreshes skipped because the template crop left the sampled search crop
    int32_t reserved;
};
#define VT_REFRESH_MAX_PERIOD 1000000
struct AppearPolicy;
struct AppearCount;
struct ConflictPolicy;
struct ConflictCount;
struct HealthPolicy;
struct HealthCount;
struct RefreshArgs {
    const FrameDesc* frames;    // [n] by slot: the frames of this pass
    StreamState* states;        // [B] by stream, as decode / cand_commit left them
    const vt_result* results;   // [n] by slot
    const int32_t* slot_stream; // [n] slot -> stream, null: the identity
    const int32_t* winner;      // candidate pass: [n] the winning slot of slot i's stream (only winners refresh); else null
    RefreshPolicy* policy;      // [B] by stream
    unsigned* tickets;          // [B] by slot, zero between launches
    bf16_t* tpl;                // the two-buffer store [B][2][nt][kpad]
    const PassOut* out;         // device copy of the pass's PassOut: host_states gets the two words too
    StreamState* host_states;   // non-null: used instead of out->host_states (candidate passes: the commit's mirror)
    int n;
    // rule 8 (appearance-capable engines; all three null elsewhere: the kernels without the rule run). With the policy's
    // flag on and tau > 0 a refresh also needs THIS pass's record of the stream (the appearance launches run ahead of this one) to
    // have status 1 and similarity >= tau; else nothing is cut and counts[stream].gated += 1
    const AppearPolicy* ap_policy;
    AppearCount* ap_counts;     // [B] by stream
    const AppearRec* ap_recs;   // [B] by stream
    // rule 9 (conflicts-capable engines; all three null elsewhere). With the policy's flag and gate on, a stream whose record
    // of THIS pass (the conflicts launch runs ahead of this one) has status 2 is not refreshed and counts[stream].gated += 1;
    // checked behind rules 1-5 and ahead of rules 6-8: no geometry skip is counted and no window-miss mark is set
    const ConflictPolicy* cf_policy;
    ConflictCount* cf_counts;   // [B] by stream
    const ConflictRec* cf_recs; // [B] by stream
    // rule 10 (health-capable engines; all three null elsewhere). With the policy's flag and gate on, a stream whose record of
    // THIS pass (rec.frames_done == st.frames_done; the health launches run ahead of this one) has flags != 0 is not refreshed
    // and counts[stream].gated += 1; checked behind rule 9 and ahead of rules 6-8. A refresh rule 9 refused is not counted
    const HealthPolicy* hl_policy;
    HealthCount* hl_counts;     // [B] by stream
    const HealthRec* hl_recs;   // [B] by stream
};
// behind the decode (candidate pass: behind the commit): per slot the gate of DESIGN.md section 3 and, where it fires, the
// template crop of this pass's frame at the committed box into the stream's other buffer + the state's two words
hipError_t launch_template_refresh(const RefreshArgs& a, const ModelDims& d, int tier, int any_layout, hipStream_t st);
