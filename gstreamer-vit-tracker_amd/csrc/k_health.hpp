// k_health.hpp — the frame health's records and launchers (k_health.hip).
#pragma once
#include "vt_common.hpp"
#include "vt_frame.hpp"

// ---- frame health (k_health.hip) ----------------------------------------------------------------------------------------
// DESIGN.md section 3 "Frame health": per stream a uint16 thumbnail of the whole frame (camera motion's cells), five exact
// integer measures of it and of its change since the stream's previous thumbnail, three flags. The rule is stated to the
// bit in include/vittrack_hip_ops.h (vt_op_frame_health); the keys: include/vittrack_hip.h. Integers only: no order of additions matters. Per stream a
// record (mirrored to pinned host memory), three counters, four accumulators, two histograms and two
// thumbnails; per slot a header. No part of StreamState or of a snapshot.
#define VT_HEALTH_MIN_CELLS 4096
#define VT_HEALTH_MAX_CELLS 262144
#define VT_HEALTH_BINS 32           // histogram bins: t >> 7, t <= 4080
#define VT_HEALTH_MAX_PERIOD 1000000
#define VT_HEALTH_STILL_CAP (1 << 30)
#define VT_HEALTH_FROZEN 1
#define VT_HEALTH_FLAT 2
#define VT_HEALTH_CUT 4
struct HealthRec {
    int32_t status;             // 0: not due; 1: measured and compared; 2: geometry; 4: no whole device frame; 5: measured
                                // without a comparable previous thumbnail
    int32_t frames_done;        // the stream's frames_done in the pass that wrote the record
    int32_t flags;              // VT_HEALTH_FROZEN | VT_HEALTH_FLAT | VT_HEALTH_CUT
    int32_t c, Wg, Hg;          // cell side in source pixels, the grid (0 where no cell exists)
    int32_t still;              // comparisons with D == 0 in a row (status 1), capped
    int32_t reserved0;
    long long S1, S2, G;        // sum t, sum t * t, the sum of absolute differences of horizontal and vertical neighbours
    long long D, HD;            // against the previous thumbnail: sum |t - p|, sum over bins |hist - hist_p| (status 1; else 0)
    long long G_ref;            // G of the last status-5 or CUT record
    // the thumbnails' bookkeeping: the buffer of the last thumbnail taken and the geometry it was taken with
    int32_t has_prev, cur, pW, pH, pc;
    int32_t reserved1;
};
static_assert(sizeof(HealthRec) == 104 && offsetof(HealthRec, S1) == 32 && offsetof(HealthRec, has_prev) == 80, "HealthRec layout");
// ONE record per engine, device memory, written by the host only ("health*" keys)
struct HealthPolicy {
    int32_t on;                 // "health": 0 / 1
    int32_t period;             // 1..VT_HEALTH_MAX_PERIOD: due when frames_done % period == 0
    int32_t cell;               // 0: automatic, else 4, 8, 16, 32
    int32_t still_run;          // FROZEN at this many identical comparisons in a row
    int32_t flat_q;             // FLAT at a standard deviation of the thumbnail <= flat_q
    int32_t cut_pm;             // CUT at this share (per mille) of the cells in another bin; 0: never
    int32_t gate;               // "health_gate": 0 / 1 - refresh rule 10
    int32_t max_cells;          // thumbnail cells per stream: fixed by the first enable
};
#define VT_HEALTH_DEFAULT_POLICY HealthPolicy{0, 1, 0, 3, 32, 500, 0, 65536}
// per stream, beside the policy: diagnostics, never rewound
struct HealthCount {
    int32_t evaluated;          // records written with status 1 or 5
    int32_t flagged;            // of which flags != 0
    int32_t gated;              // refreshes refused by rule 10
    int32_t reserved;
};
// per slot, written by the prepare launch and obeyed by the three behind it
struct HealthHead {
    int32_t status;             // -1: another slot works for the stream; 0: not due; 2, 4: nothing measured; 5: measured; 1: + compared
    int32_t stream, frames_done;
    int32_t c, Wg, Hg;
    int32_t cur;                // the thumbnail and histogram this pass fills; the previous ones are cur ^ 1
    int32_t reserved;
};
static_assert(sizeof(HealthHead) == 32, "HealthHead layout");
enum { HEALTH_ACC_S1, HEALTH_ACC_S2, HEALTH_ACC_G, HEALTH_ACC_D, HEALTH_ACCS };
struct HealthArgs {
    const FrameDesc* frames;    // [n] by slot: the frames of this pass
    const StreamState* states;  // [B] by stream, as the decode (the commit) left them: initialized, frames_done
    const int32_t* slot_stream; // [n] slot -> stream, null: the identity
    const HealthPolicy* policy; // the engine's record
    const int32_t* devflag;     // 1: the pass came through a device entry point
    HealthRec* recs;            // [B] by stream
    HealthCount* counts;        // [B] by stream
    HealthHead* heads;          // [n] by slot
    unsigned long long* accs;   // [B][HEALTH_ACCS] by stream: S1, S2, G, D of the pass
    int32_t* hist;              // [B][2][VT_HEALTH_BINS] by stream
    uint16_t* thumbs;           // [B][2][max_cells] by stream: Hg x Wg, row-major
    const PassOut* out;         // device copy of the pass's PassOut: host_health takes the records of the worked streams; may be null
    int max_cells;              // the stride of the thumbnails; fixes the launch dimensions
    int n;
};
// the four launches, in this order, behind the decode (the commit) and ahead of everything that cuts or draws: the due rule,
// the geometry, the bookkeeping and the zeroed accumulators; the thumbnail with S1, S2, D and the histogram; G; the
// comparison, the flags, the record, the counters and the mirror. Fixed launch dimensions (max_cells): workgroups of slots
// that are not evaluated leave at once.
hipError_t launch_health_prepare(const HealthArgs& a, hipStream_t st);
hipError_t launch_health_thumb(const HealthArgs& a, int any_layout, hipStream_t st);
hipError_t launch_health_measure(const HealthArgs& a, hipStream_t st);
hipError_t launch_health_decide(const HealthArgs& a, hipStream_t st);
