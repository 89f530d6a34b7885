// k_movers.hpp — the moving regions' records and launchers (k_movers.hip).
#pragma once
#include "vt_common.hpp"
#include "vt_frame.hpp"

// ---- moving regions (k_movers.hip) --------------------------------------------------------------------------------------
// DESIGN.md section 3 "Moving regions": per stream a background model of the frame thumbnail's cells (frame health's
// cells and geometry), the mask of the cells that left it, its 3x3 clean-up, the 8-connected components of what is kept and
// the largest of them as boxes in source pixels. The rule is stated to the bit in include/vittrack_hip_ops.h (vt_op_movers);
// the key table: vt_feature_keys.hpp. Integers only (the one exception: the corners of the stream's own box, see the rule):
// no order of additions or of label merges shows in any output bit. Per stream a record (mirrored to pinned host memory),
// two counters, two accumulators and, per cell, a label, three extents and an area, a background value, a thumbnail value
// and a mask byte; per slot a header. No part of StreamState or of a snapshot.
#define VT_MOVER_MIN_CELLS 4096
#define VT_MOVER_MAX_CELLS 262144
#define VT_MOVER_MAX 8
#define VT_MOVER_MAX_PERIOD 1000000
#define VT_MOVER_STILL_CAP (1 << 30)
struct MoverBox {
    int32_t x, y, w, h;         // source pixels: (i0 c, j0 c, (i1 - i0 + 1) c, (j1 - j0 + 1) c)
    int32_t area;               // cells
    int32_t label;              // the least row-major cell index of the component
};
struct MoverRec {
    int32_t status;             // 0: not due; 1: evaluated; 2: geometry; 4: no whole device frame; 5: background set, nothing
                                // evaluated; 6: evaluated, the picture changed as a whole (no components listed)
    int32_t frames_done;        // the stream's frames_done in the pass that wrote the record
    int32_t c, Wg, Hg;          // cell side in source pixels, the grid (0 where no cell exists)
    int32_t n;                  // entries of box[] that are listed
    int32_t moving, kept;       // cells of the mask, cells the clean-up kept
    int32_t components;         // 8-connected components of the kept cells, before min_area and the cut at max_n
    int32_t own_cells, own_kept;    // cells of the stream's own box, kept cells among them
    int32_t still;              // due records in a row (status 1) with own_kept == 0 and kept > 0, capped
    // the background's bookkeeping: one exists, and the geometry it was taken with
    int32_t has_bg, pW, pH, pc;
    MoverBox box[VT_MOVER_MAX]; // by area descending, then label ascending; entries from n on are zero
};
static_assert(sizeof(MoverBox) == 24 && sizeof(MoverRec) == 256 && offsetof(MoverRec, n) == 20 && offsetof(MoverRec, still) == 44 &&
              offsetof(MoverRec, has_bg) == 48 && offsetof(MoverRec, box) == 64, "MoverRec layout");
// ONE record per engine, device memory, written by the host only ("movers*" keys)
struct MoverPolicy {
    int32_t on;                 // "movers": 0 / 1
    int32_t period;             // 1..VT_MOVER_MAX_PERIOD: due when frames_done % period == 0
    int32_t cell;               // 0: automatic, else 4, 8, 16, 32
    int32_t thr;                // a cell moves iff |16 t - bg| > 16 thr
    int32_t min_area;           // components of fewer cells are dropped
    int32_t global_pm;          // status 6 where moving * 1000 > global_pm * Wg * Hg
    int32_t shape;              // learn | min_nb << 4 | max_n << 8 (vt_feature_keys.hpp: three keys, one word)
    int32_t max_cells;          // cells per stream: fixed by the first enable
};
#define VT_MOVER_SHAPE(learn, min_nb, max_n) ((learn) | (min_nb) << 4 | (max_n) << 8)
__host__ __device__ constexpr int mover_learn(int shape) { return shape & 15; }
__host__ __device__ constexpr int mover_min_nb(int shape) { return (shape >> 4) & 15; }
__host__ __device__ constexpr int mover_max_n(int shape) { return (shape >> 8) & 15; }
#define VT_MOVER_DEFAULT_POLICY MoverPolicy{0, 1, 0, 96, 4, 400, VT_MOVER_SHAPE(4, 3, 4), 65536}
// per stream, beside the policy: diagnostics, never rewound
struct MoverCount {
    int32_t evaluated;          // records written with status 1 or 6
    int32_t listed;             // the sum of their n
    int32_t reserved[2];
};
// per slot, written by the prepare launch and obeyed by the launches behind it
struct MoverHead {
    int32_t status;             // -1: another slot works for the stream; 0: not due; 2, 4: nothing measured; 5: background set; 1: evaluated
    int32_t stream, frames_done;
    int32_t c, Wg, Hg;
    int32_t reserved[2];
};
static_assert(sizeof(MoverHead) == 32 && sizeof(MoverCount) == 16, "MoverHead layout");
enum { MOVER_ACC_MOVING, MOVER_ACC_KEPT, MOVER_ACCS = 4 };
enum { MOVER_EXT_I0, MOVER_EXT_I1, MOVER_EXT_J1, MOVER_EXT_AREA, MOVER_EXTS };   // per cell, used at the index of a component's root
struct MoverArgs {
    const FrameDesc* frames;    // [n] by slot: the frames of this pass
    const StreamState* states;  // [B] by stream, as the decode (the commit) left them: initialized, frames_done, box
    const int32_t* slot_stream; // [n] slot -> stream, null: the identity
    const MoverPolicy* policy;  // the engine's record
    const int32_t* devflag;     // 1: the pass came through a device entry point
    MoverRec* recs;             // [B] by stream
    MoverCount* counts;         // [B] by stream
    MoverHead* heads;           // [n] by slot
    int32_t* accs;              // [B][MOVER_ACCS] by stream: moving, kept of the pass
    int32_t* labels;            // [B][max_cells] by stream: -1, or the cell's component (its least row-major index)
    int32_t* exts;              // [B][MOVER_EXTS][max_cells] by stream: i0, i1, j1 and the area, at the roots' indices
    uint16_t* bg;               // [B][max_cells] by stream: the background in sixteenths
    uint16_t* thumbs;           // [B][max_cells] by stream: the thumbnail of the last due pass, Hg x Wg, row-major
    uint8_t* mask;              // [B][max_cells] by stream: 0, 1 moving, 2 kept, of the last due pass
    MoverRec* host_recs;        // [B] by stream, pinned host memory: takes the records of the worked streams; may be null
    int max_cells;              // the stride of the per-cell arrays; fixes the launch dimensions
    int n;
};
// the launches, in this order, behind the decode (the commit) and ahead of everything that cuts or draws: the due rule, the
// geometry, the bookkeeping and the zeroed accumulators; the thumbnail, the mask and the background's update; the clean-up
// and the labels' start; the merges; the flat labels with areas and extents; the list, the own box, the record, the
// counters and the mirror. Fixed launch dimensions (max_cells): workgroups of slots that are not evaluated leave at once.
hipError_t launch_movers_prepare(const MoverArgs& a, hipStream_t st);
hipError_t launch_movers_thumb(const MoverArgs& a, int any_layout, hipStream_t st);
hipError_t launch_movers_label(const MoverArgs& a, hipStream_t st);     // three launches: start, merge, flatten
hipError_t launch_movers_list(const MoverArgs& a, hipStream_t st);
