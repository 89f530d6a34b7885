// k_camera_motion.hpp — the camera motion's records and launchers (k_camera_motion.hip).
#pragma once
#include "vt_common.hpp"
#include "vt_frame.hpp"

// ---- camera motion (k_camera_motion.hip) --------------------------------------------------------------------------------
// DESIGN.md section 3 "Camera motion": per stream the translation of the whole picture since the stream's last update, from
// two uint16 thumbnails of the frame and an exact integer SAD search; with mode 2 the stream's box moves by it. The rule
// is stated to the bit in include/vittrack_hip_ops.h (vt_op_camera_motion). Integer sums (vector integer atomics): no
// order of additions matters. Per stream a record (optionally mirrored to pinned host memory), two thumbnails and a SAD
// table; per slot a header. The launches run through the operator hook only: no engine pass carries them yet.
#define VT_CAM_R_MAX 16
#define VT_CAM_TABLE ((2 * VT_CAM_R_MAX + 1) * (2 * VT_CAM_R_MAX + 1))      // int64 entries of a stream's SAD table
#define VT_CAM_MIN_CELLS 4096
#define VT_CAM_MAX_CELLS 1048576
struct CamRec {
    int32_t status;             // 0: not due; 1: good; 2: geometry; 3: flat; 4: no whole device frame; 5: no previous thumbnail
                                // (or one of another geometry); 6: the minimum lies at the border of the range; 7: ambiguous
    int32_t frames_done;        // the stream's frames_done in the pass that wrote the record
    int32_t c, Wg, Hg, R;       // cell side in source pixels, the grid, the range (c, Wg, Hg: 0 where no cell exists)
    int32_t dx, dy;             // the best displacement in cells (status 1, 3, 6, 7; else 0)
    float shift[2];             // source pixels; 0 unless status is 1
    int32_t applied;            // 1: the pass moved the state box by shift
    int32_t n;                  // cells every displacement summed (status 1, 3, 6, 7; else 0)
    long long S_best, S0, S2;   // the least sum, the sum at (0, 0), the least sum at Chebyshev distance > 1 from the best
    int32_t evaluated;          // records written with status 1, 3, 6 or 7 (diagnostic)
    int32_t moved;              // passes with applied == 1
    // the thumbnails' bookkeeping: the buffer of the last thumbnail taken and the geometry it was taken with
    int32_t has_prev, cur, pW, pH, pc;
    int32_t reserved;
};
static_assert(sizeof(CamRec) == 104 && offsetof(CamRec, S_best) == 48 && offsetof(CamRec, has_prev) == 80, "CamRec layout");
// ONE record per engine, device memory, written by the host only (vt_group_set_tuning "camera_motion*")
struct CamPolicy {
    int32_t mode;               // "camera_motion": 0 off, 1 measure and report, 2 and move the box
    int32_t cell;               // 0: automatic, else 4, 8, 16, 32
    int32_t range;              // R: 2..VT_CAM_R_MAX
    int32_t conf_pm;            // 0..1000 per mille
    int32_t max_cells;          // thumbnail cells per stream: fixed by the first enable
    int32_t reserved[3];
};
#define VT_CAM_DEFAULT_POLICY CamPolicy{0, 0, 8, 800, 65536, {0, 0, 0}}
// per slot, written by the prepare launch and obeyed by the three behind it
struct CamHead {
    int32_t status;             // -1: another slot works for the stream; 0, 2, 4: nothing evaluated; 5: the thumbnail only; 1: + search
    int32_t stream, frames_done;
    int32_t c, Wg, Hg, R;
    int32_t cur;                // the thumbnail buffer this pass fills; the previous one is cur ^ 1
};
static_assert(sizeof(CamHead) == 32, "CamHead layout");
// the automatic cell: the smallest of 4, 8, 16, 32, 64 whose grid of whole cells fits max_cells; 0: none
__host__ __device__ inline int cam_auto_cell(int W, int H, int max_cells) {
    for (int c = 4; c <= 64; c *= 2)
        if ((long long)(W / c) * (H / c) <= (long long)max_cells) return c;
    return 0;
}
struct CamArgs {
    const FrameDesc* frames;    // [n] by slot: the frames of this pass
    StreamState* states;        // [B] by stream: the box moves (mode 2)
    const int32_t* slot_stream; // [n] slot -> stream, null: the identity
    const CamPolicy* policy;    // the engine's record
    const int32_t* devflag;     // 1: the pass came through a device entry point
    CamRec* recs;               // [B] by stream
    CamHead* heads;             // [n] by slot
    unsigned long long* sad;    // [B][VT_CAM_TABLE] by stream: (2R + 1)^2 sums, row dy + R, column dx + R
    uint16_t* thumbs;           // [B][2][max_cells] by stream: Hg x Wg, row-major
    StreamState* host_states;   // pinned [B] by stream or null: takes the moved x, y of a stream whose box moves
    CamRec* host_recs;          // pinned [B] by stream or null: takes the records of the worked streams
    int max_cells;              // the stride of the thumbnails; fixes the launch dimensions
    int n;
};
// the four launches, in this order (meant to be the first of a pass, ahead of motion_place, the template gather, cand_fill
// and the crop): the due rule, the geometry and the zeroed table; the thumbnail; the SAD search; the decision, the box, the record
// and the mirrors. Fixed launch dimensions (max_cells): workgroups of slots that are not due leave at once.
hipError_t launch_camera_prepare(const CamArgs& a, hipStream_t st);
hipError_t launch_camera_thumb(const CamArgs& a, int any_layout, hipStream_t st);
hipError_t launch_camera_search(const CamArgs& a, hipStream_t st);
hipError_t launch_camera_decide(const CamArgs& a, hipStream_t st);
