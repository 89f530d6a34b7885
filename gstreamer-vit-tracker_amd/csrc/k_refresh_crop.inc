// k_refresh_crop.inc — the template crop of one slot's frame at the committed box, as text around the crop kernels' bodies
// (k_preproc_body.inc, is_template = 1): the rows are the bits vt_group_init_*(stream, this frame, result.bbox) writes.
// Included by the template refresh (k_refresh.hip), the appearance probe (k_appearance.hip) and the probe launch of the peak
// arbitration (k_arbitrate.hip, whose `st` carries a peak's integer box): an edit here is an edit to all three.
// In scope at the include: MODE and ANY (template parameters: k_refresh_dev.hpp), a.frames, slot, st (the kernel's COPY of
// the stream's state), crop_rows (bf16_t*: where rows [0, nt) go), src (LDS, MODE <= 2) and LDSPX, size, patch, kpad,
// na0..na2, nb0..nb2.
    {
        const FrameDesc f = a.frames[slot];
        StreamState& s = st;
        bf16_t* __restrict__ patches = crop_rows;
        const int b = 0, ntok = 0, row_off = 0, is_template = 1;    // rows [0, nt) of `patches`
        const float factor = 2.0f;
        auto crop = [&]() {                                          // a body may return: from here
            if constexpr (MODE <= 2) {
                constexpr int PX = 8;
#define PRE_BODY 3
#include "k_preproc_body.inc"
            } else if constexpr (MODE <= 4) {
                constexpr int PX = MODE == 3 ? 8 : 2;
#define PRE_BODY 2
#include "k_preproc_body.inc"
            } else {
#define PRE_BODY 1
#include "k_preproc_body.inc"
            }
        };
        crop();
    }
