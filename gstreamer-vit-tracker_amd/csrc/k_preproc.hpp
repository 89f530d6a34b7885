// k_preproc.hpp — launchers of the crop, template-gather and NV12 conversion kernels (k_preproc.hip).
#pragma once
#include "vt_common.hpp"
#include "vt_frame.hpp"

// crop + bilinear + normalise -> patch rows; one launch covers slots [b0, b0+nb)
// tier: the tile kernel's LDS buffer (0: 16 KiB, 1: 32 KiB, 2 or more: 64 KiB), a choice of speed only
// slot_stream (device, [nb + b0] or null = identity): the stream a slot works for. Frame descriptor and patch rows are
// the slot's; the StreamState read (and its geo / frame_w / frame_h / window_miss written) is the stream's.
// any_layout: the highest pix_level of the slots' formats (above 0 the layout is read from FrameDesc.lay, at 3 the colour code as well: k_preproc_dev.hpp, fetch_rgb)
hipError_t launch_preproc(const FrameDesc* frames, StreamState* states, bf16_t* patches,
                          const ModelDims& d, int b0, int nb, bool is_template, hipStream_t st, int tier = 0,
                          const int32_t* slot_stream = nullptr, int any_layout = 0);
// subset passes: slot i's template rows [nt][kpad] of the patch matrix <- the template store tpl[slot_stream[i]]
hipError_t launch_gather_template_rows(const bf16_t* tpl, bf16_t* patches, const int32_t* slot_stream, int n,
                                       const ModelDims& d, hipStream_t st);
// the same from a store of TWO buffers per stream, tpl[B][2][nt][kpad] (engines with template refresh): a stream's rows are
// those of buffer states[stream].tpl_gen & 1. slot_stream null: the identity (a full pass)
hipError_t launch_gather_template_rows_gen(const bf16_t* tpl, bf16_t* patches, const int32_t* slot_stream,
                                           const StreamState* states, int n, const ModelDims& d, hipStream_t st);
int preproc_tier_for_box(const ModelDims& d, float w, float h, bool is_template);

hipError_t launch_nv12_to_rgb8(const uint8_t* nv12, int w, int h, uint8_t* rgb, hipStream_t st);
// n frames per launch: d_in[i] packed NV12 (nullptr: the all-zero frame of a short buffer), d_out[i] w*h*3 bytes; the
// tables are HOST arrays of device pointers (they travel in the kernel arguments, VT_NV12_BATCH_MAX frames per launch)
#define VT_NV12_BATCH_MAX 64
struct Nv12Batch { const uint8_t* in[VT_NV12_BATCH_MAX]; uint8_t* out[VT_NV12_BATCH_MAX]; };
hipError_t launch_nv12_to_rgb8_batch(const uint8_t* const* d_in, uint8_t* const* d_out, int n, int w, int h, hipStream_t st);
