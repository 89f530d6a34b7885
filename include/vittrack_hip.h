/*
 * vittrack_hip.h — C ABI of libvittrack_hip.so, the MI355X (gfx950) tracker hot path.
 *
 * This is the drop-in boundary for the reference's `vit_tracker` crate API
 * (`VitTrack::{new, init, update}`, `BBox`), which the reference host calls at
 *   - src/tracker_context.rs:21   VitTrack::new(model_path)        -> vt_create
 *   - src/tracker_context.rs:88   tracker.init(full_image, bbox)   -> vt_init_rgb8 / vt_init_nv12
 *   - src/tracker_context.rs:90   tracker.update(full_image)       -> vt_update_rgb8 / vt_update_nv12
 *   - src/tracker_context.rs:120  tracker.update(full_image)       -> vt_update_rgb8 / vt_update_nv12
 *   - src/selection_state.rs:44   BBox::new(x, y, w, h)            -> vt_bbox
 *   - src/tracker_context.rs:94   BBox::from_array(&result.bbox)   -> vt_result.bbox
 * and for the reference's own colour converter
 *   - src/nv12_convert.rs:46      nv12_full_to_rgb_parallel        -> vt_nv12_to_rgb8
 *
 * Rules that follow from the reference call sites:
 *   - plain pointers and sizes only; no C++/torch types cross this line;
 *   - every call is synchronous with respect to the caller's frame buffer: on
 *     return the library no longer reads it (the host draws overlays into the
 *     same buffer right after, src/pipeline.rs:125);
 *   - a handle has no thread affinity (created on the main thread, used on the
 *     GStreamer streaming thread, src/pipeline.rs:55-67); calls on ONE handle
 *     must be serialised by the caller (the reference holds a Mutex);
 *   - nothing throws or aborts across the boundary (release profile is
 *     panic="abort", Cargo.toml:37): every entry returns a vt_status code and
 *     vt_last_error() gives the text;
 *   - the accept gate `success && score > 0.25` stays on the caller side
 *     (src/tracker_context.rs:93,122).
 *
 * There is no CPU fallback behind this ABI: if no gfx950 device is present
 * vt_create fails with VT_ERR_NO_DEVICE.
 */
#ifndef VITTRACK_HIP_H
#define VITTRACK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VT_ABI_VERSION 5   /* 5: vt_nv12_to_rgb8_batch_device, vt_group_graph_captures, vt_group_*_streams (passes over a subset of a group's streams: added later, additions only - no struct, no existing signature or behaviour changed, so the version stays); VT_PIX_BGR8 .. VT_PIX_UYVY, vt_init_frame / vt_update_frame, then vt_group_enqueue_host_streams / vt_group_enqueue_init_host (added later still, additions only for the same reason); vt_pixfmt2 (VT_PIX2_I420 .. VT_PIX2_XBGR: further values of vt_frame.format, additions only - no function, no struct and no existing value changed, so the version stays); the operator-level test hooks (vt_op_*) moved to vittrack_hip_ops.h / libvittrack_hip_ops.so - the product library exports this header's symbols only; 4: vt_config.host_zero_copy (a former reserved slot: zero = the old default for single trackers), vt_group_set_tuning, vt_op_headconv_bf16, vt_op_headconv_ln_bf16 - additions only, a host built against 3 keeps working; 3: vt_op_gemm_bf16 / vt_op_qkv_bf16 take folded-LayerNorm terms; 2: vt_frame.window_w/h, vt_config.max_device_mib, explicit cfg/mode on vt_op_* */

typedef enum vt_status {
    VT_OK = 0,
    VT_ERR_INVALID_ARG = -1,
    VT_ERR_NO_DEVICE = -2,
    VT_ERR_IO = -3,          /* weights file missing / unreadable */
    VT_ERR_FORMAT = -4,      /* weights blob malformed or unsupported shape */
    VT_ERR_HIP = -5,         /* HIP runtime error (text in vt_last_error) */
    VT_ERR_NOT_INITIALIZED = -6, /* update before init */
    VT_ERR_SHORT_BUFFER = -7,
    VT_ERR_OOM = -8
} vt_status;

/* ≙ vit_tracker::BBox { x, y, width, height: i32 } (src/selection_state.rs:44,
 * src/tracker_context.rs:85) */
typedef struct vt_bbox {
    int32_t x, y, width, height;
} vt_bbox;

/* ≙ the value returned by VitTrack::update: fields success / score / bbox as
 * used at src/tracker_context.rs:92-95,122-125 */
typedef struct vt_result {
    int32_t success;
    float score;
    vt_bbox bbox;
} vt_result;

typedef struct vt_config {
    uint32_t struct_size;      /* = sizeof(vt_config); lets the struct grow */
    float success_threshold;   /* result.success = score >= this; <0 → blob default (0.20) */
    int32_t use_graph;         /* 1 (default): replay the frame as a hipGraph; 0: eager launches */
    int32_t n_streams;         /* vt_group_create only: independent tracked streams on this GPU,
                                * 1..VT_MAX_STREAMS */
    int32_t max_frame_width;   /* staging size for host-pointer calls; 0 → 3840 */
    int32_t max_frame_height;  /* 0 → 2160 */
    int32_t max_device_mib;    /* > 0: refuse (VT_ERR_OOM) to create an engine whose weights +
                                * activations need more HBM than this; 0: only the device's free
                                * memory limits it (checked before anything is allocated) */
    int32_t host_window_margin_pct; /* vt_group_enqueue_host: enlargement of the speculative window in
                                * percent of the crop side; 0 -> 75 (see there); < 0 -> none (tests:
                                * every moving target then takes the redo path) */
    int32_t host_zero_copy;    /* host-pointer calls on frames inside a vt_host_register range: 0 (default) =
                                * zero-copy route on single-stream engines (vt_create, n_streams 1) only,
                                * batched engines keep packing windows; 1 = zero-copy on every engine;
                                * -1 = never (always pack + copy). Measured trade-off at vt_host_register */
    int32_t reserved[5];
} vt_config;
#define VT_MAX_STREAMS 1024

typedef struct vt_model_info {
    int32_t patch, template_size, search_size, dim, heads, layers, mlp_dim;
    int32_t head_channels, tokens_template, tokens_search, kpad;
    int32_t score_grid;        /* search_size / patch */
    double flops_per_frame;    /* algorithmic FLOPs of one update (encoder+patch+head): every block on all
                                * tokens - also where the last block computes the search rows only (vt_group_set_tuning
                                * "last_rows"), so a rate derived from it keeps its denominator */
    double encoder_flops_per_frame; /* encoder + patch-embed only */
    uint64_t weight_bytes;
} vt_model_info;

typedef struct vt_tracker vt_tracker; /* one tracked stream  ≙ VitTrack */
typedef struct vt_group vt_group;     /* B independent streams batched on one GPU */

void vt_config_default(vt_config* cfg);
const char* vt_last_error(void);       /* thread-local text of the last failure */
int vt_abi_version(void);
/* "abi=5;k_gemm256=<sha256>;..." - identity of this build: the ABI version and, per kernel translation unit that a
 * committed measurement refers to, the sha256 over its sources and compile flags that build.py stamped into it
 * (bench.py ties profiles/r06_dominant_kernel_pmc.json to the kernel that is running through it). Static string. */
const char* vt_build_info(void);
int vt_device_count(void);             /* gfx950 devices visible; 0 → vt_create fails */
/* Streams per vt_group that fill the MI355X's 256 CUs in whole rounds of the 256x256 GEMM kernel
 * (the smallest batch <= max_streams whose worst encoder GEMM wastes < 2 % of its rounds; 1 if
 * there is none or the model's width does not fit that kernel). No reference counterpart: the
 * reference runs one tracker per process (src/pipeline.rs:55). Needs no GPU. */
int vt_recommended_streams(const vt_model_info* info, int max_streams);
/* How to spread n_streams over the vt_groups ("engines") of ONE GPU so that no engine pays for an
 * almost empty GEMM round: up to R = vt_recommended_streams() one engine; between R and 2R an engine
 * of R plus one with the rest (their kernels overlap on the chip: 31 streams cost 172 us per frame
 * as 30 + 1 against 197 in one engine and 164 at 30); from 2R on two engines of n/2 (three or more
 * concurrent engines measured worse than two). Writes the engine sizes (each <= VT_MAX_STREAMS) to
 * sizes[0..cap) and returns how many, 0 on bad arguments. No reference counterpart (one tracker per
 * process there, src/pipeline.rs:55). Needs no GPU. */
int vt_plan_engines(const vt_model_info* info, int n_streams, int* sizes, int cap);

/* ---- single stream: the literal drop-in ------------------------------------------------ */

/* ≙ VitTrack::new(model_path) (src/tracker_context.rs:21). */
int vt_create(const char* weights_path, int device_id, const vt_config* cfg, vt_tracker** out);
/* Same, with the weight blob already in this device's HBM (after the RCCL start-up broadcast,
 * SURVEY.md §8e). The library makes its own copy; the caller may free d_blob on return. */
int vt_create_from_device_blob(const void* d_blob, size_t bytes, int device_id,
                               const vt_config* cfg, vt_tracker** out);
void vt_destroy(vt_tracker* t);
int vt_get_model_info(const vt_tracker* t, vt_model_info* out);

/* ≙ tracker.init(&ArrayView3<u8>, bbox) with the (H,W,3) RGB8 view of src/pipeline_ir.rs:142 /
 * src/nv12_convert.rs:90: C-contiguous rows of `stride_bytes` (>= 3*w), channel order R,G,B. */
int vt_init_rgb8(vt_tracker* t, const uint8_t* rgb, int w, int h, int stride_bytes, vt_bbox box);
/* ≙ tracker.update(&ArrayView3<u8>) -> Result<{success, score, bbox}> */
int vt_update_rgb8(vt_tracker* t, const uint8_t* rgb, int w, int h, int stride_bytes,
                   vt_result* out);

/* Fused ingest: the host skips nv12_full_to_rgb_parallel (src/pipeline.rs:105); every pixel the
 * tracker samples goes through exactly the reference's integer conversion
 * (src/nv12_convert.rs:109-147). y/uv are the two NV12 planes; strides in bytes. */
int vt_init_nv12(vt_tracker* t, const uint8_t* y, const uint8_t* uv, int w, int h, int y_stride,
                 int uv_stride, vt_bbox box);
int vt_update_nv12(vt_tracker* t, const uint8_t* y, const uint8_t* uv, int w, int h,
                   int y_stride, int uv_stride, vt_result* out);

/* Fused YUY2 ingest (packed 4:2:2, stride in bytes >= 2*w, w even): the capture format of the
 * reference's live pipeline (src/pipeline_ir.rs:27-41), so the host can skip videoconvert. */
int vt_init_yuy2(vt_tracker* t, const uint8_t* yuy2, int w, int h, int stride_bytes, vt_bbox box);
int vt_update_yuy2(vt_tracker* t, const uint8_t* yuy2, int w, int h, int stride_bytes,
                   vt_result* out);

/* Same four calls with the frame already resident in this GPU's HBM (device pointers). */
int vt_init_rgb8_device(vt_tracker* t, const void* d_rgb, int w, int h, int stride_bytes,
                        vt_bbox box);
int vt_update_rgb8_device(vt_tracker* t, const void* d_rgb, int w, int h, int stride_bytes,
                          vt_result* out);
int vt_init_nv12_device(vt_tracker* t, const void* d_y, const void* d_uv, int w, int h,
                        int y_stride, int uv_stride, vt_bbox box);
int vt_update_nv12_device(vt_tracker* t, const void* d_y, const void* d_uv, int w, int h,
                          int y_stride, int uv_stride, vt_result* out);

/* ---- start-up weight broadcast over RCCL, for hosts without Python ------------------------------
 * The path shards by stream (one process / host thread per GPU, no per-frame exchange); its only
 * collective is the weight broadcast at start-up. librccl is loaded lazily
 * (dlopen; symbols already in the process - e.g. PyTorch's bundled copy - are used first), so the
 * library has no link-time dependency on it. Protocol, one caller per GPU:
 *   rank 0        vt_rccl_unique_id(id)           128 opaque bytes (ncclUniqueId); the HOST ships
 *                                                 them to the other ranks (file, socket, env, ...)
 *   every rank    vt_broadcast_weights_rccl(id, world, rank, device, path, &d_blob, &bytes)
 *                                                 rank 0 reads `path` (ignored elsewhere); one
 *                                                 ncclBroadcast of the size, one of the bytes
 *   every rank    vt_create_from_device_blob / vt_group_create_from_device_blob(d_blob, bytes, ...)
 *   every rank    vt_free_device_blob(device, d_blob)
 * VT_ERR_NO_DEVICE if librccl cannot be loaded, VT_ERR_HIP for RCCL errors (text in vt_last_error). */
#define VT_RCCL_ID_BYTES 128
int vt_rccl_unique_id(uint8_t id_out[VT_RCCL_ID_BYTES]);
int vt_broadcast_weights_rccl(const uint8_t id[VT_RCCL_ID_BYTES], int world, int rank, int device_id,
                              const char* weights_path, void** d_blob_out, size_t* bytes_out);
void vt_free_device_blob(int device_id, void* d_blob);

/* ---- B streams on one GPU (one stream per camera; no cross-stream data flow) ------------ */

/* VT_PIX_YUY2: packed 4:2:2, bytes Y0 U Y1 V per pixel pair (the format the reference's IR
 * pipeline captures, src/pipeline_ir.rs:27-41, before GStreamer's videoconvert turns it into RGB);
 * converted per sampled pixel with the same BT.601 integer formulas as NV12.
 * Formats 3-7 are byte permutations or paddings of the first three and sample exactly as they do. */
typedef enum vt_pixfmt {
    VT_PIX_RGB8 = 0,
    VT_PIX_NV12 = 1,
    VT_PIX_YUY2 = 2,
    VT_PIX_BGR8 = 3,   /* packed B,G,R, stride >= 3*w (OpenCV's order): RGB8 with the channels reversed */
    VT_PIX_RGBX = 4,   /* packed R,G,B,x, stride >= 4*w (RGBA: alpha ignored): RGB8 */
    VT_PIX_BGRX = 5,   /* packed B,G,R,x, stride >= 4*w (BGRA: alpha ignored): RGB8 with the channels reversed */
    VT_PIX_NV21 = 6,   /* Y plane + interleaved V,U plane: NV12 with U and V swapped, window rules of NV12 */
    VT_PIX_UYVY = 7    /* packed U Y0 V Y1, w even: YUY2 with the bytes reordered, window rules of YUY2 */
} vt_pixfmt;

/* Further values of vt_frame.format (vt_pixfmt itself is closed at the eight formats above). Each is DEFINED as a byte
 * re-arrangement of RGB8, NV12 or YUY2 - its sibling - and samples exactly as the sibling does. Values 8..15 and
 * everything above 22 are invalid (in bits 0..7; bits 8..15: vt_color_matrix below).
 * I420 / YV12: the chroma planes are ceil(w/2) x ceil(h/2) bytes and share stride1 (>= ceil(w/2)). plane1 is the FIRST
 * chroma plane (U for I420, V for YV12); the second begins stride1 * ceil(R/2) bytes behind plane1, R = window_h when
 * windowed == 1, else height: the contiguous layout of GStreamer's default GstVideoInfo, of av_image_fill_arrays and of
 * raw .yuv files. A frame whose chroma planes are allocated apart cannot be described. Window rules of NV12; plane1
 * points at the chroma sample of (origin_x, origin_y).
 * P010 (P012 and P016 read alike): only the high byte of every 16-bit sample is read - the sample truncated to 8 bits.
 * Strides in bytes: stride0 >= 2*w, stride1 >= 2*((w+1)&~1). Window rules of NV12, the pointers at byte 2*origin_x.
 * NV16: w even, stride0 >= w, stride1 >= w, window rules of YUY2. GRAY8, XRGB, XBGR: no window restriction; byte 0 of
 * an XRGB / XBGR pixel is never read. */
typedef enum vt_pixfmt2 {
    VT_PIX2_I420  = 16, /* Y plane; plane1 = U plane, then the V plane: three-plane 4:2:0             -> NV12 */
    VT_PIX2_YV12  = 17, /* the same with V first                                                        -> NV12 */
    VT_PIX2_P010  = 18, /* NV12's layout with 16-bit little-endian samples, value in the high bits      -> NV12 */
    VT_PIX2_NV16  = 19, /* Y plane + interleaved U,V pairs with one chroma row PER luma row (4:2:2)     -> YUY2 */
    VT_PIX2_GRAY8 = 20, /* one plane, one byte per pixel: r = g = b = that byte                         -> RGB8 */
    VT_PIX2_XRGB  = 21, /* packed x,R,G,B (ARGB: alpha ignored), stride >= 4*w                          -> RGB8 */
    VT_PIX2_XBGR  = 22  /* packed x,B,G,R (ABGR: alpha ignored), stride >= 4*w                          -> RGB8 */
} vt_pixfmt2;

/* The colour MEANING of a YUV frame, chosen per frame: vt_frame.format = pixel format | matrix << 8 | range << 12.
 * Bits 0..7 hold a vt_pixfmt / vt_pixfmt2 value, bits 8..11 the matrix (0..2), bits 12..15 the range (0..1), bits 16..31
 * are zero. VT_FRAME_FORMAT(p, VT_COLOR_BT601, VT_RANGE_LIMITED) == p: a plain format value means what it always meant,
 * the reference's BT.601 limited-range conversion. Refused with VT_ERR_INVALID_ARG, wherever a frame is checked and with
 * nothing changed: a matrix above 2, a range above 1, any bit above 15, and colour bits that are not zero on a format
 * without chroma (RGB8, BGR8, RGBX, BGRX, XRGB, XBGR, GRAY8: limited-range RGB and grey are not described); the error
 * text names the format. Chroma siting (the nearest stored sample, replicated), P010's high byte and the layouts are what
 * they are without the bits; transfer functions (PQ, HLG) are not applied.
 * The rule, to the bit, for code c = matrix * 2 + range, Y, U, V the stored samples, int32 arithmetic:
 *     yv = CY * (Y - YO)
 *     R = yv + CRV * (V - 128) + 128
 *     G = yv + CGU * (U - 128) + CGV * (V - 128) + 128
 *     B = yv + CBU * (U - 128) + 128
 *     each: min(max(x, 0), 0xffff) >> 8           (arithmetic shift)
 *     c  matrix, range      YO   CY  CRV   CGU   CGV  CBU
 *     0  BT.601 limited     16  298  409  -100  -208  516    (the reference's constants)
 *     1  BT.601 full         0  256  359   -88  -183  454
 *     2  BT.709 limited     16  298  459   -55  -136  541
 *     3  BT.709 full         0  256  403   -48  -120  475
 *     4  BT.2020 limited    16  298  430   -48  -167  548
 *     5  BT.2020 full        0  256  377   -42  -146  482
 * Each entry is rint(256 * exact) with Kr / Kb = 0.299 / 0.114, 0.2126 / 0.0722, 0.2627 / 0.0593, luma scale 255/219
 * (limited) or 1 (full), chroma scale 255/224 or 1; every channel of every row lies within 1 of the clipped, rounded
 * float64 conversion over all 2^24 triples (DESIGN.md section 3 "Colorimetry").
 * The entry points WITHOUT a format argument stay BT.601 limited range: the NV12 and YUY2 convenience calls of the single
 * tracker (init / update, host and device) and the whole-frame NV12 to RGB8 converters. A frame of another colour goes
 * through the calls that take a vt_frame: the single tracker's frame calls and every group call. */
typedef enum vt_color_matrix { VT_COLOR_BT601 = 0, VT_COLOR_BT709 = 1, VT_COLOR_BT2020 = 2 } vt_color_matrix;   /* BT.2020: non-constant luminance */
typedef enum vt_color_range  { VT_RANGE_LIMITED = 0, VT_RANGE_FULL = 1 } vt_color_range;
#define VT_FRAME_FORMAT(pix, matrix, range) ((int32_t)(pix) | ((int32_t)(matrix) << 8) | ((int32_t)(range) << 12))

typedef struct vt_frame {        /* one device-resident frame (or a window of it) */
    const void* plane0;          /* packed formats and GRAY8: the pixels; NV12 / NV21 / I420 / YV12 / P010 / NV16: Y plane */
    const void* plane1;          /* NV12 / NV21 / P010 / NV16: interleaved chroma plane; I420 / YV12: the first chroma
                                  * plane (the second follows it, see vt_pixfmt2); packed formats and GRAY8: NULL */
    int32_t width, height;       /* size of the FULL frame in pixels */
    int32_t stride0, stride1;    /* bytes */
    int32_t format;              /* vt_pixfmt or vt_pixfmt2, or with colour bits: VT_FRAME_FORMAT (vt_color_matrix) */
    /* The planes may hold only a window of the frame: plane0 points at frame pixel
     * (origin_x, origin_y) (NV12 / NV21 / I420 / YV12 / P010: both even, plane1 at the matching chroma
     * sample; YUY2 / UYVY / NV16: origin_x even). Pixels of the frame
     * outside the stored window must not be needed by the call (the tracker reads the search
     * window, side 4*sqrt(w*h) around the last box, plus one pixel). 0,0 = the whole frame. */
    int32_t origin_x, origin_y;
    int32_t windowed;            /* 1: the planes hold only window_w x window_h pixels (strides
                                  * describe that window); 0 with origin 0,0: the whole frame */
    /* Extent of the stored window in pixels (required when windowed == 1 or an origin is set; both
     * even for NV12 / NV21 / I420 / YV12 / P010, window_w even for YUY2 / UYVY / NV16, unless the window ends at the
     * frame's edge). A sample
     * that falls inside the frame but outside the stored window reads as black - never out of
     * bounds. 0,0 with no origin: width x height. */
    int32_t window_w, window_h;
} vt_frame;

/* The single tracker on a frame of any vt_pixfmt / vt_pixfmt2. on_device == 0: the planes are host addresses, read
 * like vt_init_rgb8 reads its buffer (only the search window crosses PCIe; origin fields ignored);
 * on_device == 1: they are device addresses, used like the *_device calls' (windows honoured). */
int vt_init_frame(vt_tracker* t, const vt_frame* frame, int on_device, vt_bbox box);
int vt_update_frame(vt_tracker* t, const vt_frame* frame, int on_device, vt_result* out);

int vt_group_create(const char* weights_path, int device_id, const vt_config* cfg, vt_group** out);
int vt_group_create_from_device_blob(const void* d_blob, size_t bytes, int device_id,
                                     const vt_config* cfg, vt_group** out);
void vt_group_destroy(vt_group* g);
int vt_group_streams(const vt_group* g);
int vt_group_get_model_info(const vt_group* g, vt_model_info* out);
/* (re)initialise stream `stream` of the group on a device-resident frame */
int vt_group_init_device(vt_group* g, int stream, const vt_frame* frame, vt_bbox box);
/* One hot-path pass: frames[i] feeds stream i (n == vt_group_streams). Asynchronous: the pass is
 * enqueued on the group's HIP stream; results land in the group's pinned result ring. */
int vt_group_enqueue_device(vt_group* g, const vt_frame* frames, int n);
/* Wait for every enqueued pass and copy the results of the LAST pass (n entries, in that pass's order; n may not
 * exceed that pass's size - entries beyond it are not written). */
int vt_group_wait(vt_group* g, vt_result* out, int n);
/* enqueue + wait */
int vt_group_update_device(vt_group* g, const vt_frame* frames, int n, vt_result* out);
/* HIP stream the group launches on (hipStream_t as void*), for event timing by the caller */
void* vt_group_hip_stream(vt_group* g);
/* The same with HOST frames (vt_frame.plane0/plane1 are host addresses; any pixel format, strides
 * honoured, origin fields ignored): ≙ B reference hosts calling tracker.init / tracker.update
 * (src/tracker_context.rs:88,90,120) in the same frame period. Only each stream's search window is
 * read from the caller's buffers; the windows of all n frames are packed into one pinned arena and
 * cross PCIe in one copy. Synchronous: the caller's buffers may be reused on return. */
int vt_group_init_host(vt_group* g, int stream, const vt_frame* host_frame, vt_bbox box);
int vt_group_update_host(vt_group* g, const vt_frame* host_frames, int n, vt_result* out);
/* Pipelined form of the same: the upload of pass t+1 overlaps the compute of pass t.
 *   vt_group_enqueue_host(frames of t+1)   packs the windows into one of two pinned arenas and copies
 *                                          them on a separate copy stream, then enqueues the pass
 *                                          behind that copy; returns without waiting
 *   vt_group_wait_next(out)                waits for the OLDEST pass not yet collected, returns its
 *                                          results
 * At most two passes may be outstanding (one running, one queued); the host frames of an outstanding
 * pass must stay valid and unchanged until its vt_group_wait_next returns.
 * While a pass is running its boxes are not known, so the window of the next frame is cut around the
 * last KNOWN box, enlarged to cover a target that moves by a quarter of the search crop and grows by a
 * quarter in one frame (1.75x the crop side). The pixel kernel flags a pass that needed a pixel outside
 * the window it was given; vt_group_wait_next then restores the stream states from the HOST's copy of
 * the states the previous pass left (collected by the wait_next before it) and redoes that pass (and
 * the one queued behind it) with exact windows, so the results are always those of the full frames.
 * While a pass is outstanding it owns the stream states: every entry point that would advance or
 * overwrite them (vt_group_init_*, vt_group_enqueue_device, vt_group_update_device / _host, the *_streams passes
 * other than vt_group_enqueue_host_streams, vt_group_wait, vt_group_set_state_box, vt_group_profile_device) returns
 * VT_ERR_INVALID_ARG until vt_group_wait_next has collected it; vt_group_enqueue_init_host takes a stream that is in
 * no outstanding pass. (host -> tracker: src/pipeline.rs:95-101 maps the buffer on the CPU) */
int vt_group_enqueue_host(vt_group* g, const vt_frame* host_frames, int n);
int vt_group_wait_next(vt_group* g, vt_result* out, int n);
/* passes vt_group_wait_next had to redo because a speculative window missed (since creation) */
int vt_group_host_redos(const vt_group* g);
/* hipGraph captures this engine has made since creation. The pass is replayed as a captured graph, one per
 * crop-buffer tier; all of them are captured and instantiated when the engine is created (and again by
 * vt_group_set_tuning), never inside an enqueue: a live 60-fps stream (src/pipeline.rs:26-37) whose target grows
 * across a tier boundary takes no capture stall mid-track. Passes that carry a format other than RGB8, NV12 and YUY2
 * replay a second set of graphs (crop kernels that read the byte layout): all its tiers are captured inside the init
 * call (vt_group_init_*, vt_init_*) that first initialises a stream on such a format, again never inside an enqueue.
 * A pass with such a format on an engine none of whose streams was initialised on one launches eagerly. Constant
 * after creation unless the tuning is changed or that first init happens. */
int vt_group_graph_captures(const vt_group* g);
/* One pass over the n streams streams[0..n): distinct, each initialised, 1 <= n <= vt_group_streams.
 * frames[i] feeds streams[i]; out[i] / vt_group_wait's i-th entry is its result. Streams not listed are
 * not touched (their state, template and results stay as they were) and need not be initialised.
 * ≙ a multi-camera host that calls tracker.update only for the cameras that are tracking, or confirm a selection
 * this frame (src/tracker_context.rs:88-90,120); cameras that are selecting or lost sit the frame out.
 * The pass runs the full pass's kernels on n compacted slots (M = n x the tokens of one frame): a stream's results are
 * bit-identical to those of an n-stream group given the same inputs, and the encoder's work is linear in n.
 * The full identity list (0, 1, ..., B-1) is the full pass and replays its captured graph; any other list is
 * launched eagerly (no graph is ever captured inside an update: vt_group_graph_captures stays constant).
 * Bad input - a duplicate or out-of-range index, n < 1 or n > vt_group_streams, a null pointer, an invalid frame -
 * returns VT_ERR_INVALID_ARG; a listed stream that was never initialised, VT_ERR_NOT_INITIALIZED. In both cases
 * nothing is enqueued and no state changes. Refused (VT_ERR_INVALID_ARG) while a pipelined host pass is outstanding.
 * Per-pass tensors of vt_group_read_tensor ("x", "feat", "head_out", ...) then exist only for the listed streams. */
int vt_group_enqueue_device_streams(vt_group* g, const int32_t* streams, const vt_frame* frames, int n);
/* enqueue + wait */
int vt_group_update_device_streams(vt_group* g, const int32_t* streams, const vt_frame* frames, int n,
                                   vt_result* out);
/* The same with HOST frames: stream streams[i]'s search window is cut from host_frames[i] around its own last box
 * and uploaded as by vt_group_update_host. Synchronous. */
int vt_group_update_host_streams(vt_group* g, const int32_t* streams, const vt_frame* host_frames, int n,
                                 vt_result* out);
/* The pipelined form of a subset pass, collected by vt_group_wait_next: vt_group_enqueue_host over the streams
 * streams[0..n). The list is checked as vt_group_enqueue_device_streams checks it (same status codes, nothing enqueued
 * and nothing changed on failure); host_frames[i] feeds streams[i] (any vt_pixfmt, strides honoured, origin fields
 * ignored) and must stay valid and unchanged until the pass is collected.
 * At most two passes outstanding, as for vt_group_enqueue_host. The two may have different lists, overlapping or
 * disjoint, and full and subset passes may alternate freely: the identity list (0, 1, ..., B-1) IS the full pass and
 * replays its captured graph, any other list launches eagerly (vt_group_graph_captures stays constant).
 * vt_group_wait_next returns the oldest uncollected pass's results in THAT pass's list order; n larger than that
 * pass's size writes only the pass's entries (the rule of vt_group_wait).
 * Windows: a stream that is in the pass still outstanding has a box nobody knows yet, so its window is speculative
 * (cut around the last known box, enlarged by vt_config.host_window_margin_pct); a stream that is NOT in the
 * outstanding pass has an exact known box: its window is exact and it can never cause a redo. vt_group_wait_next
 * looks at the window misses of the speculative streams of the pass it collects; on a miss it rewinds the streams of
 * that pass and of the younger one to the states they started from, redoes the pass with exact windows over the SAME
 * list, then the younger pass over ITS list (a stream's bits depend on the pass size, so only the same lists keep the
 * results those of vt_group_update_host_streams, bit for bit). Streams in neither pass are not touched.
 * vt_group_host_redos counts as before. After a collect only the listed streams' known states and results move;
 * vt_group_read_tensor behaves as after the synchronous subset pass. Frames inside a vt_host_register range take the
 * zero-copy route under the same vt_config.host_zero_copy rule. Everything refused while a pipelined pass is
 * outstanding stays refused, whichever kind of pass it is. */
int vt_group_enqueue_host_streams(vt_group* g, const int32_t* streams, const vt_frame* host_frames, int n);
/* (Re)initialise `stream` BEHIND the outstanding pipelined passes, without waiting for them: ≙ tracker.init
 * (src/tracker_context.rs:88) on one camera while the others keep tracking. Allowed only if `stream` is in no
 * outstanding pass (VT_ERR_INVALID_ARG otherwise: collect it with vt_group_wait_next first; nothing changed); with
 * nothing outstanding it is vt_group_init_host. Arguments are checked as by vt_group_init_host.
 * The window is packed into pinned memory of the call's own before it returns (the caller's buffer may be reused; a
 * frame in a vt_host_register range is packed too, since the crop runs after the call has returned), its
 * upload goes on the copy stream, the state write and the template crop on the group's stream behind the passes
 * already queued; the call does not wait for that stream. The stream may be listed from the very next
 * vt_group_enqueue_host_streams on; its first window is exact (its box is the init box). A redo behind the init
 * restores the initialised state. One exception to "does not wait": the first stream initialised on a format other
 * than RGB8 / NV12 / YUY2 has the second set of graphs captured inside this call (vt_group_graph_captures), a capture
 * needs an idle stream, so that one call waits for the outstanding passes (they stay uncollected). */
int vt_group_enqueue_init_host(vt_group* g, int stream, const vt_frame* host_frame, vt_bbox box);

/* ---- candidate passes: several search windows per stream, the best one committed -----------------
 * A stream owns one search window per update, cut around its own state box (side 4*sqrt(w*h)); once the target is
 * outside it every later update fails in the same place (≙ the reference host's Lost state, which makes no tracker
 * call for 61 frames and then waits for a new selection, src/tracker_context.rs:142-153). A candidate pass evaluates
 * several windows for such a stream in ONE pass, beside the cameras that are tracking, and decides on the device. */
typedef struct vt_candidate {
    int32_t stream;    /* the stream this slot works for; may repeat within a pass */
    int32_t has_box;   /* 0: window around the stream's own state box (what an update does); 1: around box */
    float box[4];      /* x, y, w, h in frame pixels, top-left + size; read only when has_box == 1 */
} vt_candidate;        /* 24 bytes */
/* One pass over the n slots cands[0..n), 1 <= n <= vt_group_streams(g): a pass has as many slots as the engine has
 * streams, whichever streams fill them. frames[i] feeds slot i, out[i] (not null) is slot i's result. Synchronous,
 * like vt_group_update_device_streams.
 * Slot results: every slot is a complete, independent update of cands[i].stream's template on frames[i], its window
 * cut around the slot's box. Slot i's result and per-pass tensors are bit-identical to those of slot i of an n-stream
 * group whose stream i holds cands[i].stream's template and had its box set to the slot's box (M = n x the tokens of
 * one frame, rows independent: the contract of the subset passes).
 * Winner: among the slots of one stream the one with the greatest vt_result.score; a NaN score loses to any number;
 * equal scores: the lowest slot index. winner[i] (winner may be null) is the winning slot of cands[i].stream, so
 * winner[i] == i marks the winners.
 * Commit: a listed stream's state after the pass is the winner's - crop geometry, frame size, argmax cell, unrounded
 * box, score, window-miss mark. Its update count advances by ONE per pass however many slots it had, its success
 * count by the winner's success. Its state box becomes the winner's integer box if the winner succeeded; if not it
 * stays what it was BEFORE the pass, never a candidate's box. Losing slots leave no trace in any stream's state.
 * Streams not listed are untouched, bit for bit, and need not be initialised.
 * A list in which every stream occurs once with has_box == 0 IS vt_group_update_device_streams over those streams
 * (same results, same state words; the identity list replays the captured graph). Every other list launches eagerly:
 * vt_group_graph_captures stays constant.
 * Errors return with nothing enqueued, no state changed and no result written. VT_ERR_INVALID_ARG: a null pointer, n
 * out of range, a stream index out of range, an invalid frame, a box that vt_group_set_state_box would refuse (a
 * non-finite value, a side outside 1..32768, |x| or |y| above 65536); VT_ERR_NOT_INITIALIZED: a listed stream that
 * was never initialised. Refused (VT_ERR_INVALID_ARG) while a pipelined host pass is outstanding; candidate passes
 * have no pipelined form.
 * vt_group_read_tensor(g, stream, ...) after a candidate pass reads the WINNING slot's tensors; "state" is the
 * committed state. */
int vt_group_update_device_candidates(vt_group* g, const vt_candidate* cands, const vt_frame* frames, int n,
                                      vt_result* out, int32_t* winner);
/* The same with HOST frames: slot i's window is cut from host_frames[i] around the slot's box and is exact, so no
 * redo can occur. Slots that name the SAME host frame (equal planes, strides, size and format) are staged once, as
 * the bounding rectangle of their windows - a scan whose windows overlap by half would otherwise upload every pixel
 * four times. Frames inside a vt_host_register range take the zero-copy route under the vt_config.host_zero_copy
 * rule, unchanged. Bit-identical to the device form on the same pixels. */
int vt_group_update_host_candidates(vt_group* g, const vt_candidate* cands, const vt_frame* host_frames, int n,
                                    vt_result* out, int32_t* winner);
/* The candidate state boxes whose search windows tile a frame; needs no GPU. In double precision:
 * side = 4*sqrt(box_w*box_h), stride = side*(100 - overlap_pct)/100. Per axis of length L: one centre L/2 if
 * L <= side; else n = ceil((L - side)/stride) + 1 centres side/2 + i*(L - side)/(n - 1): the first and last windows
 * are flush with the frame edges and the spacing never exceeds stride. Boxes come row by row (y outer), each
 * (cx - box_w/2, cy - box_h/2, box_w, box_h) rounded to float. An update still returns the exact box with its window
 * centre off the target by a quarter of the side, so overlap_pct = 50 covers every target position.
 * Returns the number of windows and writes min(count, cap) of them to boxes4 (4 floats each; boxes4 may be null with
 * cap 0). Returns 0 on bad arguments (overlap_pct outside 0..90, a frame side below 16 or above 65536, a box side that is not
 * finite or outside 1..32768), like vt_plan_engines. */
int vt_scan_windows(int frame_w, int frame_h, float box_w, float box_h, int overlap_pct, float* boxes4, int cap);

/* ---- template refresh ------------------------------------------------------------------------
 * A stream's template is cut at init. With a refresh policy the DEVICE cuts it again, behind the decode and inside the
 * pass - full, subset, candidate and pipelined passes alike - so a long-running stream follows its target's appearance
 * without the host draining its pipeline for a re-init.
 * Per stream: period (0 = off, else 2..1,000,000 updates) and min_score (finite, 0..1). After an update of the stream
 * with result r that left the state st, the template is refreshed iff ALL of:
 *   1. period >= 2;                      2. in a candidate pass: the slot is its stream's winner;
 *   3. r.success and r.score >= min_score (a NaN score fails);
 *   4. st.frames_done - last_frame >= period (last_frame: frames_done at the last refresh, 0 after init);
 *   5. the pass's search crop met no window miss (a speculative pipelined pass that will be redone never refreshes;
 *      its redo does);
 *   6. the tap rectangle of the template crop (factor 2, side template_size) at the new box lies inside the tap
 *      rectangle of the search crop the pass sampled; per axis, in binary32, lo = floor(0.5*scale + x0) and
 *      hi = floor((size - 0.5)*scale + x0) + 1. A due refresh that fails only this is counted in skipped_geometry
 *      (a diagnostic: a redone pass may count twice) and tried again at the stream's next update.
 *   7. the in-frame part of that template rectangle lies inside the window the pass's frame stores. Whole frames and the
 *      windows the library cuts for the stream's own box always do; a speculative pipelined window that does not is
 *      reported as a window miss, so the pass is redone with an exact window and the redo refreshes.
 * A refresh is exactly vt_group_init_*(stream, the whole frame of that update, r.bbox) as far as the template goes -
 * the same rows, bit for bit, taps outside the frame black - but box, counters and the rest of the state stay as the
 * update left them; generation += 1, last_frame = frames_done. The next pass runs on the new template.
 * The first call that enables a policy on an engine makes it refresh-capable for good: it allocates a second template
 * buffer per stream (within vt_config.max_device_mib, else VT_ERR_OOM and nothing changes) and recaptures the engine's
 * graphs; from then on every pass of that engine carries one gather and one refresh launch. Engines that never
 * enable launch what they always did.
 * stream -1: every stream of the group. VT_ERR_INVALID_ARG (nothing changed) on a bad stream, period 1, a negative
 * period or one above 1,000,000, min_score not finite or outside 0..1, and while a pipelined host pass is outstanding.
 * vt_group_read_tensor "template" returns the rows the stream's next pass will use. */
typedef struct vt_refresh_stats {   /* 32 bytes */
    int32_t period; float min_score;
    int32_t generation, last_frame;      /* refreshes since init; frames_done at the last one */
    int32_t skipped_geometry; int32_t reserved[3];
} vt_refresh_stats;
int vt_set_template_refresh(vt_tracker* t, int period, float min_score);
int vt_template_refresh_stats(vt_tracker* t, vt_refresh_stats* out);
int vt_group_set_template_refresh(vt_group* g, int stream /* -1: all */, int period, float min_score);
int vt_group_template_refresh_stats(vt_group* g, int stream, vt_refresh_stats* out);

/* ---- target chips -----------------------------------------------------------------------------
 * An engine answers where the target is; a chip answers what it looks like now: a resized crop of the stream's frame at
 * the box the update committed, cut on the DEVICE behind the decode and inside the pass - full, subset, candidate and
 * pipelined passes alike - for a re-identification or classification network, an operator's thumbnail or a zoomed
 * picture-in-picture. The host neither crops 1080p frames on the CPU nor pushes pixels over the link a second time.
 * Per ENGINE, fixed by the first vt_group_enable_chips: the chip side C (a multiple of 8, 32..512) and the kind:
 *   VT_CHIP_NORM_BF16  planar [3][C][C] bf16, out = bf16(v * norm_a[c] + norm_b[c]) - the CALLER's normalisation, not the
 *                      tracker's;                                                              chip_bytes = 6 C^2
 *   VT_CHIP_RGB8       packed [C][C][3] u8, out = (uint8)min(max(rintf(v), 0), 255);           chip_bytes = 3 C^2
 * v is the crop's bilinear value: geometry, tap order and float operation order of the tracker's own crops (taps outside
 * the frame are black), with (factor, C) in place of the search crop's (4, search_size).
 * Per STREAM a policy (vt_group_set_chips): factor (0 = off, else finite in 0.5..4: the crop side is factor * sqrt(w * h)
 * of the new box), period >= 1 (at most 1,000,000) and phase in 0..period-1. The timing is stateless: a chip is due when
 * frames_done % period == phase (frames_done: the stream's updates since init, this one included).
 * After an update of the stream with result r that left the state st, a chip is cut iff ALL of:
 *   1. factor > 0 and the chip is due;   2. in a candidate pass: the slot is its stream's winner;
 *   3. the pass's search crop met no window miss (a speculative pipelined pass that will be redone cuts nothing; its redo
 *      does);
 *   4. the chip's tap rectangle at st.box lies inside the tap rectangle of the search crop the pass sampled (rule 6 of
 *      template refresh with (factor, C) in place of (2, template_size)); else status = 2 and nothing is cut;
 *   5. the in-frame part of that rectangle lies inside the window the pass's frame stores (rule 7 of template refresh: a
 *      speculative pipelined window that fails is reported as a window miss, the pass is redone with an exact window and
 *      the redo cuts the chip).
 * There is no success rule: after a failed update st.box is the last good box, the chip is cut there and info.success
 * says so. Every pass of a chip-capable engine writes the vt_chip_info of each of its streams with factor > 0 (the winner's
 * in a candidate pass), whether or not a chip is cut; the chip bytes are written only when status == 1. Where status != 1
 * the buffer holds an EARLIER cut - after a redone pipelined pass possibly that of the abandoned speculative pass -: the
 * record is what says whether the bytes are current, never the bytes. A stream with factor 0 keeps its record and its bytes untouched.
 * The first enable makes the engine chip-capable for good: it allocates the store - one chip buffer, one info and one
 * policy per stream, within vt_config.max_device_mib, else VT_ERR_OOM and nothing changes - and recaptures the engine's
 * graphs; from then on every pass carries one more launch. Engines that never enable launch what they always did.
 * Snapshots (below) carry neither the chip policy nor chips: a stream imported into an engine takes the policy its slot
 * there has. */
typedef enum vt_chip_kind { VT_CHIP_NORM_BF16 = 0, VT_CHIP_RGB8 = 1 } vt_chip_kind;
typedef struct vt_chip_info {       /* 48 bytes */
    int32_t status;                 /* 0: not due (or the pass is being redone), 1: cut by this pass, 2: due, skipped by rule 4 */
    int32_t frames_done;            /* of the update that wrote this record */
    int32_t success; float score;   /* that update's result */
    int32_t box[4];                 /* st.box: x, y, width, height the chip is (or would be) cut at */
    float geo[3];                   /* the chip crop's geometry: x0m, y0m, scale (source pixels per chip pixel) */
    int32_t reserved[1];
} vt_chip_info;
/* VT_ERR_INVALID_ARG, nothing changed: size not a multiple of 8 in 32..512, an unknown kind, a non-finite norm (bf16 kind;
 * the norms are ignored for VT_CHIP_RGB8 and may be null), a second enable with other parameters (the same: VT_OK), a
 * pipelined host pass outstanding. */
int vt_group_enable_chips(vt_group* g, int size, int kind, const float norm_a[3], const float norm_b[3]);
/* VT_ERR_INVALID_ARG, nothing changed: a bad stream, a NaN or a factor outside {0} and 0.5..4, period < 1 or above
 * 1,000,000, phase outside 0..period-1, a call before the enable, a pipelined host pass outstanding. */
int vt_group_set_chips(vt_group* g, int stream /* -1: all */, float factor, int period, int phase);
/* Chips and infos of streams[0..n) (null: streams 0..n-1) to the host: chip i at out + i * out_stride (out_stride >=
 * chip_bytes; out may be null: infos only), infos[i] (may be null). Ordered on the group's stream behind every queued
 * pass, synchronous, ONE device-to-host copy through pinned staging of the call's own (allocated on first use, outside
 * max_device_mib like the snapshot staging). */
int vt_group_read_chips(vt_group* g, const int* streams, int n, void* out, size_t out_stride, vt_chip_info* infos);
/* Device addresses of the store for a consumer on the same GPU: chip of stream s at *d_chips + s * *stride_bytes, its
 * info at (*d_infos)[s] (any out pointer may be null). ORDERING: the contents are those of the last pass once
 * vt_group_wait / vt_group_wait_next / a synchronous update has returned, and stay valid until the next enqueue of a pass
 * on this group; a consumer on another HIP stream orders itself behind that return. */
int vt_group_chips_device(vt_group* g, void** d_chips, size_t* stride_bytes, const vt_chip_info** d_infos);
int vt_enable_chip(vt_tracker* t, int size, int kind, const float norm_a[3], const float norm_b[3]);
int vt_set_chip(vt_tracker* t, float factor, int period, int phase);
int vt_read_chip(vt_tracker* t, void* out, vt_chip_info* info);

/* ---- response peaks: how close was the call ---------------------------------------------------
 * A result names the box at the Hann-weighted maximum of the score map. When a look-alike crosses the target the map has
 * two maxima of nearly equal height and the tracker jumps between them with success = 1 on both sides. An engine can list,
 * behind the decode and inside the pass - full, subset, candidate and pipelined passes alike - up to VT_PEAKS_MAX maxima of
 * each slot's map with their decoded boxes, into pinned host memory beside the pass's results: no device-to-host copy.
 * DEFINITION: the specification's decode iterated. Peak k is the decode (score, float clamped box, cell) of the slot's
 * logits with the SCORE logit of every cell (ix, iy), |ix - bx_j| <= radius and |iy - by_j| <= radius, around each earlier
 * peak j < k set to -inf (sigmoid(-inf) = 0: such a cell has response 0, is never listed and has weight 0 in a later 3x3
 * window), at the geo / frame size of the stream's state as the pass left it. resp = score * hann[cell] (one float
 * multiply). Peak 0 is the update's own decode and always listed: score, box and cell are bit-identical to vt_result.score
 * and the state's last_fbox / last_idx. Peak k >= 1 is listed while resp > 0 and resp >= min_resp (a NaN fails both);
 * responses do not increase with k, so the list ends at the first failure. Ties go to the lowest cell.
 * box = (x1, y1, width, height), the float clamped box: round with floor(v + 0.5) for what vt_result.bbox would hold, or
 * pass it to vt_candidate.box as it is to have that place evaluated as a candidate slot of the next frame.
 * Per STREAM a policy (vt_group_set_peaks) in a device array of its own, written by the host only: never rewound, not part
 * of a snapshot. max_peaks 0 = off, else 1..VT_PEAKS_MAX; radius 1..4; min_resp finite in 0..1.
 * The first call with max_peaks > 0 makes the engine peaks-capable for good: it allocates the records and policies within
 * vt_config.max_device_mib (else VT_ERR_OOM and nothing changes) and recaptures the engine's graphs; from then on every pass
 * carries one more small launch. Engines that never enable launch what they always did.
 * RECORDS are by SLOT of a pass, like results. n == 0: the slot's stream has the policy off, or the slot lost a candidate
 * pass (only winner[i] == i slots list peaks; their geo is the committed state's) - the other words of such a record are
 * not written. There is no gate on window misses: a speculative pipelined pass that will be redone writes its records like
 * its results, and the redo overwrites both. */
#define VT_PEAKS_MAX 8
typedef struct vt_peak {            /* 32 bytes */
    float score, resp;              /* sigmoid of the cell's score logit; score * hann[cell] */
    float box[4];                   /* x1, y1, width, height: the float clamped box (what last_fbox holds for peak 0) */
    int32_t cell, reserved;         /* cell = y * score_grid + x */
} vt_peak;
typedef struct vt_peaks {           /* 272 bytes */
    int32_t n, stream, frames_done, radius;   /* peaks listed; the slot's stream; the state's count after the pass; the policy's */
    vt_peak peak[8];                /* [VT_PEAKS_MAX]: peak[0..n) in listing order, zeros behind */
} vt_peaks;
/* The policy of `stream` (-1: all). VT_ERR_INVALID_ARG, nothing changed: a bad stream, max_peaks outside 0..8, radius
 * outside 1..4, min_resp NaN or outside 0..1, max_peaks = 0 before any enable, a pipelined host pass outstanding. */
int vt_group_set_peaks(vt_group* g, int stream /* -1: all */, int max_peaks, int radius, float min_resp);
/* The records of the pass whose results the last vt_group_wait / vt_group_wait_next / synchronous update returned, in
 * that pass's slot order: min(n, pass size) entries. Reads the engine's host mirror only, never the device or its stream.
 * VT_ERR_INVALID_ARG: an engine that never enabled, a null pointer, n < 1. */
int vt_group_last_peaks(vt_group* g, vt_peaks* out, int n);
int vt_set_peaks(vt_tracker* t, int max_peaks, int radius, float min_resp);
int vt_last_peaks(vt_tracker* t, vt_peaks* out);

/* ---- stream snapshots: export, import and copy a stream between engines ---------------------------
 * A stream is a box a person chose (src/selection_state.rs) plus the template cut at that box (tracker.init,
 * src/tracker_context.rs:88) - with template refresh also the product of hours of tracking. A snapshot takes that state
 * out of one slot of one engine and puts it into any slot of any engine of the same INPUT GEOMETRY: the template is rows
 * of the patch matrix (normalised pixels in bf16, in front of the patch embedding) and neither it nor the state record
 * depends on the network's weights, so a snapshot moves between engines, GPUs, processes and checkpoints. The weights are
 * deliberately not part of any check: importing into an engine that runs another checkpoint is the upgrade path.
 *
 * One self-contained little-endian byte string per stream, vt_snapshot_bytes() long:
 *   offset  size  field
 *        0     4  magic "VTSS"
 *        4     4  version "0001"
 *        8     4  u32 total_bytes    = header_bytes + state_bytes + policy_bytes + rows_bytes
 *       12     4  u32 header_bytes   = 152
 *       16     4  u32 state_bytes    = 88
 *       20     4  u32 policy_bytes   = 16
 *       24     4  u32 rows_bytes     = tokens_template * kpad * 2
 *       28     4  u32 flags          bit 0: the source engine had captured the second graph set (a stream of it was
 *                                    initialised on a format other than RGB8 / NV12 / YUY2); every other bit zero
 *       32    20  i32 patch, template_size, search_size, kpad, tokens_template
 *       52    24  f32 norm_a[3], norm_b[3]      the pixel normalisation of the weight blob's header
 *       76     4  u32 reserved, zero
 *       80     8  u64 checksum: FNV-1a-64 (offset basis 0xcbf29ce484222325, prime 0x100000001b3) over all total_bytes
 *                 bytes with these eight read as zero
 *       88    64  u32 reserved[16], zero
 *      152    88  the stream's state record, verbatim, as 22 32-bit words (vt_group_read_tensor "state"):
 *                 f32 box[4], f32 geo[4], i32 frame_w, frame_h, initialized, frames_done, success_count, last_idx,
 *                 f32 last_fbox[4], f32 last_score, i32 window_miss, generation (refreshes since init), last_frame
 *      240    16  the stream's refresh policy: i32 period, f32 min_score, i32 skipped_geometry, i32 reserved (zero);
 *                 all zero from an engine that never enabled template refresh
 *      256     -  the stream's current template rows, [tokens_template][kpad] bf16: the bits
 *                 vt_group_read_tensor "template" returns (24,576 B at template 64 / patch 16, 221,184 B at 192 / 16)
 *
 * Validation. vt_snapshot_info and vt_group_import_stream / vt_import_state return VT_ERR_FORMAT, with nothing changed
 * and the reason in vt_last_error, for: a bad magic or version; sizes that do not add up or differ from `bytes`; a
 * non-zero reserved word or flag bit; a checksum mismatch; a geometry that is not one (or, on import, differs from the
 * engine's in patch, template_size, search_size, kpad, tokens_template or the bits of the six normalisation floats); a
 * state no pass could have left (initialized != 1, a box vt_group_set_state_box would refuse, a non-finite geo,
 * last_fbox or last_score, a frame side outside 16..65536, frames_done < 0, success_count outside 0..frames_done,
 * last_idx outside the score grid, generation < 0, last_frame outside 0..frames_done, window_miss outside
 * 0..frames_done + 1); a policy vt_group_set_template_refresh would refuse (or a negative skipped_geometry, a non-zero
 * reserved word); a non-finite bf16 in the rows. */
typedef struct vt_snapshot_desc {   /* what vt_snapshot_info reports: 128 bytes */
    uint32_t total_bytes, header_bytes, state_bytes, policy_bytes, rows_bytes, flags;
    int32_t patch, template_size, search_size, kpad, tokens_template;
    float norm_a[3], norm_b[3];
    float box[4];                        /* the stream's state box: x, y, w, h in frame pixels */
    int32_t frame_width, frame_height;
    int32_t frames_done, success_count;
    float last_score;
    int32_t period; float min_score; int32_t skipped_geometry;   /* the refresh policy */
    int32_t generation, last_frame;      /* as in vt_refresh_stats */
    int32_t reserved[1];
} vt_snapshot_desc;
/* Bytes of a snapshot of a model with info's tokens_template and kpad; 0 on bad arguments. Needs no GPU. */
size_t vt_snapshot_bytes(const vt_model_info* info);
/* The same for this engine's model. */
size_t vt_group_snapshot_bytes(const vt_group* g);
/* Validate a snapshot (everything above but the comparison with an engine) and describe it. Needs no GPU, like
 * vt_scan_windows. VT_ERR_INVALID_ARG on a null pointer. */
int vt_snapshot_info(const void* buf, size_t bytes, vt_snapshot_desc* out);
/* Write stream `stream` of the group as a snapshot into buf[0..cap); *written (may be null) gets its size. The source
 * is not changed in any bit. VT_ERR_NOT_INITIALIZED for a stream that was never initialised; VT_ERR_SHORT_BUFFER if cap
 * is too small, *written is then the size needed; VT_ERR_INVALID_ARG for a bad stream index or a null buffer.
 * While pipelined host passes are outstanding: allowed for a stream that is in none of them (VT_ERR_INVALID_ARG
 * otherwise); the call waits for the device but collects nothing and leaves those passes' results as they are.
 * State, policy and the rows of the stream's current template buffer are gathered by one launch on the group's HIP stream
 * (ordered against its passes) into staging that the first snapshot call of an engine allocates: an engine that never
 * exports or imports allocates nothing and launches what it always did. A staging record is one snapshot of device and one
 * of pinned host memory; the synchronous calls share one, every queued import that has not run yet holds one. Like the
 * staging arenas of the host-frame calls they are outside the vt_config.max_device_mib accounting, which covers weights,
 * activations and the template buffers. */
int vt_group_export_stream(vt_group* g, int stream, void* buf, size_t cap, size_t* written);
/* Make stream `stream` of the group what the snapshot's stream was when it was exported: state record, refresh policy
 * (period, min_score, skipped_geometry) and template rows - into template buffer generation & 1 of a refresh-capable
 * engine, into the only buffer otherwise. The stream is initialised afterwards, whatever it was; no other stream is
 * touched. A snapshot with period >= 2 imported into an engine that never enabled template refresh enables it first, as
 * vt_group_set_template_refresh would (VT_ERR_OOM leaves nothing changed); an engine that is not refresh-capable keeps a
 * snapshot's min_score but has no place for its skipped_geometry, a diagnostic. Flag bit 0 is treated like an init on
 * a format other than RGB8 / NV12 / YUY2: the second graph set is captured inside this call if the engine has none
 * (vt_group_graph_captures); without the bit, and without a first enabling, the call captures nothing.
 * Checked in this order: null pointers and the stream index (VT_ERR_INVALID_ARG), the snapshot (VT_ERR_FORMAT).
 * With nothing outstanding the call is synchronous, like vt_group_init_device.
 * With pipelined host passes outstanding it follows vt_group_enqueue_init_host: allowed only for a stream in no
 * outstanding pass (VT_ERR_INVALID_ARG otherwise, nothing changed); the bytes go into pinned staging of the call's own
 * before it returns, their upload on the copy stream, the state and row writes on the group's stream behind the passes
 * already queued; the call does not wait for them. The stream may be listed from the next
 * vt_group_enqueue_host_streams on, its first window is exact, and a redo behind the import restores the imported
 * state (the template store is not rewound, as for a queued init). A first enabling of template refresh recaptures
 * graphs and is refused with VT_ERR_INVALID_ARG while passes are outstanding; flag bit 0 on an engine without the
 * second graph set makes this one call wait for the outstanding passes, as documented at vt_group_enqueue_init_host. */
int vt_group_import_stream(vt_group* g, int stream, const void* buf, size_t bytes);
/* Export stream s of src and import it as stream t of dst with no caller buffer; src == dst with s != t is allowed
 * (s == t is refused). Errors and ordering are those of the two calls. Engines on one GPU: device to device - the
 * record is packed behind src's stream, dst's stream waits for an event behind it and unpacks; only the 104 bytes of
 * state and policy visit the host, for dst's host-side copies. Engines on different GPUs: through the library's pinned
 * staging, the bytes of vt_group_export_stream into vt_group_import_stream; no peer access needed. The caller
 * serialises both handles. */
int vt_group_copy_stream(vt_group* src, int s, vt_group* dst, int t);
/* The same two calls on the single tracker (its group-of-one view, stream 0): checkpoint and resume of a VitTrack. */
int vt_export_state(vt_tracker* t, void* buf, size_t cap, size_t* written);
int vt_import_state(vt_tracker* t, const void* buf, size_t bytes);

/* ---- dma-buf ingest ------------------------------------------------------------------------
 * The reference's capture side can hand out dma-bufs (v4l2src io-mode=dmabuf, src/pipeline_ir.rs:24)
 * but then maps them on the CPU (src/pipeline.rs:95-101). vt_import_dmabuf maps a dma-buf fd into
 * this device's address space (hipImportExternalMemory); *d_ptr may then be used as plane0 / plane1
 * of a vt_frame with the *_device entry points: no staging copy in host memory. The fd stays owned
 * by the caller (the library imports a dup). Whether a given exporter's buffers are importable is
 * up to the amdgpu driver; an import that the driver refuses returns VT_ERR_HIP and the caller
 * falls back to the host-pointer entry points. */
typedef struct vt_extmem vt_extmem;
int vt_import_dmabuf(int device_id, int fd, size_t bytes, vt_extmem** out, void** d_ptr);
void vt_release_dmabuf(vt_extmem* m);
/* Export the head of a hipMalloc'ed allocation as a dma-buf fd: d_ptr must be the START of the allocation (the
 * handle names the allocation, and an importer maps it from its base; a pointer inside one is refused with
 * VT_ERR_INVALID_ARG), bytes a page multiple within it; the caller closes the fd. Tooling: used by the tests to
 * exercise the import path on this machine. */
int vt_export_dmabuf(int device_id, const void* d_ptr, size_t bytes, int* fd_out);

/* ---- zero-copy ingest of host frames --------------------------------------------------------------
 * The reference maps the capture buffer on the CPU (src/pipeline.rs:95-101) and hands the tracker a view
 * of the whole frame, of which the tracker samples one window. vt_host_register page-locks such a buffer
 * (typically the capture pool, once at start-up) and maps it into the device's address space
 * (hipHostRegister + hipHostGetDevicePointer): *d_ptr + offset may then be used as plane0 / plane1 of a
 * vt_frame with the *_device entry points, and the pixel kernel reads only the pixels it samples over
 * PCIe - no staging copy, no packing on the CPU, whatever the frame size. The HOST-pointer entry points
 * (vt_init_* / vt_update_* and vt_group_*_host) recognise a frame whose planes lie inside a registered range of
 * their device and MAY take the same zero-copy route by themselves (vt_config.host_zero_copy):
 *   - single-stream engines (the reference's one tracker per process) do by default: + 1 % (1,250 -> 1,264
 *     updates/s at cfg3, 1080p), and no CPU work per frame;
 *   - batched engines do NOT by default: for them the packed-window upload is faster - 60 streams in two engines,
 *     cfg3: pipelined vt_group_enqueue_host 6,891 frames/s, synchronous vt_group_update_host 6,721, zero copy 6,369
 *     (profiles/r04_bench_cfg3_60x2_final.json) - the pixel kernel's PCIe reads are latency inside the pass, the
 *     packed upload runs beside the previous pass. host_zero_copy = 1 opts a batched engine in (a host that cannot
 *     spare the CPU time for packing: 92 % of the headline rate with no per-frame CPU work), -1 opts everything out.
 * The memory stays owned by the caller; unregister before freeing it. */
int vt_host_register(int device_id, void* host_ptr, size_t bytes, void** d_ptr);
int vt_host_unregister(int device_id, void* host_ptr);

/* ---- reference colour converter on the GPU ---------------------------------------------- */

/* ≙ nv12_full_to_rgb_parallel(nv12_data, width, height) (src/nv12_convert.rs:46-92): packed NV12
 * buffer (Y plane then interleaved UV, stride == width) -> (H,W,3) RGB8. Bit-exact with the
 * reference, including the all-zero frame when len < w*h*3/2 (src/nv12_convert.rs:48-50). For odd
 * w or h the reference reads past w*h*3/2; here len must cover those reads or the call fails with
 * VT_ERR_SHORT_BUFFER. Host pointers. */
int vt_nv12_to_rgb8(int device_id, const uint8_t* nv12, size_t len, int w, int h, uint8_t* rgb_out);
/* device-pointer form (d_rgb_out: w*h*3 bytes); enqueued on hip_stream (NULL → default) */
int vt_nv12_to_rgb8_device(int device_id, const void* d_nv12, size_t len, int w, int h,
                           void* d_rgb_out, void* hip_stream);

/* n frames per launch (a host that still wants RGB for all its cameras: the reference converts every frame,
 * src/pipeline.rs:105): frame i is d_nv12[i] (packed NV12 of lens[i] bytes, as above) -> d_rgb_out[i] (w*h*3 bytes);
 * all frames w x h. d_nv12 / lens / d_rgb_out are HOST arrays of n entries holding DEVICE pointers; they are consumed
 * before the call returns. Per frame bit-exact with vt_nv12_to_rgb8_device, including the all-zero frame for
 * lens[i] < w*h*3/2; VT_ERR_SHORT_BUFFER (nothing enqueued) if some lens[i] does not cover the conversion's reads.
 * One launch per 64 frames, enqueued on hip_stream (NULL -> default). A single 1080p conversion is a 3.9-us launch
 * bounded by its ramp-up (0.29 of the HBM roof); 30 frames in one launch stream at the rate DESIGN.md section 4 gives. */
int vt_nv12_to_rgb8_batch_device(int device_id, const void* const* d_nv12, const size_t* lens, int n, int w, int h,
                                 void* const* d_rgb_out, void* hip_stream);

/* ---- overlay drawing on the GPU (the reference's per-frame overlays) --------------------------- */

/* ≙ draw_background_nv12 / draw_text_nv12 / draw_rect_nv12 / draw_crosshair_nv12
 * (src/nv12_convert.rs:172-343) and draw_cursor / draw_selection (src/drawing.rs:5-50), applied in
 * list order to the luma plane of an NV12 frame, bit-exact with the reference's CPU loops. */
typedef enum vt_draw_type {
    VT_DRAW_BACKGROUND = 0, /* x, y, w, h; value = darkness                                */
    VT_DRAW_TEXT = 1,       /* x, y; p = scale; value = brightness; text (5x7 font, 40 glyphs) */
    VT_DRAW_RECT = 2,       /* x, y, w, h; p = thickness; value = brightness                */
    VT_DRAW_CROSSHAIR = 3,  /* x, y = centre; p = size; value = brightness                  */
    VT_DRAW_CURSOR = 4,     /* x, y                                                         */
    VT_DRAW_SELECTION = 5   /* x, y = start corner; w, h = cursor corner (dashed frame)     */
} vt_draw_type;

typedef struct vt_draw_cmd {
    int32_t type;           /* vt_draw_type */
    int32_t x, y, w, h;
    int32_t p;
    int32_t value;
    char text[36];          /* NUL-terminated, VT_DRAW_TEXT only */
} vt_draw_cmd;

/* Apply n commands to a device-resident luma plane (width x height, `stride` bytes per row),
 * enqueued on hip_stream (NULL = default stream); the command list is copied before returning.
 * It draws on any 8-bit luma plane: the Y plane of I420 / YV12 / NV16 and a GRAY8 frame as well, not P010's. */
int vt_overlay_nv12_device(int device_id, void* d_y, int width, int height, int stride,
                           const vt_draw_cmd* cmds, int n, void* hip_stream);
/* Host-pointer form: draws into the packed NV12 buffer (stride == width) in place. */
int vt_overlay_nv12(int device_id, uint8_t* nv12, int width, int height, const vt_draw_cmd* cmds,
                    int n);
/* The packed-RGB8 variants the reference's live pipeline uses (src/drawing_rgb.rs:30-129,
 * src/pipeline_ir.rs:168-202): same command list; value = 0xRRGGBB for rect / crosshair, luma for
 * text; background fills with 30, cursor is (0,255,0), selection (255,255,0) as in the reference. */
int vt_overlay_rgb8_device(int device_id, void* d_rgb, int width, int height, int stride,
                           const vt_draw_cmd* cmds, int n, void* hip_stream);
int vt_overlay_rgb8(int device_id, uint8_t* rgb, int width, int height, const vt_draw_cmd* cmds,
                    int n);

/* ---- per-kernel timing and stage taps (parity tests, bench roofline) -------------------- */

typedef struct vt_kernel_time {
    char name[48];       /* kernel family, e.g. "gemm_bf16_resid" */
    int32_t launches;    /* launches of that family in one pass */
    float ms_total;      /* summed HIP-event time of those launches in one pass */
    double flops;        /* algorithmic FLOPs of those launches (0 for byte-bound kernels) */
    double bytes;        /* algorithmic bytes of those launches */
} vt_kernel_time;

/* Run `iters` eager passes over `frames` with HIP events around every launch (events on the
 * group's own stream) and return per-family averages per pass. Advances tracker state like
 * `iters` updates. Returns the number of families written (<= max_out) or a negative vt_status. */
int vt_group_profile_device(vt_group* g, const vt_frame* frames, int n, int iters,
                            vt_kernel_time* out, int max_out);

/* Stage taps: when enabled the pass runs eagerly and keeps a copy of the residual stream after the
 * patch embedding and after every encoder block (for stage-level parity tests). */
int vt_group_enable_taps(vt_group* g, int enable);
/* Engine options and diagnostics.
 *
 * ENGINE OPTIONS - the result overlay (DESIGN.md section 3 "Result overlay"). The reference draws directly behind its update
 * (src/pipeline.rs:145-172, src/pipeline_ir.rs:182-202): a rectangle of thickness 3 at the new box, a crosshair of size 15 at
 * its centre, the text "score: NN%". With these keys a pass does that itself, as its LAST launch, for every slot at once.
 * The policy is per engine (a single tracker: through vt_tracker_as_group):
 *   key                              value                                                         default (a negative value selects it)
 *   "result_overlay"                 flags: 1 rectangle | 2 crosshair | 4 score label; 0 = off     0
 *   "result_overlay_style"           thickness | size << 8 | scale << 16: rectangle thickness       3, 15, 2 (the reference's)
 *                                    1..16, crosshair size 1..64, text scale 1..4
 *   "result_overlay_luma"            0..255: brightness on luma surfaces, of the text everywhere    255
 *   "result_overlay_rgb"             0..0xFFFFFF: rectangle and crosshair on packed-RGB surfaces    0x00FF00 (src/pipeline_ir.rs:195)
 *   "result_overlay_min_score_pct"   0..100: the score gate                                         25 (src/tracker_context.rs: score > 0.25)
 * A value outside its range returns VT_ERR_INVALID_ARG and changes nothing. A style, colour or gate value set before the
 * engine is overlay-capable is remembered. The first non-zero "result_overlay" makes the engine overlay-capable for good
 * (records within max_device_mib, else VT_ERR_OOM and nothing changes; the captured passes are captured again, here): from
 * then on every pass carries one more launch. Engines that never enable launch exactly what they always did. Later
 * changes of any of the keys, flags 0 included, are one small copy and capture nothing.
 *   A slot draws iff ALL of: (1) the flags are non-zero; (2) the pass received its frames through a device entry point -
 * vt_group_update_device*, vt_group_enqueue_device*, vt_group_update_device_candidates, vt_update_*_device, vt_update_frame
 * with on_device == 1, vt_group_profile_device; host-pointer passes never draw, the zero-copy route included (their frames
 * are the library's staging or the caller's host memory); (3) in a candidate pass the slot is its stream's winner;
 * (4) r.success != 0 and r.score > (float)pct / 100.0f (a NaN fails); (5) the frame's format is drawable: every format but
 * P010, which is counted instead.
 *   What is drawn, with b = r.bbox: the frame's bytes after the pass are those this vt_draw_cmd list leaves, applied in this
 * order to the frame before the pass - flag 1: VT_DRAW_RECT {x = b.x, y = b.y, w = b.width, h = b.height, p = thickness};
 * flag 2: VT_DRAW_CROSSHAIR {x = b.x + b.width / 2, y = b.y + b.height / 2, p = size} (C integer division, as in the
 * reference); flag 4: VT_DRAW_TEXT "score: N%", N = clamp((int)rintf(r.score * 100.0f), 0, 100) (one binary32 multiply,
 * ties to even), p = scale, x = max(b.x, 0), y = b.y - 7 * scale - 4 if that is >= 0, else b.y + b.height + 4.
 *   Surfaces. LUMA: the Y plane of NV12 / NV21 / I420 / YV12 / NV16, the Y bytes of YUY2 / UYVY, and GRAY8 - the semantics
 * of vt_overlay_nv12_device (its usize quirks included), every value the luma key, chroma never touched. PACKED RGB: RGB8 /
 * BGR8 / RGBX / BGRX / XRGB / XBGR - the semantics of vt_overlay_rgb8_device on the RGB8 sibling, rectangle and crosshair in
 * the rgb key, the text in the luma key as r = g = b, the pad byte never written. W and H of the predicates are the FULL
 * frame's; of a windowed frame (origin_*, windowed, window_w / window_h) only pixels inside the stored window are written,
 * at their address in that window. No store ever leaves the stored window.
 *   Several slots on one frame (several targets per camera; candidate slots): slots whose vt_frame are field-for-field equal
 * draw as if their lists were concatenated in slot order - where shapes overlap, the higher slot's pixel stands. Slots whose
 * descriptors differ but alias the same memory have an UNDEFINED order where their shapes overlap.
 *   Ordering: the overlay runs behind the candidate commit, the template refresh, the target chips and the response peaks
 * of the same pass, so a refreshed template and a chip are cut from UNDRAWN pixels. The frame is complete when vt_group_wait,
 * vt_group_wait_next or the synchronous call returns. THE CALLER'S NEW RULE: on an overlay-enabled engine a device pass
 * WRITES the frames it is given, although vt_frame's pointers are const - hand it memory that may be written, and do not
 * read the frame concurrently with the pass.
 *   Read-out: vt_group_read_tensor(g, stream, "result_overlay", ...). Not part of a stream snapshot (policy and counters).
 *
 * ENGINE OPTIONS - the motion prior (DESIGN.md section 3 "Motion prior"). A stream's search window is cut around its last
 * accepted box (side 4*sqrt(w*h)): a target that moves more than about 1.5 box sides between two updates of its stream - a
 * fast target, a panning gimbal, a camera served every n-th frame through a subset pass - leaves it, and every later update
 * fails in the same place (above vt_candidate). With these keys every pass first moves each of its streams' boxes by a
 * per-stream velocity estimate kept on the device, so the window is cut where the target is heading, and keeps the box
 * moving through a few failed updates (coasting through a short occlusion). The policy is per engine:
 *   key                 value                                                                    default (a negative value selects it)
 *   "motion_prior"      0 = off, 1 = on                                                          0
 *   "motion_gain_pct"   1..100: weight of the newest displacement in the velocity                 50
 *   "motion_coast"      0..60: failed updates through which the box keeps advancing               5
 *   "motion_max_pct"    0..200: per-axis limit of the velocity, percent of sqrt(w*h) of the new box  100
 * A value outside its range returns VT_ERR_INVALID_ARG and changes nothing. A value set before the engine is motion-capable
 * is remembered. The first non-zero "motion_prior" makes the engine motion-capable for good (records within max_device_mib,
 * else VT_ERR_OOM and nothing changes; the captured passes are captured again, here): from then on every pass - full,
 * subset, candidate, synchronous and pipelined host, vt_group_profile_device - carries two more launches. Engines that
 * never enable launch exactly what they always did. Later changes of any key are one small copy and capture nothing;
 * "motion_prior" 0 also zeroes every stream's record, and while it is 0 the two launches leave velocities, live counts
 * and counters alone.
 *   THE RULE. All arithmetic is binary32, every operation rounded on its own. Per stream a record (device memory, mirrored
 * to pinned host memory beside the states; no part of the 88-byte state, of a snapshot or of vt_snapshot_bytes): v[2],
 * prior[4], shift[2], live, two counters. It is zeroed by vt_group_init_*, vt_group_enqueue_init_host,
 * vt_group_set_state_box, vt_group_import_stream, vt_import_state, and on the destination of vt_group_copy_stream.
 *   PLACE - the first launch of a pass, per listed initialised stream with state box b = (x, y, w, h): (1) prior = b,
 * shift = 0. (2) If the flag is on and v != (0, 0): px = x + vx, py = y + vy, cx = px + 0.5f*w, cy = py + 0.5f*h; if
 * 0 <= cx < (float)frame_w and 0 <= cy < (float)frame_h (the state's frame size) the state box becomes (px, py, w, h) and
 * shift = v; otherwise v = 0, live = 0 and the box stays. Crop, decode, candidate fill, refresh, chips, peaks and overlay
 * read the state as they always did. In a candidate pass a has_box == 0 slot is therefore cut around the predicted box, a
 * has_box == 1 slot around its own.
 *   SETTLE - one launch directly behind the decode (candidate pass: behind the commit), ahead of refresh, chips, peaks and
 * overlay, per stream of the pass with its final result r and state box b' (candidate pass: the winner's; losing slots
 * leave no trace). Success, and the winning slot was cut around the stream's own box (every pass but a has_box == 1
 * winner): c_old = (prior.x + 0.5f*prior.w, prior.y + 0.5f*prior.h), c_new the same of b', d = c_new - c_old,
 * a = (float)gain_pct / 100.0f, v = v + a*(d - v) (a subtract, a multiply, an add per axis),
 * lim = ((float)max_pct / 100.0f) * sqrtf(b'.w * b'.h), v = fminf(fmaxf(v, -lim), lim), live = coast. Success with a
 * has_box == 1 winner (the caller placed it: the jump is no motion): v = 0, live = coast. Failure (r.success == 0; a NaN
 * score fails): if live > 0, live -= 1 and the state box stays the shifted one - the box coasts (counted when
 * shift != 0); otherwise the state box becomes prior and v = 0. The final box and the record also go to the pinned mirrors.
 *   CONSEQUENCE: on a motion-enabled engine a failed update may leave the state box advanced by v. frames_done,
 * success_count and everything else are untouched. THE TWIN IDENTITY: such an engine behaves, bit for bit (results, state
 * words, templates, chips, peaks), like a plain engine whose host calls vt_group_set_state_box(stream, prior + shift)
 * before every pass in which shift != 0 and vt_group_set_state_box(stream, prior) after a failure that restores.
 *   Host passes plan their windows around the predicted box, computed by the host from the mirrored record with the same
 * operations: an exact window stays exact. A speculative window (vt_group_enqueue_host: the stream is in the pass still
 * running) is planned around the known box moved by the known velocity - once for the pass still running, once for this one:
 * where a target at constant velocity will be - then enlarged by the margin; a miss takes the redo path, and the records
 * rewind and commit with the states they belong to. Pipelined runs stay bit-identical to the
 * synchronous calls.
 *   Read-out: vt_group_read_tensor(g, stream, "motion", ...).
 *
 * ENGINE OPTIONS - the appearance check (DESIGN.md section 3 "Appearance check"). A centre-head tracker that has slid onto a
 * look-alike keeps returning success with a high score, and a template refresh would cut the look-alike into the template.
 * With these keys every pass compares what is inside each stream's new box with what the stream was started from: the
 * zero-mean normalised correlation of two template-sized crops, in the pixel domain, reported per stream and - with a
 * gate - required of a refresh. The policy is per engine:
 *   key                   value                                                                  default (a negative value selects it)
 *   "appearance"          0 = off, 1 = on                                                        0
 *   "appearance_period"   1..1,000,000: evaluated when frames_done % period == 0                 1
 *   "appearance_gate_pm"  0..1000 per mille; 0 = report only; tau = (float)pm / 1000.0f          0
 *   "appearance_anchor"   ACTION: a stream index, or -1 for every initialised stream (any other negative value is
 *                         invalid): the stream's anchor <- its CURRENT template rows, its record zeroed
 * A value outside its range returns VT_ERR_INVALID_ARG and changes nothing. A period or gate set before the engine is
 * appearance-capable is remembered; the action needs a capable engine (else VT_ERR_INVALID_ARG) and an initialised stream
 * (VT_ERR_NOT_INITIALIZED). The first non-zero "appearance" makes the engine appearance-capable for good: per stream an
 * anchor and a probe of [Nt][Kpad] bf16, a record, counters and the reduction's partials, within max_device_mib, else
 * VT_ERR_OOM and nothing changes; the anchors of the streams that are initialised are filled from their current template
 * rows; the captured passes are captured again, here. From then on every pass - full, subset, candidate, synchronous and
 * pipelined host, vt_group_profile_device - carries two more launches; engines that never enable launch exactly what they
 * always did. Later changes of any key are one small copy and capture nothing.
 *   THE ANCHOR of a stream holds the rows vt_group_read_tensor "template" returned at the moment it was set: by
 * vt_group_init_* and vt_group_enqueue_init_host (the init's rows; the queued init on the group's stream, behind the
 * queued passes), by vt_group_import_stream, vt_import_state and on the destination of vt_group_copy_stream (the imported
 * rows), by the enable and by the action. A template refresh never writes it. It is no part of a snapshot (format 0001).
 *   THE RULE, per slot i of a pass, behind the decode (candidate pass: behind the commit) and the motion prior's settle
 * launch, ahead of refresh, chips, peaks and overlay (the probe is cut from undrawn pixels), with s the slot's stream,
 * st its state as the pass left it and r = results[i]. The slot is DUE iff ALL of: (a) "appearance" is 1; (b) in a
 * candidate pass winner[i] == i; (c) r.success != 0; (d) st.window_miss != st.frames_done; (e) st.frames_done % period == 0,
 * OR tau > 0 and rules 1, 3 and 4 of vt_group_set_template_refresh hold for s (a refresh that the gate has to judge in
 * this pass). A due slot applies refresh rules 6 and 7 unchanged: where rule 6 fails the record's status is 2; where rule
 * 7 fails the pass is marked a window miss (st.window_miss = st.frames_done, record status 0), so a speculative pipelined
 * pass is redone with an exact window and the redo evaluates. A passing slot cuts the PROBE: the crop of its frame at
 * st.box, factor 2, side template_size - bit for bit the template rows vt_group_init_*(s, that frame, r.bbox) would write.
 *   THE SCORE, over the first 3 * patch * patch columns of the Nt rows (pad columns are never read), a = anchor, p = probe,
 * every element the exact value of its bf16, in binary64: Sa = sum a, Sp = sum p, Saa = sum a*a, Spp = sum p*p,
 * Sap = sum a*p, n the element count; cov = Sap - Sa*Sp/n, va = Saa - Sa*Sa/n, vp = Spp - Sp*Sp/n;
 * sim = (va > 0 && vp > 0) ? cov / sqrt(va * vp) : 0, clamped to [-1, 1] and rounded once to binary32; status 1, or 3 when a
 * variance is not positive. The order of the additions is fixed (csrc/k_appearance.hip) and no floating-point atomic is
 * used: the record is a function of the inputs alone, and pipelined runs equal synchronous ones bit for bit.
 *   THE RECORD, per stream, on the device and mirrored to pinned host memory: status (0 = not due or not evaluated, 1, 2,
 * 3), frames_done, similarity, box[4]. Every pass writes the records of its streams (a candidate pass: at the winning slot).
 * Two diagnostic counters per stream, `evaluated` (records with status 1 or 3) and `gated`; like skipped_geometry they are
 * never rewound and may count a redone pass twice.
 *   REFRESH RULE 8. With "appearance" 1 and tau > 0 a refresh that rules 1-7 of vt_group_set_template_refresh allow
 * additionally needs THIS pass's record of the stream to have status 1 and similarity >= tau. Otherwise nothing is cut, gated += 1, and the
 * refresh is tried again at the stream's next update. With tau == 0, with "appearance" 0 (switching the check off switches
 * its gate off: no refresh is held back by records nobody writes), and on engines that never enabled the check, the
 * refresh behaves bit for bit as before. THE TWIN IDENTITY: an enabled engine with gate 0 equals a plain engine in results,
 * state words and templates, bit for bit - with ONE exception: where a due slot fails rule 7 the probe launch sets
 * st.window_miss = st.frames_done, as the refresh and chip launches do in that place. Whole frames and the library's own
 * exact windows never fail rule 7, and a speculative pipelined pass that does is redone, after which the state is the
 * plain engine's again; but a DEVICE pass on a caller-windowed frame (vt_frame.windowed, origin_*) whose window holds the
 * search crop's taps and not all of the template crop's is not redone by anybody: there the enabled engine differs from a
 * plain one in that one state word (and a following refresh or chip of the same pass, seeing the miss, does not cut).
 *   Read-out: vt_group_read_tensor(g, stream, "appearance" / "anchor" / "probe", ...).
 *
 * ENGINE OPTIONS - reacquire proposals (DESIGN.md section 3 "Reacquire proposals"). The engine can say that a target is lost,
 * not where it went: peaks, motion prior and appearance check all work inside one search window. With this option every
 * DEVICE pass slides each due stream's own template, pooled to an M x M pattern, over a coarse thumbnail of the WHOLE frame
 * and lists the best places as boxes of the stream's size - candidates for ONE vt_group_update_device_candidates pass in
 * front of the vt_scan_windows scan. Keys, per engine; a negative value selects the default; a value outside its range
 * returns VT_ERR_INVALID_ARG and changes nothing:
 *   key                      value                                                                 default
 *   "proposals"              0 = off, 1 = evaluate slots whose update failed, 2 = every update     0
 *   "proposals_period"       1..1,000,000: due when frames_done % period == 0                      1
 *   "proposals_max"          1..8 proposals listed                                                 4
 *   "proposals_min_sim_pm"   0..1000 per mille; tau = (float)pm / 1000.0f                          500
 *   "proposals_max_cells"    16,384..4,194,304 cells of thumbnail storage per slot; accepted only  262,144
 *                            before the first enable, VT_ERR_INVALID_ARG afterwards
 * Values set before the first enable are remembered. The first non-zero "proposals" makes the engine proposals-capable
 * for good: per slot an int16 thumbnail and a float32 similarity map of max_cells each, a 16 x 16 int16 pattern and a
 * header, per stream a record, a counter and the record's pinned mirror (6 bytes per cell and slot; VT_ERR_OOM under
 * vt_config.max_device_mib or when the device is full, and nothing changes; VT_ERR_INVALID_ARG where the model's template
 * size is a multiple of neither 16 nor 14), the passes captured again in that call with four more launches behind the
 * decode (the commit, motion_settle, the appearance launches), AHEAD of the refresh, chip, peaks and overlay launches.
 * Later changes of any key are one small copy and capture nothing. No part of a snapshot.
 *   THE RULE, to the bit. All arithmetic binary32 unless stated, one IEEE operation per source operation. Slot i of a
 * pass, st the state of its stream as the pass left it, r = results[i], f its frame. The slot is DUE iff ALL of: (a)
 * "proposals" != 0; (b) in a candidate pass, winner[i] == i; (c) mode 1: r.success == 0 (a NaN score fails), mode 2:
 * always; (d) st.frames_done % period == 0. A slot that is not due has status 0. A due slot has status 4, with nothing
 * evaluated, unless (e) the pass came through a device entry point (rule 2 of the result overlay: host-pointer passes, zero
 * copy included, have only their windows on the device) and (f) its planes hold the whole frame: origin 0,0 and a stored
 * extent equal to the frame's (vt_frame.windowed == 0, or a window that is the frame).
 *   Geometry, (x, y, w, h) = st.box: s = sqrtf(w * h); M = 16 if template_size % 16 == 0, else 14; c = 2.0f * s / (float)M,
 * the cell side in source pixels (the pattern is the WHOLE factor-2 template); the grid starts at X0 = Y0 =
 * -(float)(M / 4) * c: a match window may hang a quarter of its side outside the frame, a target may touch the edge; Wg =
 * (int)ceilf((float)frame_w / c) + M / 2, Hg likewise. Status 2, nothing evaluated, if c is not positive (a NaN too), if
 * either quotient exceeds 4,194,304, if Wg * Hg > max_cells, or if Wg < M or Hg < M.
 *   Thumbnail cell (i, j): sixteen sub-taps (u, v), u, v in 0..3, at px = (int)floorf(X0 + ((float)i + ((float)u + 0.5f) *
 * 0.25f) * c), py alike with j and v; each is ONE pixel of the frame as the crop kernels read it (any vt_pixfmt /
 * vt_pixfmt2), black outside the frame; g = (R * a0 + b0) + (G * a1 + b1) + (B * a2 + b2) with the blob's norm_a /
 * norm_b; the cell is the sum of its 16 g, added in (v, u) order from 0.0f; Q = clamp(rintf(sum * (4096.0f / 48.0f)),
 * -32767, 32767) as int16 (clamped in binary32: it saturates, it never wraps). A cell with ANY sub-tap outside the frame
 * is OUTSIDE and stored as -32768, which no value clamps to: what is not in the picture is no evidence for or against a
 * place, and such cells take part in no sum below (the cells of a frame edge that the frame only partly covers included).
 *   Pattern cell: the (T / M)^2 pixels x 3 channels of its block of the stream's CURRENT template rows - what "template"
 * returned before the pass: the template the pass ran on, the launches sit ahead of the refresh launch - each the exact
 * value of its bf16, added in binary64 in ascending (y, x, channel) order, times 4096.0 / (3 (T / M)^2), rint, clamped
 * to +-32767, int16. Status 3 if the WHOLE pattern is flat: M^2 Saa - Sa^2 == 0 over all its cells.
 *   Similarity at every position (px, py), 0 <= px <= Wg - M, 0 <= py <= Hg - M, from EXACT int64 sums over those cells
 * of the M x M window of the thumbnail that are not OUTSIDE, and over the pattern's cells at the same places: n their
 * number (at least 9/16 of M^2 wherever the grid's overhang of M / 4 cells is all that leaves the frame), Sa, Saa the
 * pattern's sums over them, Sp, Spp, Sap the window's; cov = n Sap - Sa Sp, va = n Saa - Sa^2, vp = n Spp - Sp^2 (all below
 * 2^53); sim = (va > 0 && vp > 0) ? (double)cov / sqrt((double)va * (double)vp) : 0, clamped to [-1, 1], rounded once to
 * binary32. A window wholly inside the frame uses the whole pattern. Integer sums: the result does not depend on any
 * order of additions, and there is no floating-point atomic. (Comparing the overhang with black instead makes frame
 * corners look like a dark ring around a brighter centre: 0.51 on the committed clip, where no other place exceeds 0.23.)
 *   Listing: proposal k is the greatest sim among the positions not suppressed, the lowest py * (Wg - M + 1) + px on a
 * tie; listed while k < proposals_max, sim >= tau and sim > 0; positions within Chebyshev distance M / 2 of a listed one
 * are suppressed. Its box: (cx - 0.5f * w, cy - 0.5f * h, w, h), cx = X0 + (float)(px + M / 2) * c, cy alike.
 *   Record, per stream, on the device and mirrored to pinned host memory like the appearance records: status, frames_done,
 * n, c, Wg, Hg, and per proposal sim, box[4], position. Every pass of a capable engine writes the records of its streams
 * (a candidate pass: at the winning slot; a redone pass again). A counter per stream counts the records written with
 * status 1 or 3 (a diagnostic, never rewound). THE TWIN IDENTITY: the option only reads - an enabled engine equals a plain
 * engine in results, state words, templates, chips, peaks and overlays, bit for bit, in every kind of pass; it marks no
 * window miss and adds no redo.
 *   Read-out: vt_group_read_tensor(g, stream, "proposals" / "proposals_pattern" / "proposals_map", ...).
 *
 * ENGINE OPTIONS - stream conflicts (DESIGN.md section 3 "Stream conflicts"). Every other option looks at one stream in
 * isolation. Streams of one picture that slide onto the same target, or whose targets cross, each keep success = 1, and a
 * template refresh then cuts the other target into the template. With these keys every pass records, per stream, which
 * other streams of the same SCENE overlap its new box and by how much, and - with the gate - keeps a conflicting stream
 * from refreshing its template. Keys, per engine; a negative value selects the default; a value outside its range returns
 * VT_ERR_INVALID_ARG and changes nothing:
 *   key                  value                                                                   default
 *   "conflicts"          0 = off, 1 = on                                                         0
 *   "conflicts_iou_pm"   1..1000 per mille; tau = (float)pm / 1000.0f                            300
 *   "conflicts_gate"     0 = report only, 1 = refresh rule 9                                     0
 *   "conflicts_scene"    ACTION: value >= 0: stream (value & 0xFFFF) goes to scene (value >> 16), stream 0xFFFF = every
 *                        stream; -1: every stream back to scene 0. Any other stream or value: VT_ERR_INVALID_ARG
 * SCENES. The device cannot tell which slots show the same picture (a host-pointer pass hands it staged windows only), so
 * the host says so: every stream has a scene number, an int32 in 0..65535 (the packed value of the key reaches 0..32767).
 * Scene 0, the default, means "compared with nobody". Scenes are policy, not stream state: they live in the option's store,
 * survive vt_group_init_*, import and copy, and are no part of a snapshot (format 0001, vt_snapshot_bytes unchanged). The
 * action needs a capable engine (else VT_ERR_INVALID_ARG); it waits for the group's stream, writes the scene words and
 * zeroes the records of the streams it names. Values of the other keys set before the first enable are remembered.
 * The first non-zero "conflicts" makes the engine conflicts-capable for good: one store - the policy, per stream a scene, a
 * 48-byte record and four counters - and the records' pinned mirror, within max_device_mib, else VT_ERR_OOM and nothing
 * changes; the captured passes are captured again, here. From then on every pass - full, subset, candidate, synchronous and
 * pipelined host, vt_group_profile_device - carries ONE more launch; engines that never enable launch exactly what they
 * always did. Later changes of any key are one small copy and capture nothing.
 *   THE RULE, to the bit. One launch directly behind the decode (candidate pass: behind the commit) and the motion prior's
 * settle launch, ahead of the appearance, proposals, refresh, chip, peaks and overlay launches; it reads device memory only.
 * With "conflicts" 0 it leaves at once and writes nothing. Otherwise, per stream s of the pass (a candidate pass: at its
 * winning slot; losing slots leave no trace), st its state as the pass left it and r its final result: s is ELIGIBLE iff ALL
 * of: (a) scene[s] != 0; (b) st.initialized != 0; (c) r.success != 0; (d) st.window_miss != st.frames_done. A stream that is
 * not eligible gets the record {status 3, st.frames_done, n_over 0, partner -1, iou 0} and is nobody's partner. An eligible
 * s with (x, y, w, h) = st.box is compared with every other eligible stream t OF THE SAME PASS with scene[t] == scene[s]:
 * streams that are not in the pass are never read, so a record is a function of one pass alone and a redone pipelined pass
 * recomputes it whole. Every operation a binary32 operation rounded on its own:
 *   ix = fminf(x_s + w_s, x_t + w_t) - fmaxf(x_s, x_t), iy likewise; if !(ix > 0 && iy > 0) the pair has IoU 0 and is not
 *   listed; else inter = ix * iy, uni = (w_s * h_s + w_t * h_t) - inter, iou = inter / uni (correctly rounded);
 * iou(s, t) and iou(t, s) are the same bits. t is OVER iff iou >= tau; n_over counts them; partner[] / iou[] hold the up
 * to 4 largest by (iou descending, stream index ascending) - the stream index, not the slot, breaks ties, so the order of
 * a subset pass's list changes no record -, unused entries partner = -1, iou = 0. status = n_over > 0 ? 2 : 1.
 *   THE RECORD, per stream, on the device and mirrored to pinned host memory like the appearance records: status (0 = no pass
 * wrote it, 1, 2, 3), frames_done, n_over, a reserved word, partner[4], iou[4]. It is zeroed by vt_group_init_*,
 * vt_group_enqueue_init_host, vt_group_set_state_box, vt_group_import_stream, vt_import_state, on the destination of
 * vt_group_copy_stream and by the scene action; a stream that was not in a pass keeps its record. Three diagnostic counters
 * per stream: `evaluated` (records with status 1 or 2), `conflicting` (status 2) and `gated`; like skipped_geometry they
 * are never rewound and may count a redone pass twice.
 *   REFRESH RULE 9. With "conflicts" 1 and "conflicts_gate" 1, a refresh that rules 1-5 of vt_group_set_template_refresh
 * allow is suppressed, and gated += 1, where THIS pass's record of the stream (frames_done == st.frames_done) has status 2.
 * The rule is checked ahead of rules 6, 7 and 8: a gated refresh counts no geometry skip and sets no window-miss mark, and
 * it is tried again at the stream's next update. Switching the flag or the gate off switches the rule off; the appearance
 * probe's own due rule is unchanged. THE TWIN IDENTITY: with gate 0 the option only reads - an enabled engine equals a plain
 * engine in results, state words, templates, chips, peaks, records of the other options and overlays, bit for bit, in every
 * kind of pass.
 *   Read-out: vt_group_read_tensor(g, stream, "conflicts", ...).
 *
 * FRAME HEALTH (csrc/k_health.hip; the rule to the bit: include/vittrack_hip_ops.h, vt_op_frame_health):
 * every option above judges the target, this one the picture - a frozen feed, a covered or blacked-out lens and a cut to
 * another scene all look like ordinary updates. Keys (a negative value selects the default):
 *   "health"             0 = off, 1 = on                                                         0
 *   "health_period"      1..1,000,000: a stream is due when frames_done % period == 0            1
 *   "health_cell"        0 = automatic, or 4, 8, 16, 32: the thumbnail cell in source pixels     0
 *   "health_still_run"   1..1000: FROZEN at this many identical comparisons in a row             3
 *   "health_flat_q"      0..4080: FLAT at a standard deviation of the thumbnail <= this          32
 *   "health_cut_pm"      0..1000 per mille of the cells in another histogram bin: CUT; 0 never   500
 *   "health_gate"        0 = report only, 1 = refresh rule 10                                    0
 *   "health_max_cells"   4,096..262,144 thumbnail cells per stream; fixed by the first enable    65,536
 * The first non-zero "health" makes the engine health-capable for good: one store - the policy, per stream a record, three
 * counters, four accumulators, two histograms and two uint16 thumbnails of max_cells -, a pinned mirror of the records, the
 * graphs captured again with four launches directly behind the decode (the commit, conflicts_check) and ahead of the
 * appearance, proposals, refresh, chip, peak and overlay launches (the thumbnail is taken from undrawn pixels) in EVERY
 * kind of pass. Per due stream of a pass whose frame is a whole frame in device memory: a thumbnail t (camera motion's
 * cell: sixteen integer luma taps), S1 = sum t, S2 = sum t * t, G = the absolute differences of horizontal and vertical
 * neighbours, a 32-bin histogram of t >> 7, and against the stream's previous thumbnail of the same geometry D = sum |t - p|
 * and HD = sum |hist - hist_p|. Status: 0 not due (the record, the previous thumbnail and the counters stay), 4 no whole
 * device frame (every host-pointer pass), 2 no geometry, 5 measured without a comparable previous thumbnail, 1 measured and
 * compared. Flags: 1 FROZEN (status 1, D == 0 in still_run comparisons in a row), 2 FLAT (n * S2 - S1 * S1 <= flat_q^2 * n^2),
 * 4 CUT (status 1, HD * 1000 >= cut_pm * 2 * n). Integers only: a pipelined run equals a synchronous one. vt_group_init_*,
 * an import and the destination of a copy clear the stream's previous thumbnail and record; "health" 0 clears every
 * stream's; no part of a snapshot.
 *   REFRESH RULE 10. With "health" 1 and "health_gate" 1, a refresh that rules 1-5 and rule 9 allow is not made when the
 * stream's record of THIS pass has flags != 0: nothing is cut, the stream's gated counter grows, no geometry skip is counted
 * and no window miss is marked; it is tried again at the next update. THE TWIN IDENTITY: with gate 0 the option only
 * reads - an enabled engine equals a plain engine in results, state words, templates, chips, peaks and overlays, bit for
 * bit, in every kind of pass.
 *   Read-out: vt_group_read_tensor(g, stream, "health" / "health_words", ...).
 *
 * PEAK ARBITRATION (csrc/k_arbitrate.hip; the rule to the bit: include/vittrack_hip_ops.h, vt_op_arbitrate; DESIGN.md section
 * 3): the options above report or gate; this one changes which box a pass commits. Where the box the decode committed (peak 0
 * of the response map) no longer looks like the stream's anchor and a runner-up peak does, the runner-up is committed instead.
 * Keys (a negative value selects the default):
 *   "arbitrate"             0 = off, 1 = on                                                      0
 *   "arbitrate_max"         2..4 peaks examined, peak 0 included                                 3
 *   "arbitrate_radius"      1..4: suppression radius of the iteration (as vt_group_set_peaks)    2
 *   "arbitrate_min_resp_pm" 0..1000: a runner-up needs response > 0 and >= pm / 1000             50
 *   "arbitrate_low_pm"      0..1000: peak 0 is challenged only while its similarity is below     300
 *                           pm / 1000; 0: never challenged (1 challenges every similarity below
 *                           0.001, the negative ones included: the step lies between 0 and 1)
 *   "arbitrate_high_pm"     0..1000: a runner-up must reach this similarity                      500
 * Each threshold is (float)pm / 1000.0f, one binary32 divide. The first non-zero "arbitrate" is refused
 * (VT_ERR_INVALID_ARG) unless the engine is appearance-capable: the anchors are the appearance store's. It makes the engine
 * arbitration-capable for good: one store - the policy, per stream a record, two counters and four probes of template rows -,
 * a pinned mirror of the records, the graphs captured again with four launches directly behind the decode (a candidate
 * pass: the commit) and ahead of motion_settle in EVERY kind of pass, so that everything that reads the new box - the
 * settle's velocity, conflicts, health, the appearance record, refresh rule 8, chips, peaks, the overlay - reads the final
 * one. It neither needs nor touches the response-peaks option. A slot is due when the flag is on, the pass is no candidate
 * pass, result.success is set, window_miss != frames_done, and at least one runner-up k >= 1 is eligible: its score >= the
 * model's success threshold and its integer box (floorf(v + 0.5f) of the four floats, as the decode rounds) passes refresh
 * rule 6. Per listed, eligible peak - peak 0 included - the template-sized crop at its integer box is scored against the
 * stream's anchor with the appearance check's sums. With sim[k] the similarity of peak k: a switch requires sim[0] < low and
 * some eligible k >= 1 with sim[k] >= high. The chosen peak is the one with the largest similarity; on a tie, the lowest k.
 * On a switch the result becomes success 1, the peak's score and integer box, and the state's last_fbox, last_score, last_idx
 * and box become the peak's, on the device and in the host's copies: exactly what the decode would have written had that peak
 * been the argmax. frames_done and success_count stay as the decode left them. Record status: 0 not due, 1 kept, 2 switched,
 * 3 candidate pass (nothing is arbitrated there), 4 refresh rule 6 failed at peak 0, 5 refresh rule 7 failed at an examined
 * peak - the pass is marked a window miss and nothing else happens: the host's redo with an exact window decides, so a
 * pipelined run equals a synchronous one. vt_group_init_*, an import and the destination of a copy zero the stream's record;
 * "arbitrate" 0 zeroes every stream's; no part of a snapshot. "arbitrate_low_pm" 0 challenges nobody, a negative similarity
 * included: the engine equals one without the option, bit for bit.
 *   Read-out: vt_group_read_tensor(g, stream, "arbitrate", ...).
 *
 * DIAGNOSTICS (A/B measurements and parity tests of alternative kernels; results are the same quantity either
 * way): key "head_band": 2 (default; any negative value selects it) = the head's convolutions on the band kernel, the
 * final LayerNorm inside the first layer's launch and the logits and the decode behind the last layer's, 1 = the same
 * with the LayerNorm as a launch of its own, 0 = implicit GEMMs + head_out + decode launches; key "crop_tier": >= 0 forces the crop
 * kernel's LDS buffer tier (0: 16 KiB, 1: 32 KiB, 2: 64 KiB), < 0 (default) = chosen per pass from the boxes the host
 * knows; key "last_rows": 1 (default; any negative value selects it) = the last encoder block computes the search rows only
 * where the pass is eligible - no taps, the attention kernel of the hot path, enough streams in the pass for the compacted
 * projection to stay on the 256x256 GEMM kernel (19 of ViT-B/16 at search 384) - 0 = every pass runs all rows. Results, "feat",
 * "head_out" and the states are the same bits either way; "last_block_rows" of vt_group_read_tensor says what the last pass
 * did. Every diagnostic key drops the captured passes and captures them again here. No key - option or diagnostic - while
 * a pipelined pass is outstanding. */
int vt_group_set_tuning(vt_group* g, const char* key, int value);
/* A single tracker viewed as a group of one (taps, profiling, stream handle). The view belongs to
 * the tracker: valid until vt_destroy(t), the same pointer on every call, never to be destroyed
 * by the caller. */
vt_group* vt_tracker_as_group(vt_tracker* t);

/* Overwrite the box the next update of `stream` crops its search window around (x, y, w, h in frame
 * pixels). Tooling hook: lets a caller evaluate the network on a window of its choosing (head
 * training data, stage tests) while keeping the template set by vt_group_init_device. */
int vt_group_set_state_box(vt_group* g, int stream, const float* box4);

/* Copy an intermediate tensor of the last pass to the host as float32.
 * names: "patches" [N,Kpad], "tokens0" [N,D], "layer<i>" [N,D] (residual stream after block i;
 * both need taps), "x" [N,D] (final residual stream; like the taps the value of the 3-byte pair it is stored
 * as: bf16 + a signed byte in units of 2^-s, s the lo_shift of the weight blob's header int 12: 0 = 12, else 6..14),
 * "xrange" [stages,12] (range report of the stream's stored residual, computed by this call: per stage lo_shift, max |x|,
 * n(|lo8| == 127) and n(|x| >= 2^k) for k = 1..9; with taps enabled the stages are tokens0, layer0 .. layer<L-1> of the
 * last pass, without them one row for "x" - a host can poll it after any pass to learn that a stream has left the
 * exact range |x| < 2^(15 - s); with taps enabled it needs a pass since vt_group_enable_taps, else VT_ERR_INVALID_ARG),
 * "rowstat" [N,2] (row terms of the last folded LayerNorm), "attn" [N,D] (last block's attention output),
 * "last_block_rows" [1] (rows per slot the last encoder block of the last pass computed: Ns where it ran on the search rows
 * only, see vt_group_set_tuning "last_rows", else N; no stream's slot is looked up for it). After such a pass "x", "attn",
 * "rowstat" and the untapped "xrange" keep their shapes: the read of "x" / "xrange" first copies the search rows to their
 * places, so the Nt template rows of "x" hold what block L-2 left there (nothing computed them in block L-1); the template
 * rows of "attn" and "rowstat" read as zero.
 * "feat" [Ns,D], "head_t3" [Ns,C], "head_out" [Ns,8] (score,ox,oy,w,h logits),
 * "state" (the stream's device state record as raw 32-bit words), "graph_replays" [3] (passes replayed so far
 * per crop-buffer tier: which of the captured graphs ran), "template" [Nt,Kpad] (the stream's current template rows in
 * the template store: what its next pass will use). After a subset pass (vt_group_*_streams) every
 * tensor but "state", "template" and "graph_replays" is that of the stream's slot in it; a stream that was not in the pass
 * returns VT_ERR_INVALID_ARG. After a candidate pass (vt_group_update_*_candidates) the stream's slot is its WINNING
 * slot. A per-pass tensor name prefixed with "slot." ("slot.head_out", ...) takes `stream` as a SLOT index of the last
 * pass instead: the way to a losing slot's tensors.
 * "result_overlay" [6] (by STREAM, whatever the last pass was; counted since the engine became overlay-capable, see
 * vt_group_set_tuning): the engine's flags, drawn by the stream's last pass (0 or 1), number of passes drawn, number gated
 * (rule 4), number on a format that is not drawable (rule 5), N of the last label drawn. VT_ERR_INVALID_ARG on an engine
 * that never enabled the overlay.
 * "motion" [8] (by STREAM, whatever the last pass was; see vt_group_set_tuning "motion_prior"): the engine flag, vx, vy,
 * live, shift x and shift y of the stream's last pass, number of passes with a non-zero shift, number of failed updates
 * that advanced the box. VT_ERR_INVALID_ARG on an engine that never enabled the motion prior.
 * "appearance" [8] (by STREAM, whatever the last pass was; see vt_group_set_tuning "appearance"): the engine flag, then the
 * stream's record - status, similarity, frames_done - as the pinned mirror holds it: that of the stream's last pass the host
 * has COLLECTED (vt_group_wait, vt_group_wait_next, a synchronous call; a pipelined pass still outstanding does not show
 * yet), its counters evaluated and gated (the device's), the period and the gate per mille.
 * "anchor" [Nt,Kpad]: the rows the stream's probes are compared with. "probe" [Nt,Kpad]: the rows of the stream's last cut
 * probe - valid where the record's status is 1 or 3, stale otherwise, and the record says which. Each of the three returns
 * VT_ERR_INVALID_ARG on an engine that never enabled the appearance check.
 * "proposals" [60] (by STREAM, whatever the last pass was; see vt_group_set_tuning "proposals"): mode, then the stream's
 * record as the pinned mirror holds it (that of its last COLLECTED pass) - status, frames_done, n, c, Wg, Hg -, the counter
 * evaluated (the device's), period, max, min_sim_pm, max_cells, then 8 x (sim, x, y, w, h, position), zero behind the n
 * listed. "proposals_pattern" [M,M] and "proposals_map" [Hg-M+1,Wg-M+1]: the pattern (integers) and the similarity map of
 * the stream's slot in the LAST pass; VT_ERR_INVALID_ARG where that slot was not evaluated (the map: status 1; the pattern:
 * 1 or 3). Each of the three returns VT_ERR_INVALID_ARG on an engine that never enabled the proposals.
 * "conflicts" [16] (by STREAM, whatever the last pass was; see vt_group_set_tuning "conflicts"): the engine flag, then the
 * stream's record as the pinned mirror holds it (that of its last COLLECTED pass) - status, frames_done, n_over,
 * partner[0..3], iou[0..3] -, its counters evaluated, conflicting and gated (the device's), and the stream's scene.
 * VT_ERR_INVALID_ARG on an engine that never enabled the stream conflicts.
 * "health" [24] (by STREAM; see vt_group_set_tuning "health"), for people: the engine flag, then the stream's record as the
 * pinned mirror holds it (that of its last COLLECTED pass) - status, frames_done, flags, c, Wg, Hg, still, S1 / n, the
 * standard deviation sqrt(S2 / n - (S1 / n)^2), D / n, HD * 1000 / (2 n), G * 1000 / G_ref (0 where G_ref is 0) -, its
 * counters evaluated, flagged and gated (the device's), then period, cell, still_run, flat_q, cut_pm, gate, 0, 0.
 * "health_words" [52] (by STREAM): the same record as exact integers - its 26 32-bit words (status, frames_done, flags, c,
 * Wg, Hg, still, 0, then S1, S2, G, D, HD, G_ref as int64 low word first, then has_prev, cur, pW, pH, pc, 0), each as two
 * floats: the low and the high 16 bits. Both: VT_ERR_INVALID_ARG on an engine that never enabled the frame health.
 * "arbitrate" [48] (by STREAM; see vt_group_set_tuning "arbitrate"): the engine flag, then the stream's record as the pinned
 * mirror holds it (that of its last COLLECTED pass) - status, frames_done, n, chosen -, its counters evaluated (status 1 or 2)
 * and switched (the device's), 0; then four peaks of ten values: cell, status (0 not cut, 1 cut and scored, 2 rule 6 failed, 3
 * a variance is not positive), score, response, similarity, the float box x, y, w, h, 0. Every value is exact.
 * In a PIPELINED host run, read between two vt_group_wait_next calls, a by-stream mirror - this one like "appearance",
 * "conflicts", "health" - may already hold the record of the successor of a pass that was redone: compare a stream's record
 * with a synchronous run's where both have collected the same pass. The counters evaluated and switched are the device's and
 * may count a redone pass twice.
 * VT_ERR_INVALID_ARG on an engine that never enabled the peak arbitration.
 * Returns the element count, or a negative vt_status. With out == NULL only the count. */
int64_t vt_group_read_tensor(vt_group* g, int stream, const char* name, float* out,
                             int64_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* VITTRACK_HIP_H */
