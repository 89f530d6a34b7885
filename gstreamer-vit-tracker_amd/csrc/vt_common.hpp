// vt_common.hpp — types shared by the host engine and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "../../include/vittrack_hip.h"

typedef uint16_t bf16_t;  // bfloat16 bit pattern
typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(4))) short bf16x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;

// Pixel layout families: every value of vt_frame.format (vt_pixfmt, vt_pixfmt2) is one family plus a layout word
// (FrameDesc.lay). The family codes are the vt_pixfmt values of the formats that defined them, so those formats'
// descriptors are unchanged.
enum PixFamily {
    // packed R,G,B(,x) / x,R,G,B / one grey byte: lay = R | G << 8 | B << 16 (byte offsets inside the pixel, 0..3) |
    // bytes per pixel << 24 (GRAY8: 1, every offset 0)
    PIXF_RGB = VT_PIX_RGB8,
    // a luma plane + chroma at half the horizontal rate. lay = U offset | V offset << 8 (0 or 1: the position in an
    // interleaved pair, or - PIXL_PLANAR - which of the two chroma planes) | the PIXL_* bits below. NV12, NV21, I420,
    // YV12, P010 and NV16 (whose sibling is YUY2: the same luma, the same chroma pair per pixel pair, one row per row)
    PIXF_420SP = VT_PIX_NV12,
    PIXF_422 = VT_PIX_YUY2        // packed pixel pairs: lay = Y0 | U << 8 | Y1 << 16 | V << 24 (byte offsets)
};
// PIXF_420SP layout bits (zero for NV12 / NV21)
#define PIXL_PLANAR (1 << 16)     // U and V in planes of their own: p1 is the first, the second lies s1 * ceil(R / 2) bytes
                                  // behind it, R = the stored rows: wh, or - PIXL_FULLH - h
#define PIXL_S16 (1 << 20)        // 16-bit little-endian samples (strides in bytes), of which ...
#define PIXL_HIBYTE (1 << 22)     // ... byte 1 is read
#define PIXL_ROWS422 (1 << 24)    // one chroma row per luma row (no row shift)
#define PIXL_FULLH (1 << 25)      // set by to_desc: the planes belong to a whole frame (vt_frame.windowed != 1)

// family of a format (-1: unknown) and its layout word
inline int pix_family(int fmt) {
    switch (fmt) {
    case VT_PIX_RGB8: case VT_PIX_BGR8: case VT_PIX_RGBX: case VT_PIX_BGRX:
    case VT_PIX2_GRAY8: case VT_PIX2_XRGB: case VT_PIX2_XBGR: return PIXF_RGB;
    case VT_PIX_NV12: case VT_PIX_NV21:
    case VT_PIX2_I420: case VT_PIX2_YV12: case VT_PIX2_P010: case VT_PIX2_NV16: return PIXF_420SP;
    case VT_PIX_YUY2: case VT_PIX_UYVY: return PIXF_422;
    default: return -1;
    }
}
inline int32_t pix_layout(int fmt) {
    switch (fmt) {
    case VT_PIX_RGB8: return 0 | 1 << 8 | 2 << 16 | 3 << 24;
    case VT_PIX_BGR8: return 2 | 1 << 8 | 0 << 16 | 3 << 24;
    case VT_PIX_RGBX: return 0 | 1 << 8 | 2 << 16 | 4 << 24;
    case VT_PIX_BGRX: return 2 | 1 << 8 | 0 << 16 | 4 << 24;
    case VT_PIX_NV12: return 0 | 1 << 8;
    case VT_PIX_NV21: return 1 | 0 << 8;
    case VT_PIX_YUY2: return 0 | 1 << 8 | 2 << 16 | 3 << 24;
    case VT_PIX_UYVY: return 1 | 0 << 8 | 3 << 16 | 2 << 24;
    case VT_PIX2_I420: return 0 | 1 << 8 | PIXL_PLANAR;
    case VT_PIX2_YV12: return 1 | 0 << 8 | PIXL_PLANAR;
    case VT_PIX2_P010: return 0 | 1 << 8 | PIXL_S16 | PIXL_HIBYTE;
    case VT_PIX2_NV16: return 0 | 1 << 8 | PIXL_ROWS422;
    case VT_PIX2_GRAY8: return 0 | 0 << 8 | 0 << 16 | 1 << 24;
    case VT_PIX2_XRGB: return 1 | 2 << 8 | 3 << 16 | 4 << 24;
    case VT_PIX2_XBGR: return 3 | 2 << 8 | 1 << 16 | 4 << 24;
    default: return 0;
    }
}
// name of a format for error texts
inline const char* pix_name(int fmt) {
    static const char* const names[] = {"rgb8", "nv12", "yuy2", "bgr8", "rgbx", "bgrx", "nv21", "uyvy"};
    static const char* const names2[] = {"i420", "yv12", "p010", "nv16", "gray8", "xrgb", "xbgr"};
    return fmt >= 0 && fmt < 8 ? names[fmt] : fmt >= VT_PIX2_I420 && fmt <= VT_PIX2_XBGR ? names2[fmt - VT_PIX2_I420] : "?";
}
// which crop kernels (k_preproc.hip, fetch_rgb<level>) read this format: 0 those of RGB8, NV12 and YUY2, 1 those that read
// the byte offsets of f.lay (every vt_pixfmt), 2 those that read the whole layout word (every vt_pixfmt2 as well). A
// kernel of a level reads every format of the levels below it.
#define PIX_LEVELS 3
inline int pix_level(int fmt) { return fmt >= VT_PIX2_I420 ? 2 : fmt != VT_PIX_RGB8 && fmt != VT_PIX_NV12 && fmt != VT_PIX_YUY2 ? 1 : 0; }
// bytes per pixel of plane 0's rows (PIXF_420SP: the luma plane)
inline int pix_row_bpp(int fmt) {
    const int fam = pix_family(fmt);
    return fam == PIXF_RGB ? pix_layout(fmt) >> 24 : fam == PIXF_422 ? 2 : (pix_layout(fmt) & PIXL_S16) ? 2 : 1;
}
// PIXF_420SP: U and V lie in two planes behind each other / chroma rows of `rows` luma rows / window rules of YUY2
// (no rule on rows) instead of NV12's
inline bool pix_planar(int fmt) { return pix_family(fmt) == PIXF_420SP && (pix_layout(fmt) & PIXL_PLANAR); }
inline bool pix_rows422(int fmt) { return pix_family(fmt) == PIXF_420SP && (pix_layout(fmt) & PIXL_ROWS422); }
inline int pix_chroma_rows(int fmt, int rows) { return pix_rows422(fmt) ? rows : (rows + 1) / 2; }
// PIXF_420SP: bytes of a chroma row (of one plane) that belong to `ww` pixels
inline int pix_chroma_row_bytes(int fmt, int ww) {
    return pix_planar(fmt) ? (ww + 1) / 2 : ((ww + 1) & ~1) * pix_row_bpp(fmt);
}

// one device-resident input frame (mirrors vt_frame, 64-bit pointers)
struct FrameDesc {
    const uint8_t* p0;  // packed pixels, or the luma plane of PIXF_420SP
    const uint8_t* p1;  // PIXF_420SP: the interleaved chroma plane, or the first of the two chroma planes
    int32_t w, h, s0, s1;
    int32_t fmt;        // PixFamily
    int32_t x0, y0;     // frame coordinates of the first stored pixel (window upload)
    int32_t ww, wh;     // extent of the stored window in pixels: samples outside it read as black
    int32_t lay;        // byte layout within the family (PixFamily)
};
static_assert(sizeof(FrameDesc) == 56, "FrameDesc layout");

// per tracked stream, lives in HBM; the decode kernel of frame t writes what the preprocessing
// kernel of frame t+1 reads, so a stream of updates never needs the host in between.
struct StreamState {
    float box[4];        // last accepted box, frame pixels: x, y, w, h (top-left + size)
    float geo[4];        // search-crop geometry of the running frame: x0m, y0m, scale, side
    int32_t frame_w, frame_h;
    int32_t initialized;
    int32_t frames_done;     // updates completed since init
    int32_t success_count;   // of which result.success
    int32_t last_idx;        // argmax cell of the last update
    float last_fbox[4];      // unrounded clipped box of the last update
    float last_score;
    // index (= frames_done + 1 at the time) of the last pass in which the crop needed a pixel that
    // lies inside the frame but outside the window the caller stored: such samples read as black, so
    // a host that uploaded a SPECULATIVE window (vt_group_enqueue_host) must redo that pass
    int32_t window_miss;
    // template refresh (k_refresh.hip): refreshes since init - the stream's current template is buffer
    // tpl_gen & 1 of a two-buffer store - and frames_done at the last one. Zero after init. They rewind and commit with
    // the state they are part of.
    int32_t tpl_gen;
    int32_t tpl_frame;
};
static_assert(sizeof(StreamState) == 88, "StreamState layout");

struct ModelDims {
    int patch, T, S, D, H, L, mlp, C, kpad;
    int gt, gs, nt, ns, ntok;   // grids and token counts
    int npad;                   // ntok rounded up to 64 (attention key padding)
    float norm_a[3], norm_b[3];
    float success_threshold, ln_eps;
};

// ---- kernel launchers (each enqueues on `st`; no allocation, no synchronisation) -------------

// q is stored multiplied by 1/sqrt(64) * log2(e), so that q·k is the softmax exponent in log2 units
// (the attention kernels use v_exp_f32 = 2^x directly); float(log2 e) / 8 is exact in float32
#define ATT_Q_SCALE (0.125f * 1.4426950408889634f)

// NUMERICAL SPECIFICATION v3 (round 6; the per-model shift: round 7). The residual stream x is stored as a 3-BYTE pair:
// Xh = bf16(x) [M][ldx] and Xl = lo8 [M][ldx] bytes, lo8 = clamp(rint((x - Xh) * 2^s), -127, 127) as a signed integer:
// x = Xh + lo8 * 2^-s. The shift s is a property of the MODEL: header int 12 of the weight blob (0 = 12, else 6..14),
// fixed for the life of an engine and carried to every kernel that reads or writes the pair as LoQuant (below).
// Until round 5 the low half was a second bf16 (4 bytes per element, 17 significant bits); the byte plane moves a
// quarter less through the X-epilogues' read-modify-write and the final LayerNorm, the phases of the pass that are
// bound by memory requests (profiles/r06_lo8_residual.txt: whole frame + 2.0 %). x - Xh is exact (Xh is x rounded to 8
// significant bits), the scaling is a power of two, rint is round-to-nearest-even, Xh + lo8 * 2^-s is exact in
// float32: oracle (oracle/vit_ref.py split_residual) and kernels can differ only through the x they start from.
// |x - Xh| <= ulp(Xh) / 2: at most 64 quanta for |x| < 2^(15 - s) - the EXACT RANGE: the byte holds the remainder with
// room to spare and the stored value is within half a quantum of x. For 2^(15 - s) <= |x| < 2^(16 - s) the remainder
// reaches 128 quanta next to a bf16 tie, where the clamp costs at most one quantum (the ONE-QUANTUM BAND); beyond
// 2^(16 - s) the clamp leaves part of the low half behind - the value SATURATES towards plain bf16, it never wraps.
// The trade: a coarser quantum protects large values at the price of small ones. The pair adds nothing to bf16 once
// the quantum exceeds half an ulp of Xh: at s = 8 an element with |x| < 1 is stored as plain bf16, at the default
// s = 12 that only happens below 2^-4. s = 12 suits the seeded models (|x| < 3.5, exact range 8); a checkpoint with
// residual outlier channels wants the largest s whose exact range still covers them ("xrange" of
// vt_group_read_tensor reports what a model's streams hold; weights.recommend_lo_shift picks s from it).
#define VT_LO_SHIFT_DEFAULT 12
#define VT_LO_SHIFT_MIN 6
#define VT_LO_SHIFT_MAX 14
// what the kernels need of s, derived once on the host (all three exact powers of two times a small integer):
// wave-uniform kernel arguments, so they sit in SGPRs
struct LoQuant {
    float q = 1.0f / 4096.0f;          // 2^-s: the quantum
    float lo_max = 127.0f / 4096.0f;   // 127 q: the clamp of the remainder
    float magic = 3072.0f;             // 1.5 * 2^(23 - s): the float whose ulp is q (x_split8)
    int shift = VT_LO_SHIFT_DEFAULT;
};
inline LoQuant lo_quant(int s) {
    LoQuant l;
    l.q = 1.0f / (float)(1 << s);
    l.lo_max = 127.0f * l.q;
    l.magic = 1.5f * (float)(1 << (23 - s));
    l.shift = s;
    return l;
}
// (comment of the v2 form, for the history of the format:)
// The residual stream x is stored as a PAIR of bf16 matrices: Xh = bf16(x), Xl = bf16(x - Xh) (17
// significant bits; Xh alone is the A operand of the GEMM that consumes the following LayerNorm). The
// three epilogues that produce x (X-epilogues) also emit, per row and per 32-column chunk, the partial
// statistics (sum, sum of squared deviations from the chunk mean) of the float32 value before the split:
// rowstat_finalize turns them into the (rstd, -mean * rstd) the consuming GEMM's epilogue applies.
enum GemmEpilogue {
    EPI_F32_POS = 0,   // x = (acc + bias) + pos[m % pos_rows] -> Xh, Xl, cstat   (patch embed)
    EPI_RESID = 1,     // x = (acc + bias) + (Xh + Xl)         -> Xh, Xl, cstat   (proj, fc2)
    EPI_GELU_BF16 = 2, // Cb bf16 = gelu(y)                                        (fc1)
    EPI_RELU_BF16 = 3, // Cb bf16 = relu(y)                                        (head convs)
    EPI_QKV = 4,       // q*ATT_Q_SCALE,k -> qk[M][2D] bf16; v -> Vt[b][h][64][npad]
    EPI_F32 = 5        // x = acc + bias                       -> Xh, Xl, cstat   (operator tests)
};
// y of the bf16 epilogues: acc + bias, or with a folded LayerNorm (rowstat != null)
//     y[m][n] = rowstat[m].x * acc + (rowstat[m].y * colsum[n] + bias[n])
// where the weights are W' = bf16(gamma * W), colsum[n] = sum_k W'[n][k], bias[n] = sum_k beta[k] W[n][k] + b[n]
#define VT_STAT_CHUNK 32

struct GemmArgs {
    const bf16_t* A; int lda;     // [M][K] row-major bf16
    const bf16_t* W; int ldw;     // [N][K] row-major bf16 (one output feature per row)
    const float* bias;            // [N]
    int M, N, K;
    bf16_t* Xh; uint8_t* Xl; int ldx;  // X-epilogues: the residual stream pair [M][ldx] - bf16 high halves, lo8 bytes (EPI_RESID: read, then written)
    float2* cstat;                // X-epilogues: [M][N / 32] chunk partials (sum, M2), or null
    // X-epilogues of the 256x256 kernel (launch_gemm reports whether it was used): the last workgroup of
    // every 256-row panel finalizes the panel's row terms itself (no launch_rowstat_finalize needed)
    float2* rowstat_out;          // [M] (rstd, -mean * rstd), or null
    unsigned* panel_cnt;          // [ceil(M / 256)] arrival counters, zero between launches
    float ln_eps;
    bf16_t* Cb; int ldcb;         // bf16 output
    const float* pos; int pos_rows;     // EPI_F32_POS: [pos_rows][ldx] f32
    const float2* rowstat;        // bf16 epilogues: folded LayerNorm row terms [M] (rstd, -mean * rstd), or null
    const float* colsum;          // ... and its column sums [N]
    const float2* cstat_in;       // 4-wave kernel only, instead of rowstat: the chunk partials [M][K / 32] of the
                                  // X-epilogue that produced A; the epilogue combines them itself (uses ln_eps)
    bf16_t* qk; bf16_t* vt; int tokens; int npad; int D;
    int vt_perm;                  // Vt key order inside each group of 16: 0 natural, 1 attn_perm16 (attention mode 3)
    unsigned long long* dbg;      // diagnostic builds only (VT_STAMPS): per-wave cycle sums
    // Implicit 3x3 convolution (zero padding) on the head's feature maps, 4-wave kernel with the ReLU
    // epilogue only: conv_grid > 0 makes A the map t[M = B*grid*grid][conv_C] (lda = conv_C) and the
    // GEMM's K = 9*conv_C the im2col row (ky*3+kx)*conv_C + c, gathered tap by tap while the LDS-DMA
    // pieces are issued (a K-tile of 64 lies inside one tap: conv_C % 64 == 0). Out-of-map taps read
    // `zeros` (>= 128 B of zeros in device memory).
    int conv_grid, conv_C;
    const bf16_t* zeros;
    // kernel of k_gemm.hip: which tiles an XCD's contiguous run of workgroups covers - 0: the launcher decides (bf16-output
    // epilogues with M < N: column tiles), 1: row panels x all columns, 2: column tiles x all rows
    int tile_order;
    LoQuant lq;                   // X-epilogues: the pair's quantum (the engine's lo_shift; default 12)
    // EPI_RESID on the 256x256 kernel only (anything else refuses them: hipErrorInvalidValue): the residual ADDEND is
    // read from another pair than the one written (null: Xh / Xl, read then written in place), and, with seg_rows > 0,
    // from a layout that has seg_skip rows nobody computes in front of every segment of seg_rows rows: output row m
    // takes its addend from input row m + (m / seg_rows + 1) * seg_skip. seg_rows is even (a row pair never straddles
    // two segments). Writes, chunk partials, the panel ticket and the row terms stay at row m. The last encoder block
    // on search rows only: seg_rows = ns, seg_skip = nt (vt_engine.hip, run_pass).
    const bf16_t* Xh_in; const uint8_t* Xl_in;
    int seg_rows, seg_skip;
};
// the arguments ask for the remapped / out-of-place addend read of EPI_RESID
inline bool gemm_addend_remapped(const GemmArgs& a) {
    return a.seg_rows != 0 || a.seg_skip != 0 || (a.Xh_in && a.Xh_in != a.Xh) || (a.Xl_in && a.Xl_in != a.Xl);
}

hipError_t launch_gemm(const GemmArgs& a, int epilogue, hipStream_t st);
// true: launch_gemm() will run an X-epilogue of these arguments on the 256x256 kernel, whose row panels
// finalize a.rowstat_out themselves; false: the caller launches launch_rowstat_finalize behind the GEMM
bool gemm_finalizes_rowstat(const GemmArgs& a, int epilogue);
hipError_t launch_gemm_cfg(const GemmArgs& a, int epilogue, int cfg, hipStream_t st);
int gemm_pick_config(int M, int N, int K, int epilogue, bool conv = false);
const char* gemm_config_name(int cfg);
hipError_t gemm_prepare();  // once per device, before the first launch / any stream capture
// k_gemm256.hip: the 256x256-tile 8-wave kernels (configs 18, 19); hipErrorInvalidValue = shape does not fit
#define GEMM_CFG_SMALL_MAX 8   // 0..8: the 4-wave kernel of k_gemm.hip (7, 8 with four loader waves beside it)
#define GEMM_CFG_256P4 18      // 2 phases of 32 MFMAs per K-tile, one tile per workgroup (17, round 1's 4-phase schedule: git history)
#define GEMM_CFG_256PP 19      // the same loop in persistent workgroups (bf16 outputs with more tiles than CUs; else = 18)
#define GEMM_CFG_256_MIN GEMM_CFG_256P4
// operands of the 256x256 kernels are addressed with unsigned 32-bit byte offsets from their base
#define VT_GEMM256_MAX_OPERAND_BYTES (1ll << 32)
hipError_t gemm256_prepare();
const char* gemm256_build_id();   // sha256 of k_gemm256.hip + the headers it includes + its compile flags (build.py: -DVT_TU_SHA256)
hipError_t launch_gemm256(const GemmArgs& a, int epilogue, bool persistent, hipStream_t st);
bool gemm256_fits(const GemmArgs& a, int epilogue);
// the tile configuration launch_gemm() runs for these arguments (the picker's choice, or the 4-wave
// kernel where a 256x256 choice does not fit the operands)
int gemm_effective_config(const GemmArgs& a, int epilogue);

// y[r] (bf16) = LN(x[in_row(r)]) ; in_row(r) = (r / group) * in_stride + in_off + r % group
hipError_t launch_layernorm(const float* x, const float* gamma, const float* beta, bf16_t* y,
                            int rows, int D, int group, int in_stride, int in_off, float eps,
                            hipStream_t st);
// the same on the split residual stream: x = xh + xl * lo_q (3-byte pair, lo_q = 2^-s)
hipError_t launch_layernorm_split(const bf16_t* xh, const uint8_t* xl, const float* gamma, const float* beta,
                                  bf16_t* y, int rows, int D, int group, int in_stride, int in_off,
                                  float eps, float lo_q, hipStream_t st);
// Range report of a stored pair (k_misc.hip, off the hot path): out[0] = max |x| as the bit pattern of a non-negative
// float, out[1] = n(|lo8| == 127), out[1 + k] = n(|x| >= 2^k), k = 1..9, accumulated into out (zero it first) over
// rows [0, rows) of xh / xl (contiguous rows of length D, D % 8 == 0), for `stages` copies of the pair that lie
// stage_stride bytes apart in BOTH planes (the tap slots), into out[stage][VT_XRANGE_WORDS]
#define VT_XRANGE_WORDS 11
hipError_t launch_xrange(const bf16_t* xh, const uint8_t* xl, unsigned* out, int rows, int D, float lo_q, int stages,
                         size_t stage_stride, hipStream_t st);
// rowstat[m] = (rstd, -mean * rstd) from the chunk partials of an X-epilogue (D = 32 * nchunk columns)
hipError_t launch_rowstat_finalize(const float2* cstat, float2* rowstat, int M, int nchunk, float eps,
                                   hipStream_t st);
// LayerNorm folded into the weights of the GEMM that consumes it (once, at engine creation):
// Wf[n][k] = bf16(gamma[k] * W[n][k]); colsum[n] = sum_k Wf[n][k]; cvec[n] = sum_k beta[k] W[n][k] + bias[n]
hipError_t launch_fold_layernorm(const bf16_t* W, const float* gamma, const float* beta, const float* bias,
                                 bf16_t* Wf, float* colsum, float* cvec, int N, int K, hipStream_t st);

// out[M][D] bf16 = softmax(q k^T) v, q/k rows in qk[M][2D], v transposed in vt[B*H][64][npad]
hipError_t launch_attention(const bf16_t* qk, const bf16_t* vt, bf16_t* out, int B, int tokens,
                            int H, int npad, hipStream_t st);

// Which attention kernel launch_attention() will run for this shape,
// and whether it wants Vt with the permuted key order (mode 3). The QKV GEMM that feeds it must be
// given the same vt_perm.
int attention_pick_mode(int tokens, int npad);
inline int attention_vt_perm(int mode) { return mode >= 3 ? 1 : 0; }
// position of key t inside its group of 16 in the permuted Vt layout: bits 2 and 3 swapped
__host__ __device__ inline int attn_perm16(int t) { return (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1); }

hipError_t attention_prepare();   // once per device, before the first launch / any stream capture
hipError_t launch_attention_mode(const bf16_t* qk, const bf16_t* vt, bf16_t* out, int B, int tokens,
                                 int H, int npad, int mode, hipStream_t st);

// mode 3 (tokens % 4 == 0, npad % 64 == 0) on the queries q0 .. q0 + nq - 1 of every stream only, keys and values all
// `tokens`: out is compact, [B * nq][H * 64], row b * nq + (q - q0). Same bits as those rows of launch_attention_mode(3)
// while every query's scores stay inside the kernel's +-32 window (k_attn.hip, attention_dma_q_kernel)
hipError_t launch_attention_queries(const bf16_t* qk, const bf16_t* vt, bf16_t* out, int B, int tokens, int H, int npad,
                                    int q0, int nq, hipStream_t st);

// crop + bilinear + normalise -> patch rows; one launch covers slots [b0, b0+nb)
// tier: the tile kernel's LDS buffer (0: 16 KiB, 1: 32 KiB, 2 or more: 64 KiB), a choice of speed only
// slot_stream (device, [nb + b0] or null = identity): the stream a slot works for. Frame descriptor and patch rows are
// the slot's; the StreamState read (and its geo / frame_w / frame_h / window_miss written) is the stream's.
// any_layout: the highest pix_level of the slots' formats (above 0 the layout is read from FrameDesc.lay: k_preproc.hip, fetch_rgb)
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


hipError_t launch_overlay(uint8_t* yplane, int width, int height, int stride, const vt_draw_cmd* d_cmds,
                          int n, hipStream_t st);

hipError_t launch_overlay_rgb(uint8_t* rgb, int width, int height, int stride, const vt_draw_cmd* d_cmds,
                              int n, hipStream_t st);

// Where a pass leaves its results for the host: pinned, device-visible host memory the decode kernel
// stores to directly (no device-to-host copy on the stream). Uploaded with the frame descriptors of
// the pass, right behind them in the same buffer.
struct MotionRec;
struct AppearRec;
struct PropRec;
struct ConflictRec;
struct HealthRec;
struct ArbRec;
struct PassOut {
    vt_result* host_results;    // [slots of the pass] or null
    StreamState* host_states;   // [B] (by stream) or null
    vt_peaks* host_peaks;       // [slots of the pass] or null: the response-peaks launch's records (k_peaks.hip)
    MotionRec* host_motion;      // [B] (by stream) or null: the motion records as the settle launch left them (k_motion.hip)
    AppearRec* host_appearance;  // [B] (by stream) or null: the appearance records of the pass's streams (k_appearance.hip)
    PropRec* host_proposals;     // [B] (by stream) or null: the proposal records of the pass's streams (k_proposals.hip)
    ConflictRec* host_conflicts; // [B] (by stream) or null: the conflict records of the pass's streams (k_conflicts.hip)
    HealthRec* host_health;      // [B] (by stream) or null: the frame-health records of the pass's streams (k_health.hip)
    ArbRec* host_arbitrate;      // [B] (by stream) or null: the arbitration records of the pass's streams (k_arbitrate.hip)
};

struct DecodeArgs {
    const bf16_t* t3;       // [B*ns][C]
    const float* w4;        // [8][C]
    const float* b4;        // [8]
    const float* hann;      // [ns]
    float* head_out;        // [B*ns][8]
    StreamState* states;    // [B]
    vt_result* results;     // [B] (device)
    const PassOut* out;     // device copy of this pass's PassOut
    // [B] slot -> stream of a subset pass (null: the identity, every full pass). head_out, results and
    // out->host_results are indexed by slot; states and out->host_states by stream.
    const int32_t* slot_stream;
    int B, ns, grid, C;     // B: slots of the pass
    float success_threshold;
};
hipError_t launch_decode(const DecodeArgs& a, hipStream_t st);     // head_out_kernel + decode_kernel (two launches)

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

// ---- target chips (k_chip.hip) ------------------------------------------------------------------------------------------
// per stream, device memory, written by the host only (never rewound)
struct ChipPolicy {
    float factor;               // 0: off, else 0.5..4: the crop side is factor * sqrt(w * h) of the new box
    int32_t period, phase;      // a chip is due when frames_done % period == phase
    int32_t reserved;
};
#define VT_CHIP_MAX_PERIOD 1000000
struct ChipArgs {
    const FrameDesc* frames;    // [n] by slot: the frames of this pass
    StreamState* states;        // [B] by stream, as decode / cand_commit (and the refresh launch) left them
    const vt_result* results;   // [n] by slot
    const int32_t* slot_stream; // [n] slot -> stream, null: the identity
    const int32_t* winner;      // candidate pass: [n] the winning slot of slot i's stream (only winners cut); else null
    const ChipPolicy* policy;   // [B] by stream
    uint8_t* chips;             // the store [B][chip_bytes], one buffer per stream
    vt_chip_info* infos;        // [B] by stream
    const PassOut* out;         // device copy of the pass's PassOut: host_states gets a window miss too
    StreamState* host_states;   // non-null: used instead of out->host_states (candidate passes: the commit's mirror)
    int n;
};
// behind the decode (candidate pass: behind the commit; behind the refresh launch where there is one): per slot the gate
// of DESIGN.md section 3 "Target chips", the stream's info record and, where the gate fires, the chip - a crop of this
// pass's frame at the committed box, side C, kind VT_CHIP_NORM_BF16 (na, nb: the caller's) or VT_CHIP_RGB8
hipError_t launch_target_chips(const ChipArgs& a, int C, int kind, const float* na, const float* nb, int search_size,
                               int tier, int any_layout, hipStream_t st);

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

// ---- motion prior (k_motion.hip) ------------------------------------------------------------------------------------------
// DESIGN.md section 3 "Motion prior". Per stream, device memory, mirrored to pinned host memory beside the states; it
// rewinds and commits with the state it belongs to, but is no part of StreamState or of a snapshot.
struct MotionRec {
    float v[2];                 // velocity estimate, pixels per update of this stream
    float prior[4];             // the state box as the place launch of the stream's last pass found it
    float shift[2];             // what that launch added to the box's x, y (0 or v)
    int32_t live;               // failed updates through which the box still advances
    int32_t n_shift;            // passes with a non-zero shift
    int32_t n_coast;            // failed updates that left the box advanced
    int32_t reserved;
};
static_assert(sizeof(MotionRec) == 48, "MotionRec layout");
// ONE record per engine, device memory, written by the host only (vt_group_set_tuning "motion_*")
struct MotionPolicy {
    int32_t on;                 // "motion_prior": 0 / 1
    int32_t gain_pct;           // 1..100
    int32_t coast;              // 0..60
    int32_t max_pct;            // 0..200
};
#define VT_MOTION_DEFAULT_POLICY MotionPolicy{0, 50, 5, 100}
// The place rule on one stream, every operation a binary32 operation of its own (this header's users are built with
// -ffp-contract=off): the box the pass is cut around. Shared by the place kernel and the host's window planning
// (vt_ingest.hip), which must agree to the bit. Returns true where the box moves: out = (x + vx, y + vy, w, h).
__host__ __device__ inline bool motion_predict(int on, const float* box, const float* v, int frame_w, int frame_h, float* out) {
    out[0] = box[0]; out[1] = box[1]; out[2] = box[2]; out[3] = box[3];
    if (!on || (v[0] == 0.0f && v[1] == 0.0f)) return false;
    const float px = box[0] + v[0], py = box[1] + v[1];
    const float hw = 0.5f * box[2], hh = 0.5f * box[3];
    const float cx = px + hw, cy = py + hh;
    if (!(cx >= 0.0f && cx < (float)frame_w && cy >= 0.0f && cy < (float)frame_h)) return false;
    out[0] = px; out[1] = py;
    return true;
}
struct MotionArgs {
    StreamState* states;        // [B] by stream
    MotionRec* recs;            // [B] by stream
    const MotionPolicy* policy; // the engine's record
    const vt_result* results;   // [n] by slot (settle)
    const int32_t* slot_stream; // [n] slot -> stream, null: the identity
    const int32_t* winner;      // candidate pass: [n] the winning slot of slot i's stream (settle: only winners); else null
    const vt_candidate* cands;  // candidate pass: [n] the slots (settle: has_box of the winner); else null
    const PassOut* out;         // device copy of the pass's PassOut: host_states, host_motion (settle); may be null
    StreamState* host_states;   // non-null: used instead of out->host_states (candidate passes: the commit's mirror)
    int n;
};
// the first launch of a pass: per listed, initialised stream (once, however many slots name it) prior = box, and the box
// moves by v where the rule allows it. One lane per slot, n <= VT_MAX_STREAMS.
hipError_t launch_motion_place(const MotionArgs& a, hipStream_t st);
// behind the decode (candidate pass: behind the commit), ahead of the refresh, chip, peaks and overlay launches: the
// velocity update / coast / restore per stream of the pass, the final box and the record to device and pinned mirrors
hipError_t launch_motion_settle(const MotionArgs& a, hipStream_t st);

// ---- appearance check (k_appearance.hip) --------------------------------------------------------------------------------
// DESIGN.md section 3 "Appearance check": the zero-mean normalised correlation of the template-sized crop at each new box
// (the probe) with the rows the stream was started from (the anchor). Per stream, device memory, mirrored to pinned host
// memory beside the states; every pass writes the records of its streams (a redone pass writes them again); no part of
// StreamState or of a snapshot.
struct AppearRec {
    int32_t status;             // 0: not due or not evaluated; 1: evaluated; 2: refresh rule 6 failed at the box; 3: a variance is not positive
    int32_t frames_done;        // the stream's frames_done in the pass that wrote the record
    float similarity;           // [-1, 1]; 0 unless status is 1
    float box[4];               // the box the probe was (or would have been) cut at: the state's box behind the pass
    int32_t reserved;
};
static_assert(sizeof(AppearRec) == 32, "AppearRec layout");
// ONE record per engine, device memory, written by the host only (vt_group_set_tuning "appearance*")
struct AppearPolicy {
    int32_t on;                 // "appearance": 0 / 1
    int32_t period;             // 1..VT_APPEAR_MAX_PERIOD: evaluated when frames_done % period == 0
    int32_t gate_pm;            // 0..1000 per mille; 0: report only
    float tau;                  // (float)gate_pm / 1000.0f, one binary32 divide (the host's)
};
#define VT_APPEAR_MAX_PERIOD 1000000
#define VT_APPEAR_DEFAULT_POLICY AppearPolicy{0, 1, 0, 0.0f}
// per stream, beside the policy: diagnostics, never rewound - a redone pass may count twice (like skipped_geometry)
struct AppearCount {
    int32_t evaluated;          // records written with status 1 or 3
    int32_t gated;              // refreshes that rules 1-7 allowed and rule 8 refused
};
#define VT_APPEAR_CHUNK_ROWS 8  // rows of the [nt][cols] matrices per workgroup of the score launch
inline int appear_chunks(int nt) { return (nt + VT_APPEAR_CHUNK_ROWS - 1) / VT_APPEAR_CHUNK_ROWS; }
struct AppearArgs {
    const FrameDesc* frames;    // [n] by slot: the frames of this pass (probe)
    StreamState* states;        // [B] by stream, as decode / cand_commit / motion_settle left them
    const vt_result* results;   // [n] by slot
    const int32_t* slot_stream; // [n] slot -> stream, null: the identity
    const int32_t* winner;      // candidate pass: [n] the winning slot of slot i's stream (only winners evaluate); else null
    const AppearPolicy* policy; // the engine's record
    AppearCount* counts;        // [B] by stream
    AppearRec* recs;            // [B] by stream
    const RefreshPolicy* refresh;   // [B] by stream or null: refresh rules 1, 3, 4 make a slot due while tau > 0
    unsigned* tickets;          // [n] by slot, zero between launches (score)
    double* partials;           // [n][appear_chunks(nt)][5] by slot (score)
    const bf16_t* anchor;       // [B][nt][kpad] by stream
    bf16_t* probe;              // [B][nt][kpad] by stream
    const PassOut* out;         // device copy of the pass's PassOut: host_states (a window miss), host_appearance; may be null
    StreamState* host_states;   // non-null: used instead of out->host_states (candidate passes: the commit's mirror)
    double* sums;               // null, or [n][5] by slot: Sa, Sp, Saa, Spp, Sap of the slots the score launch evaluated
    int n;
};
// behind the decode (candidate pass: the commit) and motion_settle, ahead of the refresh, chip, peaks and overlay launches:
// per slot the due rule, refresh rules 6 and 7, the record (status 0 / 2, or 1 = cut: the score launch completes it) and,
// where the slot passes, the template crop of this pass's frame at the committed box into probe[stream]
hipError_t launch_appearance_probe(const AppearArgs& a, const ModelDims& d, int tier, int any_layout, hipStream_t st);
// behind the probe launch: per slot whose record says "cut", the five sums over the first `cols` columns of the nt rows of
// anchor[stream] and probe[stream] in binary64, in a FIXED order (per-lane strided partials, wave and workgroup tree,
// chunk partials added in index order by the slot's last workgroup), the similarity and the final record
hipError_t launch_appearance_score(const AppearArgs& a, int nt, int cols, int kpad, hipStream_t st);

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

// ---- reacquire proposals (k_proposals.hip) ------------------------------------------------------------------------------
// DESIGN.md section 3 "Reacquire proposals": the stream's own template, pooled to an M x M pattern of int16 cells, slid
// over an int16 thumbnail of the whole frame of the pass; the best places, with boxes, in a record per stream. The rule is
// stated to the bit in include/vittrack_hip.h ("proposals*" keys). Integer sums: no order of additions matters, nothing
// here is a floating-point atomic. Per stream a record, mirrored to pinned host memory like the appearance records;
// per slot the working set (header, pattern, thumbnail, map). No part of StreamState or of a snapshot; nothing of the
// pass's results, states, templates or frames is written.
#define VT_PROP_MAX 8               // proposals a record lists at most
#define VT_PROP_M_MAX 16            // the pattern side: 16, or 14 for templates that 16 does not divide
#define VT_PROP_OUTSIDE (-32768)     // a thumbnail cell with a sub-tap outside the frame: no value clamps to it; never matched
#define VT_PROP_MIN_CELLS 16384
#define VT_PROP_MAX_CELLS 4194304
#define VT_PROP_MAX_PERIOD 1000000
struct PropEntry {
    float sim;                  // [-1, 1]
    float box[4];               // x, y, w, h: the state's size centred on the match window's centre
    int32_t pos;                // py * (Wg - M + 1) + px
};
struct PropRec {
    int32_t status;             // 0: not due; 1: evaluated; 2: geometry (grid too large or smaller than the pattern);
                                // 3: flat pattern; 4: no whole device frame (host-pointer pass or a windowed frame)
    int32_t frames_done;        // the stream's frames_done in the pass that wrote the record
    int32_t n;                  // proposals listed
    float c;                    // the cell side in source pixels (0 unless status is 1, 2 or 3)
    int32_t Wg, Hg;             // the thumbnail's grid
    int32_t reserved[2];
    PropEntry p[VT_PROP_MAX];
};
static_assert(sizeof(PropEntry) == 24 && sizeof(PropRec) == 224, "PropRec layout");
// ONE record per engine, device memory, written by the host only (vt_group_set_tuning "proposals*")
struct PropPolicy {
    int32_t mode;               // "proposals": 0 off, 1 slots whose update failed, 2 every update
    int32_t period;             // 1..VT_PROP_MAX_PERIOD: due when frames_done % period == 0
    int32_t max_n;              // 1..VT_PROP_MAX
    int32_t min_sim_pm;         // 0..1000 per mille
    float tau;                  // (float)min_sim_pm / 1000.0f, one binary32 divide (the host's)
    int32_t max_cells;          // thumbnail cells per slot: fixed by the first enable
    int32_t reserved[2];
};
#define VT_PROP_DEFAULT_POLICY PropPolicy{0, 1, 4, 500, 0.5f, 262144, {0, 0}}
// per slot, written by the prepare launch and obeyed by the three behind it
struct PropHead {
    int32_t status;             // the record's status so far: 1 = the thumbnail, map and listing run
    int32_t frames_done;
    int32_t M, Wg, Hg;
    float c, X0;                // cell side, grid origin (X0 == Y0)
    float box[4];               // the state's box as the pass left it
    int32_t reserved;
    long long Sa, Saa;          // the whole pattern's sums (status 3; a position uses those of its cells inside the frame)
};
static_assert(sizeof(PropHead) == 64, "PropHead layout");
__host__ __device__ inline int prop_pattern_side(int T) { return T % 16 == 0 ? 16 : T % 14 == 0 ? 14 : 0; }
struct PropArgs {
    const FrameDesc* frames;    // [n] by slot: the frames of this pass
    const StreamState* states;  // [B] by stream, as decode / cand_commit / motion_settle left them
    const vt_result* results;   // [n] by slot
    const int32_t* slot_stream; // [n] slot -> stream, null: the identity
    const int32_t* winner;      // candidate pass: [n] the winning slot of slot i's stream (only winners evaluate); else null
    const PropPolicy* policy;   // the engine's record
    const int32_t* devflag;     // 1: the pass came through a device entry point
    const bf16_t* tpl;          // [B][tpl_bufs][nt][kpad] by stream: the template store
    int tpl_bufs;               // 2: a stream's rows are buffer tpl_gen & 1
    PropRec* recs;              // [B] by stream
    int32_t* evaluated;         // [B] by stream: records written with status 1 or 3 (diagnostic, never rewound)
    PropHead* heads;            // [n] by slot
    int16_t* pattern;           // [n][VT_PROP_M_MAX^2] by slot: M x M, row-major
    int16_t* thumb;             // [n][max_cells] by slot: Hg x Wg, row-major
    float* map;                 // [n][max_cells] by slot: (Hg - M + 1) x (Wg - M + 1), row-major
    const PassOut* out;         // device copy of the pass's PassOut: host_proposals; may be null
    int max_cells;              // the stride of thumb and map; fixes the launch dimensions
    int n;
};
// the four launches, in this order, behind decode / commit / motion_settle / appearance and ahead of refresh, chips,
// peaks and overlay (the frame is undrawn): the due rule, geometry and pattern; the thumbnail; the similarity map; the
// listing and the record. Fixed launch dimensions (max_cells): workgroups of slots that are not due leave at once.
hipError_t launch_proposals_prepare(const PropArgs& a, const ModelDims& d, hipStream_t st);
hipError_t launch_proposals_thumb(const PropArgs& a, const ModelDims& d, int any_layout, hipStream_t st);
hipError_t launch_proposals_match(const PropArgs& a, hipStream_t st);
hipError_t launch_proposals_list(const PropArgs& a, hipStream_t st);

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

// ---- stream conflicts (k_conflicts.hip) ---------------------------------------------------------------------------------
// DESIGN.md section 3 "Stream conflicts": per stream of a pass, which other streams of the same pass and the same scene
// overlap its new box, and by how much (IoU). Per stream, device memory, mirrored to pinned host memory beside the states;
// every pass writes the records of its streams whole (a redone pass writes them again); no part of StreamState or of a
// snapshot.
#define VT_CONFLICT_MAX 4       // partners a record lists
struct ConflictRec {
    int32_t status;             // 0: no pass wrote it; 1: evaluated, nobody over tau; 2: evaluated, n_over > 0; 3: not eligible
    int32_t frames_done;        // the stream's frames_done in the pass that wrote the record
    int32_t n_over;             // partners with iou >= tau (may exceed VT_CONFLICT_MAX)
    int32_t reserved;
    int32_t partner[VT_CONFLICT_MAX];   // the over-tau partners' stream indices by (iou descending, stream ascending); unused: -1
    float iou[VT_CONFLICT_MAX];         // theirs; unused: 0
};
static_assert(sizeof(ConflictRec) == 48, "ConflictRec layout");
// ONE record per engine, device memory, written by the host only (vt_group_set_tuning "conflicts*")
struct ConflictPolicy {
    int32_t on;                 // "conflicts": 0 / 1
    int32_t iou_pm;             // 1..1000 per mille
    int32_t gate;               // "conflicts_gate": 0 / 1 - refresh rule 9
    float tau;                  // (float)iou_pm / 1000.0f, one binary32 divide (the host's)
    int32_t reserved[4];
};
#define VT_CONFLICT_DEFAULT_POLICY ConflictPolicy{0, 300, 0, 0.3f, {0, 0, 0, 0}}
#define VT_CONFLICT_MAX_SCENE 65535
// per stream, beside the policy: diagnostics, never rewound - a redone pass may count twice (like skipped_geometry)
struct ConflictCount {
    int32_t evaluated;          // records written with status 1 or 2
    int32_t conflicting;        // of which status 2
    int32_t gated;              // refreshes that rules 1-5 allowed and rule 9 refused
    int32_t reserved;
};
struct ConflictArgs {
    const StreamState* states;  // [B] by stream, as decode / cand_commit / motion_settle left them
    const vt_result* results;   // [n] by slot
    const int32_t* slot_stream; // [n] slot -> stream, null: the identity
    const int32_t* winner;      // candidate pass: [n] the winning slot of slot i's stream (only winners work); else null
    const ConflictPolicy* policy;   // the engine's record
    const int32_t* scenes;      // [B] by stream; 0: compared with nobody
    ConflictRec* recs;          // [B] by stream
    ConflictCount* counts;      // [B] by stream
    const PassOut* out;         // device copy of the pass's PassOut: host_conflicts; may be null
    int n;
};
// behind the decode (candidate pass: the commit) and motion_settle, ahead of the appearance, proposals, refresh, chip, peaks
// and overlay launches: one workgroup, one lane per slot (n <= VT_MAX_STREAMS), the records and counters of the pass's streams
hipError_t launch_conflicts_check(const ConflictArgs& a, hipStream_t st);

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

// The head's convolutions on the band kernel of k_head.hip: out[B*grid*grid][N] bf16 = relu(conv(in) + bias).
// conv3x3: in [B*grid*grid][C] (ldin >= C), W [N][9*C] with column (ky*3+kx)*C + c, zero padding (zeros: >= 256 B
// of zeros in device memory), N == C; else a 1x1 layer: in [B*grid*grid][K], W [N][K].
struct HeadConvArgs {
    const bf16_t* in; int ldin;
    const bf16_t* W; int ldw;
    const float* bias;
    bf16_t* out; int ldout;
    const bf16_t* zeros;
    int B, grid, C, N, K;
    int conv3x3;
    int R, ncb;                 // rows per band / 16-column blocks per wave; <= 0: planned by the launcher
    unsigned* band_cnt;         // fused tail only: [B] arrival counters, zero between launches
    float* band_best;           // fused tail only: [B][bands][2] each band's argmax candidate (response, cell), bands <= grid
    int bands, mbe_max;         // filled in by the launcher
    unsigned long long* dbg;    // diagnostic builds only (VT_STAMPS): per-wave cycle sums [wgs][8][4]
    // 1x1 layer with the final LayerNorm inside (xh != nullptr; `in` is ignored): the layer's input row (b, cell) is
    // LayerNorm(xh + xl)[b * in_stride + in_off + cell][0..K) with gamma ln_g, beta ln_b
    const bf16_t* xh;
    const uint8_t* xl;
    const float *ln_g, *ln_b;
    float ln_eps;
    int in_stride, in_off;
    float lo_q = 1.0f / 4096.0f;    // the pair's quantum 2^-s (LoQuant.q)
};
bool headconv_supported(int grid, int C, int N, int K, bool conv3x3);
bool headconv_ln_supported(int grid, int N, int D);
bool headconv_plannable(int grid, int C, int N, int K, bool conv3x3, bool tail);   // supported and some band height fits LDS
hipError_t headconv_prepare();     // once per device, before the first launch / any stream capture
// dec != nullptr (3x3 layers only): the 5-logit layer, the score window, the argmax and the box decode run inside
// the same launch (dec->t3 is ignored: the logits are computed from the layer's own output tile)
hipError_t launch_headconv(HeadConvArgs a, const DecodeArgs* dec, hipStream_t st);

// ---- kernel launches -----------------------------------------------------------------------------
// Every kernel of the library is launched through vt_launch. It is hipLaunchKernelGGL, except while the engine's
// instrumented pass (vt_group_profile_device) has armed a probe on the calling thread: the first launch behind the arming
// then goes through hipExtLaunchKernelGGL with the probe's two HIP events, which receive the begin and end timestamps of
// THAT dispatch - the duration rocprofv3's kernel trace reports - instead of the time between two marker packets around
// it (which adds the dispatch and marker latency, ~4 us per launch on this stack).
struct LaunchProbe { hipEvent_t start, stop; int launches; };
extern thread_local LaunchProbe* vt_launch_probe;
template <typename F, typename... Args>
inline void vt_launch(F kernel, const dim3& grid, const dim3& block, size_t smem, hipStream_t st, Args... args) {
    LaunchProbe* pr = vt_launch_probe;
    if (pr && pr->launches++ == 0) hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)smem, st, pr->start, pr->stop, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, smem, st, args...);
}

// ---- small device helpers ---------------------------------------------------------------------

__device__ __forceinline__ float bf16_to_f32(bf16_t b) {
    return __uint_as_float(((uint32_t)b) << 16);
}
// f32 -> bf16, round to nearest even, NaN kept a NaN: one v_cvt_pk_bf16_f32 (gfx950). Same
// result as the integer rounding (u + 0x7fff + ((u >> 16) & 1)) >> 16 of the oracle for every
// finite input. Observed on the MI355X through the ReLU, GELU and QKV epilogues of configurations 2, 3, 18
// and 19 (tests/test_gpu_epilogue_edges.py): every normal bf16 pattern, both tie directions at every
// exponent, the band that rounds to infinity and 4 * 10^5 ordinary values come back as the oracle's bits;
// so do the subnormal inputs (bf16 subnormal patterns, their ties, a subnormal q = y * QK_SCALE) - none is
// flushed to zero, in the scalar or in the packed form (profiles/epilogue_edges.txt).
typedef __bf16 bf16v2_t __attribute__((ext_vector_type(2)));
typedef float f32v2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ bf16_t f32_to_bf16(float f) {
    return __builtin_bit_cast(bf16_t, (__bf16)f);
}
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    const f32v2_t v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16v2_t));
}

// ---- one LayerNorm row by half a wave (D = 256 * NCH) -------------------------------------------
// Lane l32 of the half-wave owns the 8-float chunks c = l32 + 32 j, j < NCH. Two-pass variance; the sums run
// over a lane's chunks in ascending order, then over the 32 lanes as an xor butterfly (16, 8, 4, 2, 1). The ONE
// definition of this arithmetic: the LayerNorm kernel (k_misc.hip) and the head's first layer, which normalises
// its band's rows itself (k_head.hip), produce the same bits by construction.
// Sum over the 32 lanes of a half-wave, every lane gets the total: the xor butterfly 16, 8, 4, 2, 1 in registers -
// v_permlane16_swap (odd 16-lane rows of one operand <-> even rows of the other: both copies of v, so a lane ends up
// holding its own and its xor-16 partner's value), row_ror:8, two masked row shifts by 4 (DPP has no xor-4 pattern:
// banks 0 / 2 of a row take lane + 4, banks 1 / 3 lane - 4), two quad_perms. Same partners in the same order as
// "for (off = 16; off >= 1; off >>= 1) v += __shfl_xor(v, off)" and therefore the same bits (tools/dpp_xor_check.hip), without
// that form's five dependent LDS round trips (ds_bpermute) per sum.
// PRECONDITION - FULL EXEC: every lane of the wave must be active at the call. A DPP / permlane source lane that is
// masked off reads as 0 (bound_ctrl) or keeps the old value, so under divergence (`if (r < rows) ln_row(...)`) the sums
// would silently miss terms. All callers keep the wave uniform: rows past the end are CLAMPED to the last row and only
// the stores are guarded (k_misc.hip layernorm kernels, k_head.hip LNC path). The same holds for quad_sum / row16_sum /
// row8_sum of k_gemm_util.hpp and k_head.hip. The s_nop counts inside the asm are the gfx950 wait states (VALU write ->
// permlane read: 2; permlane write -> VALU read: 2) the compiler cannot check there; tools/dpp_xor_check.hip (run by
// tests/test_gpu_ops.py on the box, built with the box's ROCm) guards both the workaround and those counts.
__device__ __forceinline__ float half_wave_sum(float v) {
    // inline asm, not __builtin_amdgcn_permlane16_swap: on float operands hipcc (ROCm 7.2) adds the swap's FIRST result to
    // itself (the integer form compiles correctly; tools/dpp_xor_check.hip caught it). s_nop: VALU write -> permlane read
    // and permlane write -> VALU read wait states, which the compiler cannot see inside the asm.
    float lo, hi;
    asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %2\n\ts_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1"
                 : "=&v"(lo), "=&v"(hi) : "v"(v));
    v = lo + hi;
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x128, 0xF, 0xF, true));       // row_ror:8
    int t = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x104, 0xF, 0x5, false);                       // row_shl:4 -> banks 0, 2
    t = __builtin_amdgcn_update_dpp(t, __builtin_bit_cast(int, v), 0x114, 0xF, 0xA, false);                           // row_shr:4 -> banks 1, 3
    v += __builtin_bit_cast(float, t);
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));        // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));        // quad_perm [1,0,3,2]
    return v;
}

template <int NCH>
struct LnCoef { f32x4_t g[NCH][2], b[NCH][2]; };

template <int NCH>
__device__ __forceinline__ void ln_load_coef(const float* gamma, const float* beta, int l32, LnCoef<NCH>& k) {
    const f32x4_t* g4 = reinterpret_cast<const f32x4_t*>(gamma);
    const f32x4_t* b4 = reinterpret_cast<const f32x4_t*>(beta);
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c = l32 + 32 * j;
        k.g[j][0] = g4[2 * c]; k.g[j][1] = g4[2 * c + 1];
        k.b[j][0] = b4[2 * c]; k.b[j][1] = b4[2 * c + 1];
    }
    // hipcc otherwise sinks these loads behind the row's reductions: pin the values here, all loads issued
#pragma unroll
    for (int j = 0; j < NCH; ++j)
        asm volatile("" : "+v"(k.g[j][0]), "+v"(k.g[j][1]), "+v"(k.b[j][0]), "+v"(k.b[j][1]) : : "memory");
}

// ---- the 3-byte residual pair (specification v3, top of this file) -------------------------------------------------
// decode: element k of a lane's 8 consecutive columns = bf16 half k of h (16 B) + signed byte k of l (8 B) * q, q = 2^-s
__device__ __forceinline__ float lo8_f32(uint32_t w, int byte) {
    return (float)((int)(w << (24 - 8 * byte)) >> 24);          // sign-extended byte (v_bfe_i32 / SDWA sext) -> float
}
__device__ __forceinline__ void x_join8(const u32x4_t& hi, const u32x2_t& lo, float q, float (&x)[8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t lw = lo[e >> 1];
        x[2 * e] = __builtin_fmaf(lo8_f32(lw, (2 * e) & 3), q, __uint_as_float(hi[e] << 16));
        x[2 * e + 1] = __builtin_fmaf(lo8_f32(lw, (2 * e + 1) & 3), q, __uint_as_float(hi[e] & 0xffff0000u));
    }
}
// encode: hi = bf16(x) (round to nearest even); d = x - hi (exact); lo8 = rint(clamp(d, +-127 q) / q) by the float add of
// magic = 1.5 * 2^(23 - s): the sum's ulp is q = 2^-s, the add rounds to nearest even, and the low byte of the sum's bit
// pattern (at s = 12: 0x45400000 + n) is the two's-complement lo8 - for every s in 6..14 alike. The clamp and the magic
// are wave-uniform (LoQuant): v_med3_f32 takes the one SGPR as -lo_max and lo_max (a source modifier, one constant-bus
// read), the SDWA add its magic from a register as before. The add is issued in its SDWA form with dst_sel:BYTE_k, which writes that
// low byte straight into byte k of the destination dword - no extraction, no packing: 2 vector operations per element
// (v_med3_f32 + v_add_f32_sdwa) where clamp + add + v_perm gathering took 2.75 (same-box A/B in profiles/r06_lo8_residual.txt:
// + 0.5 % of the whole frame; without the clamp another + 0.2 %, not taken: a value beyond the range must saturate, not wrap).
__device__ __forceinline__ void x_split8(const float (&x)[8], const LoQuant& lq, u32x4_t& hi, u32x2_t& lo) {
    uint32_t h[4];
    float c[8];
    const float lo_max = lq.lo_max;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        h[e] = pack_bf16x2(x[2 * e], x[2 * e + 1]);
        c[2 * e] = __builtin_amdgcn_fmed3f(x[2 * e] - __uint_as_float(h[e] << 16), -lo_max, lo_max);
        c[2 * e + 1] = __builtin_amdgcn_fmed3f(x[2 * e + 1] - __uint_as_float(h[e] & 0xffff0000u), -lo_max, lo_max);
    }
    hi = u32x4_t{h[0], h[1], h[2], h[3]};
    const float magic = lq.magic;           // SDWA takes no literal: a register
    uint32_t w0, w1;
#define VT_LO8_BYTE(W, K, UNUSED, C) asm("v_add_f32_sdwa %0, %1, %2 dst_sel:BYTE_" #K " dst_unused:" #UNUSED " src0_sel:DWORD src1_sel:DWORD" : W : "v"(C), "v"(magic))
    VT_LO8_BYTE("=v"(w0), 0, UNUSED_PAD, c[0]); VT_LO8_BYTE("+v"(w0), 1, UNUSED_PRESERVE, c[1]);
    VT_LO8_BYTE("+v"(w0), 2, UNUSED_PRESERVE, c[2]); VT_LO8_BYTE("+v"(w0), 3, UNUSED_PRESERVE, c[3]);
    VT_LO8_BYTE("=v"(w1), 0, UNUSED_PAD, c[4]); VT_LO8_BYTE("+v"(w1), 1, UNUSED_PRESERVE, c[5]);
    VT_LO8_BYTE("+v"(w1), 2, UNUSED_PRESERVE, c[6]); VT_LO8_BYTE("+v"(w1), 3, UNUSED_PRESERVE, c[7]);
#undef VT_LO8_BYTE
    lo = u32x2_t{w0, w1};
}
// the LayerNorm readers' form: 8 values of a chunk as two float4
__device__ __forceinline__ void ln_unpack_split(const u32x4_t h, const u32x2_t l, float q, f32x4_t (&v)[2]) {
    float x[8];
    x_join8(h, l, q, x);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e >> 2][e & 3] = x[e];
}

// v: the row's values of this lane (overwritten); o[j]: the normalised chunk l32 + 32 j as 8 bf16
template <int NCH>
__device__ __forceinline__ void ln_row(f32x4_t (&v)[NCH][2], const LnCoef<NCH>& k, int D, float eps, uint4 (&o)[NCH]) {
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) sum += v[j][0][e] + v[j][1][e];
    sum = half_wave_sum(sum);
    const float mean = sum / (float)D;
    float sq = 0.0f;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[j][h][e] -= mean;
                sq += v[j][h][e] * v[j][h][e];
            }
    sq = half_wave_sum(sq);
    const float rstd = 1.0f / sqrtf(sq / (float)D + eps);
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const f32x4_t g0 = k.g[j][0], g1 = k.g[j][1], b0 = k.b[j][0], b1 = k.b[j][1];
        o[j].x = pack_bf16x2((v[j][0][0] * rstd) * g0[0] + b0[0], (v[j][0][1] * rstd) * g0[1] + b0[1]);
        o[j].y = pack_bf16x2((v[j][0][2] * rstd) * g0[2] + b0[2], (v[j][0][3] * rstd) * g0[3] + b0[3]);
        o[j].z = pack_bf16x2((v[j][1][0] * rstd) * g1[0] + b1[0], (v[j][1][1] * rstd) * g1[1] + b1[1]);
        o[j].w = pack_bf16x2((v[j][1][2] * rstd) * g1[2] + b1[2], (v[j][1][3] * rstd) * g1[3] + b1[3]);
    }
}
