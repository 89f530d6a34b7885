// k_gemm.hpp — the GEMM launch API (k_gemm.hip, k_gemm256.hip): the residual pair's specification, epilogues, GemmArgs.
#pragma once
#include "vt_common.hpp"

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
const char* gemm256_build_id();   // sha256 of k_gemm256.hip + its include closure (build.py: STAMPED, exactly that closure) + its compile flags (-DVT_TU_SHA256)
hipError_t launch_gemm256(const GemmArgs& a, int epilogue, bool persistent, hipStream_t st);
bool gemm256_fits(const GemmArgs& a, int epilogue);
// the tile configuration launch_gemm() runs for these arguments (the picker's choice, or the 4-wave
// kernel where a 256x256 choice does not fit the operands)
int gemm_effective_config(const GemmArgs& a, int epilogue);
