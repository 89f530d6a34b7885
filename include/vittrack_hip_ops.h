/*
 * vittrack_hip_ops.h — operator-level entry points of libvittrack_hip_ops.so: numerics tests and tuning
 * tools call the same kernel launchers (same objects) the tracker pass uses, on operands of their choosing.
 * NOT part of the product boundary: libvittrack_hip.so (include/vittrack_hip.h, the drop-in for the
 * reference's vit_tracker crate, src/tracker_context.rs:21,88,90,120) exports none of these; the ops
 * library is that library's objects plus csrc/vt_ops.hip and exports the boundary as well, so one handle
 * serves a test that needs both.
 */
#ifndef VITTRACK_HIP_OPS_H
#define VITTRACK_HIP_OPS_H

#include "vittrack_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- operator-level entry points (numerics tests call the same kernels the pass uses) ----
 * Every hook that hands results back puts each device buffer a kernel writes between two 4 KiB guard bands: a store into
 * a band is VT_ERR_HIP with a message naming the buffer. A pure output is filled with 0xff before the launch, so an
 * element the kernel never stores comes back as NaN (bf16, float32, the pair) or as 0xff bytes; a buffer whose start
 * value belongs to the contract keeps it (Vt and counters: zeros; an addend updated in place, states, records: the
 * caller's bytes). The timing entry points (*_bench, a hook's iters / us_out loop) are not checked. */

/* acc[M,N] = A[M,K] (bf16 bits) x W[N,K]^T (bf16 bits), float32 accumulation. Host pointers.
 * K % 64 == 0, N % 64 == 0. cfg: tile configuration as in vt_op_gemm_bench (< 0: the launcher's own
 * choice for the shape). epilogue:
 *   0  x = acc + bias                    the X-epilogues the engine keeps its residual stream with: x is
 *   1  x = (acc + bias) + c_inout        stored as the 3-byte pair (hi = bf16(x), lo8 = clamp(rint((x - hi) * 2^lo_shift), +-127))
 *   4  x = (acc + bias) + pos            and comes back as hi + lo8 * 2^-lo_shift (lo_shift 6..14, the engine's default is
 *                                        12; epilogue 1 takes c_inout through the same pair); pos = c_inout, one row per
 *                                        output row. rowstat_out (may be NULL) receives per row the terms
 *                                        (rstd, -mean * rstd) of LayerNorm(x) with `eps`, computed from the
 *                                        float32 x before the split (what the consuming GEMM multiplies with).
 *   2  GELU(y) -> bf16, 3  ReLU(y) -> bf16 (returned widened to f32); y = acc + bias, or with a folded
 *      LayerNorm (rowstat_in [M][2] and colsum [N] not NULL): y = rowstat_in[m][0] * acc +
 *      (rowstat_in[m][1] * colsum[n] + bias[n]). */
int vt_op_gemm_bf16_lo(int device_id, const uint16_t* a, const uint16_t* w, const float* bias,
                       float* c_inout, int M, int N, int K, int epilogue, int cfg,
                       const float* rowstat_in, const float* colsum, float* rowstat_out, float eps, int lo_shift);
/* The residual GEMM (epilogue 1) on the 256x256 kernel, on a pair given as it is stored, with the remapped addend read
 * the last encoder block uses: x[m] = (A W^T + bias)[m] + pair_in[m + (m / seg_rows + 1) * seg_skip], m < M - the input
 * layout has seg_skip rows nobody computes in front of every segment of seg_rows rows (seg_rows even). xh_in (bf16 bits)
 * / xl_in (signed bytes): [rows_in][N]; xh_out / xl_out [M][N]; cstat_out (may be NULL) [M][N / 32][2] the chunk
 * partials (sum, M2); rowstat_out (may be NULL) [M][2] the row terms with `eps`, finalized inside the launch.
 * seg_rows = 0 (seg_skip = 0): the launch as vt_op_gemm_bf16_lo(epilogue 1, cfg 18) runs it - rows 0 .. M-1 of the input
 * pair, read and written in place. N % 256 == 0, K % 64 == 0, K >= 128; anything the kernel does not take:
 * VT_ERR_INVALID_ARG. */
int vt_op_gemm_resid_seg_bf16(int device_id, const uint16_t* a, const uint16_t* w, const float* bias, const uint16_t* xh_in,
                              const int8_t* xl_in, int rows_in, uint16_t* xh_out, int8_t* xl_out, float* cstat_out,
                              float* rowstat_out, int M, int N, int K, int seg_rows, int seg_skip, float eps, int lo_shift);
/* Kernel-tuning helper: mean microseconds per launch of the GEMM kernel on device-resident random
 * operands. epilogue uses the library's internal numbering (0 f32+pos, 1 residual, 2 GELU, 3 ReLU,
 * 4 QKV, 5 f32); cfg: 0 = 64x64 ring 4, 1 = 128x128 ring 3, 2 = 64x64 ring 2, 3 = 128x128 ring 2
 * (K-tile depth 64); 4 = 64x64 ring 3, 5 = 64x64 ring 2, 6 = 128x128 ring 2 (K-tile depth 128, K % 128 == 0);
 * 7 = 64x64 ring 3 and 8 = 128x64 ring 3 with four loader waves (K-tile depth 128);
 * 18 / 19 = 256x256 8-wave kernels (one tile per workgroup / persistent); <0 = the launcher's own choice.
 * Bits 8-9 of a cfg >= 0 (here, in vt_op_gemm_bf16_lo and in vt_op_qkv_bf16) force the order in which an XCD's run of
 * workgroups covers the tile grid of configurations 0-8: 0 = the launcher's rule, 1 = row panels x all columns,
 * 2 = column tiles x all rows (placement only: the results are the same bits). */
int vt_op_gemm_bench(int device_id, int M, int N, int K, int epilogue, int cfg, int iters,
                     float* us_out);
/* The head's 3x3 convolution (zero padding) + bias + ReLU as the engine runs it - an implicit GEMM whose
 * A loads gather the im2col row: t [B*grid*grid][C] bf16, w [N][9*C] bf16 (column (ky*3+kx)*C + c),
 * out [B*grid*grid][N] (bf16 widened to f32). C % 64 == 0, N % 64 == 0; cfg 0..8 (4..6: C % 128 == 0; 7, 8: the
 * loader-wave forms of 0 / 4), < 0: launcher's choice. */
int vt_op_conv3x3_relu_bf16(int device_id, const uint16_t* t, const uint16_t* w, const float* bias,
                            float* out, int B, int grid, int C, int N, int cfg);
/* The head's band kernel (csrc/k_head.hip) on its own: out = relu(conv(t) + bias). conv3x3 != 0: t [B*grid*grid][Cin],
 * w [N][9*Cin] (column (ky*3+kx)*Cin + c), N == Cin, zero padding; else the 1x1 layer, w [N][Cin]. R (rows of the
 * map per workgroup) / ncb (16-column blocks per wave) <= 0: the launcher's plan. t == NULL: operands filled with a
 * fixed pseudo-random pattern (timing runs). out (nullable): bf16 values widened to f32. us_out (nullable): mean
 * microseconds per launch over `iters` launches; asking for it with iters < 1 is VT_ERR_INVALID_ARG, as in the timing
 * helpers. */
int vt_op_headconv_bf16(int device_id, const uint16_t* t, const uint16_t* w, const float* bias, float* out,
                        int B, int grid, int Cin, int N, int conv3x3, int R, int ncb, int iters, float* us_out);
/* The head's first (1x1) layer with the final LayerNorm in front of it: out[b*grid*grid + cell][n] =
 * relu(LayerNorm(xh + xl * 2^-lo_shift)[b*ntok + off + cell] . w[n] + bias[n]); xh (bf16 bits) / xl (signed bytes) [B*ntok][D] the
 * 3-byte pair of the residual stream with the quantum 2^-lo_shift (6..14, the engine's default is 12), gamma / beta [D],
 * w [N][D], D = 768 or 1024. fused != 0: ONE launch - the band kernel normalises its band's
 * rows itself (what the engine runs); fused == 0: the LayerNorm kernel, then the band kernel on its output - the fused
 * form reproduces it bit for bit: fused == 0 runs the stand-alone LayerNorm kernel's pair reader (csrc/k_misc.hip),
 * fused != 0 the band kernel's. R / ncb / iters / us_out / out as above; xh == NULL: synthetic operands (timing). */
int vt_op_headconv_ln_bf16_lo(int device_id, const uint16_t* xh, const int8_t* xl, const float* gamma, const float* beta,
                              float eps, int ntok, int off, const uint16_t* w, const float* bias, float* out, int B, int grid,
                              int D, int N, int fused, int R, int ncb, int iters, float* us_out, int lo_shift);
/* The head's decode stage (csrc/k_head.hip) on operands of the caller's choosing: the 5-logit layer, the Hann-weighted
 * argmax, the 3x3 window, the box and the write-back of states, results and the two host mirrors.
 *   form 0  launch_decode: head_out_kernel + decode_kernel on t = t3 [B*grid*grid][C] (C even; w3 / b3 / R ignored)
 *   form 1  launch_headconv with the fused tail: the last 3x3 layer (w3 [C][9*C] bf16 bits, b3 [C]) on t, then logits,
 *           hand-off and decode inside the launch, with band counters and candidates of its own (zeroed once, before
 *           the first launch). R rows per band, <= 0: the launcher's plan.
 * `launches` (>= 1) launches run back to back on the same buffers. t: bf16 bits; w4 [8][C], b4 [8], hann [grid*grid];
 * states: n_states records of 88 bytes (StreamState as vt_export_state lays it out), in and out; slot_stream (nullable)
 * [B]: slot -> stream, distinct indices < n_states (NULL: the identity, n_states >= B). Out: head_out [B*grid*grid][8],
 * results [B] (the device array), host_results [B] / host_states [n_states] (the pinned mirrors the kernel stores to;
 * their initial contents are the caller's, so untouched records are recognisable; flags bit 0 / bit 1: run with that
 * mirror null, the buffer comes back as it went in), band_cnt [B] the counters after the last launch (form 0: zeros).
 * Whatever the launchers refuse (form 1: a shape headconv_plannable rejects, R * grid > 112 cells, a band that does
 * not fit LDS) and a slot map that does not fit n_states: VT_ERR_INVALID_ARG. */
int vt_op_head_decode(int device_id, int form, const uint16_t* t, const uint16_t* w3, const float* b3, const float* w4,
                      const float* b4, const float* hann, void* states, int n_states, const int32_t* slot_stream,
                      float success_threshold, int B, int grid, int C, int R, int launches, int flags, float* head_out,
                      vt_result* results, vt_result* host_results, void* host_states, uint32_t* band_cnt);
/* The response-peaks launch (csrc/k_peaks.hip, vt_group_set_peaks of vittrack_hip.h) on given operands, and nothing
 * else: head_out [B*grid*grid][8] float logits by slot (what a decode left), hann [grid*grid], states: n_states records of
 * 88 bytes (in and out: the launch writes none of them, they come back as they went in), policies: n_states records of 16
 * bytes by stream (int32 max_peaks 0..8, int32 radius 1..4, float min_resp, int32 reserved), slot_stream (nullable) [B]:
 * slot -> stream < n_states (NULL: the identity, n_states >= B), winner (nullable) [B]: a candidate pass's winner table,
 * only slots with winner[i] == i list. In and out: records [B] (the device array) and host_records [B] (the pinned mirror
 * the kernel stores to); their initial contents are the caller's, so untouched words are recognisable. A policy or map out
 * of range, grid > 110: VT_ERR_INVALID_ARG. */
int vt_op_response_peaks(int device_id, const float* head_out, const float* hann, void* states, int n_states,
                         const void* policies, const int32_t* slot_stream, const int32_t* winner, int B, int grid,
                         vt_peaks* records, vt_peaks* host_records);
/* The result-overlay launch (csrc/k_result_overlay.hip, the "result_overlay" keys of vt_group_set_tuning in vittrack_hip.h)
 * on given operands, and nothing else. frames [n] by slot: DEVICE planes, checked like a pass's frames - they are WRITTEN;
 * results [n] by slot; slot_stream (nullable) [n]: slot -> stream < n_streams (NULL: the identity, n_streams >= n); winner
 * (nullable) [n]: a candidate pass's winner table, only slots with winner[i] == i draw; policy: 8 int32 - flags 0..7,
 * thickness 1..16, size 1..64, scale 1..4, luma 0..255, rgb 0..0xFFFFFF, min_score_pct 0..100, reserved; stats (in and
 * out): n_streams records of 8 int32 by stream - drawn by this launch, passes drawn, gated, on a format that is not
 * drawable, N of the last label, 3 reserved; device_frames: the pass's device-frames word (0: a host pass, nothing draws).
 * The boxes are the caller's: any int32 values. A policy, map or frame out of range: VT_ERR_INVALID_ARG. */
int vt_op_result_overlay(int device_id, const vt_frame* frames, const vt_result* results, const int32_t* slot_stream,
                         const int32_t* winner, int n, const int32_t* policy, int32_t* stats, int n_streams,
                         int device_frames);
/* The two launches of the motion prior (csrc/k_motion.hip, the "motion_*" keys of vt_group_set_tuning in vittrack_hip.h) on
 * given operands, and nothing else: stages bit 0 = place, bit 1 = settle, run in that order. states: n_streams records of 88
 * bytes, records: n_streams records of 48 bytes by stream (float v[2], prior[4], shift[2], int32 live, passes shifted,
 * failures coasted, reserved) - both in and out; policy: 4 int32 (on 0..1, gain_pct 1..100, coast 0..60, max_pct 0..200);
 * results [n] by slot (settle reads success); slot_stream (nullable) [n]: slot -> stream < n_streams (NULL: the identity,
 * n_streams >= n). The candidate form: cands [n] (the map is cands[i].stream, slot_stream is ignored; streams may repeat,
 * place works once per stream) with winner [n], the commit's winner table - only slots with winner[i] == i settle, with
 * their own has_box. cands and winner are both NULL or both given. host_states / host_records (nullable, in and out):
 * [n_streams] the pinned mirrors the settle launch stores the final box and the record to; their initial contents are the
 * caller's, so untouched words are recognisable. A policy or map out of range, n > 1024: VT_ERR_INVALID_ARG. */
int vt_op_motion_prior(int device_id, void* states, void* records, int n_streams, const int32_t* policy, const vt_result* results,
                       const int32_t* slot_stream, const int32_t* winner, const vt_candidate* cands, int n, int stages,
                       void* host_states, void* host_records);
/* The score launch of the appearance check (csrc/k_appearance.hip, the "appearance*" keys of vt_group_set_tuning in
 * vittrack_hip.h) on caller-supplied rows, and nothing else. anchor, probe: [n_slots][nt][kpad] bf16 bit patterns; the sums
 * run over columns [0, cols) of every row, columns [cols, kpad) are never read. Per slot: sums[5] = Sa, Sp, Saa, Spp, Sap
 * in binary64 (every element the exact value of its bf16, the kernel's fixed order of additions), similarity (binary32,
 * clamped to [-1, 1]) and status (1, or 3 where a variance is not positive: similarity 0).
 * n_slots > 1024, nt or kpad > 65536, kpad < cols: VT_ERR_INVALID_ARG. */
int vt_op_appearance_score(int device_id, const uint16_t* anchor, const uint16_t* probe, int n_slots, int nt, int kpad, int cols,
                           double* sums, float* similarity, int32_t* status);
/* The four launches of the reacquire proposals (csrc/k_proposals.hip, the "proposals*" keys of vt_group_set_tuning in
 * vittrack_hip.h) on caller-supplied operands, and nothing else. frames: [n] by slot with DEVICE planes (read only);
 * states: [n_streams] raw 88-byte stream states, of which box, frames_done and tpl_gen are read; results: [n] by slot
 * (success is read); slot_stream: [n] slot -> stream or null (the identity); winner: [n] a candidate pass's winner table
 * or null; tpl: [n_streams][tpl_bufs][(T/patch)^2][kpad] bf16 bit patterns in the patch-row layout of the template rows
 * (tpl_bufs 2: a stream's rows are buffer tpl_gen & 1); norm: a0, a1, a2, b0, b1, b2; policy: 8 int32 = mode, period, max,
 * min_sim_pm, (tau: derived here), max_cells (256..4,194,304), 0, 0; device_frames: 0 = the launches of a host-pointer pass.
 * Out: pattern [n][256] int16 (M x M at the front), thumb [n][max_cells] int16 (Hg x Wg at the front), map [n][max_cells]
 * float ((Hg - M + 1) x (Wg - M + 1) at the front), records [n_streams] of 224 bytes (status, frames_done, n, c, Wg, Hg,
 * 2 reserved words, 8 x (sim, box[4], position)), evaluated [n_streams] in and out. Every output byte no launch stored is
 * 0xff. The four device outputs sit between guard bands; a changed guard byte is VT_ERR_HIP. */
int vt_op_proposals(int device_id, const vt_frame* frames, const void* states, int n_streams, const vt_result* results,
                    const int32_t* slot_stream, const int32_t* winner, int n, const uint16_t* tpl, int tpl_bufs, int T, int patch,
                    int kpad, const float* norm, const int32_t* policy, int device_frames, int16_t* pattern, int16_t* thumb,
                    float* map, void* records, int32_t* evaluated);
/* The four launches of the camera motion (csrc/k_camera_motion.hip; DESIGN.md section 3 "Camera motion") on caller-supplied
 * operands, and nothing else: per stream the translation of the whole picture since the stream's last call, measured from
 * two uint16 thumbnails by an exact integer SAD search, and with mode 2 the stream's box moved by it. No engine pass
 * carries the launches yet: this hook is their only caller. THE RULE, to the bit:
 *   POLICY: 8 int32 = mode (0 off, 1 measure and report, 2 measure, report and move the box), cell (0 = automatic, or 4, 8,
 * 16, 32: cell side in source pixels), range (R = 2..16 cells searched each way), conf_pm (0..1000 per mille), max_cells
 * (4,096..1,048,576 thumbnail cells per stream), 0, 0, 0 - the bounds of the table kCameraKeys of csrc/vt_feature_keys.hpp,
 * which names the words "camera_motion", "camera_motion_cell", "camera_motion_range", "camera_motion_conf_pm" and
 * "camera_motion_max_cells" (defaults 0, 0, 8, 800, 65,536).
 *   DUE: slot i with stream s is due iff (a) the mode is not 0; (b) it is the first slot naming s; (c) s is initialised;
 * (d) device_frames != 0; (e) the planes hold the whole frame (windowed != 1). Not due by (a) or (c): status 0. Failing (d)
 * or (e): status 4. A listed stream that is not evaluated (status 0, 2 or 4) loses its previous thumbnail (has_prev = 0).
 *   GEOMETRY: W, H the frame's size; c the key's cell, or with 0 the smallest of 4, 8, 16, 32, 64 with (W / c) * (H / c) <=
 * max_cells (integer divisions). Wg = W / c, Hg = H / c: whole cells only, a partial column or row at the right or bottom
 * edge is not used. Status 2, nothing evaluated: no such c, Wg * Hg > max_cells, Wg - 2R < 8 or Hg - 2R < 8.
 *   THUMBNAIL cell (i, j): sixteen taps (u, v), u, v in 0..3, at px = i * c + u * (c / 4) + c / 8 and py likewise (integer
 * expressions; every tap lies inside the frame). A tap is one pixel as the crop reads it - any vt_pixfmt / vt_pixfmt2,
 * integers R, G, B in 0..255 -, its value Y = (77 * R + 150 * G + 29 * B + 128) >> 8; the cell is the sum of the sixteen
 * (0..4080), a uint16.
 *   PREVIOUS: if the stream has no previous thumbnail, or one of another W, H or c: status 5, shift 0, the current thumbnail
 * is kept as the previous one of the next pass.
 *   SEARCH: for dx, dy in -R..R: S(dx, dy) = sum over j in [R, Hg - R), i in [R, Wg - R) of |cur(i, j) - prev(i - dx, j - dy)|,
 * exact in int64; every displacement sums the same n = (Wg - 2R) * (Hg - 2R) cells. Content that moved by +d cells gives
 * S(d) = 0. No floating-point operation, no floating-point atomic: the sums do not depend on the order of additions.
 *   DECISION: the best (dx, dy) is the least (S, dx * dx + dy * dy, (dy + R) * (2R + 1) + (dx + R)) in lexicographic order:
 * ties prefer the smaller displacement, a still picture gives (0, 0). S0 = S(0, 0); S2 = the least S among displacements at
 * Chebyshev distance > 1 from the best. Status, in this order of tests: 3 (flat) S2 == 0; 6 (at the border: the motion may
 * exceed the range) |dx| == R or |dy| == R; 7 (ambiguous) S_best * 1000 > conf_pm * S2 (int64); else 1 (good). The shift is
 * 0 for every status other than 1.
 *   SUB-CELL SHIFT (status 1), per axis with the two neighbours Sm, Sp of the best along that axis: den = Sm - 2 * S_best + Sp
 * (int64); off = (den > 0 && S_best > 0) ? (0.5f * (float)(Sm - Sp)) / (float)den : 0.0f - an exact match (S_best == 0) is a
 * whole-cell shift, whatever its neighbours are -; shift = ((float)d + off) * (float)c. Binary32, one IEEE operation per
 * source operation; the int64 -> binary32 conversions round to nearest even.
 *   APPLY (mode 2, status 1, shift != (0, 0)): px = x + shift_x, py = y + shift_y; if the moved centre (px + 0.5f * w, py +
 * 0.5f * h) satisfies 0 <= cx < (float)frame_w and 0 <= cy < (float)frame_h (the place rule of the motion prior) the state
 * box becomes (px, py, w, h) and applied = 1, else the box stays and applied = 0. The box moves whether or not the update
 * then succeeds: a lost target's last position stays fixed in the scene, not in the picture.
 *   RECORD, per stream: status, frames_done, c, Wg, Hg, R, dx, dy, shift[2], applied, n, S_best, S0, S2 (int64) and the
 * counters evaluated (status 1, 3, 6, 7) and moved (applied); behind them the thumbnails' bookkeeping: has_prev, cur (the
 * buffer of the last thumbnail), pW, pH, pc (the geometry it was taken with).
 *   OPERANDS: frames: [n] by slot with DEVICE planes (read only); states: [n_streams] raw 88-byte stream states, in and out
 * (box[0], box[1] move in mode 2; frame_w, frame_h, initialized, frames_done are read); slot_stream: [n] slot -> stream or
 * null (the identity). In and out: thumbs [n_streams][2][max_cells] uint16 (Hg x Wg at the front of each buffer) and
 * records [n_streams] of 104 bytes. Out: sad [n_streams][1089] int64, (2R + 1)^2 sums at the front of a stream's table,
 * row dy + R, column dx + R; every byte of it no launch stored is 0xff. host_states / host_records (nullable, in and out):
 * [n_streams] pinned mirrors the decide launch stores the moved x, y and the record to. The three device buffers sit
 * between guard bands; a changed guard byte is VT_ERR_HIP. A policy or map out of range, n > 1024: VT_ERR_INVALID_ARG. */
int vt_op_camera_motion(int device_id, const vt_frame* frames, void* states, int n_streams, const int32_t* slot_stream, int n,
                        const int32_t* policy, int device_frames, uint16_t* thumbs, void* records, int64_t* sad,
                        void* host_states, void* host_records);
/* The four launches of the frame health (csrc/k_health.hip; DESIGN.md section 3 "Frame health") on caller-supplied operands,
 * and nothing else: per stream a thumbnail of the whole frame, five exact integer measures of it and of its change since the
 * stream's previous thumbnail, and three flags: the picture is FROZEN, FLAT (covered, blacked out) or CUT to another scene.
 * The engine runs them in every pass of a health-enabled engine (include/vittrack_hip.h, "health*" keys), where refresh rule
 * 10 reads the record and counts `gated`. THE RULE, to the bit:
 *   POLICY: 8 int32 = on (0 / 1), period (1..1,000,000), cell (0 = automatic, or 4, 8, 16, 32), still_run (1..1000), flat_q
 * (0..4080), cut_pm (0..1000 per mille, 0: never), gate (0 / 1: refresh rule 10; read by no launch of this hook), max_cells (4,096..262,144
 * thumbnail cells per stream) - the bounds of the table kHealthKeys of csrc/vt_feature_keys.hpp, which names the words
 * "health", "health_period", "health_cell", "health_still_run", "health_flat_q", "health_cut_pm", "health_gate" and
 * "health_max_cells" (defaults 0, 1, 0, 3, 32, 500, 0, 65,536).
 *   SLOTS: the first slot that names a stream works for it; a later slot of that stream gets header status -1 and does nothing.
 *   STATUS of the working slot, in this order of tests. 0 (not due): on == 0, the stream is not initialised, or frames_done %
 * period != 0 - record, bookkeeping, counters and the previous thumbnail stay as they are. 4: device_frames == 0 or the
 * planes do not hold the whole frame (windowed: x0, y0 != 0 or ww, wh != w, h). 2 (no geometry): with c the key's cell, or
 * with 0 the smallest of 4, 8, 16, 32, 64 with (W / c) * (H / c) <= max_cells (integer divisions), Wg = W / c, Hg = H / c,
 * n = Wg * Hg: no such c, n > max_cells, Wg < 8 or Hg < 8. 5: measured, but the stream has no previous thumbnail, or one of
 * another W, H or c. 1: measured and compared. Statuses 4 and 2 write the record with zero measures and flags (c, Wg, Hg as
 * far as they exist), G_ref = 0, and clear has_prev and still. frames_done is the state's value as the hook receives it.
 *   THUMBNAIL t[j][i], uint16 <= 4080: the cell of vt_op_camera_motion above (sixteen taps, (77 R + 150 G + 29 B + 128) >> 8
 * each, summed). Statuses 1 and 5 store it to the stream's other buffer (cur ^ 1 of the last one; buffer 0 with has_prev 0)
 * and set has_prev = 1, cur, pW, pH, pc.
 *   MEASURES, int64: S1 = sum t; S2 = sum t * t; G = sum over j, i < Wg - 1 of |t[j][i + 1] - t[j][i]| + sum over j < Hg - 1, i
 * of |t[j + 1][i] - t[j][i]|; hist[b] = #{cells: t >> 7 == b}, b = 0..31, int32. Status 1, with p the previous thumbnail and
 * hist_p its histogram: D = sum |t - p|, HD = sum over b of |hist[b] - hist_p[b]|; status 5: D = HD = 0.
 *   STILL: status 1: still = (D == 0) ? min(still + 1, 1 << 30) : 0; status 5: still = 0.
 *   FLAGS: FROZEN (1): status 1 and still >= still_run. FLAT (2): status 1 or 5 and n * S2 - S1 * S1 <= flat_q * flat_q * n * n
 * (the thumbnail's standard deviation is at most flat_q; all products below 2^61). CUT (4): status 1, cut_pm > 0 and HD * 1000
 * >= cut_pm * 2 * n (HD counts every moved cell twice). G_ref := G at status 5 and at a CUT; it stays otherwise.
 *   COUNTERS per stream: evaluated (status 1 or 5), flagged (of which flags != 0), gated (no launch of this hook counts it).
 *   RECORD, per stream, 104 bytes: status, frames_done, flags, c, Wg, Hg, still, a reserved word; S1, S2, G, D, HD, G_ref
 * (int64); has_prev, cur, pW, pH, pc, a reserved word.
 *   OPERANDS: frames: [n] by slot with DEVICE planes (read only); states: [n_streams] raw 88-byte stream states (initialized
 * and frames_done are read; they come back as they went in); slot_stream: [n] slot -> stream or null (the identity). In and
 * out: thumbs [n_streams][2][max_cells] uint16 (Hg x Wg at the front of each buffer), hist [n_streams][2][32] int32, records
 * [n_streams] of 104 bytes, counts [n_streams] of 16 bytes. Out: accs [n_streams][4] int64 = S1, S2, G, D as the launches
 * summed them, heads [n] of 32 bytes (status, stream, frames_done, c, Wg, Hg, cur, 0); every byte of accs no launch stored is
 * 0xff. host_records (nullable, in and out): the [n_streams] pinned mirror of the records. All seven device arrays sit between
 * guard bands; a changed guard byte is VT_ERR_HIP. A policy or map out of range, n > 1024: VT_ERR_INVALID_ARG. */
int vt_op_frame_health(int device_id, const vt_frame* frames, void* states, int n_streams, const int32_t* slot_stream, int n,
                       const int32_t* policy, int device_frames, uint16_t* thumbs, int64_t* accs, int32_t* hist, void* heads,
                       void* records, void* counts, void* host_records);
/* The launches of the moving regions (csrc/k_movers.hip; DESIGN.md section 3 "Moving regions") on caller-supplied operands,
 * and nothing else: per stream a background model of the frame thumbnail's cells, the cells that left it, and the largest
 * 8-connected groups of them as boxes in source pixels. No engine pass carries the launches yet: no "movers*" key of
 * vt_group_set_tuning exists, the names below are those of the key table the hook validates with. THE RULE, to the bit:
 *   POLICY: 8 int32 = on (0 / 1), period (1..1,000,000), cell (0 = automatic, or 4, 8, 16, 32), thr (0..4080), min_area
 * (1..262,144), global_pm (0..1000 per mille; 1000: never), shape = learn (0..8) | min_nb (1..9) << 4 | max_n (1..8) << 8,
 * max_cells (4,096..262,144 cells per stream) - the bounds of the table kMoverKeys of csrc/vt_feature_keys.hpp, which names
 * them "movers", "movers_period", "movers_cell", "movers_thr", "movers_min_area", "movers_global_pm", "movers_learn",
 * "movers_min_nb", "movers_max" (three four-bit fields of one word) and "movers_max_cells" (defaults 0, 1, 0, 96, 4, 400,
 * 4, 3, 4, 65,536). A shape word with a bit set beside its three fields is refused.
 *   SLOTS, STATUS 0, 4, 2: those of vt_op_frame_health above, unchanged - the first slot that names a stream works for it (a
 * later one: header status -1); not due, no whole device frame, no geometry (Wg = W / c, Hg = H / c, Wg, Hg >= 8, Wg * Hg <=
 * max_cells). 5: the stream has no background, or one of another W, H or c. 1: evaluated. Statuses 4 and 2 write the record
 * with zeros (c, Wg, Hg as far as they exist) and clear has_bg and still. frames_done is the state's value as the hook receives it.
 *   THUMBNAIL t[j][i], uint16 <= 4080: the cell of vt_op_camera_motion above. Statuses 1 and 5 store it.
 *   BACKGROUND bg[j][i], uint16 in sixteenths of t (16 * 4080 = 65,280 fits). Status 5: bg = 16 t, every mask byte 0, nothing
 * else is evaluated: the record carries c, Wg, Hg and zeros, still = 0. Status 1: d = 16 t - bg (int32, signed), then bg += d
 * >> learn, where >> is the ARITHMETIC shift of the signed value, floor(d / 2^learn) - a negative d of small size moves bg by
 * -1, never by 0; learn = 0 is plain frame differencing.
 *   MASK: a cell is moving iff |d| > 16 thr, with the d of the background from BEFORE the update.
 *   CLEAN-UP: a cell is kept iff it is moving and at least min_nb of the nine cells of its 3x3 neighbourhood, itself
 * included, are moving; cells outside the grid count as not moving. mask byte: 0, 1 moving, 2 kept.
 *   GLOBAL CHANGE: moving * 1000 > global_pm * Wg * Hg (int64): the record's status is 6, n = 0, components = 0; moving, kept,
 * own_cells and own_kept are written; still = 0.
 *   COMPONENTS (status 1): 8-connectivity over the kept cells. A component's label is the least row-major index j * Wg + i
 * of its cells. Per component its area in cells and the inclusive cell bounding box i0..i1, j0..j1. components = their number,
 * before the two filters below.
 *   LIST: components with area < min_area are dropped; of the rest up to max_n, by area descending, then label ascending.
 * Entry k: x = i0 c, y = j0 c, w = (i1 - i0 + 1) c, h = (j1 - j0 + 1) c (source pixels, int32; an evaluated frame is whole,
 * so the origin of a windowed descriptor is never added: such a frame is status 4), area, label. Entries from n on are zero.
 *   OWN BOX, statuses 1 and 6, from the state's committed box x, y, w, h (binary32 - the one place of the rule that is not
 * integer: each product below is by the power of two 1 / c, exact): x0 = floor(x / c), y0 = floor(y / c), x1 = ceil((x + w) /
 * c), y1 = ceil((y + h) / c), with x + w and y + h binary32 sums, each clipped to 0..Wg or 0..Hg; x1 >= x0 and y1 >= y0
 * forced. own_cells = (x1 - x0)(y1 - y0); own_kept = the kept cells with x0 <= i < x1, y0 <= j < y1.
 *   STILL: status 1: still = (own_kept == 0 and kept > 0) ? min(still + 1, 1 << 30) : 0; statuses 5 and 6: 0.
 *   COUNTERS per stream, never rewound: evaluated (status 1 or 6), listed (the sum of their n).
 *   RECORD, per stream, 256 bytes of int32: status, frames_done, c, Wg, Hg, n, moving, kept, components, own_cells, own_kept,
 * still; has_bg, pW, pH, pc (the background's bookkeeping); eight entries of x, y, w, h, area, label.
 *   OPERANDS: frames: [n] by slot with DEVICE planes (read only); states: [n_streams] raw 88-byte stream states
 * (initialized, frames_done and box are read; they come back as they went in); slot_stream: [n] slot -> stream or null (the
 * identity). In and out: bg [n_streams][max_cells] uint16, mask [n_streams][max_cells] bytes, records [n_streams] of 256
 * bytes, counts [n_streams] of 16 bytes (evaluated, listed, two reserved words). Out: thumbs [n_streams][max_cells] uint16,
 * labels [n_streams][max_cells] int32 (status 1 without a global change: -1, or the cell's component), exts
 * [n_streams][4][max_cells] int32 (at a component's label: i0, i1, j1, area), accs [n_streams][4] int32 (moving, kept), heads
 * [n] of 32 bytes (status, stream, frames_done, c, Wg, Hg, 0, 0); every byte of the five no launch stored is 0xff.
 * host_records (nullable, in and out): the [n_streams] pinned mirror of the records. All ten device arrays sit between guard
 * bands; a changed guard byte is VT_ERR_HIP. A policy or map out of range, n > 1024: VT_ERR_INVALID_ARG. */
int vt_op_movers(int device_id, const vt_frame* frames, void* states, int n_streams, const int32_t* slot_stream, int n,
                 const int32_t* policy, int device_frames, uint16_t* bg, uint16_t* thumbs, uint8_t* mask, int32_t* labels, int32_t* exts,
                 int32_t* accs, void* heads, void* records, void* counts, void* host_records);
/* The one launch of the stream conflicts (csrc/k_conflicts.hip; the rule: include/vittrack_hip.h above the "conflicts*" keys,
 * DESIGN.md section 3 "Stream conflicts") on caller-supplied operands, and nothing else. states: [n_streams] raw 88-byte
 * stream states (box, initialized, frames_done, window_miss are read); results: [n] by slot; slot_stream: [n] slot -> stream
 * or null (the identity); winner: [n] the winning slot of slot i's stream, or null - then the FIRST slot that names a stream
 * works for it; scenes: [n_streams] in 0..65535; policy: 8 int32 = flag, iou_pm, gate, then words the hook ignores (tau is
 * computed from iou_pm as the key does) - validated with the table kConflictKeys of csrc/vt_feature_keys.hpp. In and out:
 * records [n_streams] of 48 bytes and counts [n_streams] of 16 bytes (evaluated, conflicting, gated, reserved), which the
 * caller pre-fills with a pattern: every byte of a stream no lane worked for, and with flag 0 every byte, comes back as it
 * went in. host_records (nullable, in and out): the [n_streams] pinned mirror. Records and counters sit between guard
 * bands; a changed guard byte is VT_ERR_HIP. A policy, scene or map out of range, n > 1024: VT_ERR_INVALID_ARG. */
int vt_op_stream_conflicts(int device_id, const void* states, int n_streams, const vt_result* results, const int32_t* slot_stream,
                           const int32_t* winner, int n, const int32_t* scenes, const int32_t* policy, void* records, void* counts,
                           void* host_records);
/* The four launches of the peak arbitration (csrc/k_arbitrate.hip; DESIGN.md section 3 "Peak arbitration") on caller-supplied
 * operands, and nothing else: arbitrate_list, arbitrate_probe, arbitrate_score, arbitrate_commit, in that order. Where the box
 * the decode committed (peak 0 of the response map) no longer looks like the stream's anchor and a runner-up peak does, the
 * runner-up is committed instead. The engine runs them in every pass of an arbitration-enabled engine (include/vittrack_hip.h,
 * "arbitrate*" keys), directly behind the decode and ahead of motion_settle. THE RULE, to the bit:
 *   POLICY: 8 int32 = on (0 / 1), max (2..4 peaks examined, peak 0 included), radius (1..4), min_resp_pm, low_pm, high_pm
 * (0..1000 per mille each), two reserved words - the bounds of the table kArbKeys of csrc/vt_feature_keys.hpp, which names the
 * words "arbitrate", "arbitrate_max", "arbitrate_radius", "arbitrate_min_resp_pm", "arbitrate_low_pm" and
 * "arbitrate_high_pm" (defaults 0, 3, 2, 50, 300, 500). Each threshold is (float)pm / 1000.0f, one binary32 divide.
 *   LIST: the iteration of vt_op_response_peaks above with max_peaks = max, radius and min_resp = min_resp_pm's threshold:
 * the same cells, scores, responses and float boxes, bit for bit. The integer box of a peak is floorf(v + 0.5f) of its four
 * floats, as the decode rounds.
 *   DUE: on != 0, the pass is no candidate pass (winner == NULL), result.success != 0, window_miss != frames_done, and at
 * least one runner-up k >= 1 is eligible. A runner-up is eligible when its score >= success_threshold (a NaN fails) and its
 * integer box passes refresh rule 6 (the template crop's taps at that box lie inside the taps of the search crop the pass
 * sampled: state.geo). Peaks are examined in listing order, peak 0 first, and the first of these ends the examination:
 * peak 0 fails rule 6 - record status 4; peak 0 or a runner-up with a passing score and rule 6 fails refresh rule 7 (the
 * in-frame part of the template's taps leaves the window stored of the slot's frame) - record status 5, window_miss =
 * frames_done in the state and its mirror, nothing else. Not due: status 0; a candidate pass with on != 0: status 3 for the
 * winning slots' streams, nothing else written.
 *   PROBE: for peak 0 and every eligible runner-up of a due slot the template-sized crop (factor 2, side T) of the slot's
 * frame at the peak's integer box into probe[stream][k]: the rows vt_group_init_* would write at that box, bit for bit.
 *   SCORE: per cut peak the five binary64 sums of vt_op_appearance_score below on anchor[stream] and probe[stream][k], in the
 * same order of additions: the same similarity bits. Peak status 1: scored; 3: a variance is not positive (similarity 0).
 *   COMMIT: with sim[k] the similarity of a peak of status 1, low and high the thresholds: a switch requires sim[0] < low and
 * some eligible k >= 1 with sim[k] >= high. The chosen peak is the one with the largest similarity; on a tie, the lowest k.
 * low_pm 0 challenges nobody (a negative similarity included): the option is inert there.
 * On a switch (record status 2, chosen = k) the result (device and mirror) becomes success 1, the peak's score, its integer
 * box; the state's last_fbox becomes the peak's float box, last_score its score, last_idx its cell, box its integer box, in
 * the state and its mirror. frames_done and success_count stay as the decode left them. Otherwise status 1, chosen = 0 and
 * nothing but the record is written. Counters per stream: evaluated (status 1 or 2), switched (status 2).
 *   RECORD, per stream, 176 bytes: status, frames_done, n (peaks listed; 0 where the slot left before the list), chosen; then
 * four peaks of 40 bytes: cell, status (0: not cut; 1: cut and scored; 2: rule 6 failed; 3: a variance is not positive),
 * score, resp, similarity, a reserved word, the float box. Peaks are marked 1 only in records of status 1 and 2.
 *   OPERANDS: head_out [n * grid^2][8] and hann [grid^2] as for vt_op_response_peaks; frames: [n] by slot with DEVICE planes
 * (read only); states: [n_streams] raw 88-byte stream states, in and out; results: [n] by slot, in and out; slot_stream: [n]
 * slot -> stream or null (the identity); winner: non-null marks a candidate pass; anchor: [n_streams][nt][kpad] bf16 bits, nt
 * = (T / patch)^2; norm: a0, a1, a2, b0, b1, b2 of the crop's normalisation; tier 0..2: the crop body's LDS tier. Out: records
 * [n_streams] of 176 bytes and probe [n_streams][4][nt][kpad], both 0xff where no launch stored; counts [n_streams][2] int32,
 * in and out. host_results [n], host_states [n_streams], host_records [n_streams] (nullable, in and out): pinned mirrors.
 * States, results, records, probe rows, counters, tickets and partials sit between guard bands; a changed guard byte or a
 * ticket left non-zero is VT_ERR_HIP. A policy word the table refuses, a map out of range, n > 1024, and - with winner == NULL -
 * a stream named by two slots: VT_ERR_INVALID_ARG. */
int vt_op_arbitrate(int device_id, const float* head_out, const float* hann, const vt_frame* frames, void* states, int n_streams,
                    vt_result* results, const int32_t* slot_stream, const int32_t* winner, int n, int grid, const uint16_t* anchor,
                    int T, int S, int patch, int kpad, const float* norm, float success_threshold, const int32_t* policy, int tier,
                    void* records, int32_t* counts, uint16_t* probe, vt_result* host_results, void* host_states,
                    void* host_records);
/* The QKV projection with its attention-layout epilogue: a [B*tokens, D], w [3D, D], bias [3D] ->
 * qk_out [B*tokens, 2D] (q scaled by 1/8, then k) and vt_out [B*H, 64, npad] (v transposed per head,
 * npad = tokens rounded up to 64, padding zero); bf16 results widened to f32. cfg as above;
 * vt_perm = 1: Vt in the key order attention mode 3 reads (attn_perm16 inside every 16 keys).
 * rowstat_in [B*tokens][2] / colsum [3D] (both or neither NULL): a folded LayerNorm as in vt_op_gemm_bf16_lo. */
int vt_op_qkv_bf16(int device_id, const uint16_t* a, const uint16_t* w, const float* bias,
                   float* qk_out, float* vt_out, int B, int tokens, int D, int cfg, int vt_perm,
                   const float* rowstat_in, const float* colsum);
/* out[B,N,H*64] (bf16 widened to f32) = softmax(q k^T) v per head; q,k,v: [B,N,H*64] bf16 bits
 * (q already scaled). mode as in vt_op_attention_bench.
 * This hook and the next one put the device output between two 4 KiB guard bands and fill it with 0xff before the
 * launch: a row the kernel never stores comes back as NaN, a store into a guard band as VT_ERR_HIP with a message. */
int vt_op_attention_bf16(int device_id, const uint16_t* q, const uint16_t* k, const uint16_t* v,
                         float* out, int B, int N, int H, int mode);
/* Attention mode 3 on the queries q0 .. q0 + nq - 1 of every stream only (keys and values: all N tokens):
 * out [B, nq, H*64], row b * nq + (q - q0). N % 4 == 0. The same bits as those rows of vt_op_attention_bf16(mode 3)
 * while every query's scores stay within +-32 log2 units; beyond, a query may take the kernel's other pass. */
int vt_op_attention_queries_bf16(int device_id, const uint16_t* q, const uint16_t* k, const uint16_t* v,
                                 float* out, int B, int N, int H, int q0, int nq);
/* Kernel-tuning helper: mean microseconds per launch of the attention kernel on random data;
 * mode 0 key-split, 1 independent waves, 2 LDS-shared tiles, 3 LDS-DMA ring (permuted Vt),
 * <0 the launcher's choice. */
int vt_op_attention_bench(int device_id, int B, int N, int H, int mode, int iters, float* us_out);
/* Kernel-timing helper: mean microseconds per launch of the whole-frame NV12 -> RGB8 converter
 * (the reference's nv12_full_to_rgb_parallel, src/nv12_convert.rs:46-92) on a device-resident
 * w x h frame of random bytes (HIP events around `iters` launches). Algorithmic traffic is
 * 1.5 + 3 bytes per pixel. */
int vt_op_nv12_to_rgb8_bench(int device_id, int w, int h, int iters, float* us_out);
/* The same for vt_nv12_to_rgb8_batch_device: n frames of w x h converted by one launch per 64 frames. */
int vt_op_nv12_to_rgb8_batch_bench(int device_id, int w, int h, int n, int iters, float* us_out);
/* y[M,D] (bf16 widened) = LayerNorm(x[M,D] f32; gamma, beta, eps=1e-6) */
int vt_op_layernorm(int device_id, const float* x, const float* gamma, const float* beta,
                    float* y, int M, int D);
/* The folded LayerNorm of an encoder block as the engine runs it, M = B * tokens rows of x [M][D] (float32, host):
 *   producer  the X-epilogue "+ pos" with all-zero operands and pos = x: (0 + 0) + x is x exactly, so any float32
 *             matrix goes through the real split (xh_out bf16 bits / xl_out signed bytes, quantum 2^-lo_shift) and the
 *             real chunk statistics (cstat_out [M][D / 32][2]: sum, M2);
 *   row terms (rstd, -mean * rstd) with `eps`, by route: 0 a launch of the finalize kernel, 1 the last workgroup of
 *             each 256-row panel inside the 256x256 producer, 2 the consumer's own epilogue from the chunk partials.
 *             rowstat_out [M][2]; route 2 never writes it (it stays 0xff);
 *   fold      Wf = bf16(gamma * W) (wf_out [N][D]), colsum_out [N] = sum_k Wf, cvec_out [N] = sum_k beta W + bias,
 *             from w [N][D] (bf16 bits), gamma, beta [D], bias [N];
 *   consumer  2 GELU, 3 ReLU: out [M][N] = f(rstd * (xh Wf^T) + (-mean * rstd * colsum + cvec)) (bf16 widened);
 *             4 QKV (N == 3 * D, tokens % 4 == 0): out = qk [M][2D], vt_out = Vt [B * D / 64][64][npad] in natural key
 *             order, as vt_op_qkv_bf16 returns them (pad columns of Vt stay 0xff);
 *             0 the fold alone (x, B, tokens, route and the configurations are ignored; N >= 1, D even).
 * producer_cfg / consumer_cfg as in vt_op_gemm_bf16_lo (< 0: the launcher's choice). The chain runs `launches` (1..16)
 * times on the same buffers; the panel counters of route 1 must be zero afterwards (VT_ERR_HIP otherwise). Every
 * device output starts as 0xff between guard bands; a changed guard byte is VT_ERR_HIP. VT_ERR_INVALID_ARG, with
 * nothing launched and no output written: route 1 with a producer configuration below 18, D % 256 or D > 1536;
 * route 2 with a consumer configuration above 8, D % 128 or D > 1024; QKV with N != 3 * D or tokens % 4; D > 2048;
 * a configuration the launcher refuses for the shape. Output pointers other than `out` (and vt_out for QKV) may be NULL. */
int vt_op_ln_chain_bf16(int device_id, const float* x, int B, int tokens, int D, const uint16_t* w, const float* gamma,
                        const float* beta, const float* bias, int N, int consumer, int route, int producer_cfg,
                        int consumer_cfg, float eps, int lo_shift, int launches, float* out, float* vt_out,
                        uint16_t* xh_out, int8_t* xl_out, float* cstat_out, float* rowstat_out, uint16_t* wf_out,
                        float* colsum_out, float* cvec_out);

#ifdef __cplusplus
}
#endif
#endif /* VITTRACK_HIP_OPS_H */
