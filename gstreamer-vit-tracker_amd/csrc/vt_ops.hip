// vt_ops.hip — operator-level entry points (include/vittrack_hip_ops.h): numerics tests and tuning tools call the
// same kernel launchers the pass uses. Linked into libvittrack_hip_ops.so only; the product library does not carry them.
#include "vt_engine.hpp"
#include "../../include/vittrack_hip_ops.h"

extern "C" {

// ---- operator-level entry points ---------------------------------------------------------------------------

// host-side helpers of the operator entry points: float32 <-> the 3-byte pair of the residual stream
static inline bf16_t host_bf16(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return (bf16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
static inline float host_f32(bf16_t b) {
    const uint32_t u = ((uint32_t)b) << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// epilogue: 0 x = acc + bias, 1 x = (acc + bias) + c_inout, 4 x = (acc + bias) + pos (pos = c_inout, one
// row per output row) - the X-epilogues: c_inout goes in and comes back through the 3-byte pair (hi + lo8 * 2^-s: bf16 and
// an absolute quantum of 2^-s, s = lo_shift), rowstat_out (if given) receives the finalized row terms (rstd, -mean * rstd) of x;
// 2 gelu, 3 relu -> bf16, with an optional folded LayerNorm (rowstat_in [M][2], colsum [N]).
int vt_op_gemm_bf16_lo(int device_id, const uint16_t* a, const uint16_t* w, const float* bias, float* c_inout,
                       int M, int N, int K, int epilogue, int cfg, const float* rowstat_in, const float* colsum,
                       float* rowstat_out, float eps, int lo_shift) try {
    if (!a || !w || !c_inout || M <= 0 || N <= 0 || K <= 0) return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (lo_shift < VT_LO_SHIFT_MIN || lo_shift > VT_LO_SHIFT_MAX) return set_err(VT_ERR_INVALID_ARG, "gemm: lo_shift %d out of range", lo_shift);
    if (N % 64 || K % 64) return set_err(VT_ERR_INVALID_ARG, "gemm: N and K must be multiples of 64");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    HIPCHK(gemm_prepare()); HIPCHK(attention_prepare()); HIPCHK(headconv_prepare());
    const size_t MN = (size_t)M * N;
    DevBuf da, dw, db, dxh, dxl, dpos, dcb, dcs, drs, dcst, dro;
    HIPCHK(da.alloc((size_t)M * K * 2)); HIPCHK(dw.alloc((size_t)N * K * 2)); HIPCHK(db.alloc((size_t)N * 4));
    HIPCHK(dxh.alloc(MN * 2)); HIPCHK(dxl.alloc(MN * 2)); HIPCHK(dcb.alloc(MN * 2));
    HIPCHK(hipMemcpy(da.p, a, (size_t)M * K * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dw.p, w, (size_t)N * K * 2, hipMemcpyHostToDevice));
    std::vector<float> zb((size_t)N, 0.0f);
    HIPCHK(hipMemcpy(db.p, bias ? bias : zb.data(), (size_t)N * 4, hipMemcpyHostToDevice));
    GemmArgs g{};
    g.A = (const bf16_t*)da.p; g.lda = K; g.W = (const bf16_t*)dw.p; g.ldw = K; g.bias = (const float*)db.p;
    g.M = M; g.N = N; g.K = K; g.Xh = (bf16_t*)dxh.p; g.Xl = (uint8_t*)dxl.p; g.ldx = N; g.Cb = (bf16_t*)dcb.p; g.ldcb = N;
    g.lq = lo_quant(lo_shift);
    int epi;
    switch (epilogue) {
        case 0: epi = EPI_F32; break;
        case 1: epi = EPI_RESID; break;
        case 2: epi = EPI_GELU_BF16; break;
        case 3: epi = EPI_RELU_BF16; break;
        case 4: epi = EPI_F32_POS; break;
        default: return set_err(VT_ERR_INVALID_ARG, "gemm: unknown epilogue %d", epilogue);
    }
    const bool x_epi = epi == EPI_F32 || epi == EPI_RESID || epi == EPI_F32_POS;
    // the 3-byte pair of specification v3 (vt_common.hpp): hi = bf16(x), lo8 = clamp(rint((x - hi) * 2^s), -127, 127)
    std::vector<bf16_t> hi;
    std::vector<int8_t> lo;
    if (epi == EPI_RESID) {
        hi.resize(MN); lo.resize(MN);
        for (size_t i = 0; i < MN; ++i) {
            hi[i] = host_bf16(c_inout[i]);
            const float q = nearbyintf((c_inout[i] - host_f32(hi[i])) * (float)(1 << lo_shift));
            lo[i] = (int8_t)(q < -127.0f ? -127.0f : q > 127.0f ? 127.0f : q);
        }
        HIPCHK(hipMemcpy(dxh.p, hi.data(), MN * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dxl.p, lo.data(), MN, hipMemcpyHostToDevice));
    } else if (epi == EPI_F32_POS) {
        HIPCHK(dpos.alloc(MN * 4));
        HIPCHK(hipMemcpy(dpos.p, c_inout, MN * 4, hipMemcpyHostToDevice));
        g.pos = (const float*)dpos.p; g.pos_rows = M;
    }
    if (x_epi) {
        HIPCHK(dcst.alloc((size_t)M * (N / VT_STAT_CHUNK) * 8));
        g.cstat = (float2*)dcst.p;
    } else if (rowstat_in) {
        if (!colsum) return set_err(VT_ERR_INVALID_ARG, "gemm: rowstat without colsum");
        HIPCHK(drs.alloc((size_t)M * 8 + 16)); HIPCHK(dcs.alloc((size_t)N * 4));
        HIPCHK(hipMemcpy(drs.p, rowstat_in, (size_t)M * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dcs.p, colsum, (size_t)N * 4, hipMemcpyHostToDevice));
        g.rowstat = (const float2*)drs.p; g.colsum = (const float*)dcs.p;
    }
    // X-epilogues on the 256x256 kernel finalize the row terms themselves (last workgroup of each row panel)
    DevBuf dcnt;
    bool fused = false;
    if (cfg >= 0) { g.tile_order = (cfg >> 8) & 3; cfg &= 0xff; }   // bits 8-9 of a given configuration: the XCD tile order (1 rows, 2 columns)
    if (x_epi && rowstat_out) {
        HIPCHK(dro.alloc((size_t)M * 8));
        HIPCHK(dcnt.alloc((size_t)((M + 255) / 256 + 1) * 4));
        HIPCHK(hipMemset(dcnt.p, 0, (size_t)((M + 255) / 256 + 1) * 4));
        HIPCHK(hipMemset(dro.p, 0xff, (size_t)M * 8));
        const int eff = cfg < 0 ? gemm_effective_config(g, epi) : cfg;
        if (eff >= GEMM_CFG_256_MIN) {
            g.rowstat_out = (float2*)dro.p; g.panel_cnt = (unsigned*)dcnt.p; g.ln_eps = eps;
            fused = true;
        }
    }
    if (cfg < 0) HIPCHK(launch_gemm(g, epi, nullptr));
    else if (launch_gemm_cfg(g, epi, cfg, nullptr) != hipSuccess)
        return set_err(VT_ERR_INVALID_ARG, "gemm: tile configuration %d does not fit M=%d N=%d K=%d", cfg, M, N, K);
    if (x_epi && rowstat_out && !fused)
        HIPCHK(launch_rowstat_finalize(g.cstat, (float2*)dro.p, M, N / VT_STAT_CHUNK, eps, nullptr));
    if (fused) {      // launch it twice more: the counters must come back to zero by themselves
        for (int rep = 0; rep < 2 && (epi == EPI_F32 || epi == EPI_F32_POS); ++rep) HIPCHK(launch_gemm_cfg(g, epi, cfg < 0 ? gemm_effective_config(g, epi) : cfg, nullptr));
    }
    HIPCHK(hipDeviceSynchronize());
    if (x_epi) {
        hi.resize(MN); lo.resize(MN);
        HIPCHK(hipMemcpy(hi.data(), dxh.p, MN * 2, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(lo.data(), dxl.p, MN, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < MN; ++i) c_inout[i] = host_f32(hi[i]) + (float)lo[i] * g.lq.q;
        if (rowstat_out) HIPCHK(hipMemcpy(rowstat_out, dro.p, (size_t)M * 8, hipMemcpyDeviceToHost));
    } else {
        std::vector<bf16_t> tmp(MN);
        HIPCHK(hipMemcpy(tmp.data(), dcb.p, tmp.size() * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < tmp.size(); ++i) c_inout[i] = host_f32(tmp[i]);
    }
    return VT_OK;
} VT_NOTHROW_INT

int vt_op_gemm_bf16(int device_id, const uint16_t* a, const uint16_t* w, const float* bias, float* c_inout,
                    int M, int N, int K, int epilogue, int cfg, const float* rowstat_in, const float* colsum,
                    float* rowstat_out, float eps) {
    return vt_op_gemm_bf16_lo(device_id, a, w, bias, c_inout, M, N, K, epilogue, cfg, rowstat_in, colsum, rowstat_out, eps,
                              VT_LO_SHIFT_DEFAULT);
}

// The residual GEMM of the 256x256 kernel on a pair given as it is stored, with the remapped addend read of the last
// encoder block (GemmArgs.seg_rows / seg_skip / Xh_in): see include/vittrack_hip_ops.h
int vt_op_gemm_resid_seg_bf16(int device_id, const uint16_t* a, const uint16_t* w, const float* bias, const uint16_t* xh_in,
                              const int8_t* xl_in, int rows_in, uint16_t* xh_out, int8_t* xl_out, float* cstat_out,
                              float* rowstat_out, int M, int N, int K, int seg_rows, int seg_skip, float eps, int lo_shift) try {
    if (!a || !w || !xh_in || !xl_in || !xh_out || !xl_out || M <= 0 || N <= 0 || K <= 0 || rows_in <= 0 || seg_rows < 0 || seg_skip < 0)
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (lo_shift < VT_LO_SHIFT_MIN || lo_shift > VT_LO_SHIFT_MAX) return set_err(VT_ERR_INVALID_ARG, "gemm: lo_shift %d out of range", lo_shift);
    // every input row the kernel may read exists: the last output row's place in the input layout
    const long long last_in = seg_rows > 0 ? (long long)(M - 1) + ((long long)((M - 1) / seg_rows) + 1) * seg_skip : (long long)M - 1;
    if (last_in >= rows_in) return set_err(VT_ERR_INVALID_ARG, "gemm: the input pair has %d rows, the addend read reaches row %lld", rows_in, last_in);
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    HIPCHK(gemm_prepare());
    const size_t MN = (size_t)M * N, IN = (size_t)rows_in * N, nchunk = (size_t)N / VT_STAT_CHUNK;
    DevBuf da, dw, db, dih, dil, doh, dol, dcst, dro, dcnt;
    HIPCHK(da.alloc((size_t)M * K * 2)); HIPCHK(dw.alloc((size_t)N * K * 2)); HIPCHK(db.alloc((size_t)N * 4));
    HIPCHK(dih.alloc(IN * 2)); HIPCHK(dil.alloc(IN)); HIPCHK(doh.alloc(MN * 2)); HIPCHK(dol.alloc(MN));
    HIPCHK(dcst.alloc((size_t)M * nchunk * 8)); HIPCHK(dro.alloc((size_t)M * 8));
    HIPCHK(dcnt.alloc((size_t)((M + 255) / 256 + 1) * 4));
    HIPCHK(hipMemcpy(da.p, a, (size_t)M * K * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dw.p, w, (size_t)N * K * 2, hipMemcpyHostToDevice));
    std::vector<float> zb((size_t)N, 0.0f);
    HIPCHK(hipMemcpy(db.p, bias ? bias : zb.data(), (size_t)N * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dih.p, xh_in, IN * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dil.p, xl_in, IN, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(dcnt.p, 0, (size_t)((M + 255) / 256 + 1) * 4));
    HIPCHK(hipMemset(dcst.p, 0xff, (size_t)M * nchunk * 8)); HIPCHK(hipMemset(dro.p, 0xff, (size_t)M * 8));
    GemmArgs g{};
    g.A = (const bf16_t*)da.p; g.lda = K; g.W = (const bf16_t*)dw.p; g.ldw = K; g.bias = (const float*)db.p;
    g.M = M; g.N = N; g.K = K; g.Xh = (bf16_t*)doh.p; g.Xl = (uint8_t*)dol.p; g.ldx = N;
    g.cstat = (float2*)dcst.p; g.rowstat_out = (float2*)dro.p; g.panel_cnt = (unsigned*)dcnt.p; g.ln_eps = eps;
    g.lq = lo_quant(lo_shift);
    if (seg_rows > 0) {     // addend from the input pair through the remap, output compact
        g.Xh_in = (const bf16_t*)dih.p; g.Xl_in = (const uint8_t*)dil.p; g.seg_rows = seg_rows; g.seg_skip = seg_skip;
        HIPCHK(hipMemset(doh.p, 0xff, MN * 2)); HIPCHK(hipMemset(dol.p, 0xff, MN));
    } else {                // the launch as it always was: rows 0 .. M-1 of the pair, read and written in place
        HIPCHK(hipMemcpy(doh.p, dih.p, MN * 2, hipMemcpyDeviceToDevice));
        HIPCHK(hipMemcpy(dol.p, dil.p, MN, hipMemcpyDeviceToDevice));
    }
    if (launch_gemm_cfg(g, EPI_RESID, GEMM_CFG_256P4, nullptr) != hipSuccess)
        return set_err(VT_ERR_INVALID_ARG, "gemm: the 256x256 kernel does not take M=%d N=%d K=%d seg_rows=%d seg_skip=%d", M, N, K, seg_rows, seg_skip);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(xh_out, doh.p, MN * 2, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(xl_out, dol.p, MN, hipMemcpyDeviceToHost));
    if (cstat_out) HIPCHK(hipMemcpy(cstat_out, dcst.p, (size_t)M * nchunk * 8, hipMemcpyDeviceToHost));
    if (rowstat_out) HIPCHK(hipMemcpy(rowstat_out, dro.p, (size_t)M * 8, hipMemcpyDeviceToHost));
    return VT_OK;
} VT_NOTHROW_INT

// Timing helper for kernel tuning: runs the GEMM kernel `iters` times on device-resident random
// operands with tile configuration `cfg` (<0: the launcher's own choice) and returns the mean time
// per launch in microseconds (HIP events on the null stream).
int vt_op_gemm_bench(int device_id, int M, int N, int K, int epilogue, int cfg, int iters, float* us_out) try {
    if (M <= 0 || N % 64 || K % 64 || iters < 1 || !us_out) return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    HIPCHK(gemm_prepare()); HIPCHK(attention_prepare()); HIPCHK(headconv_prepare());
    const int D = N / 3, tokens = 4 * ((M + 3) / 4), npad = (tokens + 63) / 64 * 64;
    DevBuf da, dw, db, dc, dcb, dvt, dxl, dcst, drs;
    HIPCHK(da.alloc((size_t)M * K * 2)); HIPCHK(dw.alloc((size_t)N * K * 2)); HIPCHK(db.alloc((size_t)N * 4));
    HIPCHK(dc.alloc((size_t)M * N * 4)); HIPCHK(dcb.alloc((size_t)M * N * 2)); HIPCHK(dxl.alloc((size_t)M * N * 2));
    HIPCHK(dcst.alloc((size_t)M * (N / VT_STAT_CHUNK) * 8)); HIPCHK(drs.alloc((size_t)M * 8 + 16));
    HIPCHK(dvt.alloc((size_t)(N / 64 + 1) * 64 * npad * 2));
    std::vector<bf16_t> ha((size_t)M * K), hw((size_t)N * K);
    uint32_t seed = 12345u;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (bf16_t)(0x3c00u + ((seed >> 9) & 0x3ffu) + ((seed >> 3) & 0x8000u)); };
    for (auto& v : ha) v = rnd();
    for (auto& v : hw) v = rnd();
    HIPCHK(hipMemcpy(da.p, ha.data(), ha.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dw.p, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(db.p, 0, (size_t)N * 4));
    HIPCHK(hipMemset(dc.p, 0, (size_t)M * N * 4));
    HIPCHK(hipMemset(dcb.p, 0, (size_t)M * N * 2)); HIPCHK(hipMemset(dxl.p, 0, (size_t)M * N * 2));
    {   // folded-LayerNorm row terms as the engine passes them to the QKV / fc1 GEMMs: (1, 0) per row
        std::vector<float> rs((size_t)M * 2);
        for (int i = 0; i < M; ++i) { rs[2 * (size_t)i] = 1.0f; rs[2 * (size_t)i + 1] = 0.0f; }
        HIPCHK(hipMemcpy(drs.p, rs.data(), rs.size() * 4, hipMemcpyHostToDevice));
    }
    GemmArgs g{};
    g.A = (const bf16_t*)da.p; g.lda = K; g.W = (const bf16_t*)dw.p; g.ldw = K; g.bias = (const float*)db.p;
    g.M = M; g.N = N; g.K = K; g.Cb = (bf16_t*)dcb.p; g.ldcb = N;
    const bool x_epi = epilogue == EPI_F32 || epilogue == EPI_RESID || epilogue == EPI_F32_POS;
    DevBuf dcnt, dro;
    if (x_epi) {      // as the engine launches it: chunk partials + the row terms finalized by the last workgroup of each panel
        g.Xh = (bf16_t*)dcb.p; g.Xl = (uint8_t*)dxl.p; g.ldx = N; g.cstat = (float2*)dcst.p;
        HIPCHK(dcnt.alloc((size_t)((M + 255) / 256 + 1) * 4)); HIPCHK(dro.alloc((size_t)M * 8 + 16));
        HIPCHK(hipMemset(dcnt.p, 0, (size_t)((M + 255) / 256 + 1) * 4));
        g.rowstat_out = (float2*)dro.p; g.panel_cnt = (unsigned*)dcnt.p; g.ln_eps = 1e-6f;
    }
    else if (epilogue == EPI_QKV || epilogue == EPI_GELU_BF16) { g.rowstat = (const float2*)drs.p; g.colsum = (const float*)db.p; }
    g.pos = (const float*)dc.p; g.pos_rows = M;
    g.qk = (bf16_t*)dcb.p; g.vt = (bf16_t*)dvt.p; g.tokens = tokens; g.npad = npad; g.D = D;
    if (epilogue == EPI_QKV && (N % 192 || tokens != M)) return set_err(VT_ERR_INVALID_ARG, "qkv bench: N = 3D, D %% 64 == 0, M %% 4 == 0");
    if (cfg >= 0) { g.tile_order = (cfg >> 8) & 3; cfg &= 0xff; }   // sweeps: bits 8-9 force the XCD tile order (1 rows, 2 columns)
    if (cfg < 0) cfg = gemm_pick_config(M, N, K, epilogue);
    DevBuf ddbg;
    const size_t dbg_words = (size_t)((M + 63) / 64) * (N / 64) * 8 * 4;
#ifdef VT_STAMPS   // diagnostic builds only: per-wave cycle sums of the main loop
    HIPCHK(ddbg.alloc(dbg_words * 8));
    HIPCHK(hipMemset(ddbg.p, 0, dbg_words * 8));
    g.dbg = (unsigned long long*)ddbg.p;
#else
    (void)dbg_words;
#endif
    for (int i = 0; i < 3; ++i) HIPCHK(launch_gemm_cfg(g, epilogue, cfg, nullptr));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, nullptr));
    for (int i = 0; i < iters; ++i) HIPCHK(launch_gemm_cfg(g, epilogue, cfg, nullptr));
    HIPCHK(hipEventRecord(e1, nullptr));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *us_out = ms * 1000.0f / iters;
    if (g.dbg) {   // diagnostic build: mean per-wave cycle split of the main loop
        std::vector<unsigned long long> h(dbg_words);
        HIPCHK(hipMemcpy(h.data(), ddbg.p, dbg_words * 8, hipMemcpyDeviceToHost));
        double s[4] = {0, 0, 0, 0};
        size_t n = 0;
        for (size_t i = 0; i + 3 < dbg_words; i += 4)
            if (h[i + 3]) { for (int k = 0; k < 4; ++k) s[k] += (double)h[i + k]; ++n; }
        if (n) fprintf(stderr, "stamps cfg %d: waves %zu  wait %.0f  issue %.0f  compute %.0f  loop total %.0f cycles/wave\n",
                       cfg, n, s[0] / n, s[1] / n, s[2] / n, s[3] / n);
    }
    return VT_OK;
} VT_NOTHROW_INT

int vt_op_qkv_bf16(int device_id, const uint16_t* a, const uint16_t* w, const float* bias, float* qk_out,
                   float* vt_out, int B, int tokens, int D, int cfg, int vt_perm, const float* rowstat_in,
                   const float* colsum) try {
    // QKV GEMM with the attention-layout epilogue: qk_out [B*tokens][2D], vt_out [B*H][64][npad]
    if (!a || !w || !bias || !qk_out || !vt_out || B <= 0 || tokens <= 0 || D % 64 || (tokens & 3))
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    HIPCHK(gemm_prepare()); HIPCHK(attention_prepare()); HIPCHK(headconv_prepare());
    const int M = B * tokens, H = D / 64, npad = (tokens + 63) / 64 * 64;
    DevBuf da, dw, db, dqk, dvt;
    HIPCHK(da.alloc((size_t)M * D * 2)); HIPCHK(dw.alloc((size_t)3 * D * D * 2)); HIPCHK(db.alloc((size_t)3 * D * 4));
    HIPCHK(dqk.alloc((size_t)M * 2 * D * 2)); HIPCHK(dvt.alloc((size_t)B * H * 64 * npad * 2));
    HIPCHK(hipMemcpy(da.p, a, (size_t)M * D * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dw.p, w, (size_t)3 * D * D * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(db.p, bias, (size_t)3 * D * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(dvt.p, 0, (size_t)B * H * 64 * npad * 2));
    GemmArgs g{};
    g.A = (const bf16_t*)da.p; g.lda = D; g.W = (const bf16_t*)dw.p; g.ldw = D; g.bias = (const float*)db.p;
    g.M = M; g.N = 3 * D; g.K = D; g.qk = (bf16_t*)dqk.p; g.vt = (bf16_t*)dvt.p; g.tokens = tokens; g.npad = npad; g.D = D;
    g.vt_perm = vt_perm ? 1 : 0;   // 1: the key order attention mode 3 reads
    DevBuf drs, dcs;
    if (rowstat_in) {              // folded LayerNorm: [M][2] row terms, [3D] column sums
        if (!colsum) return set_err(VT_ERR_INVALID_ARG, "qkv: rowstat without colsum");
        HIPCHK(drs.alloc((size_t)M * 8 + 16)); HIPCHK(dcs.alloc((size_t)3 * D * 4));
        HIPCHK(hipMemcpy(drs.p, rowstat_in, (size_t)M * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dcs.p, colsum, (size_t)3 * D * 4, hipMemcpyHostToDevice));
        g.rowstat = (const float2*)drs.p; g.colsum = (const float*)dcs.p;
    }
    if (cfg >= 0) { g.tile_order = (cfg >> 8) & 3; cfg &= 0xff; }   // as in vt_op_gemm_bf16
    if (cfg < 0) HIPCHK(launch_gemm(g, EPI_QKV, nullptr));
    else if (launch_gemm_cfg(g, EPI_QKV, cfg, nullptr) != hipSuccess)
        return set_err(VT_ERR_INVALID_ARG, "qkv: tile configuration %d does not fit this shape", cfg);
    HIPCHK(hipDeviceSynchronize());
    auto widen = [](const DevBuf& d, size_t count, float* out) -> hipError_t {
        std::vector<bf16_t> tmp(count);
        hipError_t e = hipMemcpy(tmp.data(), d.p, count * 2, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        for (size_t i = 0; i < count; ++i) { uint32_t u = ((uint32_t)tmp[i]) << 16; memcpy(out + i, &u, 4); }
        return hipSuccess;
    };
    HIPCHK(widen(dqk, (size_t)M * 2 * D, qk_out));
    HIPCHK(widen(dvt, (size_t)B * H * 64 * npad, vt_out));
    return VT_OK;
} VT_NOTHROW_INT

// The output buffer of an attention hook between two guard bands: the bands carry a byte pattern, the output 0xff (a
// bf16 NaN), so a row the kernel never stores arrives as NaN instead of whatever a reused allocation held, and a store
// just outside the buffer (a slip in a row or block index) is reported instead of landing in a neighbour's memory.
struct GuardedOut {
    static constexpr size_t kGuard = 4096;      // bytes on each side; keeps out() 4 KiB aligned
    static constexpr int kPattern = 0xA5;
    DevBuf buf;
    size_t bytes = 0;
    hipError_t alloc(size_t n) {
        bytes = n;
        hipError_t e = buf.alloc(n + 2 * kGuard);
        if (e != hipSuccess) return e;
        e = hipMemset(buf.p, kPattern, n + 2 * kGuard);
        if (e != hipSuccess) return e;
        return hipMemset(out(), 0xff, n);
    }
    void* out() const { return static_cast<char*>(buf.p) + kGuard; }
    // after the synchronise: *where = 0 when both bands are intact, otherwise the signed distance in bytes of the first
    // changed byte from the output (negative: in front of it, positive: 1 = the first byte behind it)
    hipError_t check(long* where) const {
        std::vector<unsigned char> g(2 * kGuard);
        hipError_t e = hipMemcpy(g.data(), buf.p, kGuard, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        e = hipMemcpy(g.data() + kGuard, static_cast<char*>(buf.p) + kGuard + bytes, kGuard, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        *where = 0;
        for (size_t i = 0; i < 2 * kGuard && !*where; ++i)
            if (g[i] != kPattern) *where = i < kGuard ? (long)i - (long)kGuard : (long)(i - kGuard) + 1;
        return hipSuccess;
    }
};

int vt_op_attention_bf16(int device_id, const uint16_t* q, const uint16_t* k, const uint16_t* v, float* out,
                         int B, int N, int H, int mode) try {
    if (!q || !k || !v || !out || B <= 0 || N <= 0 || H <= 0) return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    HIPCHK(attention_prepare());
    const int D = H * 64, M = B * N, npad = (N + 63) / 64 * 64;
    // host-side packing into the layouts the QKV epilogue produces
    if (mode < 0) mode = attention_pick_mode(N, npad);
    const bool perm = attention_vt_perm(mode) != 0;
    std::vector<bf16_t> qk((size_t)M * 2 * D), vt((size_t)B * H * 64 * npad, 0);
    for (int m = 0; m < M; ++m) {
        memcpy(&qk[(size_t)m * 2 * D], q + (size_t)m * D, (size_t)D * 2);
        memcpy(&qk[(size_t)m * 2 * D + D], k + (size_t)m * D, (size_t)D * 2);
        const int b = m / N, t = m % N, tp = perm ? attn_perm16(t) : t;
        for (int c = 0; c < D; ++c)
            vt[((size_t)(b * H + c / 64) * 64 + c % 64) * npad + tp] = v[(size_t)m * D + c];
    }
    DevBuf dqk, dvt;
    GuardedOut dout;
    HIPCHK(dqk.alloc(qk.size() * 2)); HIPCHK(dvt.alloc(vt.size() * 2)); HIPCHK(dout.alloc((size_t)M * D * 2));
    HIPCHK(hipMemcpy(dqk.p, qk.data(), qk.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dvt.p, vt.data(), vt.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(launch_attention_mode((const bf16_t*)dqk.p, (const bf16_t*)dvt.p, (bf16_t*)dout.out(), B, N, H, npad, mode, nullptr));
    HIPCHK(hipDeviceSynchronize());
    long where = 0;
    HIPCHK(dout.check(&where));
    if (where) return set_err(VT_ERR_HIP, "attention mode %d wrote outside its output: guard byte %ld changed", mode, where);
    std::vector<bf16_t> tmp((size_t)M * D);
    HIPCHK(hipMemcpy(tmp.data(), dout.out(), tmp.size() * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < tmp.size(); ++i) { uint32_t u = ((uint32_t)tmp[i]) << 16; memcpy(out + i, &u, 4); }
    return VT_OK;
} VT_NOTHROW_INT

// Attention mode 3 on the queries q0 .. q0 + nq - 1 of every stream (the last encoder block): out compact [B*nq][H*64]
int vt_op_attention_queries_bf16(int device_id, const uint16_t* q, const uint16_t* k, const uint16_t* v, float* out,
                                 int B, int N, int H, int q0, int nq) try {
    if (!q || !k || !v || !out || B <= 0 || N <= 0 || H <= 0 || (N & 3) || q0 < 0 || nq < 1 || q0 + nq > N)
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    HIPCHK(attention_prepare());
    const int D = H * 64, M = B * N, npad = (N + 63) / 64 * 64;
    std::vector<bf16_t> qk((size_t)M * 2 * D), vt((size_t)B * H * 64 * npad, 0);
    for (int m = 0; m < M; ++m) {       // the layouts the QKV epilogue produces for mode 3
        memcpy(&qk[(size_t)m * 2 * D], q + (size_t)m * D, (size_t)D * 2);
        memcpy(&qk[(size_t)m * 2 * D + D], k + (size_t)m * D, (size_t)D * 2);
        const int b = m / N, tp = attn_perm16(m % N);
        for (int c = 0; c < D; ++c)
            vt[((size_t)(b * H + c / 64) * 64 + c % 64) * npad + tp] = v[(size_t)m * D + c];
    }
    const size_t MO = (size_t)B * nq * D;
    DevBuf dqk, dvt;
    GuardedOut dout;
    HIPCHK(dqk.alloc(qk.size() * 2)); HIPCHK(dvt.alloc(vt.size() * 2)); HIPCHK(dout.alloc(MO * 2));
    HIPCHK(hipMemcpy(dqk.p, qk.data(), qk.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dvt.p, vt.data(), vt.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(launch_attention_queries((const bf16_t*)dqk.p, (const bf16_t*)dvt.p, (bf16_t*)dout.out(), B, N, H, npad, q0, nq, nullptr));
    HIPCHK(hipDeviceSynchronize());
    long where = 0;
    HIPCHK(dout.check(&where));
    if (where) return set_err(VT_ERR_HIP, "attention on queries %d..%d wrote outside its output: guard byte %ld changed", q0, q0 + nq - 1, where);
    std::vector<bf16_t> tmp(MO);
    HIPCHK(hipMemcpy(tmp.data(), dout.out(), tmp.size() * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < tmp.size(); ++i) { uint32_t u = ((uint32_t)tmp[i]) << 16; memcpy(out + i, &u, 4); }
    return VT_OK;
} VT_NOTHROW_INT

// Timing helper: mean microseconds per launch of the attention kernel (mode as VT_ATTN_MODE, <0 =
// the launcher's choice) on device-resident random data.
int vt_op_attention_bench(int device_id, int B, int N, int H, int mode, int iters, float* us_out) try {
    if (B <= 0 || N <= 0 || H <= 0 || iters < 1 || !us_out) return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    HIPCHK(attention_prepare());
    const int D = H * 64, M = B * N, npad = (N + 63) / 64 * 64;
    std::vector<bf16_t> qk((size_t)M * 2 * D), vt((size_t)B * H * 64 * npad);
    uint32_t seed = 777u;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (bf16_t)(0x3c00u + ((seed >> 9) & 0x3ffu) + ((seed >> 3) & 0x8000u)); };
    for (auto& v : qk) v = rnd();
    for (auto& v : vt) v = rnd();
    DevBuf dqk, dvt, dout;
    HIPCHK(dqk.alloc(qk.size() * 2)); HIPCHK(dvt.alloc(vt.size() * 2)); HIPCHK(dout.alloc((size_t)M * D * 2));
    HIPCHK(hipMemcpy(dqk.p, qk.data(), qk.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dvt.p, vt.data(), vt.size() * 2, hipMemcpyHostToDevice));
    for (int i = 0; i < 3; ++i)
        HIPCHK(launch_attention_mode((const bf16_t*)dqk.p, (const bf16_t*)dvt.p, (bf16_t*)dout.p, B, N, H, npad, mode, nullptr));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, nullptr));
    for (int i = 0; i < iters; ++i)
        HIPCHK(launch_attention_mode((const bf16_t*)dqk.p, (const bf16_t*)dvt.p, (bf16_t*)dout.p, B, N, H, npad, mode, nullptr));
    HIPCHK(hipEventRecord(e1, nullptr));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *us_out = ms * 1000.0f / iters;
    return VT_OK;
} VT_NOTHROW_INT

int vt_op_nv12_to_rgb8_bench(int device_id, int w, int h, int iters, float* us_out) try {
    if (w < 2 || h < 2 || w > 16384 || h > 16384 || iters < 1 || !us_out) return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    const size_t in_bytes = nv12_bytes_read(w, h) + 16, out_bytes = (size_t)w * h * 3;
    DevBuf din, dout;
    HIPCHK(din.alloc(in_bytes)); HIPCHK(dout.alloc(out_bytes));
    std::vector<uint8_t> host(in_bytes);
    uint32_t seed = 2463534242u;
    for (auto& v : host) { seed ^= seed << 13; seed ^= seed >> 17; seed ^= seed << 5; v = (uint8_t)seed; }
    HIPCHK(hipMemcpy(din.p, host.data(), in_bytes, hipMemcpyHostToDevice));
    for (int i = 0; i < 3; ++i) HIPCHK(launch_nv12_to_rgb8((const uint8_t*)din.p, w, h, (uint8_t*)dout.p, nullptr));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, nullptr));
    for (int i = 0; i < iters; ++i) HIPCHK(launch_nv12_to_rgb8((const uint8_t*)din.p, w, h, (uint8_t*)dout.p, nullptr));
    HIPCHK(hipEventRecord(e1, nullptr));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *us_out = ms * 1000.0f / iters;
    return VT_OK;
} VT_NOTHROW_INT

int vt_op_nv12_to_rgb8_batch_bench(int device_id, int w, int h, int n, int iters, float* us_out) try {
    if (w < 2 || h < 2 || w > 16384 || h > 16384 || n < 1 || n > 1024 || iters < 1 || !us_out) return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    const size_t in_bytes = (nv12_bytes_read(w, h) + 16 + 255) & ~(size_t)255, out_bytes = ((size_t)w * h * 3 + 255) & ~(size_t)255;
    DevBuf din, dout;
    HIPCHK(din.alloc(in_bytes * n)); HIPCHK(dout.alloc(out_bytes * n));
    std::vector<uint8_t> host(in_bytes);
    uint32_t seed = 2463534242u;
    for (auto& v : host) { seed ^= seed << 13; seed ^= seed >> 17; seed ^= seed << 5; v = (uint8_t)seed; }
    std::vector<const uint8_t*> ins((size_t)n);
    std::vector<uint8_t*> outs((size_t)n);
    for (int i = 0; i < n; ++i) {
        ins[(size_t)i] = (const uint8_t*)din.p + (size_t)i * in_bytes;
        outs[(size_t)i] = (uint8_t*)dout.p + (size_t)i * out_bytes;
        HIPCHK(hipMemcpy((void*)ins[(size_t)i], host.data(), in_bytes, hipMemcpyHostToDevice));
    }
    for (int i = 0; i < 3; ++i) HIPCHK(launch_nv12_to_rgb8_batch(ins.data(), outs.data(), n, w, h, nullptr));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, nullptr));
    for (int i = 0; i < iters; ++i) HIPCHK(launch_nv12_to_rgb8_batch(ins.data(), outs.data(), n, w, h, nullptr));
    HIPCHK(hipEventRecord(e1, nullptr));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *us_out = ms * 1000.0f / iters;
    return VT_OK;
} VT_NOTHROW_INT

int vt_op_layernorm(int device_id, const float* x, const float* gamma, const float* beta, float* y, int M, int D) try {
    if (!x || !gamma || !beta || !y || M <= 0 || D % 128) return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    DevBuf dx, dg, db, dy;
    HIPCHK(dx.alloc((size_t)M * D * 4)); HIPCHK(dg.alloc((size_t)D * 4)); HIPCHK(db.alloc((size_t)D * 4)); HIPCHK(dy.alloc((size_t)M * D * 2));
    HIPCHK(hipMemcpy(dx.p, x, (size_t)M * D * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dg.p, gamma, (size_t)D * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(db.p, beta, (size_t)D * 4, hipMemcpyHostToDevice));
    HIPCHK(launch_layernorm((const float*)dx.p, (const float*)dg.p, (const float*)db.p, (bf16_t*)dy.p, M, D, M, 0, 0, 1e-6f, nullptr));
    HIPCHK(hipDeviceSynchronize());
    std::vector<bf16_t> tmp((size_t)M * D);
    HIPCHK(hipMemcpy(tmp.data(), dy.p, tmp.size() * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < tmp.size(); ++i) { uint32_t u = ((uint32_t)tmp[i]) << 16; memcpy(y + i, &u, 4); }
    return VT_OK;
} VT_NOTHROW_INT

// The head's 3x3 convolution (zero padding) + bias + ReLU as the engine runs it: an implicit GEMM over
// t [B*grid*grid][C] (bf16) with w [N][9*C] (bf16, column (ky*3+kx)*C + c); out [B*grid*grid][N] bf16
// widened to f32. cfg 0..3 (4-wave kernel), < 0: the launcher's choice.
int vt_op_conv3x3_relu_bf16(int device_id, const uint16_t* t, const uint16_t* w, const float* bias, float* out,
                            int B, int grid, int C, int N, int cfg) try {
    if (!t || !w || !bias || !out || B < 1 || grid < 1 || C % 64 || N % 64 || cfg > GEMM_CFG_SMALL_MAX)
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    HIPCHK(gemm_prepare());
    const size_t M = (size_t)B * grid * grid;
    DevBuf dt, dw, db, dout, dz;
    HIPCHK(dt.alloc(M * C * 2)); HIPCHK(dw.alloc((size_t)N * 9 * C * 2)); HIPCHK(db.alloc((size_t)N * 4));
    HIPCHK(dout.alloc(M * N * 2)); HIPCHK(dz.alloc(256));
    HIPCHK(hipMemcpy(dt.p, t, M * C * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dw.p, w, (size_t)N * 9 * C * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(db.p, bias, (size_t)N * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(dz.p, 0, 256));
    GemmArgs g{};
    g.A = (const bf16_t*)dt.p; g.lda = C; g.W = (const bf16_t*)dw.p; g.ldw = 9 * C; g.bias = (const float*)db.p;
    g.M = (int)M; g.N = N; g.K = 9 * C; g.Cb = (bf16_t*)dout.p; g.ldcb = N;
    g.conv_grid = grid; g.conv_C = C; g.zeros = (const bf16_t*)dz.p;
    if (cfg < 0) HIPCHK(launch_gemm(g, EPI_RELU_BF16, nullptr));
    else HIPCHK(launch_gemm_cfg(g, EPI_RELU_BF16, cfg, nullptr));
    HIPCHK(hipDeviceSynchronize());
    std::vector<bf16_t> tmp(M * N);
    HIPCHK(hipMemcpy(tmp.data(), dout.p, tmp.size() * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < tmp.size(); ++i) { uint32_t u = ((uint32_t)tmp[i]) << 16; memcpy(out + i, &u, 4); }
    return VT_OK;
} VT_NOTHROW_INT

// The head's band kernel (k_head.hip) on its own: out = relu(conv(t) + bias), conv3x3 != 0: t [B*grid*grid][Cin],
// w [N][9*Cin], N == Cin; else the 1x1 layer: w [N][Cin]. R / ncb <= 0: the launcher's plan. t == NULL: operands
// filled with a fixed pseudo-random pattern (timing runs). out (nullable): [B*grid*grid][N] bf16 values widened
// to f32. iters > 0 and us_out: mean microseconds per launch over iters launches.
int vt_op_headconv_bf16(int device_id, const uint16_t* t, const uint16_t* w, const float* bias, float* out,
                        int B, int grid, int Cin, int N, int conv3x3, int R, int ncb, int iters, float* us_out) try {
    if (B < 1 || grid < 1 || Cin % 64 || N % 64 || (t && (!w || !bias)))
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    const int K = conv3x3 ? 9 * Cin : Cin;
    if (!headconv_supported(grid, conv3x3 ? Cin : N, N, K, conv3x3 != 0))
        return set_err(VT_ERR_INVALID_ARG, "shape not supported by the band kernel");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    HIPCHK(headconv_prepare());
    const size_t M = (size_t)B * grid * grid;
    DevBuf dt, dw, db, dout, dz;
    HIPCHK(dt.alloc(M * Cin * 2)); HIPCHK(dw.alloc((size_t)N * K * 2)); HIPCHK(db.alloc((size_t)N * 4));
    HIPCHK(dout.alloc(M * N * 2)); HIPCHK(dz.alloc(256));
    if (t) {
        HIPCHK(hipMemcpy(dt.p, t, M * Cin * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dw.p, w, (size_t)N * K * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(db.p, bias, (size_t)N * 4, hipMemcpyHostToDevice));
    } else {
        std::vector<bf16_t> ht(M * Cin), hw((size_t)N * K);
        uint32_t seed = 777u;
        auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (bf16_t)(0x3c00u + ((seed >> 9) & 0x3ffu) + ((seed >> 3) & 0x8000u)); };
        for (auto& v : ht) v = rnd();
        for (auto& v : hw) v = rnd();
        HIPCHK(hipMemcpy(dt.p, ht.data(), ht.size() * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dw.p, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(db.p, 0, (size_t)N * 4));
    }
    HIPCHK(hipMemset(dz.p, 0, 256));
    HeadConvArgs h{};
    h.in = (const bf16_t*)dt.p; h.ldin = Cin; h.W = (const bf16_t*)dw.p; h.ldw = K; h.bias = (const float*)db.p;
    h.out = (bf16_t*)dout.p; h.ldout = N; h.zeros = (const bf16_t*)dz.p;
    h.B = B; h.grid = grid; h.C = conv3x3 ? Cin : N; h.N = N; h.K = K; h.conv3x3 = conv3x3 ? 1 : 0;
    h.R = R; h.ncb = ncb;
    HIPCHK(launch_headconv(h, nullptr, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (out) {
        std::vector<bf16_t> tmp(M * N);
        HIPCHK(hipMemcpy(tmp.data(), dout.p, tmp.size() * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < tmp.size(); ++i) { uint32_t u = ((uint32_t)tmp[i]) << 16; memcpy(out + i, &u, 4); }
    }
#ifdef VT_STAMPS   // diagnostic builds only: per-wave cycle sums of the main loop, medians printed
    DevBuf ddbg;
    const size_t dbg_words = (size_t)B * grid * 2 * 8 * 4;
    HIPCHK(ddbg.alloc(dbg_words * 8));
    HIPCHK(hipMemset(ddbg.p, 0, dbg_words * 8));
    h.dbg = (unsigned long long*)ddbg.p;
#endif
    if (iters > 0 && us_out) {
        for (int i = 0; i < 3; ++i) HIPCHK(launch_headconv(h, nullptr, nullptr));
        hipEvent_t e0, e1;
        HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
        HIPCHK(hipEventRecord(e0, nullptr));
        for (int i = 0; i < iters; ++i) HIPCHK(launch_headconv(h, nullptr, nullptr));
        HIPCHK(hipEventRecord(e1, nullptr));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        *us_out = ms * 1000.0f / iters;
    }
#ifdef VT_STAMPS
    {
        std::vector<unsigned long long> hd(dbg_words);
        HIPCHK(hipMemcpy(hd.data(), ddbg.p, dbg_words * 8, hipMemcpyDeviceToHost));
        std::vector<unsigned long long> col[2][4];
        for (size_t wg = 0; wg < dbg_words / 32; ++wg)
            for (int wv = 0; wv < 8; ++wv) {
                const unsigned long long* d = &hd[(wg * 8 + wv) * 4];
                if (d[3] == 0) continue;
                for (int k = 0; k < 4; ++k) col[wv >= 4][k].push_back(d[k]);
            }
        auto med = [](std::vector<unsigned long long>& v) { if (v.empty()) return 0ull; std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
        fprintf(stderr, "headconv stamps (median cycles per wave over the main loop): computing waves [-, barrier, compute, total] = "
                "%llu %llu %llu %llu; loader waves [vmcnt wait, barrier, issue, total] = %llu %llu %llu %llu\n",
                med(col[0][0]), med(col[0][1]), med(col[0][2]), med(col[0][3]), med(col[1][0]), med(col[1][1]), med(col[1][2]), med(col[1][3]));
    }
#endif
    return VT_OK;
} VT_NOTHROW_INT

// The head's first layer with the final LayerNorm: out[b * ns + cell][n] = ReLU(LayerNorm(xh + xl * 2^-lo_shift)[b * ntok + off + cell] . w[n] + bias[n])
// as bf16. fused != 0: one launch (the band kernel normalises its rows itself); fused == 0: the LayerNorm kernel, then the
// band kernel on its output - the form the fused one must reproduce bit for bit. xh == nullptr: synthetic operands (timing).
int vt_op_headconv_ln_bf16_lo(int device_id, const uint16_t* xh, const int8_t* xl, const float* gamma, const float* beta,
                              float eps, int ntok, int off, const uint16_t* w, const float* bias, float* out, int B, int grid,
                              int D, int N, int fused, int R, int ncb, int iters, float* us_out, int lo_shift) try {
    const int ns = grid * grid;
    if (lo_shift < VT_LO_SHIFT_MIN || lo_shift > VT_LO_SHIFT_MAX) return set_err(VT_ERR_INVALID_ARG, "headconv_ln: lo_shift %d out of range", lo_shift);
    const float lo_q = lo_quant(lo_shift).q;
    if (B < 1 || grid < 1 || off < 0 || ntok < off + ns || (xh && (!xl || !gamma || !beta || !w || !bias)))
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (!headconv_ln_supported(grid, N, D))
        return set_err(VT_ERR_INVALID_ARG, "shape not supported by the band kernel with the LayerNorm inside");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    HIPCHK(headconv_prepare());
    const size_t Mx = (size_t)B * ntok, M = (size_t)B * ns;
    DevBuf dh, dl, dg, dbt, dw, db, dfeat, dout;
    HIPCHK(dh.alloc(Mx * D * 2)); HIPCHK(dl.alloc(Mx * D * 2)); HIPCHK(dg.alloc((size_t)D * 4)); HIPCHK(dbt.alloc((size_t)D * 4));
    HIPCHK(dw.alloc((size_t)N * D * 2)); HIPCHK(db.alloc((size_t)N * 4)); HIPCHK(dfeat.alloc(M * D * 2)); HIPCHK(dout.alloc(M * N * 2));
    if (xh) {
        HIPCHK(hipMemcpy(dh.p, xh, Mx * D * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dl.p, xl, Mx * D, hipMemcpyHostToDevice));       // lo8 bytes
        HIPCHK(hipMemcpy(dg.p, gamma, (size_t)D * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dbt.p, beta, (size_t)D * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dw.p, w, (size_t)N * D * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(db.p, bias, (size_t)N * 4, hipMemcpyHostToDevice));
    } else {
        std::vector<bf16_t> hx(Mx * D), hw((size_t)N * D);
        std::vector<float> ones((size_t)D, 1.0f);
        uint32_t seed = 4242u;
        auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (bf16_t)(0x3c00u + ((seed >> 9) & 0x3ffu) + ((seed >> 3) & 0x8000u)); };
        for (auto& v : hx) v = rnd();
        for (auto& v : hw) v = rnd();
        HIPCHK(hipMemcpy(dh.p, hx.data(), hx.size() * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(dl.p, 0, Mx * D * 2));
        HIPCHK(hipMemcpy(dg.p, ones.data(), (size_t)D * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(dbt.p, 0, (size_t)D * 4));
        HIPCHK(hipMemcpy(dw.p, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(db.p, 0, (size_t)N * 4));
    }
    HeadConvArgs h{};
    h.W = (const bf16_t*)dw.p; h.ldw = D; h.bias = (const float*)db.p; h.out = (bf16_t*)dout.p; h.ldout = N;
    h.B = B; h.grid = grid; h.C = N; h.N = N; h.K = D; h.conv3x3 = 0; h.R = R; h.ncb = ncb;
    if (fused) {
        h.xh = (const bf16_t*)dh.p; h.xl = (const uint8_t*)dl.p; h.ln_g = (const float*)dg.p; h.ln_b = (const float*)dbt.p;
        h.ln_eps = eps; h.in_stride = ntok; h.in_off = off; h.lo_q = lo_q;
    } else {
        h.in = (const bf16_t*)dfeat.p; h.ldin = D;
    }
    auto run = [&]() -> hipError_t {
        if (!fused) {
            hipError_t e = launch_layernorm_split((const bf16_t*)dh.p, (const uint8_t*)dl.p, (const float*)dg.p, (const float*)dbt.p,
                                                  (bf16_t*)dfeat.p, (int)M, D, ns, ntok, off, eps, lo_q, nullptr);
            if (e != hipSuccess) return e;
        }
        return launch_headconv(h, nullptr, nullptr);
    };
    HIPCHK(run());
    HIPCHK(hipDeviceSynchronize());
    if (out) {
        std::vector<bf16_t> tmp(M * N);
        HIPCHK(hipMemcpy(tmp.data(), dout.p, tmp.size() * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < tmp.size(); ++i) { uint32_t u = ((uint32_t)tmp[i]) << 16; memcpy(out + i, &u, 4); }
    }
    if (iters > 0 && us_out) {
        for (int i = 0; i < 3; ++i) HIPCHK(run());
        hipEvent_t e0, e1;
        HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
        HIPCHK(hipEventRecord(e0, nullptr));
        for (int i = 0; i < iters; ++i) HIPCHK(run());
        HIPCHK(hipEventRecord(e1, nullptr));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        *us_out = ms * 1000.0f / iters;
    }
    return VT_OK;
} VT_NOTHROW_INT

int vt_op_headconv_ln_bf16(int device_id, const uint16_t* xh, const int8_t* xl, const float* gamma, const float* beta,
                           float eps, int ntok, int off, const uint16_t* w, const float* bias, float* out, int B, int grid,
                           int D, int N, int fused, int R, int ncb, int iters, float* us_out) {
    return vt_op_headconv_ln_bf16_lo(device_id, xh, xl, gamma, beta, eps, ntok, off, w, bias, out, B, grid, D, N, fused, R, ncb,
                                     iters, us_out, VT_LO_SHIFT_DEFAULT);
}

// pinned, device-visible host memory (what PassOut points the decode at)
struct PinnedBuf {
    void* p = nullptr;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t n) { return hipHostMalloc(&p, n ? n : 4); }
};

// The decode stage on given operands: see include/vittrack_hip_ops.h. A thin launcher: everything is checked here or by
// the launchers themselves before a kernel runs.
int vt_op_head_decode(int device_id, int form, const uint16_t* t, const uint16_t* w3, const float* b3, const float* w4,
                      const float* b4, const float* hann, void* states, int n_states, const int32_t* slot_stream,
                      float success_threshold, int B, int grid, int C, int R, int launches, int flags, float* head_out,
                      vt_result* results, vt_result* host_results, void* host_states, uint32_t* band_cnt) try {
    if ((form != 0 && form != 1) || !t || !w4 || !b4 || !hann || !states || !head_out || !results || !host_results ||
        !host_states || !band_cnt || B < 1 || B > 4096 || grid < 1 || grid > 16 * 7 || C < 2 || C > 4096 || n_states < 1 ||
        launches < 1 || launches > 64 || (form == 1 && (!w3 || !b3)))
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (C % 2) return set_err(VT_ERR_INVALID_ARG, "head_decode: C must be even");
    if (!slot_stream && n_states < B)
        return set_err(VT_ERR_INVALID_ARG, "head_decode: %d states for %d slots", n_states, B);
    if (slot_stream) {      // every slot's stream exists, and no two slots write one state
        std::vector<char> seen((size_t)n_states, 0);
        for (int b = 0; b < B; ++b) {
            const int32_t s = slot_stream[b];
            if (s < 0 || s >= n_states) return set_err(VT_ERR_INVALID_ARG, "head_decode: slot %d names stream %d of %d", b, (int)s, n_states);
            if (seen[(size_t)s]) return set_err(VT_ERR_INVALID_ARG, "head_decode: stream %d listed twice", (int)s);
            seen[(size_t)s] = 1;
        }
    }
    if (form == 1 && !headconv_plannable(grid, C, C, 9 * C, true, true))
        return set_err(VT_ERR_INVALID_ARG, "head_decode: grid %d, C %d is no shape of the band kernel's fused tail", grid, C);
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    HIPCHK(headconv_prepare());
    const int ns = grid * grid;
    const size_t M = (size_t)B * ns;
    DevBuf dt, dt3, dw3, db3, dw4, db4, dhann, dho, dst, dres, dpo, dmap, dcnt, dbest, dz;
    PinnedBuf hres, hst;
    HIPCHK(dt.alloc(M * C * 2)); HIPCHK(dw4.alloc((size_t)8 * C * 4)); HIPCHK(db4.alloc(8 * 4)); HIPCHK(dhann.alloc((size_t)ns * 4));
    HIPCHK(dho.alloc(M * 8 * 4)); HIPCHK(dst.alloc((size_t)n_states * sizeof(StreamState))); HIPCHK(dres.alloc((size_t)B * sizeof(vt_result)));
    HIPCHK(dpo.alloc(sizeof(PassOut))); HIPCHK(dcnt.alloc((size_t)B * 4)); HIPCHK(dbest.alloc((size_t)B * grid * 2 * 4));
    HIPCHK(hres.alloc((size_t)B * sizeof(vt_result))); HIPCHK(hst.alloc((size_t)n_states * sizeof(StreamState)));
    HIPCHK(hipMemcpy(dt.p, t, M * C * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dw4.p, w4, (size_t)8 * C * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(db4.p, b4, 8 * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dhann.p, hann, (size_t)ns * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dst.p, states, (size_t)n_states * sizeof(StreamState), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(dho.p, 0xff, M * 8 * 4));
    HIPCHK(hipMemset(dres.p, 0xff, (size_t)B * sizeof(vt_result)));
    HIPCHK(hipMemset(dcnt.p, 0, (size_t)B * 4));
    HIPCHK(hipMemset(dbest.p, 0, (size_t)B * grid * 2 * 4));
    memcpy(hres.p, host_results, (size_t)B * sizeof(vt_result));
    memcpy(hst.p, host_states, (size_t)n_states * sizeof(StreamState));
    const PassOut po{(flags & 1) ? nullptr : (vt_result*)hres.p, (flags & 2) ? nullptr : (StreamState*)hst.p};
    HIPCHK(hipMemcpy(dpo.p, &po, sizeof(po), hipMemcpyHostToDevice));
    if (slot_stream) {
        HIPCHK(dmap.alloc((size_t)B * 4));
        HIPCHK(hipMemcpy(dmap.p, slot_stream, (size_t)B * 4, hipMemcpyHostToDevice));
    }
    DecodeArgs dec{};
    dec.w4 = (const float*)dw4.p; dec.b4 = (const float*)db4.p; dec.hann = (const float*)dhann.p;
    dec.head_out = (float*)dho.p; dec.states = (StreamState*)dst.p; dec.results = (vt_result*)dres.p;
    dec.out = (const PassOut*)dpo.p; dec.slot_stream = slot_stream ? (const int32_t*)dmap.p : nullptr;
    dec.B = B; dec.ns = ns; dec.grid = grid; dec.C = C; dec.success_threshold = success_threshold;
    HeadConvArgs h{};
    if (form == 0) {
        dec.t3 = (const bf16_t*)dt.p;
    } else {
        HIPCHK(dt3.alloc(M * C * 2)); HIPCHK(dw3.alloc((size_t)C * 9 * C * 2)); HIPCHK(db3.alloc((size_t)C * 4)); HIPCHK(dz.alloc(256));
        HIPCHK(hipMemcpy(dw3.p, w3, (size_t)C * 9 * C * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(db3.p, b3, (size_t)C * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(dz.p, 0, 256));
        HIPCHK(hipMemset(dt3.p, 0xff, M * C * 2));
        dec.t3 = (const bf16_t*)dt3.p;
        h.in = (const bf16_t*)dt.p; h.ldin = C; h.W = (const bf16_t*)dw3.p; h.ldw = 9 * C; h.bias = (const float*)db3.p;
        h.out = (bf16_t*)dt3.p; h.ldout = C; h.zeros = (const bf16_t*)dz.p;
        h.B = B; h.grid = grid; h.C = C; h.N = C; h.K = 9 * C; h.conv3x3 = 1;
        h.R = R > 0 ? R : 0; h.ncb = R > 0 ? C / 64 : 0;      // a given R keeps the tail's one column group; else both planned
        h.band_cnt = (unsigned*)dcnt.p; h.band_best = (float*)dbest.p;
    }
    for (int i = 0; i < launches; ++i) {
        const hipError_t e = form == 0 ? launch_decode(dec, nullptr) : launch_headconv(h, &dec, nullptr);
        if (e == hipErrorInvalidValue) {      // refused before any kernel ran; earlier launches of this call drain first
            (void)hipDeviceSynchronize();
            return set_err(VT_ERR_INVALID_ARG, "head_decode: the launcher refuses grid %d, C %d, R %d", grid, C, R);
        }
        HIPCHK(e);
    }
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(head_out, dho.p, M * 8 * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(results, dres.p, (size_t)B * sizeof(vt_result), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(states, dst.p, (size_t)n_states * sizeof(StreamState), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(band_cnt, dcnt.p, (size_t)B * 4, hipMemcpyDeviceToHost));
    memcpy(host_results, hres.p, (size_t)B * sizeof(vt_result));
    memcpy(host_states, hst.p, (size_t)n_states * sizeof(StreamState));
    return VT_OK;
} VT_NOTHROW_INT

// The response-peaks launch on given operands: see include/vittrack_hip_ops.h. Nothing runs but launch_response_peaks.
int vt_op_response_peaks(int device_id, const float* head_out, const float* hann, void* states, int n_states,
                         const void* policies, const int32_t* slot_stream, const int32_t* winner, int B, int grid,
                         vt_peaks* records, vt_peaks* host_records) try {
    if (!head_out || !hann || !states || !policies || !records || !host_records || B < 1 || B > 4096 || grid < 1 || grid > 110 ||
        n_states < 1)
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (!slot_stream && n_states < B) return set_err(VT_ERR_INVALID_ARG, "response_peaks: %d states for %d slots", n_states, B);
    const PeaksPolicy* pol = (const PeaksPolicy*)policies;
    for (int s = 0; s < n_states; ++s)
        if (pol[s].max_peaks < 0 || pol[s].max_peaks > VT_PEAKS_MAX || pol[s].radius < 1 || pol[s].radius > 4)
            return set_err(VT_ERR_INVALID_ARG, "response_peaks: policy %d: max_peaks %d, radius %d", s, pol[s].max_peaks, pol[s].radius);
    for (int b = 0; b < B; ++b) {
        if (slot_stream && (slot_stream[b] < 0 || slot_stream[b] >= n_states))
            return set_err(VT_ERR_INVALID_ARG, "response_peaks: slot %d names stream %d of %d", b, (int)slot_stream[b], n_states);
        if (winner && (winner[b] < 0 || winner[b] >= B))
            return set_err(VT_ERR_INVALID_ARG, "response_peaks: winner[%d] = %d of %d slots", b, (int)winner[b], B);
    }
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    const int ns = grid * grid;
    const size_t M = (size_t)B * ns;
    DevBuf dho, dhann, dst, dpol, dmap, dwin, drec, dpo;
    PinnedBuf hrec;
    HIPCHK(dho.alloc(M * 8 * 4)); HIPCHK(dhann.alloc((size_t)ns * 4)); HIPCHK(dst.alloc((size_t)n_states * sizeof(StreamState)));
    HIPCHK(dpol.alloc((size_t)n_states * sizeof(PeaksPolicy))); HIPCHK(drec.alloc((size_t)B * sizeof(vt_peaks)));
    HIPCHK(dpo.alloc(sizeof(PassOut))); HIPCHK(hrec.alloc((size_t)B * sizeof(vt_peaks)));
    HIPCHK(hipMemcpy(dho.p, head_out, M * 8 * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dhann.p, hann, (size_t)ns * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dst.p, states, (size_t)n_states * sizeof(StreamState), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dpol.p, policies, (size_t)n_states * sizeof(PeaksPolicy), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(drec.p, records, (size_t)B * sizeof(vt_peaks), hipMemcpyHostToDevice));
    memcpy(hrec.p, host_records, (size_t)B * sizeof(vt_peaks));
    const PassOut po{nullptr, nullptr, (vt_peaks*)hrec.p};
    HIPCHK(hipMemcpy(dpo.p, &po, sizeof(po), hipMemcpyHostToDevice));
    if (slot_stream) {
        HIPCHK(dmap.alloc((size_t)B * 4));
        HIPCHK(hipMemcpy(dmap.p, slot_stream, (size_t)B * 4, hipMemcpyHostToDevice));
    }
    if (winner) {
        HIPCHK(dwin.alloc((size_t)B * 4));
        HIPCHK(hipMemcpy(dwin.p, winner, (size_t)B * 4, hipMemcpyHostToDevice));
    }
    const PeaksArgs pa{(const float*)dho.p, (const float*)dhann.p, (const StreamState*)dst.p,
                       slot_stream ? (const int32_t*)dmap.p : nullptr, winner ? (const int32_t*)dwin.p : nullptr,
                       (const PeaksPolicy*)dpol.p, (vt_peaks*)drec.p, (const PassOut*)dpo.p, B, ns, grid};
    const hipError_t e = launch_response_peaks(pa, nullptr);
    if (e == hipErrorInvalidValue) return set_err(VT_ERR_INVALID_ARG, "response_peaks: the launcher refuses grid %d", grid);
    HIPCHK(e);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(records, drec.p, (size_t)B * sizeof(vt_peaks), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(states, dst.p, (size_t)n_states * sizeof(StreamState), hipMemcpyDeviceToHost));
    memcpy(host_records, hrec.p, (size_t)B * sizeof(vt_peaks));
    return VT_OK;
} VT_NOTHROW_INT

// The result-overlay launch on given operands: see include/vittrack_hip_ops.h. Nothing runs but launch_result_overlay.
int vt_op_result_overlay(int device_id, const vt_frame* frames, const vt_result* results, const int32_t* slot_stream,
                         const int32_t* winner, int n, const int32_t* policy, int32_t* stats, int n_streams,
                         int device_frames) try {
    if (!frames || !results || !policy || !stats || n < 1 || n > VT_RESULT_OVERLAY_MAX_SLOTS || n_streams < 1)
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (!slot_stream && n_streams < n) return set_err(VT_ERR_INVALID_ARG, "result_overlay: %d streams for %d slots", n_streams, n);
    OverlayPolicy pol;
    memcpy(&pol, policy, sizeof(pol));
    if (pol.flags < 0 || pol.flags > 7 || pol.thickness < 1 || pol.thickness > 16 || pol.size < 1 || pol.size > 64 || pol.scale < 1 ||
        pol.scale > 4 || pol.luma < 0 || pol.luma > 255 || pol.rgb < 0 || pol.rgb > 0xFFFFFF || pol.min_score_pct < 0 ||
        pol.min_score_pct > 100)
        return set_err(VT_ERR_INVALID_ARG, "result_overlay: policy out of range");
    std::vector<FrameDesc> desc((size_t)n);
    for (int b = 0; b < n; ++b) {
        if (int rc = check_frame(frames[b])) return rc;
        to_desc(frames[b], &desc[(size_t)b]);
        if (slot_stream && (slot_stream[b] < 0 || slot_stream[b] >= n_streams))
            return set_err(VT_ERR_INVALID_ARG, "result_overlay: slot %d names stream %d of %d", b, (int)slot_stream[b], n_streams);
        if (winner && (winner[b] < 0 || winner[b] >= n))
            return set_err(VT_ERR_INVALID_ARG, "result_overlay: winner[%d] = %d of %d slots", b, (int)winner[b], n);
    }
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    DevBuf dfr, dres, dmap, dwin, dpol, dst, dflag;
    HIPCHK(dfr.alloc((size_t)n * sizeof(FrameDesc))); HIPCHK(dres.alloc((size_t)n * sizeof(vt_result)));
    HIPCHK(dpol.alloc(sizeof(OverlayPolicy))); HIPCHK(dst.alloc((size_t)n_streams * sizeof(OverlayStats))); HIPCHK(dflag.alloc(4));
    HIPCHK(hipMemcpy(dfr.p, desc.data(), (size_t)n * sizeof(FrameDesc), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dres.p, results, (size_t)n * sizeof(vt_result), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dpol.p, &pol, sizeof(pol), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dst.p, stats, (size_t)n_streams * sizeof(OverlayStats), hipMemcpyHostToDevice));
    const int32_t flag = device_frames != 0;
    HIPCHK(hipMemcpy(dflag.p, &flag, 4, hipMemcpyHostToDevice));
    if (slot_stream) {
        HIPCHK(dmap.alloc((size_t)n * 4));
        HIPCHK(hipMemcpy(dmap.p, slot_stream, (size_t)n * 4, hipMemcpyHostToDevice));
    }
    if (winner) {
        HIPCHK(dwin.alloc((size_t)n * 4));
        HIPCHK(hipMemcpy(dwin.p, winner, (size_t)n * 4, hipMemcpyHostToDevice));
    }
    const ResultOverlayArgs oa{(const FrameDesc*)dfr.p, (const vt_result*)dres.p, slot_stream ? (const int32_t*)dmap.p : nullptr,
                               winner ? (const int32_t*)dwin.p : nullptr, (const OverlayPolicy*)dpol.p, (OverlayStats*)dst.p,
                               (const int32_t*)dflag.p, n};
    HIPCHK(hipDeviceSynchronize());     // the caller's frames may have been filled on another stream
    HIPCHK(launch_result_overlay(oa, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(stats, dst.p, (size_t)n_streams * sizeof(OverlayStats), hipMemcpyDeviceToHost));
    return VT_OK;
} VT_NOTHROW_INT

// The two launches of the motion prior on given operands: see include/vittrack_hip_ops.h. Nothing runs but
// launch_motion_place (stages & 1) and launch_motion_settle (stages & 2), in that order.
int vt_op_motion_prior(int device_id, void* states, void* records, int n_streams, const int32_t* policy, const vt_result* results,
                       const int32_t* slot_stream, const int32_t* winner, const vt_candidate* cands, int n, int stages,
                       void* host_states, void* host_records) try {
    if (!states || !records || !policy || !results || n < 1 || n > VT_MAX_STREAMS || n_streams < 1 || stages < 1 || stages > 3)
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (!slot_stream && !cands && n_streams < n) return set_err(VT_ERR_INVALID_ARG, "motion_prior: %d streams for %d slots", n_streams, n);
    if ((cands != nullptr) != (winner != nullptr))
        return set_err(VT_ERR_INVALID_ARG, "motion_prior: the candidate form needs both the slots and the winner list");
    MotionPolicy pol;
    memcpy(&pol, policy, sizeof(pol));
    if (pol.on < 0 || pol.on > 1 || pol.gain_pct < 1 || pol.gain_pct > 100 || pol.coast < 0 || pol.coast > 60 || pol.max_pct < 0 ||
        pol.max_pct > 200)
        return set_err(VT_ERR_INVALID_ARG, "motion_prior: policy out of range");
    std::vector<int32_t> map;
    if (cands || slot_stream) map.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (!map.empty()) map[(size_t)i] = cands ? cands[i].stream : slot_stream[i];
        if (!map.empty() && (map[(size_t)i] < 0 || map[(size_t)i] >= n_streams))
            return set_err(VT_ERR_INVALID_ARG, "motion_prior: slot %d names stream %d of %d", i, (int)map[(size_t)i], n_streams);
        if (winner && (winner[i] < 0 || winner[i] >= n))
            return set_err(VT_ERR_INVALID_ARG, "motion_prior: winner[%d] = %d of %d slots", i, (int)winner[i], n);
    }
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    const size_t sb = (size_t)n_streams * sizeof(StreamState), rb = (size_t)n_streams * sizeof(MotionRec);
    DevBuf dst, drec, dpol, dres, dmap, dwin, dcand, dpo;
    PinnedBuf hst, hrec;
    HIPCHK(dst.alloc(sb)); HIPCHK(drec.alloc(rb)); HIPCHK(dpol.alloc(sizeof(pol))); HIPCHK(dres.alloc((size_t)n * sizeof(vt_result)));
    HIPCHK(dpo.alloc(sizeof(PassOut)));
    HIPCHK(hipMemcpy(dst.p, states, sb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(drec.p, records, rb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dpol.p, &pol, sizeof(pol), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dres.p, results, (size_t)n * sizeof(vt_result), hipMemcpyHostToDevice));
    if (host_states) { HIPCHK(hst.alloc(sb)); memcpy(hst.p, host_states, sb); }
    if (host_records) { HIPCHK(hrec.alloc(rb)); memcpy(hrec.p, host_records, rb); }
    const PassOut po{nullptr, (StreamState*)hst.p, nullptr, (MotionRec*)hrec.p};
    HIPCHK(hipMemcpy(dpo.p, &po, sizeof(po), hipMemcpyHostToDevice));
    if (!map.empty()) {
        HIPCHK(dmap.alloc((size_t)n * 4));
        HIPCHK(hipMemcpy(dmap.p, map.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    }
    if (cands) {
        HIPCHK(dwin.alloc((size_t)n * 4)); HIPCHK(dcand.alloc((size_t)n * sizeof(vt_candidate)));
        HIPCHK(hipMemcpy(dwin.p, winner, (size_t)n * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dcand.p, cands, (size_t)n * sizeof(vt_candidate), hipMemcpyHostToDevice));
    }
    const MotionArgs ma{(StreamState*)dst.p, (MotionRec*)drec.p, (const MotionPolicy*)dpol.p, (const vt_result*)dres.p,
                        map.empty() ? nullptr : (const int32_t*)dmap.p, cands ? (const int32_t*)dwin.p : nullptr,
                        cands ? (const vt_candidate*)dcand.p : nullptr, (const PassOut*)dpo.p, nullptr, n};
    if (stages & 1) HIPCHK(launch_motion_place(ma, nullptr));
    if (stages & 2) HIPCHK(launch_motion_settle(ma, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(states, dst.p, sb, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(records, drec.p, rb, hipMemcpyDeviceToHost));
    if (host_states) memcpy(host_states, hst.p, sb);
    if (host_records) memcpy(host_records, hrec.p, rb);
    return VT_OK;
} VT_NOTHROW_INT

// The score launch of the appearance check on given rows: see include/vittrack_hip_ops.h. Nothing runs but
// launch_appearance_score, on records the hook marks "cut" for every slot (the identity map: slot i is stream i).
int vt_op_appearance_score(int device_id, const uint16_t* anchor, const uint16_t* probe, int n_slots, int nt, int kpad, int cols,
                           double* sums, float* similarity, int32_t* status) try {
    if (!anchor || !probe || !sums || !similarity || !status || n_slots < 1 || n_slots > VT_MAX_STREAMS || nt < 1 || nt > 65536 ||
        cols < 1 || kpad < cols || kpad > 65536)
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    const size_t n = (size_t)n_slots, rows = n * (size_t)nt * (size_t)kpad * sizeof(bf16_t);
    const size_t nch = (size_t)appear_chunks(nt);
    DevBuf da, dp, dpol, drec, dcnt, dtick, dpart, dsum;
    HIPCHK(da.alloc(rows)); HIPCHK(dp.alloc(rows)); HIPCHK(dpol.alloc(sizeof(AppearPolicy))); HIPCHK(drec.alloc(n * sizeof(AppearRec)));
    HIPCHK(dcnt.alloc(n * sizeof(AppearCount))); HIPCHK(dtick.alloc(n * sizeof(unsigned)));
    HIPCHK(dpart.alloc(n * nch * 5 * sizeof(double))); HIPCHK(dsum.alloc(n * 5 * sizeof(double)));
    HIPCHK(hipMemcpy(da.p, anchor, rows, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dp.p, probe, rows, hipMemcpyHostToDevice));
    const AppearPolicy pol{1, 1, 0, 0.0f};
    HIPCHK(hipMemcpy(dpol.p, &pol, sizeof(pol), hipMemcpyHostToDevice));
    std::vector<AppearRec> recs(n, AppearRec{1, 0, 0.0f, {0.0f, 0.0f, 0.0f, 0.0f}, 0});
    HIPCHK(hipMemcpy(drec.p, recs.data(), n * sizeof(AppearRec), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(dcnt.p, 0, n * sizeof(AppearCount)));
    HIPCHK(hipMemset(dtick.p, 0, n * sizeof(unsigned)));
    HIPCHK(hipMemset(dpart.p, 0xff, n * nch * 5 * sizeof(double)));      // NaN: a partial nobody wrote would show
    HIPCHK(hipMemset(dsum.p, 0xff, n * 5 * sizeof(double)));
    AppearArgs a{};
    a.policy = (const AppearPolicy*)dpol.p; a.counts = (AppearCount*)dcnt.p; a.recs = (AppearRec*)drec.p;
    a.tickets = (unsigned*)dtick.p; a.partials = (double*)dpart.p;
    a.anchor = (const bf16_t*)da.p; a.probe = (bf16_t*)dp.p; a.sums = (double*)dsum.p; a.n = n_slots;
    HIPCHK(launch_appearance_score(a, nt, cols, kpad, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(recs.data(), drec.p, n * sizeof(AppearRec), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(sums, dsum.p, n * 5 * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<unsigned> ticks(n);
    HIPCHK(hipMemcpy(ticks.data(), dtick.p, n * sizeof(unsigned), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
        if (ticks[i] != 0) return set_err(VT_ERR_HIP, "appearance_score: slot %zu left its ticket at %u", i, ticks[i]);
        similarity[i] = recs[i].similarity;
        status[i] = recs[i].status;
    }
    return VT_OK;
} VT_NOTHROW_INT

// The four launches of the reacquire proposals on given operands: see include/vittrack_hip_ops.h. Nothing runs but
// launch_proposals_prepare, _thumb, _match and _list, in that order. Pattern, thumbnail, map and records each sit between
// guard bands and start as 0xff bytes: what a slot that is not due leaves untouched comes back as 0xff.
int vt_op_proposals(int device_id, const vt_frame* frames, const void* states, int n_streams, const vt_result* results,
                    const int32_t* slot_stream, const int32_t* winner, int n, const uint16_t* tpl, int tpl_bufs, int T, int patch,
                    int kpad, const float* norm, const int32_t* policy, int device_frames, int16_t* pattern, int16_t* thumb,
                    float* map, void* records, int32_t* evaluated) try {
    if (!frames || !states || !results || !tpl || !norm || !policy || !pattern || !thumb || !map || !records || !evaluated || n < 1 ||
        n > VT_MAX_STREAMS || n_streams < 1 || n_streams > VT_MAX_STREAMS || patch < 1 || T < patch || T % patch != 0 ||
        kpad < 3 * patch * patch || kpad > 65536 || (tpl_bufs != 1 && tpl_bufs != 2))
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (prop_pattern_side(T) == 0) return set_err(VT_ERR_INVALID_ARG, "proposals: template size %d is a multiple of neither 16 nor 14", T);
    if (!slot_stream && n_streams < n) return set_err(VT_ERR_INVALID_ARG, "proposals: %d streams for %d slots", n_streams, n);
    PropPolicy pol;
    memcpy(&pol, policy, sizeof(pol));
    if (pol.mode < 0 || pol.mode > 2 || pol.period < 1 || pol.period > VT_PROP_MAX_PERIOD || pol.max_n < 1 || pol.max_n > VT_PROP_MAX ||
        pol.min_sim_pm < 0 || pol.min_sim_pm > 1000 || pol.max_cells < VT_PROP_M_MAX * VT_PROP_M_MAX || pol.max_cells > VT_PROP_MAX_CELLS)
        return set_err(VT_ERR_INVALID_ARG, "proposals: policy out of range");
    pol.tau = (float)pol.min_sim_pm / 1000.0f;
    std::vector<FrameDesc> desc((size_t)n);
    for (int b = 0; b < n; ++b) {
        if (int rc = check_frame(frames[b])) return rc;
        to_desc(frames[b], &desc[(size_t)b]);
        if (slot_stream && (slot_stream[b] < 0 || slot_stream[b] >= n_streams))
            return set_err(VT_ERR_INVALID_ARG, "proposals: slot %d names stream %d of %d", b, (int)slot_stream[b], n_streams);
        if (winner && (winner[b] < 0 || winner[b] >= n))
            return set_err(VT_ERR_INVALID_ARG, "proposals: winner[%d] = %d of %d slots", b, (int)winner[b], n);
    }
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    ModelDims d{};
    d.T = T; d.patch = patch; d.gt = T / patch; d.nt = d.gt * d.gt; d.kpad = kpad;
    for (int c = 0; c < 3; ++c) { d.norm_a[c] = norm[c]; d.norm_b[c] = norm[3 + c]; }
    const size_t ns = (size_t)n, mc = (size_t)pol.max_cells, pm = VT_PROP_M_MAX * VT_PROP_M_MAX;
    const size_t tpl_b = (size_t)n_streams * tpl_bufs * d.nt * kpad * sizeof(bf16_t);
    DevBuf dfr, dst, dres, dmap, dwin, dpol, dflag, dtpl, dcnt, dhead, dpo;
    GuardedOut gpat, gth, gmap, grec;
    HIPCHK(dfr.alloc(ns * sizeof(FrameDesc))); HIPCHK(dst.alloc((size_t)n_streams * sizeof(StreamState)));
    HIPCHK(dres.alloc(ns * sizeof(vt_result))); HIPCHK(dpol.alloc(sizeof(pol))); HIPCHK(dflag.alloc(4)); HIPCHK(dtpl.alloc(tpl_b));
    HIPCHK(dcnt.alloc((size_t)n_streams * 4)); HIPCHK(dhead.alloc(ns * sizeof(PropHead))); HIPCHK(dpo.alloc(sizeof(PassOut)));
    HIPCHK(gpat.alloc(ns * pm * sizeof(int16_t))); HIPCHK(gth.alloc(ns * mc * sizeof(int16_t))); HIPCHK(gmap.alloc(ns * mc * sizeof(float)));
    HIPCHK(grec.alloc((size_t)n_streams * sizeof(PropRec)));
    HIPCHK(hipMemcpy(dfr.p, desc.data(), ns * sizeof(FrameDesc), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dst.p, states, (size_t)n_streams * sizeof(StreamState), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dres.p, results, ns * sizeof(vt_result), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dpol.p, &pol, sizeof(pol), hipMemcpyHostToDevice));
    const int32_t flag = device_frames != 0;
    HIPCHK(hipMemcpy(dflag.p, &flag, 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dtpl.p, tpl, tpl_b, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dcnt.p, evaluated, (size_t)n_streams * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(dhead.p, 0, ns * sizeof(PropHead)));
    const PassOut po{};
    HIPCHK(hipMemcpy(dpo.p, &po, sizeof(po), hipMemcpyHostToDevice));
    if (slot_stream) {
        HIPCHK(dmap.alloc(ns * 4));
        HIPCHK(hipMemcpy(dmap.p, slot_stream, ns * 4, hipMemcpyHostToDevice));
    }
    if (winner) {
        HIPCHK(dwin.alloc(ns * 4));
        HIPCHK(hipMemcpy(dwin.p, winner, ns * 4, hipMemcpyHostToDevice));
    }
    const PropArgs pa{(const FrameDesc*)dfr.p, (const StreamState*)dst.p, (const vt_result*)dres.p,
                      slot_stream ? (const int32_t*)dmap.p : nullptr, winner ? (const int32_t*)dwin.p : nullptr,
                      (const PropPolicy*)dpol.p, (const int32_t*)dflag.p, (const bf16_t*)dtpl.p, tpl_bufs, (PropRec*)grec.out(),
                      (int32_t*)dcnt.p, (PropHead*)dhead.p, (int16_t*)gpat.out(), (int16_t*)gth.out(), (float*)gmap.out(),
                      (const PassOut*)dpo.p, pol.max_cells, n};
    HIPCHK(hipDeviceSynchronize());     // the caller's frames may have been filled on another stream
    HIPCHK(launch_proposals_prepare(pa, d, nullptr));
    int level = 0;
    for (int b = 0; b < n; ++b) level = std::max(level, pix_level(frames[b].format));
    HIPCHK(launch_proposals_thumb(pa, d, level, nullptr));
    HIPCHK(launch_proposals_match(pa, nullptr));
    HIPCHK(launch_proposals_list(pa, nullptr));
    HIPCHK(hipDeviceSynchronize());
    const GuardedOut* outs[] = {&gpat, &gth, &gmap, &grec};
    const char* const names[] = {"pattern", "thumbnail", "map", "records"};
    for (int k = 0; k < 4; ++k) {
        long where = 0;
        HIPCHK(outs[k]->check(&where));
        if (where) return set_err(VT_ERR_HIP, "proposals wrote outside its %s: guard byte %ld changed", names[k], where);
    }
    HIPCHK(hipMemcpy(pattern, gpat.out(), gpat.bytes, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(thumb, gth.out(), gth.bytes, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(map, gmap.out(), gmap.bytes, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(records, grec.out(), grec.bytes, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(evaluated, dcnt.p, (size_t)n_streams * 4, hipMemcpyDeviceToHost));
    return VT_OK;
} VT_NOTHROW_INT

// The folded LayerNorm as the engine runs it, end to end (see include/vittrack_hip_ops.h): X-epilogue producer -> row
// terms by one of the three routes of the xgemm lambda (vt_engine.hip) -> launch_fold_layernorm -> the consuming GEMM
// on the hi half of the pair. Every device output lies between guard bands and starts as 0xff.
int vt_op_ln_chain_bf16(int device_id, const float* x, int B, int tokens, int D, const uint16_t* w, const float* gamma,
                        const float* beta, const float* bias, int N, int consumer, int route, int producer_cfg,
                        int consumer_cfg, float eps, int lo_shift, int launches, float* out, float* vt_out,
                        uint16_t* xh_out, int8_t* xl_out, float* cstat_out, float* rowstat_out, uint16_t* wf_out,
                        float* colsum_out, float* cvec_out) try {
    if (!w || !gamma || !beta || !bias || D <= 0 || (D & 1) || N <= 0 || launches < 1 || launches > 16)
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    const bool fold_only = consumer == 0;
    int epi = 0;
    switch (consumer) {
        case 0: break;
        case 2: epi = EPI_GELU_BF16; break;
        case 3: epi = EPI_RELU_BF16; break;
        case 4: epi = EPI_QKV; break;
        default: return set_err(VT_ERR_INVALID_ARG, "ln chain: unknown consumer %d", consumer);
    }
    const long long Mll = (long long)B * tokens;
    int pcfg = producer_cfg, ccfg = consumer_cfg;
    GemmArgs pa{}, ca{};
    if (!fold_only) {
        if (!x || !out || B <= 0 || tokens <= 0 || Mll > (1 << 20) || D % 64 || N % 64 || D > 2048 || !(eps >= 0.0f))
            return set_err(VT_ERR_INVALID_ARG, "bad argument");
        if (lo_shift < VT_LO_SHIFT_MIN || lo_shift > VT_LO_SHIFT_MAX) return set_err(VT_ERR_INVALID_ARG, "ln chain: lo_shift %d out of range", lo_shift);
        if (route < 0 || route > 2) return set_err(VT_ERR_INVALID_ARG, "ln chain: unknown route %d", route);
        if (epi == EPI_QKV && (N != 3 * D || (tokens & 3) || !vt_out))
            return set_err(VT_ERR_INVALID_ARG, "ln chain: QKV takes N == 3 * D, tokens %% 4 == 0 and vt_out");
        // the shapes of the two launches, enough of them to ask the launcher which configuration it would take
        pa.M = (int)Mll; pa.N = D; pa.K = 128; pa.lda = 128; pa.ldw = 128; pa.ldx = D; pa.pos_rows = (int)Mll;
        ca.M = (int)Mll; ca.N = N; ca.K = D; ca.lda = D; ca.ldw = D; ca.ldcb = N;
        ca.tokens = tokens; ca.npad = (tokens + 63) / 64 * 64; ca.D = D;
        if (route == 1 && (D % 256 || D > 1536 || (pcfg >= 0 && pcfg < GEMM_CFG_256_MIN)))
            return set_err(VT_ERR_INVALID_ARG, "ln chain: route 1 takes a 256x256 producer, D %% 256 == 0, D <= 1536");
        if (route == 2 && (D % 128 || D > 1024 || ccfg > GEMM_CFG_SMALL_MAX))
            return set_err(VT_ERR_INVALID_ARG, "ln chain: route 2 takes a 4-wave consumer, D %% 128 == 0, D <= 1024");
    }
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    const size_t WN = (size_t)N * D;
    DevBuf dw, dg, dbeta, dbias;
    GuardedOut gwf, gcs, gcv;
    HIPCHK(dw.alloc(WN * 2)); HIPCHK(dg.alloc((size_t)D * 4)); HIPCHK(dbeta.alloc((size_t)D * 4)); HIPCHK(dbias.alloc((size_t)N * 4));
    HIPCHK(gwf.alloc(WN * 2)); HIPCHK(gcs.alloc((size_t)N * 4)); HIPCHK(gcv.alloc((size_t)N * 4));
    HIPCHK(hipMemcpy(dw.p, w, WN * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dg.p, gamma, (size_t)D * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dbeta.p, beta, (size_t)D * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dbias.p, bias, (size_t)N * 4, hipMemcpyHostToDevice));
    auto fold = [&] {
        return launch_fold_layernorm((const bf16_t*)dw.p, (const float*)dg.p, (const float*)dbeta.p, (const float*)dbias.p,
                                     (bf16_t*)gwf.out(), (float*)gcs.out(), (float*)gcv.out(), N, D, nullptr);
    };
    auto guards = [&](std::initializer_list<std::pair<const GuardedOut*, const char*>> outs) -> int {
        for (const auto& o : outs) {
            if (!o.first->bytes) continue;
            long where = 0;
            HIPCHK(o.first->check(&where));
            if (where) return set_err(VT_ERR_HIP, "ln chain wrote outside its %s: guard byte %ld changed", o.second, where);
        }
        return VT_OK;
    };
    auto fold_back = [&]() -> int {
        if (wf_out) HIPCHK(hipMemcpy(wf_out, gwf.out(), WN * 2, hipMemcpyDeviceToHost));
        if (colsum_out) HIPCHK(hipMemcpy(colsum_out, gcs.out(), (size_t)N * 4, hipMemcpyDeviceToHost));
        if (cvec_out) HIPCHK(hipMemcpy(cvec_out, gcv.out(), (size_t)N * 4, hipMemcpyDeviceToHost));
        return VT_OK;
    };
    if (fold_only) {
        for (int rep = 0; rep < launches; ++rep) HIPCHK(fold());
        HIPCHK(hipDeviceSynchronize());
        if (int rc = guards({{&gwf, "folded weights"}, {&gcs, "column sums"}, {&gcv, "constant vector"}})) return rc;
        return fold_back();
    }
    HIPCHK(gemm_prepare());
    const int M = (int)Mll, nchunk = D / VT_STAT_CHUNK, H = D / 64, npad = ca.npad;
    const size_t MD = (size_t)M * D, n_out = epi == EPI_QKV ? (size_t)M * 2 * D : (size_t)M * N,
                 n_vt = epi == EPI_QKV ? (size_t)B * H * 64 * npad : 0, n_cnt = (size_t)(M + 255) / 256 + 1;
    DevBuf dza, dzw, dzb, dpos, dcnt;
    GuardedOut gxh, gxl, gcst, grs, gout, gvt;
    HIPCHK(dza.alloc((size_t)M * 128 * 2)); HIPCHK(dzw.alloc((size_t)D * 128 * 2)); HIPCHK(dzb.alloc((size_t)D * 4));
    HIPCHK(dpos.alloc(MD * 4)); HIPCHK(dcnt.alloc(n_cnt * 4));
    HIPCHK(gxh.alloc(MD * 2)); HIPCHK(gxl.alloc(MD)); HIPCHK(gcst.alloc((size_t)M * nchunk * 8)); HIPCHK(grs.alloc((size_t)M * 8));
    HIPCHK(gout.alloc(n_out * 2));
    if (n_vt) HIPCHK(gvt.alloc(n_vt * 2));
    HIPCHK(hipMemset(dza.p, 0, (size_t)M * 128 * 2)); HIPCHK(hipMemset(dzw.p, 0, (size_t)D * 128 * 2));
    HIPCHK(hipMemset(dzb.p, 0, (size_t)D * 4)); HIPCHK(hipMemset(dcnt.p, 0, n_cnt * 4));
    HIPCHK(hipMemcpy(dpos.p, x, MD * 4, hipMemcpyHostToDevice));
    // producer: (0 + 0) + pos = x exactly, through the X-epilogue's statistics and split
    pa.A = (const bf16_t*)dza.p; pa.W = (const bf16_t*)dzw.p; pa.bias = (const float*)dzb.p;
    pa.pos = (const float*)dpos.p; pa.Xh = (bf16_t*)gxh.out(); pa.Xl = (uint8_t*)gxl.out();
    pa.cstat = (float2*)gcst.out(); pa.ln_eps = eps; pa.lq = lo_quant(lo_shift);
    if (pcfg >= 0) { pa.tile_order = (pcfg >> 8) & 3; pcfg &= 0xff; }
    if (route == 1) { pa.rowstat_out = (float2*)grs.out(); pa.panel_cnt = (unsigned*)dcnt.p; }
    if (pcfg < 0) pcfg = gemm_effective_config(pa, EPI_F32_POS);
    if (route == 1 && !(pcfg >= GEMM_CFG_256_MIN && gemm256_fits(pa, EPI_F32_POS)))
        return set_err(VT_ERR_INVALID_ARG, "ln chain: route 1 takes a 256x256 producer (configuration %d chosen)", pcfg);
    // consumer: A = the hi half, W = the folded weights, bias = cvec, row terms by route
    ca.A = (const bf16_t*)gxh.out(); ca.W = (const bf16_t*)gwf.out(); ca.bias = (const float*)gcv.out();
    ca.colsum = (const float*)gcs.out(); ca.ln_eps = eps;
    if (epi == EPI_QKV) { ca.qk = (bf16_t*)gout.out(); ca.vt = (bf16_t*)gvt.out(); }
    else ca.Cb = (bf16_t*)gout.out();
    if (ccfg >= 0) { ca.tile_order = (ccfg >> 8) & 3; ccfg &= 0xff; }
    if (route == 2) ca.cstat_in = (const float2*)gcst.out();
    else ca.rowstat = (const float2*)grs.out();        // the pair load of the last even row ends in the guard band
    if (ccfg < 0) ccfg = gemm_effective_config(ca, epi);
    if (route == 2 && ccfg > GEMM_CFG_SMALL_MAX)
        return set_err(VT_ERR_INVALID_ARG, "ln chain: route 2 takes a 4-wave consumer (configuration %d chosen)", ccfg);
    for (int rep = 0; rep < launches; ++rep) {
        if (launch_gemm_cfg(pa, EPI_F32_POS, pcfg, nullptr) != hipSuccess)
            return set_err(VT_ERR_INVALID_ARG, "ln chain: producer configuration %d does not fit M=%d D=%d", pcfg, M, D);
        if (route == 0) HIPCHK(launch_rowstat_finalize(pa.cstat, (float2*)grs.out(), M, nchunk, eps, nullptr));
        HIPCHK(fold());
        if (launch_gemm_cfg(ca, epi, ccfg, nullptr) != hipSuccess)
            return set_err(VT_ERR_INVALID_ARG, "ln chain: consumer configuration %d does not fit M=%d N=%d D=%d", ccfg, M, N, D);
    }
    HIPCHK(hipDeviceSynchronize());
    if (int rc = guards({{&gxh, "hi half"}, {&gxl, "lo8 half"}, {&gcst, "chunk partials"}, {&grs, "row terms"}, {&gout, "output"},
                         {&gvt, "Vt"}, {&gwf, "folded weights"}, {&gcs, "column sums"}, {&gcv, "constant vector"}})) return rc;
    std::vector<unsigned> cnt(n_cnt);
    HIPCHK(hipMemcpy(cnt.data(), dcnt.p, n_cnt * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n_cnt; ++i)
        if (cnt[i]) return set_err(VT_ERR_HIP, "ln chain: panel counter %zu is %u after %d launches", i, cnt[i], launches);
    auto widen = [](const void* d, size_t count, float* o) -> hipError_t {
        std::vector<bf16_t> tmp(count);
        hipError_t e = hipMemcpy(tmp.data(), d, count * 2, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        for (size_t i = 0; i < count; ++i) { uint32_t u = ((uint32_t)tmp[i]) << 16; memcpy(o + i, &u, 4); }
        return hipSuccess;
    };
    HIPCHK(widen(gout.out(), n_out, out));
    if (n_vt) HIPCHK(widen(gvt.out(), n_vt, vt_out));
    if (xh_out) HIPCHK(hipMemcpy(xh_out, gxh.out(), MD * 2, hipMemcpyDeviceToHost));
    if (xl_out) HIPCHK(hipMemcpy(xl_out, gxl.out(), MD, hipMemcpyDeviceToHost));
    if (cstat_out) HIPCHK(hipMemcpy(cstat_out, gcst.out(), (size_t)M * nchunk * 8, hipMemcpyDeviceToHost));
    if (rowstat_out) HIPCHK(hipMemcpy(rowstat_out, grs.out(), (size_t)M * 8, hipMemcpyDeviceToHost));
    return fold_back();
} VT_NOTHROW_INT

}  // extern "C"
