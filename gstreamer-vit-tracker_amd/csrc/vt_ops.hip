// vt_ops.hip — operator-level entry points (include/vittrack_hip_ops.h): numerics tests and tuning tools call the
// same kernel launchers the pass uses. Linked into libvittrack_hip_ops.so only; the product library does not carry them.
// What the hooks share lives in vt_ops_host.hpp (host arithmetic) and vt_ops_util.hpp (device buffers, guard bands, timing,
// and for the in-the-pass launches the slot maps, the frame list, the pinned mirrors and the policy words through a key table).
// Every buffer a kernel writes and a hook downloads is a GuardedOut, checked with guards_intact() after the synchronise;
// the timing entry points and loops are not.
#include "vt_ops_util.hpp"
#include "k_movers.hpp"
#include "../../include/vittrack_hip_ops.h"

// q, k, v [B*N][D] packed into the layouts the QKV epilogue produces: qk [B*N][2D], vt [B*H][64][npad] (perm: in the key
// order attention mode 3 reads)
static void pack_qkv(const uint16_t* q, const uint16_t* k, const uint16_t* v, int B, int N, int H, int npad, bool perm,
                     std::vector<bf16_t>& qk, std::vector<bf16_t>& vt) {
    const int D = H * 64, M = B * N;
    qk.assign((size_t)M * 2 * D, 0);
    vt.assign((size_t)B * H * 64 * npad, 0);
    for (int m = 0; m < M; ++m) {
        memcpy(&qk[(size_t)m * 2 * D], q + (size_t)m * D, (size_t)D * 2);
        memcpy(&qk[(size_t)m * 2 * D + D], k + (size_t)m * D, (size_t)D * 2);
        const int b = m / N, t = m % N, tp = perm ? attn_perm16(t) : t;
        for (int c = 0; c < D; ++c)
            vt[((size_t)(b * H + c / 64) * 64 + c % 64) * npad + tp] = v[(size_t)m * D + c];
    }
}

using namespace vtkeys;     // the key tables (vt_feature_keys.hpp) under their own names, as in vt_features.hip

extern "C" {

// ---- operator-level entry points ---------------------------------------------------------------------------

// epilogue: 0 x = acc + bias, 1 x = (acc + bias) + c_inout, 4 x = (acc + bias) + pos (pos = c_inout, one
// row per output row) - the X-epilogues: c_inout goes in and comes back through the 3-byte pair (hi + lo8 * 2^-s: bf16 and
// an absolute quantum of 2^-s, s = lo_shift), rowstat_out (if given) receives the finalized row terms (rstd, -mean * rstd) of x;
// 2 gelu, 3 relu -> bf16, with an optional folded LayerNorm (rowstat_in [M][2], colsum [N]).
int vt_op_gemm_bf16_lo(int device_id, const uint16_t* a, const uint16_t* w, const float* bias, float* c_inout,
                       int M, int N, int K, int epilogue, int cfg, const float* rowstat_in, const float* colsum,
                       float* rowstat_out, float eps, int lo_shift) try {
    if (!a || !w || !c_inout || M <= 0 || N <= 0 || K <= 0) return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (!lo_shift_ok(lo_shift)) return set_err(VT_ERR_INVALID_ARG, "gemm: lo_shift %d out of range", lo_shift);
    if (N % 64 || K % 64) return set_err(VT_ERR_INVALID_ARG, "gemm: N and K must be multiples of 64");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    HIPCHK(gemm_prepare()); HIPCHK(attention_prepare()); HIPCHK(headconv_prepare());
    const size_t MN = (size_t)M * N, cnt_bytes = (size_t)((M + 255) / 256 + 1) * 4;
    GemmArgs g{};
    GemmOperands ops;
    HIPCHK(ops.upload(g, a, w, bias, M, N, K, K));
    DevArr dpos, dcs, drs, dcnt;
    GuardedOut dxh, dxl, dcb, dcst, dro;
    HIPCHK(dcb.alloc(MN * 2));
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
    std::vector<bf16_t> hi(MN);
    std::vector<int8_t> lo(MN);
    if (epi == EPI_RESID) {     // the addend goes in as the pair the engine would hold, and stays between the bands
        pair_pack(c_inout, MN, lo_shift, hi.data(), lo.data());
        HIPCHK(dxh.upload(hi.data(), MN * 2)); HIPCHK(dxl.upload(lo.data(), MN));
    } else {
        HIPCHK(dxh.alloc(MN * 2)); HIPCHK(dxl.alloc(MN));
    }
    if (epi == EPI_F32_POS) {
        HIPCHK(dpos.upload(c_inout, MN * 4));
        g.pos = dpos.as<const float>(); g.pos_rows = M;
    }
    g.Xh = dxh.as<bf16_t>(); g.Xl = dxl.as<uint8_t>(); g.ldx = N; g.Cb = dcb.as<bf16_t>(); g.ldcb = N;
    if (x_epi) {
        HIPCHK(dcst.alloc((size_t)M * (N / VT_STAT_CHUNK) * 8));
        g.cstat = dcst.as<float2>();
    } else if (rowstat_in) {
        if (!colsum) return set_err(VT_ERR_INVALID_ARG, "gemm: rowstat without colsum");
        HIPCHK(drs.upload(rowstat_in, (size_t)M * 8, 16)); HIPCHK(dcs.upload(colsum, (size_t)N * 4));
        g.rowstat = drs.as<const float2>(); g.colsum = dcs.as<const float>();
    }
    // X-epilogues on the 256x256 kernel finalize the row terms themselves (last workgroup of each row panel)
    bool fused = false;
    const TileCfg tc = split_cfg(cfg);
    g.tile_order = tc.order; cfg = tc.cfg;
    if (x_epi && rowstat_out) {
        HIPCHK(dro.alloc((size_t)M * 8));
        HIPCHK(dcnt.zeros(cnt_bytes));
        const int eff = cfg < 0 ? gemm_effective_config(g, epi) : cfg;
        if (eff >= GEMM_CFG_256_MIN) {
            g.rowstat_out = dro.as<float2>(); g.panel_cnt = dcnt.as<unsigned>(); g.ln_eps = eps;
            fused = true;
        }
    }
    if (cfg < 0) HIPCHK(launch_gemm(g, epi, nullptr));
    else if (launch_gemm_cfg(g, epi, cfg, nullptr) != hipSuccess)
        return set_err(VT_ERR_INVALID_ARG, "gemm: tile configuration %d does not fit M=%d N=%d K=%d", cfg, M, N, K);
    if (x_epi && rowstat_out && !fused)
        HIPCHK(launch_rowstat_finalize(g.cstat, dro.as<float2>(), M, N / VT_STAT_CHUNK, eps, nullptr));
    if (fused) {      // launch it twice more: the counters must come back to zero by themselves
        for (int rep = 0; rep < 2 && (epi == EPI_F32 || epi == EPI_F32_POS); ++rep) HIPCHK(launch_gemm_cfg(g, epi, cfg < 0 ? gemm_effective_config(g, epi) : cfg, nullptr));
    }
    HIPCHK(hipDeviceSynchronize());
    char what[48];
    snprintf(what, sizeof(what), "gemm epilogue %d", epilogue);
    if (int rc = guards_intact(what, {{&dcb, "bf16 output"}, {&dxh, "hi half"}, {&dxl, "lo8 half"}, {&dcst, "chunk partials"},
                                      {&dro, "row terms"}})) return rc;
    if (x_epi) {
        HIPCHK(dxh.download(hi.data())); HIPCHK(dxl.download(lo.data()));
        pair_value(hi.data(), lo.data(), MN, g.lq.q, c_inout);
        if (rowstat_out) HIPCHK(dro.download(rowstat_out));
    } else {
        HIPCHK(download_bf16(dcb.out(), MN, c_inout));
    }
    return VT_OK;
} VT_NOTHROW_INT

// The residual GEMM of the 256x256 kernel on a pair given as it is stored, with the remapped addend read of the last
// encoder block (GemmArgs.seg_rows / seg_skip / Xh_in): see include/vittrack_hip_ops.h
int vt_op_gemm_resid_seg_bf16(int device_id, const uint16_t* a, const uint16_t* w, const float* bias, const uint16_t* xh_in,
                              const int8_t* xl_in, int rows_in, uint16_t* xh_out, int8_t* xl_out, float* cstat_out,
                              float* rowstat_out, int M, int N, int K, int seg_rows, int seg_skip, float eps, int lo_shift) try {
    if (!a || !w || !xh_in || !xl_in || !xh_out || !xl_out || M <= 0 || N <= 0 || K <= 0 || rows_in <= 0 || seg_rows < 0 || seg_skip < 0)
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (!lo_shift_ok(lo_shift)) return set_err(VT_ERR_INVALID_ARG, "gemm: lo_shift %d out of range", lo_shift);
    // every input row the kernel may read exists: the last output row's place in the input layout
    const long long last_in = seg_rows > 0 ? (long long)(M - 1) + ((long long)((M - 1) / seg_rows) + 1) * seg_skip : (long long)M - 1;
    if (last_in >= rows_in) return set_err(VT_ERR_INVALID_ARG, "gemm: the input pair has %d rows, the addend read reaches row %lld", rows_in, last_in);
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    HIPCHK(gemm_prepare());
    const size_t MN = (size_t)M * N, IN = (size_t)rows_in * N, nchunk = (size_t)N / VT_STAT_CHUNK;
    GemmArgs g{};
    GemmOperands ops;
    HIPCHK(ops.upload(g, a, w, bias, M, N, K, K));
    DevArr dih, dil, dcnt;
    GuardedOut doh, dol, dcst, dro;
    HIPCHK(dih.upload(xh_in, IN * 2)); HIPCHK(dil.upload(xl_in, IN));
    HIPCHK(dcnt.zeros((size_t)((M + 255) / 256 + 1) * 4));
    HIPCHK(dcst.alloc((size_t)M * nchunk * 8)); HIPCHK(dro.alloc((size_t)M * 8));
    if (seg_rows > 0) {     // addend from the input pair through the remap, output compact
        g.Xh_in = dih.as<const bf16_t>(); g.Xl_in = dil.as<const uint8_t>(); g.seg_rows = seg_rows; g.seg_skip = seg_skip;
        HIPCHK(doh.alloc(MN * 2)); HIPCHK(dol.alloc(MN));
    } else {                // the launch as it always was: rows 0 .. M-1 of the pair, read and written in place
        HIPCHK(doh.upload(xh_in, MN * 2)); HIPCHK(dol.upload(xl_in, MN));
    }
    g.Xh = doh.as<bf16_t>(); g.Xl = dol.as<uint8_t>(); g.ldx = N;
    g.cstat = dcst.as<float2>(); g.rowstat_out = dro.as<float2>(); g.panel_cnt = dcnt.as<unsigned>(); g.ln_eps = eps;
    g.lq = lo_quant(lo_shift);
    if (launch_gemm_cfg(g, EPI_RESID, GEMM_CFG_256P4, nullptr) != hipSuccess)
        return set_err(VT_ERR_INVALID_ARG, "gemm: the 256x256 kernel does not take M=%d N=%d K=%d seg_rows=%d seg_skip=%d", M, N, K, seg_rows, seg_skip);
    HIPCHK(hipDeviceSynchronize());
    if (int rc = guards_intact("gemm resid_seg", {{&doh, "hi half"}, {&dol, "lo8 half"}, {&dcst, "chunk partials"}, {&dro, "row terms"}}))
        return rc;
    HIPCHK(doh.download(xh_out)); HIPCHK(dol.download(xl_out));
    if (cstat_out) HIPCHK(dcst.download(cstat_out));
    if (rowstat_out) HIPCHK(dro.download(rowstat_out));
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
    std::vector<bf16_t> ha((size_t)M * K), hw((size_t)N * K);
    fill_lcg_bf16(hw.data(), hw.size(), fill_lcg_bf16(ha.data(), ha.size(), 12345u));
    GemmArgs g{};
    GemmOperands ops;           // the bias: zeros
    HIPCHK(ops.upload(g, ha.data(), hw.data(), nullptr, M, N, K, K));
    DevArr dc, dcb, dvt, dxl, dcst, drs;
    HIPCHK(dc.zeros((size_t)M * N * 4)); HIPCHK(dcb.zeros((size_t)M * N * 2)); HIPCHK(dxl.zeros((size_t)M * N * 2));
    HIPCHK(dcst.alloc((size_t)M * (N / VT_STAT_CHUNK) * 8));
    HIPCHK(dvt.alloc((size_t)(N / 64 + 1) * 64 * npad * 2));
    {   // folded-LayerNorm row terms as the engine passes them to the QKV / fc1 GEMMs: (1, 0) per row
        std::vector<float> rs((size_t)M * 2);
        for (int i = 0; i < M; ++i) { rs[2 * (size_t)i] = 1.0f; rs[2 * (size_t)i + 1] = 0.0f; }
        HIPCHK(drs.upload(rs.data(), rs.size() * 4, 16));
    }
    g.Cb = dcb.as<bf16_t>(); g.ldcb = N;
    const bool x_epi = epilogue == EPI_F32 || epilogue == EPI_RESID || epilogue == EPI_F32_POS;
    DevArr dcnt, dro;
    if (x_epi) {      // as the engine launches it: chunk partials + the row terms finalized by the last workgroup of each panel
        g.Xh = dcb.as<bf16_t>(); g.Xl = dxl.as<uint8_t>(); g.ldx = N; g.cstat = dcst.as<float2>();
        HIPCHK(dcnt.zeros((size_t)((M + 255) / 256 + 1) * 4)); HIPCHK(dro.alloc((size_t)M * 8 + 16));
        g.rowstat_out = dro.as<float2>(); g.panel_cnt = dcnt.as<unsigned>(); g.ln_eps = 1e-6f;
    }
    else if (epilogue == EPI_QKV || epilogue == EPI_GELU_BF16) { g.rowstat = drs.as<const float2>(); g.colsum = ops.bias.as<const float>(); }
    g.pos = dc.as<const float>(); g.pos_rows = M;
    g.qk = dcb.as<bf16_t>(); g.vt = dvt.as<bf16_t>(); g.tokens = tokens; g.npad = npad; g.D = D;
    if (epilogue == EPI_QKV && (N % 192 || tokens != M)) return set_err(VT_ERR_INVALID_ARG, "qkv bench: N = 3D, D %% 64 == 0, M %% 4 == 0");
    const TileCfg tc = split_cfg(cfg);      // sweeps force the XCD tile order
    g.tile_order = tc.order; cfg = tc.cfg;
    if (cfg < 0) cfg = gemm_pick_config(M, N, K, epilogue);
    DevArr ddbg;
    const size_t dbg_words = (size_t)((M + 63) / 64) * (N / 64) * 8 * 4;
#ifdef VT_STAMPS   // diagnostic builds only: per-wave cycle sums of the main loop
    HIPCHK(ddbg.zeros(dbg_words * 8));
    g.dbg = ddbg.as<unsigned long long>();
#else
    (void)dbg_words;
#endif
    HIPCHK(time_launches(iters, [&] { return launch_gemm_cfg(g, epilogue, cfg, nullptr); }, us_out));
    if (g.dbg) {   // diagnostic build: mean per-wave cycle split of the main loop
        std::vector<unsigned long long> h(dbg_words);
        HIPCHK(ddbg.download(h.data()));
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
    const size_t n_qk = (size_t)M * 2 * D, n_vt = (size_t)B * H * 64 * npad;
    GemmArgs g{};
    GemmOperands ops;
    HIPCHK(ops.upload(g, a, w, bias, M, 3 * D, D, D));
    DevArr drs, dcs;
    GuardedOut dqk, dvt;    // Vt starts as zeros: the kernels leave its padding positions alone, the engine zeroes it once
    HIPCHK(dqk.alloc(n_qk * 2)); HIPCHK(dvt.alloc(n_vt * 2, 0));
    g.qk = dqk.as<bf16_t>(); g.vt = dvt.as<bf16_t>(); g.tokens = tokens; g.npad = npad; g.D = D;
    g.vt_perm = vt_perm ? 1 : 0;   // 1: the key order attention mode 3 reads
    if (rowstat_in) {              // folded LayerNorm: [M][2] row terms, [3D] column sums
        if (!colsum) return set_err(VT_ERR_INVALID_ARG, "qkv: rowstat without colsum");
        HIPCHK(drs.upload(rowstat_in, (size_t)M * 8, 16)); HIPCHK(dcs.upload(colsum, (size_t)3 * D * 4));
        g.rowstat = drs.as<const float2>(); g.colsum = dcs.as<const float>();
    }
    const TileCfg tc = split_cfg(cfg);
    g.tile_order = tc.order; cfg = tc.cfg;
    if (cfg < 0) HIPCHK(launch_gemm(g, EPI_QKV, nullptr));
    else if (launch_gemm_cfg(g, EPI_QKV, cfg, nullptr) != hipSuccess)
        return set_err(VT_ERR_INVALID_ARG, "qkv: tile configuration %d does not fit this shape", cfg);
    HIPCHK(hipDeviceSynchronize());
    if (int rc = guards_intact("qkv", {{&dqk, "qk"}, {&dvt, "Vt"}})) return rc;
    HIPCHK(download_bf16(dqk.out(), n_qk, qk_out));
    HIPCHK(download_bf16(dvt.out(), n_vt, vt_out));
    return VT_OK;
} VT_NOTHROW_INT

int vt_op_attention_bf16(int device_id, const uint16_t* q, const uint16_t* k, const uint16_t* v, float* out,
                         int B, int N, int H, int mode) try {
    if (!q || !k || !v || !out || B <= 0 || N <= 0 || H <= 0) return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    HIPCHK(attention_prepare());
    const int npad = (N + 63) / 64 * 64;
    const size_t n_out = (size_t)B * N * H * 64;
    if (mode < 0) mode = attention_pick_mode(N, npad);
    std::vector<bf16_t> qk, vt;
    pack_qkv(q, k, v, B, N, H, npad, attention_vt_perm(mode) != 0, qk, vt);
    DevArr dqk, dvt;
    GuardedOut dout;
    HIPCHK(dqk.upload(qk.data(), qk.size() * 2)); HIPCHK(dvt.upload(vt.data(), vt.size() * 2)); HIPCHK(dout.alloc(n_out * 2));
    HIPCHK(launch_attention_mode(dqk.as<const bf16_t>(), dvt.as<const bf16_t>(), dout.as<bf16_t>(), B, N, H, npad, mode, nullptr));
    HIPCHK(hipDeviceSynchronize());
    char what[48];
    snprintf(what, sizeof(what), "attention mode %d", mode);
    if (int rc = guards_intact(what, {{&dout, "output"}})) return rc;
    HIPCHK(download_bf16(dout.out(), n_out, out));
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
    const int npad = (N + 63) / 64 * 64;
    const size_t n_out = (size_t)B * nq * H * 64;
    std::vector<bf16_t> qk, vt;
    pack_qkv(q, k, v, B, N, H, npad, true, qk, vt);
    DevArr dqk, dvt;
    GuardedOut dout;
    HIPCHK(dqk.upload(qk.data(), qk.size() * 2)); HIPCHK(dvt.upload(vt.data(), vt.size() * 2)); HIPCHK(dout.alloc(n_out * 2));
    HIPCHK(launch_attention_queries(dqk.as<const bf16_t>(), dvt.as<const bf16_t>(), dout.as<bf16_t>(), B, N, H, npad, q0, nq, nullptr));
    HIPCHK(hipDeviceSynchronize());
    char what[64];
    snprintf(what, sizeof(what), "attention on queries %d..%d", q0, q0 + nq - 1);
    if (int rc = guards_intact(what, {{&dout, "output"}})) return rc;
    HIPCHK(download_bf16(dout.out(), n_out, out));
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
    fill_lcg_bf16(vt.data(), vt.size(), fill_lcg_bf16(qk.data(), qk.size(), 777u));
    DevArr dqk, dvt, dout;
    HIPCHK(dqk.upload(qk.data(), qk.size() * 2)); HIPCHK(dvt.upload(vt.data(), vt.size() * 2)); HIPCHK(dout.alloc((size_t)M * D * 2));
    HIPCHK(time_launches(iters, [&] {
        return launch_attention_mode(dqk.as<const bf16_t>(), dvt.as<const bf16_t>(), dout.as<bf16_t>(), B, N, H, npad, mode, nullptr);
    }, us_out));
    return VT_OK;
} VT_NOTHROW_INT

int vt_op_nv12_to_rgb8_bench(int device_id, int w, int h, int iters, float* us_out) try {
    if (w < 2 || h < 2 || w > 16384 || h > 16384 || iters < 1 || !us_out) return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    std::vector<uint8_t> host(nv12_bytes_read(w, h) + 16);
    fill_xorshift_u8(host.data(), host.size());
    DevArr din, dout;
    HIPCHK(din.upload(host.data(), host.size())); HIPCHK(dout.alloc((size_t)w * h * 3));
    HIPCHK(time_launches(iters, [&] { return launch_nv12_to_rgb8(din.as<const uint8_t>(), w, h, dout.as<uint8_t>(), nullptr); }, us_out));
    return VT_OK;
} VT_NOTHROW_INT

int vt_op_nv12_to_rgb8_batch_bench(int device_id, int w, int h, int n, int iters, float* us_out) try {
    if (w < 2 || h < 2 || w > 16384 || h > 16384 || n < 1 || n > 1024 || iters < 1 || !us_out) return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    const size_t in_bytes = (nv12_bytes_read(w, h) + 16 + 255) & ~(size_t)255, out_bytes = ((size_t)w * h * 3 + 255) & ~(size_t)255;
    DevArr din, dout;
    HIPCHK(din.alloc(in_bytes * n)); HIPCHK(dout.alloc(out_bytes * n));
    std::vector<uint8_t> host(in_bytes);
    fill_xorshift_u8(host.data(), host.size());
    std::vector<const uint8_t*> ins((size_t)n);
    std::vector<uint8_t*> outs((size_t)n);
    for (int i = 0; i < n; ++i) {       // every frame the same bytes
        ins[(size_t)i] = din.as<const uint8_t>() + (size_t)i * in_bytes;
        outs[(size_t)i] = dout.as<uint8_t>() + (size_t)i * out_bytes;
        HIPCHK(hipMemcpy((void*)ins[(size_t)i], host.data(), in_bytes, hipMemcpyHostToDevice));
    }
    HIPCHK(time_launches(iters, [&] { return launch_nv12_to_rgb8_batch(ins.data(), outs.data(), n, w, h, nullptr); }, us_out));
    return VT_OK;
} VT_NOTHROW_INT

int vt_op_layernorm(int device_id, const float* x, const float* gamma, const float* beta, float* y, int M, int D) try {
    if (!x || !gamma || !beta || !y || M <= 0 || D % 128) return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    const size_t MD = (size_t)M * D;
    DevArr dx, dg, db;
    GuardedOut dy;
    HIPCHK(dx.upload(x, MD * 4)); HIPCHK(dg.upload(gamma, (size_t)D * 4)); HIPCHK(db.upload(beta, (size_t)D * 4)); HIPCHK(dy.alloc(MD * 2));
    HIPCHK(launch_layernorm(dx.as<const float>(), dg.as<const float>(), db.as<const float>(), dy.as<bf16_t>(), M, D, M, 0, 0, 1e-6f, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (int rc = guards_intact("layernorm", {{&dy, "output"}})) return rc;
    HIPCHK(download_bf16(dy.out(), MD, y));
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
    GemmArgs g{};
    GemmOperands ops;
    HIPCHK(ops.upload(g, t, w, bias, M, N, 9 * C, C));
    DevArr dz;
    GuardedOut dout;
    HIPCHK(dout.alloc(M * N * 2)); HIPCHK(dz.zeros(256));
    g.Cb = dout.as<bf16_t>(); g.ldcb = N;
    g.conv_grid = grid; g.conv_C = C; g.zeros = dz.as<const bf16_t>();
    if (cfg < 0) HIPCHK(launch_gemm(g, EPI_RELU_BF16, nullptr));
    else HIPCHK(launch_gemm_cfg(g, EPI_RELU_BF16, cfg, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (int rc = guards_intact("conv3x3", {{&dout, "output"}})) return rc;
    HIPCHK(download_bf16(dout.out(), M * N, out));
    return VT_OK;
} VT_NOTHROW_INT

// The head's band kernel (k_head.hip) on its own: out = relu(conv(t) + bias), conv3x3 != 0: t [B*grid*grid][Cin],
// w [N][9*Cin], N == Cin; else the 1x1 layer: w [N][Cin]. R / ncb <= 0: the launcher's plan. t == NULL: operands
// filled with a fixed pseudo-random pattern (timing runs). out (nullable): [B*grid*grid][N] bf16 values widened
// to f32. us_out (nullable): mean microseconds per launch over iters >= 1 launches.
int vt_op_headconv_bf16(int device_id, const uint16_t* t, const uint16_t* w, const float* bias, float* out,
                        int B, int grid, int Cin, int N, int conv3x3, int R, int ncb, int iters, float* us_out) try {
    if (B < 1 || grid < 1 || Cin % 64 || N % 64 || (t && (!w || !bias)) || (us_out && iters < 1))
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    const int K = conv3x3 ? 9 * Cin : Cin;
    if (!headconv_supported(grid, conv3x3 ? Cin : N, N, K, conv3x3 != 0))
        return set_err(VT_ERR_INVALID_ARG, "shape not supported by the band kernel");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    HIPCHK(headconv_prepare());
    const size_t M = (size_t)B * grid * grid, t_bytes = M * Cin * 2, w_bytes = (size_t)N * K * 2, b_bytes = (size_t)N * 4;
    DevArr dt, dw, db, dz;
    GuardedOut dout;        // checked after the first launch; the timing loop behind it runs unchecked
    if (t) {
        HIPCHK(dt.upload(t, t_bytes)); HIPCHK(dw.upload(w, w_bytes)); HIPCHK(db.upload(bias, b_bytes));
    } else {
        std::vector<bf16_t> ht(t_bytes / 2), hw(w_bytes / 2);
        fill_lcg_bf16(hw.data(), hw.size(), fill_lcg_bf16(ht.data(), ht.size(), 777u));
        HIPCHK(dt.upload(ht.data(), t_bytes)); HIPCHK(dw.upload(hw.data(), w_bytes)); HIPCHK(db.zeros(b_bytes));
    }
    HIPCHK(dout.alloc(M * N * 2)); HIPCHK(dz.zeros(256));
    HeadConvArgs h{};
    h.in = dt.as<const bf16_t>(); h.ldin = Cin; h.W = dw.as<const bf16_t>(); h.ldw = K; h.bias = db.as<const float>();
    h.out = dout.as<bf16_t>(); h.ldout = N; h.zeros = dz.as<const bf16_t>();
    h.B = B; h.grid = grid; h.C = conv3x3 ? Cin : N; h.N = N; h.K = K; h.conv3x3 = conv3x3 ? 1 : 0;
    h.R = R; h.ncb = ncb;
    HIPCHK(launch_headconv(h, nullptr, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (int rc = guards_intact("headconv", {{&dout, "output"}})) return rc;
    if (out) HIPCHK(download_bf16(dout.out(), M * N, out));
#ifdef VT_STAMPS   // diagnostic builds only: per-wave cycle sums of the main loop, medians printed
    DevArr ddbg;
    const size_t dbg_words = (size_t)B * grid * 2 * 8 * 4;
    HIPCHK(ddbg.zeros(dbg_words * 8));
    h.dbg = ddbg.as<unsigned long long>();
#endif
    if (us_out) HIPCHK(time_launches(iters, [&] { return launch_headconv(h, nullptr, nullptr); }, us_out));
#ifdef VT_STAMPS
    {
        std::vector<unsigned long long> hd(dbg_words);
        HIPCHK(ddbg.download(hd.data()));
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
    if (!lo_shift_ok(lo_shift)) return set_err(VT_ERR_INVALID_ARG, "headconv_ln: lo_shift %d out of range", lo_shift);
    const float lo_q = lo_quant(lo_shift).q;
    if (B < 1 || grid < 1 || off < 0 || ntok < off + ns || (xh && (!xl || !gamma || !beta || !w || !bias)) || (us_out && iters < 1))
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if (!headconv_ln_supported(grid, N, D))
        return set_err(VT_ERR_INVALID_ARG, "shape not supported by the band kernel with the LayerNorm inside");
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    HIPCHK(headconv_prepare());
    const size_t MxD = (size_t)B * ntok * D, M = (size_t)B * ns, w_bytes = (size_t)N * D * 2, d_bytes = (size_t)D * 4, b_bytes = (size_t)N * 4;
    DevArr dh, dl, dg, dbt, dw, db;
    GuardedOut dfeat, dout; // checked after the first run; the timing loop behind it runs unchecked
    if (xh) {
        HIPCHK(dh.upload(xh, MxD * 2)); HIPCHK(dl.upload(xl, MxD));       // lo8 bytes
        HIPCHK(dg.upload(gamma, d_bytes)); HIPCHK(dbt.upload(beta, d_bytes));
        HIPCHK(dw.upload(w, w_bytes)); HIPCHK(db.upload(bias, b_bytes));
    } else {
        std::vector<bf16_t> hx(MxD), hw(w_bytes / 2);
        std::vector<float> ones((size_t)D, 1.0f);
        fill_lcg_bf16(hw.data(), hw.size(), fill_lcg_bf16(hx.data(), hx.size(), 4242u));
        HIPCHK(dh.upload(hx.data(), MxD * 2)); HIPCHK(dl.zeros(MxD * 2));
        HIPCHK(dg.upload(ones.data(), d_bytes)); HIPCHK(dbt.zeros(d_bytes));
        HIPCHK(dw.upload(hw.data(), w_bytes)); HIPCHK(db.zeros(b_bytes));
    }
    HIPCHK(dfeat.alloc(M * D * 2)); HIPCHK(dout.alloc(M * N * 2));
    HeadConvArgs h{};
    h.W = dw.as<const bf16_t>(); h.ldw = D; h.bias = db.as<const float>(); h.out = dout.as<bf16_t>(); h.ldout = N;
    h.B = B; h.grid = grid; h.C = N; h.N = N; h.K = D; h.conv3x3 = 0; h.R = R; h.ncb = ncb;
    if (fused) {
        h.xh = dh.as<const bf16_t>(); h.xl = dl.as<const uint8_t>(); h.ln_g = dg.as<const float>(); h.ln_b = dbt.as<const float>();
        h.ln_eps = eps; h.in_stride = ntok; h.in_off = off; h.lo_q = lo_q;
    } else {
        h.in = dfeat.as<const bf16_t>(); h.ldin = D;
    }
    auto run = [&]() -> hipError_t {
        if (!fused) {
            hipError_t e = launch_layernorm_split(dh.as<const bf16_t>(), dl.as<const uint8_t>(), dg.as<const float>(), dbt.as<const float>(),
                                                  dfeat.as<bf16_t>(), (int)M, D, ns, ntok, off, eps, lo_q, nullptr);
            if (e != hipSuccess) return e;
        }
        return launch_headconv(h, nullptr, nullptr);
    };
    HIPCHK(run());
    HIPCHK(hipDeviceSynchronize());
    if (int rc = guards_intact("headconv_ln", {{&dfeat, "normalised rows"}, {&dout, "output"}})) return rc;
    if (out) HIPCHK(download_bf16(dout.out(), M * N, out));
    if (us_out) HIPCHK(time_launches(iters, run, us_out));
    return VT_OK;
} VT_NOTHROW_INT

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
    SlotMaps maps{slot_stream, nullptr, B, n_states};       // every slot's stream exists, and no two slots write one state
    if (int rc = maps.check_all("head_decode", "states")) return rc;
    if (int rc = maps.check_unique("head_decode", "listed twice")) return rc;
    if (form == 1 && !headconv_plannable(grid, C, C, 9 * C, true, true))
        return set_err(VT_ERR_INVALID_ARG, "head_decode: grid %d, C %d is no shape of the band kernel's fused tail", grid, C);
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    HIPCHK(headconv_prepare());
    const int ns = grid * grid;
    const size_t M = (size_t)B * ns, res_bytes = (size_t)B * sizeof(vt_result), st_bytes = (size_t)n_states * sizeof(StreamState);
    DevArr dt, dw3, db3, dw4, db4, dhann, dpo, dbest, dz;
    GuardedOut dt3, dho, dst, dres, dcnt;   // states: the caller's; band counters: zeros; the rest 0xff
    Mirror hres, hst;
    HIPCHK(dt.upload(t, M * C * 2)); HIPCHK(dw4.upload(w4, (size_t)8 * C * 4)); HIPCHK(db4.upload(b4, 8 * 4));
    HIPCHK(dhann.upload(hann, (size_t)ns * 4)); HIPCHK(dst.upload(states, st_bytes));
    HIPCHK(dho.alloc(M * 8 * 4)); HIPCHK(dres.alloc(res_bytes));
    HIPCHK(dcnt.alloc((size_t)B * 4, 0)); HIPCHK(dbest.zeros((size_t)B * grid * 2 * 4));
    HIPCHK(hres.from(host_results, res_bytes)); HIPCHK(hst.from(host_states, st_bytes));
    const PassOut po{(flags & 1) ? nullptr : hres.as<vt_result>(), (flags & 2) ? nullptr : hst.as<StreamState>()};
    HIPCHK(dpo.upload(&po, sizeof(po)));
    HIPCHK(maps.upload());
    DecodeArgs dec{};
    dec.w4 = dw4.as<const float>(); dec.b4 = db4.as<const float>(); dec.hann = dhann.as<const float>();
    dec.head_out = dho.as<float>(); dec.states = dst.as<StreamState>(); dec.results = dres.as<vt_result>();
    dec.out = dpo.as<const PassOut>(); dec.slot_stream = maps.dev_slot_stream();
    dec.B = B; dec.ns = ns; dec.grid = grid; dec.C = C; dec.success_threshold = success_threshold;
    HeadConvArgs h{};
    if (form == 0) {
        dec.t3 = dt.as<const bf16_t>();
    } else {
        HIPCHK(dw3.upload(w3, (size_t)C * 9 * C * 2)); HIPCHK(db3.upload(b3, (size_t)C * 4));
        HIPCHK(dz.zeros(256)); HIPCHK(dt3.alloc(M * C * 2));
        dec.t3 = dt3.as<const bf16_t>();
        h.in = dt.as<const bf16_t>(); h.ldin = C; h.W = dw3.as<const bf16_t>(); h.ldw = 9 * C; h.bias = db3.as<const float>();
        h.out = dt3.as<bf16_t>(); h.ldout = C; h.zeros = dz.as<const bf16_t>();
        h.B = B; h.grid = grid; h.C = C; h.N = C; h.K = 9 * C; h.conv3x3 = 1;
        h.R = R > 0 ? R : 0; h.ncb = R > 0 ? C / 64 : 0;      // a given R keeps the tail's one column group; else both planned
        h.band_cnt = dcnt.as<unsigned>(); h.band_best = dbest.as<float>();
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
    if (int rc = guards_intact("head_decode", {{&dt3, "conv output"}, {&dho, "head output"}, {&dst, "states"}, {&dres, "results"},
                                               {&dcnt, "band counters"}})) return rc;
    HIPCHK(dho.download(head_out)); HIPCHK(dres.download(results)); HIPCHK(dst.download(states)); HIPCHK(dcnt.download(band_cnt));
    hres.back(); hst.back();
    return VT_OK;
} VT_NOTHROW_INT

// The response-peaks launch on given operands: see include/vittrack_hip_ops.h. Nothing runs but launch_response_peaks.
int vt_op_response_peaks(int device_id, const float* head_out, const float* hann, void* states, int n_states,
                         const void* policies, const int32_t* slot_stream, const int32_t* winner, int B, int grid,
                         vt_peaks* records, vt_peaks* host_records) try {
    if (!head_out || !hann || !states || !policies || !records || !host_records || B < 1 || B > 4096 || grid < 1 || grid > 110 ||
        n_states < 1)
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    // a per-stream record with a float and no key table: the ranges are checked here
    const PeaksPolicy* pol = (const PeaksPolicy*)policies;
    for (int s = 0; s < n_states; ++s)
        if (pol[s].max_peaks < 0 || pol[s].max_peaks > VT_PEAKS_MAX || pol[s].radius < 1 || pol[s].radius > 4)
            return set_err(VT_ERR_INVALID_ARG, "response_peaks: policy %d: max_peaks %d, radius %d", s, pol[s].max_peaks, pol[s].radius);
    SlotMaps maps{slot_stream, winner, B, n_states};
    if (int rc = maps.check_all("response_peaks", "states")) return rc;
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    const int ns = grid * grid;
    const size_t rec_bytes = (size_t)B * sizeof(vt_peaks);
    DevArr dho, dhann, dpol, dpo;
    GuardedOut dst, drec;   // both start as the caller's bytes
    Mirror hrec;
    HIPCHK(dho.upload(head_out, (size_t)B * ns * 8 * 4)); HIPCHK(dhann.upload(hann, (size_t)ns * 4));
    HIPCHK(dst.upload(states, (size_t)n_states * sizeof(StreamState))); HIPCHK(dpol.upload(policies, (size_t)n_states * sizeof(PeaksPolicy)));
    HIPCHK(drec.upload(records, rec_bytes));
    HIPCHK(hrec.from(host_records, rec_bytes));
    const PassOut po{nullptr, nullptr, hrec.as<vt_peaks>()};
    HIPCHK(dpo.upload(&po, sizeof(po)));
    HIPCHK(maps.upload());
    const PeaksArgs pa{dho.as<const float>(), dhann.as<const float>(), dst.as<const StreamState>(), maps.dev_slot_stream(),
                       maps.dev_winner(), dpol.as<const PeaksPolicy>(), drec.as<vt_peaks>(), dpo.as<const PassOut>(), B, ns, grid};
    const hipError_t e = launch_response_peaks(pa, nullptr);
    if (e == hipErrorInvalidValue) return set_err(VT_ERR_INVALID_ARG, "response_peaks: the launcher refuses grid %d", grid);
    HIPCHK(e);
    HIPCHK(hipDeviceSynchronize());
    if (int rc = guards_intact("response_peaks", {{&drec, "records"}, {&dst, "states"}})) return rc;
    HIPCHK(drec.download(records)); HIPCHK(dst.download(states));
    hrec.back();
    return VT_OK;
} VT_NOTHROW_INT

// The result-overlay launch on given operands: see include/vittrack_hip_ops.h. Nothing runs but launch_result_overlay.
int vt_op_result_overlay(int device_id, const vt_frame* frames, const vt_result* results, const int32_t* slot_stream,
                         const int32_t* winner, int n, const int32_t* policy, int32_t* stats, int n_streams,
                         int device_frames) try {
    if (!frames || !results || !policy || !stats || n < 1 || n > VT_RESULT_OVERLAY_MAX_SLOTS || n_streams < 1)
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    // thickness, size and scale are one packed key of the table and three words here: the ranges are checked by hand
    OverlayPolicy pol;
    memcpy(&pol, policy, sizeof(pol));
    if (pol.flags < 0 || pol.flags > 7 || pol.thickness < 1 || pol.thickness > 16 || pol.size < 1 || pol.size > 64 || pol.scale < 1 ||
        pol.scale > 4 || pol.luma < 0 || pol.luma > 255 || pol.rgb < 0 || pol.rgb > 0xFFFFFF || pol.min_score_pct < 0 ||
        pol.min_score_pct > 100)
        return set_err(VT_ERR_INVALID_ARG, "result_overlay: policy out of range");
    HookFrames fr;
    SlotMaps maps{slot_stream, winner, n, n_streams};
    if (int rc = fr.check(frames, n)) return rc;
    if (int rc = maps.check_all("result_overlay")) return rc;
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    DevArr dres, dpol;
    GuardedOut dst;         // the counters start as the caller's; the frames are the caller's own memory
    HIPCHK(dres.upload(results, (size_t)n * sizeof(vt_result)));
    HIPCHK(dpol.upload(&pol, sizeof(pol))); HIPCHK(dst.upload(stats, (size_t)n_streams * sizeof(OverlayStats)));
    HIPCHK(maps.upload());
    HIPCHK(fr.upload(device_frames));
    const ResultOverlayArgs oa{fr.dev(), dres.as<const vt_result>(), maps.dev_slot_stream(), maps.dev_winner(),
                               dpol.as<const OverlayPolicy>(), dst.as<OverlayStats>(), fr.dev_flag(), n};
    HIPCHK(launch_result_overlay(oa, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (int rc = guards_intact("result_overlay", {{&dst, "counters"}})) return rc;
    HIPCHK(dst.download(stats));
    return VT_OK;
} VT_NOTHROW_INT

// The two launches of the motion prior on given operands: see include/vittrack_hip_ops.h. Nothing runs but
// launch_motion_place (stages & 1) and launch_motion_settle (stages & 2), in that order.
int vt_op_motion_prior(int device_id, void* states, void* records, int n_streams, const int32_t* policy, const vt_result* results,
                       const int32_t* slot_stream, const int32_t* winner, const vt_candidate* cands, int n, int stages,
                       void* host_states, void* host_records) try {
    if (!states || !records || !policy || !results || n < 1 || n > VT_MAX_STREAMS || n_streams < 1 || stages < 1 || stages > 3)
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    if ((cands != nullptr) != (winner != nullptr))
        return set_err(VT_ERR_INVALID_ARG, "motion_prior: the candidate form needs both the slots and the winner list");
    static_assert(sizeof(MotionPolicy) == 4 * MO_WORDS, "MotionPolicy");
    MotionPolicy pol;
    if (int rc = policy_from_words("motion_prior", kMotionKeys, apply_motion, VT_MOTION_DEFAULT_POLICY, policy, &pol)) return rc;
    std::vector<int32_t> map;       // the candidate form's map is its slots' streams
    for (int i = 0; i < n && cands; ++i) map.push_back(cands[i].stream);
    SlotMaps maps{cands ? map.data() : slot_stream, winner, n, n_streams};
    if (int rc = maps.check_all("motion_prior")) return rc;
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    const size_t sb = (size_t)n_streams * sizeof(StreamState), rb = (size_t)n_streams * sizeof(MotionRec);
    DevArr dpol, dres, dcand, dpo;
    GuardedOut dst, drec;   // both start as the caller's bytes
    Mirror hst, hrec;
    HIPCHK(dst.upload(states, sb)); HIPCHK(drec.upload(records, rb)); HIPCHK(dpol.upload(&pol, sizeof(pol)));
    HIPCHK(dres.upload(results, (size_t)n * sizeof(vt_result)));
    HIPCHK(hst.from(host_states, sb)); HIPCHK(hrec.from(host_records, rb));
    const PassOut po{nullptr, hst.as<StreamState>(), nullptr, hrec.as<MotionRec>()};
    HIPCHK(dpo.upload(&po, sizeof(po)));
    HIPCHK(maps.upload());
    HIPCHK(dcand.upload(cands, (size_t)n * sizeof(vt_candidate)));
    const MotionArgs ma{dst.as<StreamState>(), drec.as<MotionRec>(), dpol.as<const MotionPolicy>(), dres.as<const vt_result>(),
                        maps.dev_slot_stream(), maps.dev_winner(), dcand.as<const vt_candidate>(), dpo.as<const PassOut>(), nullptr, n};
    if (stages & 1) HIPCHK(launch_motion_place(ma, nullptr));
    if (stages & 2) HIPCHK(launch_motion_settle(ma, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (int rc = guards_intact("motion_prior", {{&dst, "states"}, {&drec, "records"}})) return rc;
    HIPCHK(dst.download(states)); HIPCHK(drec.download(records));
    hst.back(); hrec.back();
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
    const AppearPolicy pol{1, 1, 0, 0.0f};
    std::vector<AppearRec> recs(n, AppearRec{1, 0, 0.0f, {0.0f, 0.0f, 0.0f, 0.0f}, 0});
    DevArr da, dp, dpol, dcnt;
    GuardedOut drec, dtick, dpart, dsum;
    HIPCHK(da.upload(anchor, rows)); HIPCHK(dp.upload(probe, rows)); HIPCHK(dpol.upload(&pol, sizeof(pol)));
    HIPCHK(drec.upload(recs.data(), n * sizeof(AppearRec)));
    HIPCHK(dcnt.zeros(n * sizeof(AppearCount))); HIPCHK(dtick.alloc(n * sizeof(unsigned), 0));
    HIPCHK(dpart.alloc(n * nch * 5 * sizeof(double)));      // NaN: a partial nobody wrote would show
    HIPCHK(dsum.alloc(n * 5 * sizeof(double)));
    AppearArgs a{};
    a.policy = dpol.as<const AppearPolicy>(); a.counts = dcnt.as<AppearCount>(); a.recs = drec.as<AppearRec>();
    a.tickets = dtick.as<unsigned>(); a.partials = dpart.as<double>();
    a.anchor = da.as<const bf16_t>(); a.probe = dp.as<bf16_t>(); a.sums = dsum.as<double>(); a.n = n_slots;
    HIPCHK(launch_appearance_score(a, nt, cols, kpad, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (int rc = guards_intact("appearance_score", {{&drec, "records"}, {&dtick, "tickets"}, {&dpart, "partials"}, {&dsum, "sums"}}))
        return rc;
    HIPCHK(drec.download(recs.data())); HIPCHK(dsum.download(sums));
    if (int rc = tickets_returned("appearance_score", dtick, 1)) return rc;
    for (size_t i = 0; i < n; ++i) {
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
    // max_cells from VT_PROP_M_MAX^2 here, from 16384 as the engine's key: the op tests use small stores, so no table
    PropPolicy pol;
    memcpy(&pol, policy, sizeof(pol));
    if (pol.mode < 0 || pol.mode > 2 || pol.period < 1 || pol.period > VT_PROP_MAX_PERIOD || pol.max_n < 1 || pol.max_n > VT_PROP_MAX ||
        pol.min_sim_pm < 0 || pol.min_sim_pm > 1000 || pol.max_cells < VT_PROP_M_MAX * VT_PROP_M_MAX || pol.max_cells > VT_PROP_MAX_CELLS)
        return set_err(VT_ERR_INVALID_ARG, "proposals: policy out of range");
    pol.tau = (float)pol.min_sim_pm / 1000.0f;
    HookFrames fr;
    SlotMaps maps{slot_stream, winner, n, n_streams};
    if (int rc = fr.check(frames, n)) return rc;
    if (int rc = maps.check_all("proposals")) return rc;
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    const ModelDims d = model_dims(T, 0, patch, kpad, norm);
    const size_t ns = (size_t)n, mc = (size_t)pol.max_cells, pm = VT_PROP_M_MAX * VT_PROP_M_MAX;
    const PassOut po{};
    DevArr dst, dres, dpol, dtpl, dcnt, dhead, dpo;
    GuardedOut gpat, gth, gmap, grec;
    HIPCHK(dst.upload(states, (size_t)n_streams * sizeof(StreamState)));
    HIPCHK(dres.upload(results, ns * sizeof(vt_result))); HIPCHK(dpol.upload(&pol, sizeof(pol)));
    HIPCHK(dtpl.upload(tpl, (size_t)n_streams * tpl_bufs * d.nt * kpad * sizeof(bf16_t)));
    HIPCHK(dcnt.upload(evaluated, (size_t)n_streams * 4)); HIPCHK(dhead.zeros(ns * sizeof(PropHead))); HIPCHK(dpo.upload(&po, sizeof(po)));
    HIPCHK(gpat.alloc(ns * pm * sizeof(int16_t))); HIPCHK(gth.alloc(ns * mc * sizeof(int16_t))); HIPCHK(gmap.alloc(ns * mc * sizeof(float)));
    HIPCHK(grec.alloc((size_t)n_streams * sizeof(PropRec)));
    HIPCHK(maps.upload());
    HIPCHK(fr.upload(device_frames));
    const PropArgs pa{fr.dev(), dst.as<const StreamState>(), dres.as<const vt_result>(), maps.dev_slot_stream(),
                      maps.dev_winner(), dpol.as<const PropPolicy>(), fr.dev_flag(), dtpl.as<const bf16_t>(), tpl_bufs,
                      grec.as<PropRec>(), dcnt.as<int32_t>(), dhead.as<PropHead>(), gpat.as<int16_t>(), gth.as<int16_t>(),
                      gmap.as<float>(), dpo.as<const PassOut>(), pol.max_cells, n};
    HIPCHK(launch_proposals_prepare(pa, d, nullptr));
    HIPCHK(launch_proposals_thumb(pa, d, fr.level, nullptr));
    HIPCHK(launch_proposals_match(pa, nullptr));
    HIPCHK(launch_proposals_list(pa, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (int rc = guards_intact("proposals", {{&gpat, "pattern"}, {&gth, "thumbnail"}, {&gmap, "map"}, {&grec, "records"}})) return rc;
    HIPCHK(gpat.download(pattern)); HIPCHK(gth.download(thumb)); HIPCHK(gmap.download(map)); HIPCHK(grec.download(records));
    HIPCHK(dcnt.download(evaluated));
    return VT_OK;
} VT_NOTHROW_INT

// The four launches of the camera motion on given operands: see include/vittrack_hip_ops.h. Nothing runs but
// launch_camera_prepare, _thumb, _search and _decide, in that order. Thumbnails, records and tables each sit between guard
// bands; the tables start as 0xff bytes, the thumbnails and records as the caller's.
int vt_op_camera_motion(int device_id, const vt_frame* frames, void* states, int n_streams, const int32_t* slot_stream, int n,
                        const int32_t* policy, int device_frames, uint16_t* thumbs, void* records, int64_t* sad,
                        void* host_states, void* host_records) try {
    if (!frames || !states || !policy || !thumbs || !records || !sad || n < 1 || n > VT_MAX_STREAMS || n_streams < 1 ||
        n_streams > VT_MAX_STREAMS)
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    static_assert(sizeof(CamPolicy) == 4 * CM_WORDS && kCameraKeys[2].hi == VT_CAM_R_MAX && kCameraKeys[4].lo == VT_CAM_MIN_CELLS &&
                  kCameraKeys[4].hi == VT_CAM_MAX_CELLS, "CamPolicy");
    CamPolicy pol;
    if (int rc = policy_from_words("camera_motion", kCameraKeys, apply_camera_motion, VT_CAM_DEFAULT_POLICY, policy, &pol)) return rc;
    HookFrames fr;
    SlotMaps maps{slot_stream, nullptr, n, n_streams};
    if (int rc = fr.check(frames, n)) return rc;
    if (int rc = maps.check_all("camera_motion")) return rc;
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    const size_t ns = (size_t)n_streams, sb = ns * sizeof(StreamState), rb = ns * sizeof(CamRec);
    const size_t tb = ns * 2 * (size_t)pol.max_cells * sizeof(uint16_t), ab = ns * VT_CAM_TABLE * sizeof(long long);
    DevArr dst, dpol, dhead;
    GuardedOut gth, grec, gsad;
    Mirror hst, hrec;
    HIPCHK(dst.upload(states, sb));
    HIPCHK(dpol.upload(&pol, sizeof(pol))); HIPCHK(dhead.zeros((size_t)n * sizeof(CamHead)));
    HIPCHK(gth.upload(thumbs, tb)); HIPCHK(grec.upload(records, rb)); HIPCHK(gsad.alloc(ab));
    HIPCHK(hst.from(host_states, sb)); HIPCHK(hrec.from(host_records, rb));
    HIPCHK(maps.upload());
    HIPCHK(fr.upload(device_frames));
    const CamArgs ca{fr.dev(), dst.as<StreamState>(), maps.dev_slot_stream(), dpol.as<const CamPolicy>(),
                     fr.dev_flag(), grec.as<CamRec>(), dhead.as<CamHead>(), gsad.as<unsigned long long>(),
                     gth.as<uint16_t>(), hst.as<StreamState>(), hrec.as<CamRec>(), pol.max_cells, n};
    HIPCHK(launch_camera_prepare(ca, nullptr));
    HIPCHK(launch_camera_thumb(ca, fr.level, nullptr));
    HIPCHK(launch_camera_search(ca, nullptr));
    HIPCHK(launch_camera_decide(ca, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (int rc = guards_intact("camera_motion", {{&gth, "thumbnails"}, {&grec, "records"}, {&gsad, "tables"}})) return rc;
    HIPCHK(gth.download(thumbs)); HIPCHK(grec.download(records)); HIPCHK(gsad.download(sad)); HIPCHK(dst.download(states));
    hst.back(); hrec.back();
    return VT_OK;
} VT_NOTHROW_INT

// The four launches of the peak arbitration on given operands: see include/vittrack_hip_ops.h. Nothing runs but
// launch_arbitrate_list, _probe, _score and _commit, in that order. Every array a launch may write sits between guard bands;
// records, probe rows and partials start as 0xff bytes, the tickets as zeros, the others as the caller's.
int vt_op_arbitrate(int device_id, const float* head_out, const float* hann, const vt_frame* frames, void* states, int n_streams,
                    vt_result* results, const int32_t* slot_stream, const int32_t* winner, int n, int grid, const uint16_t* anchor,
                    int T, int S, int patch, int kpad, const float* norm, float success_threshold, const int32_t* policy, int tier,
                    void* records, int32_t* counts, uint16_t* probe, vt_result* host_results, void* host_states,
                    void* host_records) try {
    if (!head_out || !hann || !frames || !states || !results || !anchor || !norm || !policy || !records || !counts || !probe || n < 1 ||
        n > VT_MAX_STREAMS || n_streams < 1 || n_streams > VT_MAX_STREAMS || grid < 1 || grid > 110 || patch < 1 || T < patch ||
        T % patch != 0 || S < T || kpad < 3 * patch * patch || kpad > 65536 || tier < 0 || tier > 2)
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    static_assert(sizeof(ArbPolicy) == 4 * AR_WORDS && kArbKeys[1].hi == VT_ARB_MAX, "ArbPolicy");
    ArbPolicy pol;
    if (int rc = policy_from_words("arbitrate", kArbKeys, apply_arbitrate, VT_ARB_DEFAULT_POLICY, policy, &pol)) return rc;
    HookFrames fr;
    SlotMaps maps{slot_stream, winner, n, n_streams};
    if (int rc = fr.check(frames, n)) return rc;
    if (int rc = maps.check_all("arbitrate")) return rc;
    // outside a candidate pass a stream has ONE slot (every pass of the engine is built so)
    if (int rc = maps.check_unique("arbitrate", "is named by two slots")) return rc;
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    const ModelDims d = model_dims(T, S, patch, kpad, norm);
    const int ns = grid * grid, cols = 3 * patch * patch;
    const size_t nn = (size_t)n, nst = (size_t)n_streams, rows = (size_t)d.nt * kpad * sizeof(bf16_t);
    const size_t sb = nst * sizeof(StreamState), rb = nst * sizeof(ArbRec), resb = nn * sizeof(vt_result);
    const size_t pairs = nn * VT_ARB_MAX, nch = (size_t)appear_chunks(d.nt);
    DevArr dho, dhann, dpol, danchor, dpo;
    GuardedOut gst, gres, grec, gcnt, gprobe, gtick, gpart;
    Mirror hres, hst, hrec;
    HIPCHK(dho.upload(head_out, nn * ns * 8 * 4)); HIPCHK(dhann.upload(hann, (size_t)ns * 4));
    HIPCHK(dpol.upload(&pol, sizeof(pol)));
    HIPCHK(danchor.upload(anchor, nst * rows));
    HIPCHK(gst.upload(states, sb)); HIPCHK(gres.upload(results, resb)); HIPCHK(grec.alloc(rb));
    HIPCHK(gcnt.upload(counts, nst * sizeof(ArbCount))); HIPCHK(gprobe.alloc(nst * VT_ARB_MAX * rows));
    HIPCHK(gtick.alloc(pairs * sizeof(unsigned), 0));
    HIPCHK(gpart.alloc(pairs * nch * 5 * sizeof(double)));      // NaN: a partial nobody wrote would show
    HIPCHK(hres.from(host_results, resb)); HIPCHK(hst.from(host_states, sb)); HIPCHK(hrec.from(host_records, rb));
    const PassOut po{hres.as<vt_result>(), hst.as<StreamState>()};
    HIPCHK(dpo.upload(&po, sizeof(po)));
    HIPCHK(maps.upload());
    HIPCHK(fr.upload());
    ArbArgs a{};
    a.head_out = dho.as<const float>(); a.hann = dhann.as<const float>(); a.frames = fr.dev();
    a.states = gst.as<StreamState>(); a.results = gres.as<vt_result>(); a.slot_stream = maps.dev_slot_stream();
    a.winner = maps.dev_winner(); a.policy = dpol.as<const ArbPolicy>(); a.recs = grec.as<ArbRec>(); a.counts = gcnt.as<ArbCount>();
    a.tickets = gtick.as<unsigned>(); a.partials = gpart.as<double>(); a.anchor = danchor.as<const bf16_t>();
    a.probe = gprobe.as<bf16_t>(); a.out = dpo.as<const PassOut>(); a.host_recs = hrec.as<ArbRec>();
    a.n = n; a.ns = ns; a.grid = grid; a.success_threshold = success_threshold;
    HIPCHK(launch_arbitrate_list(a, d, nullptr));
    HIPCHK(launch_arbitrate_probe(a, d, tier, fr.level, nullptr));
    HIPCHK(launch_arbitrate_score(a, d.nt, cols, kpad, nullptr));
    HIPCHK(launch_arbitrate_commit(a, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (int rc = guards_intact("arbitrate", {{&gst, "states"}, {&gres, "results"}, {&grec, "records"}, {&gcnt, "counters"},
                                             {&gprobe, "probe rows"}, {&gtick, "tickets"}, {&gpart, "partials"}})) return rc;
    if (int rc = tickets_returned("arbitrate", gtick, VT_ARB_MAX)) return rc;
    HIPCHK(gst.download(states)); HIPCHK(gres.download(results)); HIPCHK(grec.download(records)); HIPCHK(gcnt.download(counts));
    HIPCHK(gprobe.download(probe));
    hres.back(); hst.back(); hrec.back();
    return VT_OK;
} VT_NOTHROW_INT

// The four launches of the frame health on given operands: see include/vittrack_hip_ops.h. Nothing runs but
// launch_health_prepare, _thumb, _measure and _decide, in that order. Every array the launches may write sits between guard
// bands; headers and accumulators start as 0xff bytes, the others as the caller's.
int vt_op_frame_health(int device_id, const vt_frame* frames, void* states, int n_streams, const int32_t* slot_stream, int n,
                       const int32_t* policy, int device_frames, uint16_t* thumbs, int64_t* accs, int32_t* hist, void* heads,
                       void* records, void* counts, void* host_records) try {
    if (!frames || !states || !policy || !thumbs || !accs || !hist || !heads || !records || !counts || n < 1 || n > VT_MAX_STREAMS ||
        n_streams < 1 || n_streams > VT_MAX_STREAMS)
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    static_assert(sizeof(HealthPolicy) == 4 * HL_WORDS, "HealthPolicy");
    HealthPolicy pol;
    if (int rc = policy_from_words("frame_health", kHealthKeys, apply_health, VT_HEALTH_DEFAULT_POLICY, policy, &pol)) return rc;
    HookFrames fr;
    SlotMaps maps{slot_stream, nullptr, n, n_streams};
    if (int rc = fr.check(frames, n)) return rc;
    if (int rc = maps.check_all("frame_health")) return rc;
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    const size_t ns = (size_t)n_streams, sb = ns * sizeof(StreamState), rb = ns * sizeof(HealthRec), cb = ns * sizeof(HealthCount);
    const size_t tb = ns * 2 * (size_t)pol.max_cells * sizeof(uint16_t), ab = ns * HEALTH_ACCS * sizeof(long long);
    const size_t hb = ns * 2 * VT_HEALTH_BINS * sizeof(int32_t), hdb = (size_t)n * sizeof(HealthHead);
    DevArr dpol, dpo;
    GuardedOut gst, gth, gacc, ghist, ghead, grec, gcnt;
    Mirror hrec;
    HIPCHK(dpol.upload(&pol, sizeof(pol)));
    HIPCHK(gst.upload(states, sb)); HIPCHK(gth.upload(thumbs, tb)); HIPCHK(ghist.upload(hist, hb)); HIPCHK(grec.upload(records, rb));
    HIPCHK(gcnt.upload(counts, cb)); HIPCHK(gacc.alloc(ab)); HIPCHK(ghead.alloc(hdb));
    HIPCHK(hrec.from(host_records, rb));
    PassOut po{};
    po.host_health = hrec.as<HealthRec>();
    HIPCHK(dpo.upload(&po, sizeof(po)));
    HIPCHK(maps.upload());
    HIPCHK(fr.upload(device_frames));
    const HealthArgs ha{fr.dev(), gst.as<const StreamState>(), maps.dev_slot_stream(), dpol.as<const HealthPolicy>(),
                        fr.dev_flag(), grec.as<HealthRec>(), gcnt.as<HealthCount>(), ghead.as<HealthHead>(),
                        gacc.as<unsigned long long>(), ghist.as<int32_t>(), gth.as<uint16_t>(), dpo.as<const PassOut>(), pol.max_cells, n};
    HIPCHK(launch_health_prepare(ha, nullptr));
    HIPCHK(launch_health_thumb(ha, fr.level, nullptr));
    HIPCHK(launch_health_measure(ha, nullptr));
    HIPCHK(launch_health_decide(ha, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (int rc = guards_intact("frame_health", {{&gst, "states"}, {&gth, "thumbnails"}, {&gacc, "accumulators"}, {&ghist, "histograms"},
                                                {&ghead, "headers"}, {&grec, "records"}, {&gcnt, "counters"}})) return rc;
    HIPCHK(gst.download(states)); HIPCHK(gth.download(thumbs)); HIPCHK(gacc.download(accs)); HIPCHK(ghist.download(hist));
    HIPCHK(ghead.download(heads)); HIPCHK(grec.download(records)); HIPCHK(gcnt.download(counts));
    hrec.back();
    return VT_OK;
} VT_NOTHROW_INT

// The launches of the moving regions on given operands: see include/vittrack_hip_ops.h. Nothing runs but
// launch_movers_prepare, _thumb, _label and _list, in that order. Every array the launches may write sits between guard
// bands; headers, accumulators, labels, extents and thumbnails start as 0xff bytes, the others as the caller's.
int vt_op_movers(int device_id, const vt_frame* frames, void* states, int n_streams, const int32_t* slot_stream, int n,
                 const int32_t* policy, int device_frames, uint16_t* bg, uint16_t* thumbs, uint8_t* mask, int32_t* labels, int32_t* exts,
                 int32_t* accs, void* heads, void* records, void* counts, void* host_records) try {
    if (!frames || !states || !policy || !bg || !thumbs || !mask || !labels || !exts || !accs || !heads || !records || !counts || n < 1 ||
        n > VT_MAX_STREAMS || n_streams < 1 || n_streams > VT_MAX_STREAMS)
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    static_assert(sizeof(MoverPolicy) == 4 * MV_WORDS, "MoverPolicy");
    MoverPolicy pol;
    if (int rc = policy_from_words("movers", kMoverKeys, apply_movers, VT_MOVER_DEFAULT_POLICY, policy, &pol)) return rc;
    HookFrames fr;
    SlotMaps maps{slot_stream, nullptr, n, n_streams};
    if (int rc = fr.check(frames, n)) return rc;
    if (int rc = maps.check_all("movers")) return rc;
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    const size_t ns = (size_t)n_streams, sb = ns * sizeof(StreamState), rb = ns * sizeof(MoverRec), cb = ns * sizeof(MoverCount);
    const size_t cells = ns * (size_t)pol.max_cells, ab = ns * MOVER_ACCS * sizeof(int32_t), hdb = (size_t)n * sizeof(MoverHead);
    DevArr dpol;
    GuardedOut gst, gbg, gth, gmask, glab, gext, gacc, ghead, grec, gcnt;
    Mirror hrec;
    HIPCHK(dpol.upload(&pol, sizeof(pol)));
    HIPCHK(gst.upload(states, sb)); HIPCHK(gbg.upload(bg, cells * 2)); HIPCHK(gmask.upload(mask, cells)); HIPCHK(grec.upload(records, rb));
    HIPCHK(gcnt.upload(counts, cb)); HIPCHK(gth.alloc(cells * 2)); HIPCHK(glab.alloc(cells * 4)); HIPCHK(gext.alloc(cells * 4 * MOVER_EXTS));
    HIPCHK(gacc.alloc(ab)); HIPCHK(ghead.alloc(hdb));
    HIPCHK(hrec.from(host_records, rb));
    HIPCHK(maps.upload());
    HIPCHK(fr.upload(device_frames));
    const MoverArgs va{fr.dev(), gst.as<const StreamState>(), maps.dev_slot_stream(), dpol.as<const MoverPolicy>(), fr.dev_flag(),
                       grec.as<MoverRec>(), gcnt.as<MoverCount>(), ghead.as<MoverHead>(), gacc.as<int32_t>(), glab.as<int32_t>(),
                       gext.as<int32_t>(), gbg.as<uint16_t>(), gth.as<uint16_t>(), gmask.as<uint8_t>(), hrec.as<MoverRec>(),
                       pol.max_cells, n};
    HIPCHK(launch_movers_prepare(va, nullptr));
    HIPCHK(launch_movers_thumb(va, fr.level, nullptr));
    HIPCHK(launch_movers_label(va, nullptr));
    HIPCHK(launch_movers_list(va, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (int rc = guards_intact("movers", {{&gst, "states"}, {&gbg, "backgrounds"}, {&gth, "thumbnails"}, {&gmask, "mask"}, {&glab, "labels"},
                                          {&gext, "extents"}, {&gacc, "accumulators"}, {&ghead, "headers"}, {&grec, "records"},
                                          {&gcnt, "counters"}})) return rc;
    HIPCHK(gst.download(states)); HIPCHK(gbg.download(bg)); HIPCHK(gth.download(thumbs)); HIPCHK(gmask.download(mask));
    HIPCHK(glab.download(labels)); HIPCHK(gext.download(exts)); HIPCHK(gacc.download(accs)); HIPCHK(ghead.download(heads));
    HIPCHK(grec.download(records)); HIPCHK(gcnt.download(counts));
    hrec.back();
    return VT_OK;
} VT_NOTHROW_INT

// The one launch of the stream conflicts on given operands: see include/vittrack_hip_ops.h. Nothing runs but
// launch_conflicts_check. Records and counters sit between guard bands and start as the caller's bytes.
int vt_op_stream_conflicts(int device_id, const void* states, int n_streams, const vt_result* results, const int32_t* slot_stream,
                           const int32_t* winner, int n, const int32_t* scenes, const int32_t* policy, void* records, void* counts,
                           void* host_records) try {
    if (!states || !results || !scenes || !policy || !records || !counts || n < 1 || n > VT_MAX_STREAMS || n_streams < 1 ||
        n_streams > VT_MAX_STREAMS)
        return set_err(VT_ERR_INVALID_ARG, "bad argument");
    static_assert(sizeof(ConflictPolicy) == 4 * CF_WORDS, "ConflictPolicy");
    ConflictPolicy pol;         // tau is the table's
    if (int rc = policy_from_words("stream_conflicts", kConflictKeys, apply_conflicts, VT_CONFLICT_DEFAULT_POLICY, policy, &pol)) return rc;
    SlotMaps maps{slot_stream, winner, n, n_streams};
    if (int rc = maps.check_all("stream_conflicts")) return rc;
    for (int s = 0; s < n_streams; ++s)
        if (scenes[s] < 0 || scenes[s] > VT_CONFLICT_MAX_SCENE)
            return set_err(VT_ERR_INVALID_ARG, "stream_conflicts: scene %d of stream %d (0..%d)", (int)scenes[s], s, VT_CONFLICT_MAX_SCENE);
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    const size_t ns = (size_t)n_streams, rb = ns * sizeof(ConflictRec), cb = ns * sizeof(ConflictCount);
    DevArr dst, dres, dsc, dpol, dpo;
    GuardedOut grec, gcnt;
    Mirror hrec;
    HIPCHK(dst.upload(states, ns * sizeof(StreamState))); HIPCHK(dres.upload(results, (size_t)n * sizeof(vt_result)));
    HIPCHK(dsc.upload(scenes, ns * 4)); HIPCHK(dpol.upload(&pol, sizeof(pol)));
    HIPCHK(grec.upload(records, rb)); HIPCHK(gcnt.upload(counts, cb));
    HIPCHK(hrec.from(host_records, rb));
    PassOut po{};
    po.host_conflicts = hrec.as<ConflictRec>();
    HIPCHK(dpo.upload(&po, sizeof(po)));
    HIPCHK(maps.upload());
    const ConflictArgs ca{dst.as<const StreamState>(), dres.as<const vt_result>(), maps.dev_slot_stream(), maps.dev_winner(),
                          dpol.as<const ConflictPolicy>(), dsc.as<const int32_t>(), grec.as<ConflictRec>(), gcnt.as<ConflictCount>(),
                          dpo.as<const PassOut>(), n};
    HIPCHK(launch_conflicts_check(ca, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (int rc = guards_intact("stream_conflicts", {{&grec, "records"}, {&gcnt, "counters"}})) return rc;
    HIPCHK(grec.download(records)); HIPCHK(gcnt.download(counts));
    hrec.back();
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
        if (!lo_shift_ok(lo_shift)) return set_err(VT_ERR_INVALID_ARG, "ln chain: lo_shift %d out of range", lo_shift);
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
    DevArr dw, dg, dbeta, dbias;
    GuardedOut gwf, gcs, gcv;
    HIPCHK(dw.upload(w, WN * 2)); HIPCHK(dg.upload(gamma, (size_t)D * 4)); HIPCHK(dbeta.upload(beta, (size_t)D * 4));
    HIPCHK(dbias.upload(bias, (size_t)N * 4));
    HIPCHK(gwf.alloc(WN * 2)); HIPCHK(gcs.alloc((size_t)N * 4)); HIPCHK(gcv.alloc((size_t)N * 4));
    auto fold = [&] {
        return launch_fold_layernorm(dw.as<const bf16_t>(), dg.as<const float>(), dbeta.as<const float>(), dbias.as<const float>(),
                                     gwf.as<bf16_t>(), gcs.as<float>(), gcv.as<float>(), N, D, nullptr);
    };
    auto fold_back = [&]() -> int {
        if (wf_out) HIPCHK(gwf.download(wf_out));
        if (colsum_out) HIPCHK(gcs.download(colsum_out));
        if (cvec_out) HIPCHK(gcv.download(cvec_out));
        return VT_OK;
    };
    if (fold_only) {
        for (int rep = 0; rep < launches; ++rep) HIPCHK(fold());
        HIPCHK(hipDeviceSynchronize());
        if (int rc = guards_intact("ln chain", {{&gwf, "folded weights"}, {&gcs, "column sums"}, {&gcv, "constant vector"}})) return rc;
        return fold_back();
    }
    HIPCHK(gemm_prepare());
    const int M = (int)Mll, nchunk = D / VT_STAT_CHUNK, H = D / 64, npad = ca.npad;
    const size_t MD = (size_t)M * D, n_out = epi == EPI_QKV ? (size_t)M * 2 * D : (size_t)M * N,
                 n_vt = epi == EPI_QKV ? (size_t)B * H * 64 * npad : 0, n_cnt = (size_t)(M + 255) / 256 + 1;
    DevArr dza, dzw, dzb, dpos, dcnt;
    GuardedOut gxh, gxl, gcst, grs, gout, gvt;
    HIPCHK(dza.zeros((size_t)M * 128 * 2)); HIPCHK(dzw.zeros((size_t)D * 128 * 2)); HIPCHK(dzb.zeros((size_t)D * 4));
    HIPCHK(dcnt.zeros(n_cnt * 4)); HIPCHK(dpos.upload(x, MD * 4));
    HIPCHK(gxh.alloc(MD * 2)); HIPCHK(gxl.alloc(MD)); HIPCHK(gcst.alloc((size_t)M * nchunk * 8)); HIPCHK(grs.alloc((size_t)M * 8));
    HIPCHK(gout.alloc(n_out * 2));
    if (n_vt) HIPCHK(gvt.alloc(n_vt * 2));
    // producer: (0 + 0) + pos = x exactly, through the X-epilogue's statistics and split
    pa.A = dza.as<const bf16_t>(); pa.W = dzw.as<const bf16_t>(); pa.bias = dzb.as<const float>();
    pa.pos = dpos.as<const float>(); pa.Xh = gxh.as<bf16_t>(); pa.Xl = gxl.as<uint8_t>();
    pa.cstat = gcst.as<float2>(); pa.ln_eps = eps; pa.lq = lo_quant(lo_shift);
    pa.tile_order = split_cfg(pcfg).order; pcfg = split_cfg(pcfg).cfg;
    if (route == 1) { pa.rowstat_out = grs.as<float2>(); pa.panel_cnt = dcnt.as<unsigned>(); }
    if (pcfg < 0) pcfg = gemm_effective_config(pa, EPI_F32_POS);
    if (route == 1 && !(pcfg >= GEMM_CFG_256_MIN && gemm256_fits(pa, EPI_F32_POS)))
        return set_err(VT_ERR_INVALID_ARG, "ln chain: route 1 takes a 256x256 producer (configuration %d chosen)", pcfg);
    // consumer: A = the hi half, W = the folded weights, bias = cvec, row terms by route
    ca.A = gxh.as<const bf16_t>(); ca.W = gwf.as<const bf16_t>(); ca.bias = gcv.as<const float>();
    ca.colsum = gcs.as<const float>(); ca.ln_eps = eps;
    if (epi == EPI_QKV) { ca.qk = gout.as<bf16_t>(); ca.vt = gvt.as<bf16_t>(); }
    else ca.Cb = gout.as<bf16_t>();
    ca.tile_order = split_cfg(ccfg).order; ccfg = split_cfg(ccfg).cfg;
    if (route == 2) ca.cstat_in = gcst.as<const float2>();
    else ca.rowstat = grs.as<const float2>();        // the pair load of the last even row ends in the guard band
    if (ccfg < 0) ccfg = gemm_effective_config(ca, epi);
    if (route == 2 && ccfg > GEMM_CFG_SMALL_MAX)
        return set_err(VT_ERR_INVALID_ARG, "ln chain: route 2 takes a 4-wave consumer (configuration %d chosen)", ccfg);
    for (int rep = 0; rep < launches; ++rep) {
        if (launch_gemm_cfg(pa, EPI_F32_POS, pcfg, nullptr) != hipSuccess)
            return set_err(VT_ERR_INVALID_ARG, "ln chain: producer configuration %d does not fit M=%d D=%d", pcfg, M, D);
        if (route == 0) HIPCHK(launch_rowstat_finalize(pa.cstat, grs.as<float2>(), M, nchunk, eps, nullptr));
        HIPCHK(fold());
        if (launch_gemm_cfg(ca, epi, ccfg, nullptr) != hipSuccess)
            return set_err(VT_ERR_INVALID_ARG, "ln chain: consumer configuration %d does not fit M=%d N=%d D=%d", ccfg, M, N, D);
    }
    HIPCHK(hipDeviceSynchronize());
    if (int rc = guards_intact("ln chain", {{&gxh, "hi half"}, {&gxl, "lo8 half"}, {&gcst, "chunk partials"}, {&grs, "row terms"},
                                            {&gout, "output"}, {&gvt, "Vt"}, {&gwf, "folded weights"}, {&gcs, "column sums"},
                                            {&gcv, "constant vector"}})) return rc;
    std::vector<unsigned> cnt(n_cnt);
    HIPCHK(dcnt.download(cnt.data()));
    for (size_t i = 0; i < n_cnt; ++i)
        if (cnt[i]) return set_err(VT_ERR_HIP, "ln chain: panel counter %zu is %u after %d launches", i, cnt[i], launches);
    HIPCHK(download_bf16(gout.out(), n_out, out));
    if (n_vt) HIPCHK(download_bf16(gvt.out(), n_vt, vt_out));
    if (xh_out) HIPCHK(gxh.download(xh_out));
    if (xl_out) HIPCHK(gxl.download(xl_out));
    if (cstat_out) HIPCHK(gcst.download(cstat_out));
    if (rowstat_out) HIPCHK(grs.download(rowstat_out));
    return fold_back();
} VT_NOTHROW_INT

}  // extern "C"
