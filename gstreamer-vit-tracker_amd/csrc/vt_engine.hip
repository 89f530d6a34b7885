// vt_engine.hip — host side of libvittrack_hip.so: weight blob, per-GPU buffers, the per-frame
// launch plan (eager or one hipGraph replay) and the one path that builds and submits a pass. The
// extern "C" ABI of include/vittrack_hip.h is in vt_abi.hip and vt_ingest.hip.
//
// One Engine = B independent tracked streams on one GPU. Everything a frame needs stays in HBM:
// the decode kernel of frame t writes the box that the preprocessing kernel of frame t+1 reads, so
// a stream of updates is a pure device-side chain; the host only supplies frame pointers and
// collects 24 B of result per stream.
#include "vt_engine.hpp"

static thread_local char g_err[512] = "";
char* vt_err_text() { return g_err; }
int set_err(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

thread_local LaunchProbe* vt_launch_probe = nullptr;

// kernel-family label of a GEMM launch (built only when a profiler is attached): the tile configuration
// in it is the one launch_gemm() really runs for these arguments
static const char* gemm_name(int epi, const GemmArgs& a) {
    static const char* tags[] = {"xpos", "xresid", "gelu", "relu", "qkv", "x"};
    static thread_local char buf[96];
    snprintf(buf, sizeof(buf), "gemm_bf16_%s_%s_n%dk%d", tags[epi], gemm_config_name(gemm_effective_config(a, epi)), a.N, a.K);
    return buf;
}


void Engine::destroy() {
    if (!stream && !d_blob) return;
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    drop_graphs();
    void* devp[] = {d_blob, d_patches, d_tpl, d_qk, d_vt, d_attn, d_mlp, d_feat, d_ta, d_tb, d_zeros,
                    d_xh, d_xl, d_cstat, d_rstat, d_panel_cnt, d_band_cnt, d_band_best, d_foldw, d_foldv, d_headout, d_taps, d_states, d_frames,
                    d_results, d_cand_states, d_cands, d_winner, d_xrange, d_policy, d_tickets, d_chips, d_chip_policy, d_peaks};     // d_chip_infos: part of d_chips, d_peaks_policy: of d_peaks
    for (void* p : devp)
        if (p) (void)hipFree(p);
    for (const KeyedFeature& f : keyed_features())      // the keyed features' stores: from their list
        if (this->*f.store) (void)hipFree(this->*f.store);
    if (h_chip_stage) (void)hipHostFree(h_chip_stage);
    if (h_cands) (void)hipHostFree(h_cands);
    if (h_winner) (void)hipHostFree(h_winner);
    if (h_frames) (void)hipHostFree(h_frames);
    if (h_state) (void)hipHostFree(h_state);
    stage.release();
    PassOut own = pass_sinks(nullptr, true);     // a mirror of a feature the engine is not capable of: null
    sinks_free(&own, SINK_ALL);
    for (HostSlot& sl : hs) {
        sl.arena.release();
        sinks_free(&sl.out, SINK_ALL);
        if (sl.up_ev) (void)hipEventDestroy(sl.up_ev);
        if (sl.done_ev) (void)hipEventDestroy(sl.done_ev);
        sl = HostSlot();
    }
    for (QueuedInit* q : qinits) {
        if (!q) continue;
        q->arena.release();
        if (q->h_state) (void)hipHostFree(q->h_state);
        if (q->h_desc) (void)hipHostFree(q->h_desc);
        if (q->up_ev) (void)hipEventDestroy(q->up_ev);
        if (q->done_ev) (void)hipEventDestroy(q->done_ev);
        delete q;
    }
    qinits.clear();
    for (SnapStage* sg : snaps) {
        if (!sg) continue;
        if (sg->d) (void)hipFree(sg->d);
        if (sg->h) (void)hipHostFree(sg->h);
        if (sg->up_ev) (void)hipEventDestroy(sg->up_ev);
        if (sg->done_ev) (void)hipEventDestroy(sg->done_ev);
        delete sg;
    }
    snaps.clear();
    if (copy_stream) { (void)hipStreamSynchronize(copy_stream); (void)hipStreamDestroy(copy_stream); copy_stream = nullptr; }
    for (int i = 0; i < RING; ++i)
        if (ring_ev[i]) (void)hipEventDestroy(ring_ev[i]);
    if (stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
    d_blob = nullptr;
}

void Engine::drop_graphs() {
    for (auto& set : graphs)
        for (PassGraph& g : set) {
            if (g.exec) (void)hipGraphExecDestroy(g.exec);
            if (g.graph) (void)hipGraphDestroy(g.graph);
            g = PassGraph();
        }
}

// The crop kernel's buffer tier for the pass about to be enqueued: the largest any stream's last known box needs (the
// boxes of a pipelined pass are one pass old: targets change by a few per cent per frame, the tier has headroom, and a
// tile that does not fit its buffer after all takes the per-pixel path - slower, never wrong).
// A subset pass considers the boxes of its own streams only.
int Engine::pick_crop_tier(const int32_t* streams, int n) const {
    if (crop_tier_forced >= 0) return std::min(crop_tier_forced, TIERS - 1);
    int t = 0;
    const int cnt = streams ? n : B;
    for (int i = 0; i < cnt && t < TIERS - 1; ++i) {
        const StreamState& k = known[streams ? streams[i] : i];
        t = std::max(t, std::min(preproc_tier_for_box(d, k.box[2], k.box[3], false), TIERS - 1));
    }
    return t;
}

// A candidate pass looks at its slots' own boxes: a slot without one works on its stream's known box.
int Engine::pick_crop_tier(const vt_candidate* cands, int n) const {
    if (crop_tier_forced >= 0) return std::min(crop_tier_forced, TIERS - 1);
    int t = 0;
    for (int i = 0; i < n && t < TIERS - 1; ++i) {
        const float* box = cands[i].has_box ? cands[i].box : known[(size_t)cands[i].stream].box;
        t = std::max(t, std::min(preproc_tier_for_box(d, box[2], box[3], false), TIERS - 1));
    }
    return t;
}

int Engine::slot_of(int stream) const {
    if (pass_streams.empty()) return stream < pass_n ? stream : -1;
    for (size_t i = 0; i < pass_streams.size(); ++i)
        if (pass_streams[i] == stream) return i < pass_winner.size() ? (int)pass_winner[i] : (int)i;
    return -1;
}

int Engine::index_blob(const uint8_t* hc, size_t bytes) {
    if (bytes < kHeaderBytes || memcmp(hc, kMagic, 8) != 0)
        return set_err(VT_ERR_FORMAT, "weight blob: bad magic or truncated header");
    int32_t ints[20];
    float fl[8];
    memcpy(ints, hc + 8, sizeof(ints));
    memcpy(fl, hc + 8 + 80, sizeof(fl));
    if (ints[0] != 1) return set_err(VT_ERR_FORMAT, "weight blob: unsupported version %d", ints[0]);
    d.patch = ints[1]; d.T = ints[2]; d.S = ints[3]; d.D = ints[4]; d.H = ints[5]; d.L = ints[6];
    d.mlp = ints[7]; d.C = ints[8]; d.kpad = ints[9];
    const int n_tensors = ints[10];
    for (int i = 0; i < 3; ++i) { d.norm_a[i] = fl[i]; d.norm_b[i] = fl[3 + i]; }
    d.success_threshold = fl[6];
    d.ln_eps = fl[7];
    // header int 12: the shift of the residual pair's quantum (k_gemm.hpp, specification v3). 0: the default
    if (ints[12] != 0 && (ints[12] < VT_LO_SHIFT_MIN || ints[12] > VT_LO_SHIFT_MAX))
        return set_err(VT_ERR_FORMAT, "weight blob: lo_shift %d out of range (0 = %d, or %d..%d)", ints[12],
                       VT_LO_SHIFT_DEFAULT, VT_LO_SHIFT_MIN, VT_LO_SHIFT_MAX);
    lq = lo_quant(ints[12] ? ints[12] : VT_LO_SHIFT_DEFAULT);
    // every dimension is bounded BEFORE anything is derived from it (a corrupt or crafted blob must
    // not overflow the int arithmetic below or make layers.resize() throw)
    if (d.patch < 2 || d.patch > 64 || d.T < d.patch || d.S < d.patch || d.T > 4096 || d.S > 4096 ||
        d.T % d.patch || d.S % d.patch)
        return set_err(VT_ERR_FORMAT, "weight blob: patch %d / template %d / search %d out of range or "
                       "not multiples of the patch", d.patch, d.T, d.S);
    if (d.L < 1 || d.L > 64 || d.D < 128 || d.D > 1536 || d.mlp < 64 || d.mlp > 16384 || d.C < 64 ||
        d.C > 1024 || d.kpad < 64 || d.kpad > 16384)
        return set_err(VT_ERR_FORMAT, "weight blob: model dimensions out of range (layers=%d D=%d "
                       "mlp=%d C=%d kpad=%d)", d.L, d.D, d.mlp, d.C, d.kpad);
    d.gt = d.T / d.patch; d.gs = d.S / d.patch;
    d.nt = d.gt * d.gt; d.ns = d.gs * d.gs; d.ntok = d.nt + d.ns;
    d.npad = (d.ntok + 63) / 64 * 64;
    if (d.ntok > 16384)
        return set_err(VT_ERR_FORMAT, "weight blob: %d tokens per frame (limit 16384)", d.ntok);
    {   // widths the LayerNorm kernels are instantiated for (k_misc.hip launch_layernorm)
        const int q = d.D / 128;
        const bool ln_ok = d.D % 128 == 0 && (q <= 4 || q == 6 || q == 8 || q == 10 || q == 12);
        if (!ln_ok)
            return set_err(VT_ERR_FORMAT, "weight blob: embedding width D=%d is not supported (LayerNorm "
                           "kernels exist for D in {128, 256, 384, 512, 768, 1024, 1280, 1536})", d.D);
    }
    if (d.H != d.D / 64 || d.mlp % 64 || d.C % 64 || d.kpad % 64 ||
        d.kpad < 3 * d.patch * d.patch || (d.ntok & 3) || (d.ns & 3))
        return set_err(VT_ERR_FORMAT, "weight blob: unsupported model shape (D=%d H=%d mlp=%d C=%d "
                       "kpad=%d tokens=%d)", d.D, d.H, d.mlp, d.C, d.kpad, d.ntok);
    if (n_tensors <= 0 || n_tensors > 4096 || kHeaderBytes + (size_t)n_tensors * kEntryBytes > bytes)
        return set_err(VT_ERR_FORMAT, "weight blob: tensor table out of range");
    const uint64_t table_end = kHeaderBytes + (uint64_t)n_tensors * kEntryBytes;
    tens.clear();
    for (int i = 0; i < n_tensors; ++i) {
        BlobEntry e;
        memcpy(&e, hc + kHeaderBytes + (size_t)i * kEntryBytes, sizeof(e));
        e.name[31] = 0;
        const uint64_t esz = e.dtype == 1 ? 2 : 4;
        // offset/nbytes checked without forming offset + nbytes (which wraps for offset near 2^64);
        // data may not overlap the header or the table
        if (e.dtype > 1 || e.offset % 16 || e.offset < table_end || e.offset > bytes ||
            e.nbytes > bytes - e.offset || e.rows == 0 || e.cols == 0 || e.rows > (1u << 20) ||
            e.cols > (1u << 20) || e.nbytes != (uint64_t)e.rows * e.cols * esz)
            return set_err(VT_ERR_FORMAT, "weight blob: tensor '%s' malformed", e.name);
        TensorRef r;
        r.ptr = d_blob + e.offset;
        r.dtype = e.dtype; r.rows = e.rows; r.cols = e.cols;
        tens[e.name] = r;
    }
    auto need = [&](const std::string& n, uint32_t dt, uint32_t rows, uint32_t cols) -> const void* {
        const TensorRef* t = find(n);
        if (!t || t->dtype != dt || t->rows != rows || t->cols != cols) {
            set_err(VT_ERR_FORMAT, "weight blob: tensor '%s' missing or wrong shape", n.c_str());
            return nullptr;
        }
        return t->ptr;
    };
    const uint32_t D = d.D, C = d.C;
    if (!need("patch_w", 1, D, d.kpad) || !need("patch_b", 0, 1, D) || !need("pos", 0, d.ntok, D) ||
        !need("norm_g", 0, 1, D) || !need("norm_b", 0, 1, D) || !need("head.w0", 1, C, D) ||
        !need("head.b0", 0, 1, C) || !need("head.w1", 1, C, 9 * C) || !need("head.b1", 0, 1, C) ||
        !need("head.w2", 1, C, 9 * C) || !need("head.b2", 0, 1, C) ||
        !need("head.w3", 1, C, 9 * C) || !need("head.b3", 0, 1, C) || !need("head.w4", 0, 8, C) ||
        !need("head.b4", 0, 1, 8) || !need("hann", 0, 1, d.ns))
        return VT_ERR_FORMAT;
    layers.resize(d.L);
    for (int l = 0; l < d.L; ++l) {
        const std::string p = "l" + std::to_string(l) + ".";
        LayerW& w = layers[l];
        w.ln1_g = (const float*)need(p + "ln1_g", 0, 1, D);
        w.ln1_b = (const float*)need(p + "ln1_b", 0, 1, D);
        w.qkv_w = (const bf16_t*)need(p + "qkv_w", 1, 3 * D, D);
        w.qkv_b = (const float*)need(p + "qkv_b", 0, 1, 3 * D);
        w.proj_w = (const bf16_t*)need(p + "proj_w", 1, D, D);
        w.proj_b = (const float*)need(p + "proj_b", 0, 1, D);
        w.ln2_g = (const float*)need(p + "ln2_g", 0, 1, D);
        w.ln2_b = (const float*)need(p + "ln2_b", 0, 1, D);
        w.fc1_w = (const bf16_t*)need(p + "fc1_w", 1, d.mlp, D);
        w.fc1_b = (const float*)need(p + "fc1_b", 0, 1, d.mlp);
        w.fc2_w = (const bf16_t*)need(p + "fc2_w", 1, D, d.mlp);
        w.fc2_b = (const float*)need(p + "fc2_b", 0, 1, D);
        if (!w.ln1_g || !w.ln1_b || !w.qkv_w || !w.qkv_b || !w.proj_w || !w.proj_b || !w.ln2_g ||
            !w.ln2_b || !w.fc1_w || !w.fc1_b || !w.fc2_w || !w.fc2_b)
            return VT_ERR_FORMAT;
    }
    return VT_OK;
}

int Engine::load_blob_host(const std::vector<uint8_t>& blob) {
    blob_bytes = blob.size();
    HIPCHK(hipMalloc((void**)&d_blob, blob_bytes));
    HIPCHK(hipMemcpy(d_blob, blob.data(), blob_bytes, hipMemcpyHostToDevice));
    return index_blob(blob.data(), blob_bytes);
}

int Engine::load_blob_device(const void* d_src, size_t bytes) {
    if (bytes < kHeaderBytes) return set_err(VT_ERR_FORMAT, "weight blob: truncated");
    std::vector<uint8_t> head(kHeaderBytes);
    HIPCHK(hipMemcpy(head.data(), d_src, kHeaderBytes, hipMemcpyDeviceToHost));
    if (memcmp(head.data(), kMagic, 8) != 0) return set_err(VT_ERR_FORMAT, "weight blob: bad magic");
    int32_t n_tensors;
    memcpy(&n_tensors, head.data() + 8 + 10 * 4, 4);
    const size_t tbl = kHeaderBytes + (size_t)std::max(n_tensors, 0) * kEntryBytes;
    if (n_tensors <= 0 || tbl > bytes) return set_err(VT_ERR_FORMAT, "weight blob: bad table");
    // host copy of header + table only; index_blob checks offsets against the full size
    std::vector<uint8_t> hc(tbl);
    HIPCHK(hipMemcpy(hc.data(), d_src, tbl, hipMemcpyDeviceToHost));
    blob_bytes = bytes;
    HIPCHK(hipMalloc((void**)&d_blob, blob_bytes));
    HIPCHK(hipMemcpy(d_blob, d_src, blob_bytes, hipMemcpyDeviceToDevice));
    HIPCHK(hipStreamSynchronize(nullptr));      // a device-to-device hipMemcpy may return early; the engine's
                                                // stream (non-blocking) is not ordered behind the null stream
    hc.resize(tbl);
    // index_blob only touches [0, tbl) of the host copy
    return index_blob(hc.data(), blob_bytes);
}


// HBM the activations of B streams need (bytes), as alloc_buffers() lays them out
size_t Engine::activation_bytes() const {
    const size_t M = (size_t)B * d.ntok, Ms = (size_t)B * d.ns;
    const size_t fold_rows = (size_t)d.L * (3 * d.D + d.mlp);      // folded QKV + fc1 weights of every layer
    return 2 * (M * d.kpad + M * d.D + M * 2 * d.D + (size_t)B * d.H * 64 * d.npad + M * d.D + M * d.mlp +
                Ms * d.D + 2 * Ms * d.C + fold_rows * d.D) + M * d.D /* lo8 plane */ +
           8 * (M * (d.D / VT_STAT_CHUNK) + M) + 4 * (Ms * 8 + 2 * fold_rows) +
           (size_t)B * (sizeof(StreamState) + sizeof(FrameDesc) + sizeof(vt_result) + 4 /* slot map */) +
           2 * (size_t)B * d.nt * d.kpad /* template store */;
}

int Engine::alloc_buffers() {
    const size_t M = (size_t)B * d.ntok, Ms = (size_t)B * d.ns;
    {   // fail early and cleanly (VT_ERR_OOM) instead of half-way through a dozen hipMallocs
        const size_t need = activation_bytes();
        if (max_device_bytes && need + blob_bytes > max_device_bytes)
            return set_err(VT_ERR_OOM, "%d streams need %.1f MiB of HBM (+ %.1f MiB of weights); "
                           "vt_config.max_device_mib allows %.1f", B, need / 1048576.0,
                           blob_bytes / 1048576.0, max_device_bytes / 1048576.0);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b)
            return set_err(VT_ERR_OOM, "%d streams need %.1f MiB of HBM for activations; %.1f MiB "
                           "are free on device %d", B, need / 1048576.0, free_b / 1048576.0, device);
    }
    HIPCHK(dalloc0(&d_patches, M * d.kpad, stream));
    HIPCHK(dalloc0(&d_tpl, (size_t)B * d.nt * d.kpad, stream));
    HIPCHK(dalloc0(&d_xh, M * d.D, stream));
    HIPCHK(dalloc0(&d_xl, M * d.D, stream));       // bytes
    HIPCHK(dalloc0(&d_cstat, M * (d.D / VT_STAT_CHUNK), stream));
    HIPCHK(dalloc0(&d_rstat, M + 1, stream));      // + 1: the 4-wave kernel fetches row terms as aligned pairs
    HIPCHK(dalloc0(&d_panel_cnt, (M + 255) / 256 + 1, stream));
    {   // fold LayerNorm 1 / 2 of every layer into the QKV / fc1 weights
        const size_t rows = (size_t)3 * d.D + d.mlp;
        HIPCHK(dalloc0(&d_foldw, (size_t)d.L * rows * d.D, stream));
        HIPCHK(dalloc0(&d_foldv, (size_t)d.L * 2 * rows, stream));
        for (int l = 0; l < d.L; ++l) {
            LayerW& w = layers[l];
            bf16_t* fw = d_foldw + (size_t)l * rows * d.D;
            float* fv = d_foldv + (size_t)l * 2 * rows;
            HIPCHK(launch_fold_layernorm(w.qkv_w, w.ln1_g, w.ln1_b, w.qkv_b, fw, fv, fv + rows, 3 * d.D, d.D, stream));
            HIPCHK(launch_fold_layernorm(w.fc1_w, w.ln2_g, w.ln2_b, w.fc1_b, fw + (size_t)3 * d.D * d.D, fv + 3 * d.D,
                                         fv + rows + 3 * d.D, d.mlp, d.D, stream));
            w.qkv_wf = fw; w.qkv_cs = fv; w.qkv_c = fv + rows;
            w.fc1_wf = fw + (size_t)3 * d.D * d.D; w.fc1_cs = fv + 3 * d.D; w.fc1_c = fv + rows + 3 * d.D;
        }
        HIPCHK(hipStreamSynchronize(stream));
    }
    HIPCHK(dalloc0(&d_qk, M * 2 * d.D, stream));
    HIPCHK(dalloc0(&d_vt, (size_t)B * d.H * 64 * d.npad, stream));
    HIPCHK(dalloc0(&d_attn, M * d.D, stream));
    HIPCHK(dalloc0(&d_mlp, M * d.mlp, stream));
    HIPCHK(dalloc0(&d_feat, Ms * d.D, stream));
    HIPCHK(dalloc0(&d_ta, Ms * d.C, stream));
    HIPCHK(dalloc0(&d_tb, Ms * d.C, stream));
    HIPCHK(dalloc0(&d_zeros, (size_t)128, stream));
    HIPCHK(dalloc0(&d_headout, Ms * 8, stream));
    HIPCHK(dalloc0(&d_states, (size_t)B, stream));
    HIPCHK(dalloc0(&d_band_cnt, (size_t)B + 1, stream));
    HIPCHK(dalloc0(&d_band_best, (size_t)B * d.gs * 2, stream));
    {   // B frame descriptors + the pass's PassOut + the slot map behind them (one upload per pass)
        void* p = nullptr;
        HIPCHK(hipMalloc(&p, frames_block_bytes()));
        HIPCHK(hipMemsetAsync(p, 0, frames_block_bytes(), stream));
        d_frames = (FrameDesc*)p;
    }
    HIPCHK(dalloc0(&d_results, (size_t)B, stream));
    HIPCHK(hipHostMalloc((void**)&h_frames, frames_block_bytes() * RING));
    HIPCHK(hipHostMalloc((void**)&h_results, sizeof(vt_result) * B));
    HIPCHK(hipHostMalloc((void**)&h_state, sizeof(StreamState)));
    HIPCHK(hipHostMalloc((void**)&h_states_all, sizeof(StreamState) * B));
    memset(h_states_all, 0, sizeof(StreamState) * B);
    memset(h_results, 0, sizeof(vt_result) * B);
    for (int i = 0; i < RING; ++i) HIPCHK(hipEventCreateWithFlags(&ring_ev[i], hipEventDisableTiming));
    h_initialized.assign(B, 0);
    pass_n = B;                     // no pass yet: reads as a full pass (pass_streams is empty)
    known.assign((size_t)B, StreamState{});
    known_motion.assign((size_t)B, MotionRec{});
    h_policy.assign((size_t)B, RefreshPolicy{});
    HIPCHK(hipStreamSynchronize(stream));       // every fill has landed before the handle is handed out
    return VT_OK;
}

// the algorithmic count, every block on all ntok rows: the last block on search rows only (last_block_compact) does not
// change it - what the benchmark divides by stays what it was
double Engine::flops_encoder() const {
    const double n = d.ntok, D = d.D;
    const double per_layer = 2 * n * D * 3 * D + 2 * n * D * D + 4 * n * D * d.mlp + 4 * n * n * D;
    return d.L * per_layer + 2 * n * (3.0 * d.patch * d.patch) * D;
}
double Engine::flops_head() const {
    const double C = d.C;
    return 2.0 * d.ns * (d.D * C + 27 * C * C + 8 * C);
}

// One hot-path pass over ps.n slots: all B streams (slot_stream null: slot b is stream b), or a subset pass, whose slot i
// works for stream slot_stream[i] (device map). Between the crop and the decode every kernel is slot-indexed and
// sized by M = n * ntok. A candidate pass (ps.cand) runs the same kernels on its slots' candidate states - the map then
// only says whose template a slot takes - between the fill and the commit of k_cand.hip. With prof != nullptr every launch is bracketed by HIP events on this engine's stream.
int Engine::run_pass(Profiler* prof, const PassShape& ps) {
    const int n = ps.n;
    const int32_t* slot_stream = ps.slot_stream;
    // whose state a slot reads and writes: its stream's through the map, or its own candidate state
    StreamState* const states = ps.cand ? ps.cand->cand_states : d_states;
    const int32_t* const state_map = ps.cand ? nullptr : slot_stream;
    const int M = n * d.ntok, Ms = n * d.ns, D = d.D;
    hipError_t lerr = hipSuccess;
    auto L = [&](const char* name, double flops, double bytes, auto&& fn) {
        if (lerr != hipSuccess) return;
        if (prof) {
            Profiler::Rec r;
            r.fam = prof->family(name);
            (void)hipEventCreate(&r.a);
            (void)hipEventCreate(&r.b);
            (void)hipEventCreate(&r.k.start);
            (void)hipEventCreate(&r.k.stop);
            r.k.launches = 0;
            (void)hipEventRecord(r.a, stream);
            vt_launch_probe = &r.k;
            lerr = fn();
            vt_launch_probe = nullptr;
            (void)hipEventRecord(r.b, stream);
            prof->recs.push_back(r);
            prof->fams[r.fam].launches += 1;
            prof->fams[r.fam].flops += flops;
            prof->fams[r.fam].bytes += bytes;
        } else {
            lerr = fn();
        }
    };
    auto gemm = [&](int epi, GemmArgs a) {
        a.lq = lq;
        const double fl = 2.0 * a.M * a.N * a.K;
        // algorithmic bytes: operands once, output once; the 3-byte residual pair is read and written (3 + 3 B)
        const double by = 2.0 * ((double)a.M * a.K + (double)a.N * a.K) +
                          (epi == EPI_RESID ? 6.0 : epi == EPI_F32_POS ? 3.0 : 2.0) * a.M * a.N;
        L(prof ? gemm_name(epi, a) : "", fl, by, [&] { return launch_gemm(a, epi, stream); });
    };
    auto tap = [&](int slot) {
        if (taps && lerr == hipSuccess) {     // both halves of the residual stream: [slot][hi | lo][M][D]
            uint8_t* dst = d_taps + (size_t)slot * tap_slot_bytes();
            lerr = hipMemcpyAsync(dst, d_xh, sizeof(bf16_t) * M * D, hipMemcpyDeviceToDevice, stream);
            if (lerr == hipSuccess)
                lerr = hipMemcpyAsync(dst + sizeof(bf16_t) * M * D, d_xl, (size_t)M * D, hipMemcpyDeviceToDevice, stream);
        }
    };
    const int nchunk = D / VT_STAT_CHUNK;
    // An X-epilogue GEMM (writes the residual pair) followed by the row terms (rstd, -mean * rstd) of the
    // LayerNorm that consumes it: finalized inside the GEMM by the last workgroup of every row panel (the
    // 256x256 kernel), else by a small launch of their own from the chunk partials
    // ... or, where the consumer runs on the 4-wave kernel (few streams), by the consumer's own epilogue:
    // `consumer` (the GEMM with the folded LayerNorm, arguments complete but for the row terms) gets
    // rowstat or cstat_in set accordingly.
    auto xgemm = [&](int epi, GemmArgs a, GemmArgs* consumer, int consumer_epi) {
        const bool stats = consumer != nullptr;
        if (!a.Xh) { a.Xh = d_xh; a.Xl = d_xl; }    // the compacted last block names its own pair
        a.ldx = D;
        a.cstat = stats ? d_cstat : nullptr;
        a.rowstat_out = stats ? d_rstat : nullptr;
        a.panel_cnt = d_panel_cnt;
        a.ln_eps = d.ln_eps;
        const bool fused = stats && gemm_finalizes_rowstat(a, epi);
        if (!fused) a.rowstat_out = nullptr;
        gemm(epi, a);
        if (!stats) return;
        consumer->ln_eps = d.ln_eps;
        if (!fused && gemm_effective_config(*consumer, consumer_epi) <= GEMM_CFG_SMALL_MAX && consumer->K <= 1024 && consumer->K % 128 == 0) {
            consumer->cstat_in = d_cstat;       // combined in the consumer's epilogue
            return;
        }
        consumer->rowstat = d_rstat;
        if (!fused)
            L("rowstat", 0, (double)a.M * (nchunk + 1) * 8,
              [&] { return launch_rowstat_finalize(d_cstat, d_rstat, a.M, nchunk, d.ln_eps, stream); });
    };
    auto qkv_args = [&](int l) {
        const LayerW& w = layers[l];
        GemmArgs a{};
        a.A = d_xh; a.lda = D; a.W = w.qkv_wf; a.ldw = D; a.bias = w.qkv_c; a.colsum = w.qkv_cs;
        a.M = M; a.N = 3 * D; a.K = D;
        a.qk = d_qk; a.vt = d_vt; a.tokens = d.ntok; a.npad = d.npad; a.D = D;
        a.vt_perm = attention_vt_perm(attention_pick_mode(d.ntok, d.npad));   // layout the attention kernel reads
        return a;
    };
    GemmArgs qkv = qkv_args(0);             // LayerNorm 1 is folded into the QKV GEMM

    // the motion prior: the listed streams' boxes move ahead before anything reads them (k_motion.hip)
    MotionArgs ma{};
    if (motion_capable)
        ma = MotionArgs{d_states, d_motion_recs(), d_motion_policy(), d_results, slot_stream, ps.cand ? ps.cand->winner : nullptr,
                        ps.cand ? ps.cand->cands : nullptr, (const PassOut*)(d_frames + B), ps.cand ? ps.cand->host_states : nullptr, n};
    if (motion_capable)
        L("motion_place", 0, (double)n * (sizeof(StreamState) + 2.0 * sizeof(MotionRec)), [&] { return launch_motion_place(ma, stream); });
    // K1: crop + resize + normalise the search window of every stream -> patch rows
    if (refresh_capable)    // every pass, from the stream's current buffer of the two-buffer store
        L("gather_template", 0, 4.0 * n * d.nt * d.kpad,
          [&] { return launch_gather_template_rows_gen(d_tpl, d_patches, slot_stream, d_states, n, d, stream); });
    else if (slot_stream)   // the slots' template rows from the store (a full pass finds them in place)
        L("gather_template", 0, 4.0 * n * d.nt * d.kpad,
          [&] { return launch_gather_template_rows(d_tpl, d_patches, slot_stream, n, d, stream); });
    if (ps.cand)
        L("cand_fill", 0, 2.0 * n * sizeof(StreamState), [&] { return launch_cand_fill(*ps.cand, stream); });
    L("preproc_search", 0, (double)n * (d.S * d.S * 3 * 2 + 1.5 * d.S * d.S),
      [&] { return launch_preproc(d_frames, states, d_patches, d, 0, n, false, stream, ps.tier, state_map, ps.any_layout); });
    // K2: patch embedding (+bias +pos) -> residual stream (3-byte pair + chunk statistics)
    {
        GemmArgs a{};
        a.A = d_patches; a.lda = d.kpad;
        a.W = (const bf16_t*)find("patch_w")->ptr; a.ldw = d.kpad;
        a.bias = (const float*)find("patch_b")->ptr;
        a.M = M; a.N = D; a.K = d.kpad;
        a.pos = (const float*)find("pos")->ptr; a.pos_rows = d.ntok;
        xgemm(EPI_F32_POS, a, &qkv, EPI_QKV);       // + the row terms of block 0's LayerNorm 1
    }
    tap(0);
    for (int l = 0; l < d.L; ++l) {
        const LayerW& w = layers[l];
        gemm(EPI_QKV, qkv);
        // The last block of a compacted pass (vt_engine.hpp, last_block_compact): the search queries only, from here on
        // every buffer is compact - Ml = n * ns rows - and the kernels behind the attention are the ordinary ones
        const bool cl = ps.compact && l == d.L - 1;
        const int Ml = cl ? Ms : M, rows = cl ? d.ns : d.ntok;
        L(cl ? "attention_search" : "attention", 4.0 * n * (double)rows * d.ntok * D, ((double)M * 6 + (double)Ml * 2) * D, [&] {
            return cl ? launch_attention_queries(d_qk, d_vt, d_attn, n, d.ntok, d.H, d.npad, d.nt, d.ns, stream)
                      : launch_attention(d_qk, d_vt, d_attn, n, d.ntok, d.H, d.npad, stream);
        });
        {
            GemmArgs a{};
            a.A = d_attn; a.lda = D; a.W = w.proj_w; a.ldw = D; a.bias = w.proj_b;
            a.M = Ml; a.N = D; a.K = D;
            if (cl) {       // addend: the whole-layout pair, search rows through the remap; output: the compact pair (d_qk is dead)
                a.Xh = xc_hi(); a.Xl = xc_lo();
                a.Xh_in = d_xh; a.Xl_in = d_xl; a.seg_rows = d.ns; a.seg_skip = d.nt;
            }
            GemmArgs f{};                   // LayerNorm 2 is folded into fc1
            f.A = cl ? xc_hi() : d_xh; f.lda = D; f.W = w.fc1_wf; f.ldw = D; f.bias = w.fc1_c; f.colsum = w.fc1_cs;
            f.M = Ml; f.N = d.mlp; f.K = D; f.Cb = d_mlp; f.ldcb = d.mlp;
            xgemm(EPI_RESID, a, &f, EPI_GELU_BF16);      // + the row terms of LayerNorm 2
            gemm(EPI_GELU_BF16, f);
        }
        {
            GemmArgs a{};
            a.A = d_mlp; a.lda = d.mlp; a.W = w.fc2_w; a.ldw = d.mlp; a.bias = w.fc2_b;
            a.M = Ml; a.N = D; a.K = d.mlp;
            if (cl) { a.Xh = xc_hi(); a.Xl = xc_lo(); }
            if (l + 1 < d.L) {              // + the next block's LayerNorm 1 (the final LayerNorm reads the rows itself)
                qkv = qkv_args(l + 1);
                xgemm(EPI_RESID, a, &qkv, EPI_QKV);
            } else {
                xgemm(EPI_RESID, a, nullptr, 0);
            }
        }
        tap(1 + l);
    }
    // final LayerNorm on the search tokens only, compacted to [B*ns][D] - as a launch of its own unless the head's
    // first layer normalises its rows itself (k_head.hip, LNC)
    const bool band = head_band(), ln_fused = head_ln_fused();
    if (!ln_fused)
        L("layernorm", 0, (double)Ms * D * 6, [&] { return final_layernorm(n, ps.compact); });
    // centre head: 1x1 conv, three 3x3 convs, then the f32 5-logit layer + decode. On the band kernel of
    // k_head.hip (the A image of a band resident in LDS, logits + decode fused behind the last layer: 4 launches)
    // where the shape allows it, else as implicit GEMMs on the 4-wave kernel + head_out + decode (6 launches).
    DecodeArgs dec{};
    dec.w4 = (const float*)find("head.w4")->ptr;
    dec.b4 = (const float*)find("head.b4")->ptr;
    dec.hann = (const float*)find("hann")->ptr;
    dec.head_out = d_headout; dec.states = states; dec.results = d_results;
    dec.out = (const PassOut*)(d_frames + B);      // behind the B descriptors whatever the pass's slot count
    dec.slot_stream = state_map;
    dec.B = n; dec.ns = d.ns; dec.grid = d.gs; dec.C = d.C;
    dec.success_threshold = success_threshold;
    bf16_t* cur = d_ta;
    bf16_t* nxt = d_tb;
    if (band) {
        HeadConvArgs h{};
        h.in = d_feat; h.ldin = D; h.W = (const bf16_t*)find("head.w0")->ptr; h.ldw = D;
        h.bias = (const float*)find("head.b0")->ptr; h.out = d_ta; h.ldout = d.C; h.zeros = d_zeros;
        h.B = n; h.grid = d.gs; h.C = d.C; h.N = d.C; h.K = D; h.conv3x3 = 0;
        if (ln_fused) {
            h.in = nullptr;
            h.xh = d_xh; h.xl = d_xl; h.ln_g = (const float*)find("norm_g")->ptr; h.ln_b = (const float*)find("norm_b")->ptr;
            h.ln_eps = d.ln_eps; h.in_stride = d.ntok; h.in_off = d.nt; h.lo_q = lq.q;
            if (ps.compact) { h.xh = xc_hi(); h.xl = xc_lo(); h.in_stride = d.ns; h.in_off = 0; }
        }
        L(prof ? (ln_fused ? "head_ln_conv1x1" : "head_conv1x1") : "", 2.0 * Ms * d.C * D,
          2.0 * ((double)Ms * D * (ln_fused ? 2 : 1) + (double)d.C * D + (double)Ms * d.C),
          [&] { return launch_headconv(h, nullptr, stream); });
        for (int k = 1; k <= 3; ++k) {
            const std::string wn = "head.w" + std::to_string(k), bn = "head.b" + std::to_string(k);
            HeadConvArgs c{};
            c.in = cur; c.ldin = d.C; c.W = (const bf16_t*)find(wn)->ptr; c.ldw = 9 * d.C;
            c.bias = (const float*)find(bn)->ptr; c.out = nxt; c.ldout = d.C; c.zeros = d_zeros;
            c.B = n; c.grid = d.gs; c.C = d.C; c.N = d.C; c.K = 9 * d.C; c.conv3x3 = 1;
            c.band_cnt = d_band_cnt; c.band_best = d_band_best;
            const bool tail = k == 3;
            const double fl = 2.0 * Ms * d.C * 9.0 * d.C + (tail ? 2.0 * Ms * d.C * 5 : 0.0);
            const double by = 2.0 * (2.0 * Ms * d.C + 9.0 * d.C * d.C);
            L(prof ? (tail ? "head_conv3x3_logits_decode" : "head_conv3x3") : "", fl, by,
              [&] { return launch_headconv(c, tail ? &dec : nullptr, stream); });
            std::swap(cur, nxt);
        }
    } else {
        {
            GemmArgs a{};
            a.A = d_feat; a.lda = D; a.W = (const bf16_t*)find("head.w0")->ptr; a.ldw = D;
            a.bias = (const float*)find("head.b0")->ptr;
            a.M = Ms; a.N = d.C; a.K = D; a.Cb = d_ta; a.ldcb = d.C;
            gemm(EPI_RELU_BF16, a);
        }
        for (int k = 1; k <= 3; ++k) {     // 3x3 convs as implicit GEMMs: the im2col row is gathered by the A loads
            GemmArgs a{};
            const std::string wn = "head.w" + std::to_string(k), bn = "head.b" + std::to_string(k);
            a.A = cur; a.lda = d.C; a.W = (const bf16_t*)find(wn)->ptr; a.ldw = 9 * d.C;
            a.bias = (const float*)find(bn)->ptr;
            a.M = Ms; a.N = d.C; a.K = 9 * d.C; a.Cb = nxt; a.ldcb = d.C;
            a.conv_grid = d.gs; a.conv_C = d.C; a.zeros = d_zeros;
            gemm(EPI_RELU_BF16, a);
            std::swap(cur, nxt);
        }
        dec.t3 = cur;
        L("decode", 2.0 * Ms * d.C * 5, (double)Ms * d.C * 2, [&] { return launch_decode(dec, stream); });
    }
    if (ps.cand)
        L("cand_commit", 0, 2.0 * n * sizeof(StreamState), [&] { return launch_cand_commit(*ps.cand, stream); });
    if (arb_capable) {      // directly behind the decode / the commit: everything below reads the box the arbitration left (k_arbitrate.hip)
        ArbArgs aa{};
        aa.head_out = d_headout; aa.hann = dec.hann; aa.frames = d_frames; aa.states = d_states; aa.results = d_results;
        aa.slot_stream = slot_stream; aa.winner = ps.cand ? ps.cand->winner : nullptr; aa.policy = d_arb_policy();
        aa.recs = d_arb_recs(); aa.counts = d_arb_counts(); aa.tickets = d_arb_tickets(); aa.partials = d_arb_partials();
        aa.anchor = d_anchor(); aa.probe = d_arb_probe(); aa.out = (const PassOut*)(d_frames + B);
        aa.host_states = ps.cand ? ps.cand->host_states : nullptr;
        aa.n = n; aa.ns = d.ns; aa.grid = d.gs; aa.success_threshold = success_threshold;
        const int cols = 3 * d.patch * d.patch;
        L("arbitrate_list", 0, (double)n * (d.ns * 8.0 * 4 + sizeof(StreamState) + sizeof(ArbRec)), [&] { return launch_arbitrate_list(aa, d, stream); });
        L("arbitrate_probe", 0, 0, [&] { return launch_arbitrate_probe(aa, d, ps.tier, ps.any_layout, stream); });
        L("arbitrate_score", 0, 0, [&] { return launch_arbitrate_score(aa, d.nt, cols, d.kpad, stream); });
        L("arbitrate_commit", 0, (double)n * 2.0 * sizeof(ArbRec), [&] { return launch_arbitrate_commit(aa, stream); });
    }
    if (motion_capable)     // ahead of everything that reads the new box: the velocity, the coast or the restore
        L("motion_settle", 0, (double)n * (sizeof(StreamState) + sizeof(vt_result) + 3.0 * sizeof(MotionRec)),
          [&] { return launch_motion_settle(ma, stream); });
    if (conflict_capable) { // directly behind the final boxes, ahead of the refresh launch, whose rule 9 reads the records: k_conflicts.hip
        const ConflictArgs ca{d_states, d_results, slot_stream, ps.cand ? ps.cand->winner : nullptr, d_conflict_policy(),
                              d_conflict_scenes(), d_conflict_recs(), d_conflict_counts(), (const PassOut*)(d_frames + B), n};
        L("conflicts_check", 10.0 * n * n, (double)n * (sizeof(StreamState) + sizeof(vt_result) + 2.0 * sizeof(ConflictRec)),
          [&] { return launch_conflicts_check(ca, stream); });
    }
    if (health_capable) {   // directly behind conflicts_check, ahead of the refresh launch, whose rule 10 reads the records; undrawn pixels: k_health.hip
        const HealthArgs ha{d_frames, d_states, slot_stream, d_health_policy(), d_devflag(), d_health_recs(), d_health_counts(),
                            d_health_heads(), d_health_accs(), d_health_hist(), d_health_thumbs(), (const PassOut*)(d_frames + B),
                            health_policy.max_cells, n};
        L("health_prepare", 0, (double)n * (sizeof(StreamState) + sizeof(HealthHead)), [&] { return launch_health_prepare(ha, stream); });
        L("health_thumb", 0, 0, [&] { return launch_health_thumb(ha, ps.any_layout, stream); });
        L("health_measure", 0, 0, [&] { return launch_health_measure(ha, stream); });
        L("health_decide", 0, (double)n * 2.0 * sizeof(HealthRec), [&] { return launch_health_decide(ha, stream); });
    }
    if (appear_capable) {   // ahead of everything that cuts or draws: the probe at the new box and its similarity to the anchor
        const AppearArgs aa{d_frames, d_states, d_results, slot_stream, ps.cand ? ps.cand->winner : nullptr, d_appear_policy(),
                            d_appear_counts(), d_appear_recs(), refresh_capable ? d_policy : nullptr, d_appear_tickets(),
                            d_appear_partials(), d_anchor(), d_probe(), (const PassOut*)(d_frames + B),
                            ps.cand ? ps.cand->host_states : nullptr, nullptr, n};
        const int cols = 3 * d.patch * d.patch;
        L("appearance_probe", 0, (double)n * (sizeof(StreamState) + sizeof(vt_result) + sizeof(AppearRec)),
          [&] { return launch_appearance_probe(aa, d, ps.tier, ps.any_layout, stream); });
        L("appearance_score", 10.0 * n * d.nt * cols, 4.0 * n * d.nt * cols,
          [&] { return launch_appearance_score(aa, d.nt, cols, d.kpad, stream); });
    }
    if (prop_capable) {     // ahead of the refresh: the pattern is the template this pass ran on; ahead of the overlay: undrawn pixels
        const PropArgs pa{d_frames, d_states, d_results, slot_stream, ps.cand ? ps.cand->winner : nullptr, d_prop_policy(),
                          d_devflag(), d_tpl, tpl_bufs(), d_prop_recs(), d_prop_counts(), d_prop_heads(), d_prop_pattern(),
                          d_prop_thumb(), d_prop_map(), (const PassOut*)(d_frames + B), prop_policy.max_cells, n};
        L("proposals_prepare", 0, (double)n * (sizeof(StreamState) + sizeof(vt_result) + sizeof(PropHead)),
          [&] { return launch_proposals_prepare(pa, d, stream); });
        L("proposals_thumb", 0, 0, [&] { return launch_proposals_thumb(pa, d, ps.any_layout, stream); });
        L("proposals_match", 0, 0, [&] { return launch_proposals_match(pa, stream); });
        L("proposals_list", 0, (double)n * 2.0 * sizeof(PropRec), [&] { return launch_proposals_list(pa, stream); });
    }
    if (refresh_capable) {  // the streams' policies, on what the decode (the commit) left: k_refresh.hip
        RefreshArgs ra{d_frames, d_states, d_results, slot_stream, ps.cand ? ps.cand->winner : nullptr, d_policy,
                       d_tickets, d_tpl, (const PassOut*)(d_frames + B), ps.cand ? ps.cand->host_states : nullptr, n};
        if (appear_capable) { ra.ap_policy = d_appear_policy(); ra.ap_counts = d_appear_counts(); ra.ap_recs = d_appear_recs(); }
        if (conflict_capable) { ra.cf_policy = d_conflict_policy(); ra.cf_counts = d_conflict_counts(); ra.cf_recs = d_conflict_recs(); }
        if (health_capable) { ra.hl_policy = d_health_policy(); ra.hl_counts = d_health_counts(); ra.hl_recs = d_health_recs(); }
        L("refresh_template", 0, 2.0 * n * (sizeof(StreamState) + sizeof(vt_result)),
          [&] { return launch_template_refresh(ra, d, ps.tier, ps.any_layout, stream); });
    }
    if (chip_capable) {     // the streams' chips at the boxes the decode (the commit) left: k_chip.hip
        const ChipArgs ca{d_frames, d_states, d_results, slot_stream, ps.cand ? ps.cand->winner : nullptr, d_chip_policy,
                          d_chips, d_chip_infos, (const PassOut*)(d_frames + B), ps.cand ? ps.cand->host_states : nullptr, n};
        L("target_chips", 0, (double)n * (sizeof(StreamState) + sizeof(vt_result) + sizeof(vt_chip_info)), [&] {
            return launch_target_chips(ca, chip_size, chip_kind, chip_na, chip_nb, d.S, ps.tier, ps.any_layout, stream);
        });
    }
    if (peaks_capable) {    // the slots' runner-up maxima, on the logits and states the launches above left: k_peaks.hip
        const PeaksArgs pa{d_headout, dec.hann, d_states, slot_stream, ps.cand ? ps.cand->winner : nullptr, d_peaks_policy,
                           d_peaks, (const PassOut*)(d_frames + B), n, d.ns, d.gs};
        L("response_peaks", 0, (double)n * (d.ns * 8.0 * sizeof(float) + 2.0 * sizeof(vt_peaks)),
          [&] { return launch_response_peaks(pa, stream); });
    }
    if (overlay_capable) {  // LAST: the slots' boxes into their frames - the refresh and chip launches above cut undrawn pixels
        const ResultOverlayArgs oa{d_frames, d_results, slot_stream, ps.cand ? ps.cand->winner : nullptr, d_overlay_policy(),
                                   d_overlay_stats(), d_devflag(), n};
        L("result_overlay", 0, (double)n * (sizeof(FrameDesc) + sizeof(vt_result) + sizeof(OverlayStats)),
          [&] { return launch_result_overlay(oa, stream); });
    }
    if (lerr != hipSuccess)
        return set_err(VT_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(lerr));
    return VT_OK;     // results and states reach the host through the decode kernel's own stores (PassOut)
}

hipError_t Engine::final_layernorm(int n, bool compact) {
    return launch_layernorm_split(compact ? xc_hi() : d_xh, compact ? xc_lo() : d_xl, (const float*)find("norm_g")->ptr,
                                  (const float*)find("norm_b")->ptr, d_feat, (int)((size_t)n * d.ns), d.D, d.ns,
                                  compact ? d.ns : d.ntok, compact ? 0 : d.nt, d.ln_eps, lq.q, stream);
}

bool Engine::last_block_compact(int n, bool with_taps) const {
    if (!last_rows || with_taps || n < 1 || d.nt < 1 || (d.ns & 1)) return false;
    if (attention_pick_mode(d.ntok, d.npad) != 3) return false;
    GemmArgs a{};       // the compact proj as run_pass launches it
    a.A = d_attn; a.lda = d.D; a.W = layers[(size_t)d.L - 1].proj_w; a.ldw = d.D; a.bias = layers[(size_t)d.L - 1].proj_b;
    a.M = n * d.ns; a.N = d.D; a.K = d.D;
    a.Xh = xc_hi(); a.Xl = xc_lo(); a.ldx = d.D;
    a.Xh_in = d_xh; a.Xl_in = d_xl; a.seg_rows = d.ns; a.seg_skip = d.nt;
    return gemm_effective_config(a, EPI_RESID) >= GEMM_CFG_256_MIN;
}

int Engine::expand_last_block() {
    if (!pass_compact) return VT_OK;
    const size_t seg = (size_t)d.ns * d.D, full = (size_t)d.ntok * d.D, off = (size_t)d.nt * d.D;
    HIPCHK(hipMemcpy2DAsync(d_xh + off, full * sizeof(bf16_t), xc_hi(), seg * sizeof(bf16_t), seg * sizeof(bf16_t), (size_t)pass_n,
                            hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipMemcpy2DAsync(d_xl + off, full, xc_lo(), seg, seg, (size_t)pass_n, hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return VT_OK;
}

int Engine::capture_graph(int tier, int any_layout) {
    HIPCHK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    int rc = run_pass(nullptr, PassShape{B, nullptr, tier, any_layout, nullptr, last_block_compact(B, false)});
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(stream, &g);
    if (rc != VT_OK) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
    }
    if (e != hipSuccess) return set_err(VT_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
    hipGraphExec_t x = nullptr;
    e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
    if (e != hipSuccess) {          // nothing half-built stays behind: the next attempt starts from scratch
        (void)hipGraphDestroy(g);
        return set_err(e == hipErrorOutOfMemory ? VT_ERR_OOM : VT_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
    }
    graphs[any_layout][tier] = PassGraph{g, x};
    graph_captures += 1;
    return VT_OK;
}

// Every crop-buffer tier's pass, captured and instantiated NOW (engine creation, vt_group_set_tuning): the hot path only
// replays. A live stream whose target grows across a tier boundary (~130 / ~200 px at search 384) must not pay a
// capture + instantiate inside an update (60 fps: /root/reference/src/pipeline.rs:26-37).
// With a bit of want_levels, the passes of the crop kernels of that level too (Engine::init_stream sets it).
int Engine::capture_all_graphs() {
    if (!use_graph) return VT_OK;
    for (int any = 0; any < PIX_LEVELS; ++any)
        for (int t = 0; t < TIERS && (any == 0 || (want_levels >> any & 1)); ++t)
            if (!graphs[any][t].exec)
                if (int rc = capture_graph(t, any)) return rc;
    return VT_OK;
}

// The first stream on a format of a level (pix_level) above 0: every tier's pass with the crop kernels of that level
// is captured at its init, on the idle stream, so that no update of such a stream captures (a failure leaves the
// engine as it was, apart from the tiers already captured, which stay valid).
int Engine::capture_graphs_for(int format) {
    const int level = pix_level(format);
    if (!use_graph || level == 0 || (want_levels >> level & 1)) return VT_OK;
    HIPCHK(hipStreamSynchronize(stream));
    want_levels |= 1u << level;
    if (int rc = capture_all_graphs()) { want_levels &= ~(1u << level); return rc; }
    return VT_OK;
}

// every format is checked by its family (vt_frame.hpp: PixFamily): a luma plane with chroma planes by the rules of NV12
// (NV16: the window rules of YUY2) on the bytes of its samples and planes, packed 4:2:2 by those of YUY2, packed RGB and
// grey by the bytes per pixel
int check_frame(const vt_frame& f) {
    if (!f.plane0 || f.width < 16 || f.height < 16 || f.width > 16384 || f.height > 16384)
        return set_err(VT_ERR_INVALID_ARG, "frame: null plane or size out of range");
    const int fam = pix_family(f.format);
    if (fam < 0) {
        if (const char* why = pix_refusal(f.format))    // a known format with colour bits the boundary refuses
            return set_err(VT_ERR_INVALID_ARG, "%s frame format 0x%x: %s", pix_name(f.format), (unsigned)f.format, why);
        return set_err(VT_ERR_INVALID_ARG, "unknown pixel format %d", f.format);
    }
    const bool window = f.origin_x != 0 || f.origin_y != 0 || f.windowed == 1;
    const bool rows422 = pix_rows422(f.format);     // NV16: pairs along x only
    if (f.origin_x < 0 || f.origin_y < 0 || f.origin_x >= f.width || f.origin_y >= f.height ||
        (fam == PIXF_420SP && ((f.origin_x | (rows422 ? 0 : f.origin_y)) & 1)) ||
        (fam == PIXF_422 && (f.origin_x & 1)))
        return set_err(VT_ERR_INVALID_ARG, "%s frame window origin %d,%d invalid", pix_name(f.format), f.origin_x, f.origin_y);
    // extent of what the planes hold: the kernels never read outside it (fetch_rgb, k_preproc.hip)
    int ww = f.width, wh = f.height;
    (void)wh;
    if (window) {
        if (f.window_w < 1 || f.window_h < 1 || f.window_w > f.width - f.origin_x ||
            f.window_h > f.height - f.origin_y)
            return set_err(VT_ERR_INVALID_ARG, "windowed frame needs window_w/window_h inside the frame "
                           "(got %dx%d at %d,%d of %dx%d)", f.window_w, f.window_h, f.origin_x, f.origin_y,
                           f.width, f.height);
        ww = f.window_w; wh = f.window_h;
        if (fam == PIXF_420SP && (((ww & 1) && f.origin_x + ww != f.width) ||
                                  (!rows422 && (wh & 1) && f.origin_y + wh != f.height)))
            return set_err(VT_ERR_INVALID_ARG, "%s window extent must be even unless it ends at the frame edge",
                           pix_name(f.format));
    } else if (f.window_w != 0 || f.window_h != 0) {
        if (f.window_w != f.width || f.window_h != f.height)
            return set_err(VT_ERR_INVALID_ARG, "window_w/window_h set on a frame that is not windowed");
    }
    if (fam == PIXF_RGB) {
        const int bpp = pix_row_bpp(f.format);
        if (f.stride0 < ww * bpp) return set_err(VT_ERR_INVALID_ARG, "%s stride < %d*width", pix_name(f.format), bpp);
    } else if (fam == PIXF_420SP) {
        if (!f.plane1 || f.stride0 < ww * pix_row_bpp(f.format) || f.stride1 < pix_chroma_row_bytes(f.format, ww))
            return set_err(VT_ERR_INVALID_ARG, "%s: null UV plane or stride too small", pix_name(f.format));
        if (rows422 && (f.width & 1))
            return set_err(VT_ERR_INVALID_ARG, "%s: odd width", pix_name(f.format));
    } else {
        if ((f.width & 1) || f.stride0 < ((ww + 1) & ~1) * 2)
            return set_err(VT_ERR_INVALID_ARG, "%s: odd width or stride < 2*width", pix_name(f.format));
    }
    return VT_OK;
}

void to_desc(const vt_frame& f, FrameDesc* o) {
    const bool window = f.origin_x != 0 || f.origin_y != 0 || f.windowed == 1;
    o->p0 = (const uint8_t*)f.plane0;
    o->p1 = (const uint8_t*)f.plane1;
    o->w = f.width; o->h = f.height; o->s0 = f.stride0; o->s1 = f.stride1;
    o->fmt = pix_family(f.format);      // RGB8, NV12, YUY2: their own value
    o->x0 = f.origin_x; o->y0 = f.origin_y;
    o->ww = window ? f.window_w : f.width;
    o->wh = window ? f.window_h : f.height;
    o->lay = pix_layout(f.format);
    // two chroma planes: the second one lies behind the rows of the first, those of the whole frame unless the planes hold a
    // packed window (vittrack_hip.h: vt_pixfmt2)
    if (pix_planar(f.format) && f.windowed != 1) o->lay |= PIXL_FULLH;
    // the colour code of a YUV frame (0 for every plain format value: the word is then what it was): read by the kernels
    // of level 3 alone, the only ones that see a frame with it set (pix_level)
    o->lay |= pix_color_code(f.format) << PIXL_CODE_SHIFT;
}

int Engine::check_init_box(vt_bbox box) const {
    if (box.width < 1 || box.height < 1 || box.width > 32768 || box.height > 32768 ||
        box.x < -32768 || box.y < -32768 || box.x > 32768 || box.y > 32768)
        return set_err(VT_ERR_INVALID_ARG, "init: bbox %d,%d %dx%d out of range", box.x, box.y,
                       box.width, box.height);
    return VT_OK;
}

int Engine::launch_init(int b, const vt_frame* f, vt_bbox box, StreamState* h_st, FrameDesc* h_desc) {
    memset(h_st, 0, sizeof(StreamState));
    h_st->box[0] = (float)box.x; h_st->box[1] = (float)box.y;
    h_st->box[2] = (float)box.width; h_st->box[3] = (float)box.height;
    h_st->frame_w = f->width; h_st->frame_h = f->height;
    h_st->initialized = 1;
    HIPCHK(hipMemcpyAsync(d_states + b, h_st, sizeof(StreamState), hipMemcpyHostToDevice, stream));
    if (int rc = reset_records(RESET_INIT, b, b + 1)) return rc;    // every record spoke of the target the stream had
    to_desc(*f, h_desc);
    // entry b of the per-pass block: every pass uploads its own block ahead of its kernels, in stream order
    HIPCHK(hipMemcpyAsync(d_frames + b, h_desc, sizeof(FrameDesc), hipMemcpyHostToDevice, stream));
    HIPCHK(launch_preproc(d_frames, d_states, d_patches, d, b, 1, true, stream,
                          preproc_tier_for_box(d, (float)box.width, (float)box.height, true), nullptr,
                          pix_level(f->format)));
    // the stream's template rows, kept for the subset passes that run it in another slot (and for the full pass that
    // follows one: restore_segments puts every stream's rows back from here, these included)
    HIPCHK(hipMemcpyAsync(tpl_init_rows(b), d_patches + (size_t)b * d.ntok * d.kpad,
                          sizeof(bf16_t) * d.nt * d.kpad, hipMemcpyDeviceToDevice, stream));
    HIPCHK(anchor_from_template(b, 0));     // the appearance anchor: the init's rows (buffer 0)
    return VT_OK;
}

int Engine::init_stream(int b, const vt_frame* f, vt_bbox box) {
    if (b < 0 || b >= B || !f) return set_err(VT_ERR_INVALID_ARG, "init: bad stream index");
    if (int rc = check_frame(*f)) return rc;
    if (int rc = check_init_box(box)) return rc;
    DEVICE_SCOPE(device);
    HIPCHK(hipStreamSynchronize(stream));
    if (int rc = capture_graphs_for(f->format)) return rc;      // before anything changes
    // stream is idle: h_state and ring slot 0 are free
    if (int rc = launch_init(b, f, box, h_state, h_frames)) return rc;
    HIPCHK(hipStreamSynchronize(stream));
    h_states_all[b] = *h_state;
    known[b] = *h_state;
    h_initialized[b] = 1;
    return VT_OK;
}

// After a subset pass the segments of d_patches hold other streams' template rows: one strided copy puts every stream's
// rows back into its own segment before a full pass (its captured graph expects them in place).
int Engine::restore_segments() {
    if (refresh_capable) segments_moved = false;    // every pass gathers its rows: nothing is ever "in place"
    if (!segments_moved) return VT_OK;
    const size_t row = sizeof(bf16_t) * d.nt * d.kpad;
    HIPCHK(hipMemcpy2DAsync(d_patches, sizeof(bf16_t) * (size_t)d.ntok * d.kpad, d_tpl, row, row, (size_t)B,
                            hipMemcpyDeviceToDevice, stream));
    segments_moved = false;
    return VT_OK;
}

int Engine::check_streams(const int32_t* streams, int n) const {
    if (!streams) {
        if (n != B) return set_err(VT_ERR_INVALID_ARG, "pass over all streams: need exactly %d frames", B);
    } else {
        if (n < 1 || n > B) return set_err(VT_ERR_INVALID_ARG, "pass over %d streams: need 1..%d", n, B);
        std::vector<char> seen((size_t)B, 0);
        for (int i = 0; i < n; ++i) {
            const int s = streams[i];
            if (s < 0 || s >= B) return set_err(VT_ERR_INVALID_ARG, "streams[%d] = %d out of range (0..%d)", i, s, B - 1);
            if (seen[(size_t)s]) return set_err(VT_ERR_INVALID_ARG, "stream %d listed twice", s);
            seen[(size_t)s] = 1;
        }
    }
    for (int i = 0; i < n; ++i) {
        const int s = streams ? streams[i] : i;
        if (!h_initialized[s]) return set_err(VT_ERR_NOT_INITIALIZED, "stream %d: update before init", s);
    }
    return VT_OK;
}

// The one place a pass's block is built (vt_engine.hpp), behind whatever the stream is doing: prepare_pass and
// enqueue_candidates add only what is theirs.
int Engine::build_block(const int32_t* map, const vt_frame* frames, int n, const PassOut* sinks, bool by_stream_states,
                        PassShape* ps) {
    const int slot = ring_pos;
    ring_pos = (ring_pos + 1) % RING;
    HIPCHK(hipEventSynchronize(ring_ev[slot]));  // the copies that last used this ring position are done
    FrameDesc* hf = h_block(slot);
    *ps = PassShape{n, map ? d_map() : nullptr, 0, 0, nullptr};
    for (int i = 0; i < n; ++i) {
        to_desc(frames[i], hf + i);
        ps->any_layout = std::max(ps->any_layout, pix_level(frames[i].format));
    }
    *(PassOut*)(hf + B) = pass_sinks(sinks, by_stream_states);
    if (map) std::copy(map, map + n, (int32_t*)((char*)hf + map_offset()));
    *(int32_t*)((char*)hf + devflag_offset()) = frames_on_device;
    HIPCHK(hipMemcpyAsync(d_frames, hf, frames_block_bytes(), hipMemcpyHostToDevice, stream));
    HIPCHK(hipEventRecord(ring_ev[slot], stream));
    pass_n = n;
    if (map) pass_streams.assign(map, map + n);
    else pass_streams.clear();
    pass_winner.clear();
    if (taps) taps_filled = true;
    feat_in_head = head_ln_fused();
    ps->compact = pass_compact = last_block_compact(n, taps);
    return VT_OK;
}

// A pass over the streams streams[0..n) on n compacted slots: slot i takes frames[i] and works for stream streams[i];
// no other stream's state is touched. A null list or the full identity list is the full pass: every stream's template
// rows in its own segment, no slot map.
int Engine::prepare_pass(const int32_t* streams, const vt_frame* frames, int n, const PassOut* sinks, PassShape* ps) {
    if (int rc = check_streams(streams, n)) return rc;
    if (!frames) return set_err(VT_ERR_INVALID_ARG, "null frames");
    for (int i = 0; i < n; ++i)
        if (int rc = check_frame(frames[i])) return rc;
    bool full = n == B;
    for (int i = 0; streams && i < n && full; ++i) full = streams[i] == i;
    if (int rc = build_block(full ? nullptr : streams, frames, n, sinks, true, ps)) return rc;
    cand_pending = false;
    if (!full) segments_moved = true;
    else if (int rc = restore_segments()) return rc;
    ps->tier = pick_crop_tier(full ? nullptr : streams, n);     // a subset pass: from the boxes of its own streams
    return VT_OK;
}

// The one entry every pass takes. The full pass replays its captured graph; a subset pass runs eagerly - never a
// capture inside an update - behind the gather of its template rows.
int Engine::enqueue(const int32_t* streams, const vt_frame* frames, int n, const PassOut* sinks) {
    DEVICE_SCOPE(device);
    PassShape ps;
    if (int rc = prepare_pass(streams, frames, n, sinks, &ps)) return rc;
    if (!ps.slot_stream && use_graph && !taps) {
        // the captured set of the lowest level that reads every format of the pass
        // (a pass of level 1 or 2 on an engine whose only further set came from a coloured init replays the level-3 set:
        // code 0 is row 0 of the table, the same values from the kernels that load their coefficients. A snapshot of an
        // engine with any further set says "any graphs": its import captures the level-1 set, as it always did)
        int level = ps.any_layout;
        while (level > 0 && level + 1 < PIX_LEVELS && !graphs[level][ps.tier].exec) ++level;
        const PassGraph& g = graphs[level][ps.tier];
        if (!ps.any_layout && !g.exec)   // not reached after a successful creation (capture_all_graphs); kept as the safe path
            if (int rc = capture_graph(ps.tier, 0)) return rc;
        // passes with another format replay the graphs captured when a stream was initialised on one; without them
        // (every stream was initialised on RGB8 / NV12 / YUY2) the pass launches eagerly: no capture inside an update
        if (g.exec) {
            HIPCHK(hipGraphLaunch(g.exec, stream));
            graph_replays[ps.tier] += 1;
            return VT_OK;
        }
    }
    return run_pass(nullptr, ps);
}

int Engine::wait(vt_result* out, int n) {
    if (n > pass_n) n = pass_n;         // the results of the last pass, in its slot order
    DEVICE_SCOPE(device);
    HIPCHK(hipStreamSynchronize(stream));
    if (out)
        for (int b = 0; b < n; ++b) out[b] = h_results[b];
    if (host_seq == host_collected) {               // no pipelined pass owns the stream states
        for (int b = 0; b < B; ++b) known[b] = h_states_all[b];
        for (int b = 0; b < B && motion_capable; ++b) known_motion[(size_t)b] = h_motion_all[b];
        peaks_n = pass_n;                           // h_peaks holds the records of the pass just waited for
    }
    return VT_OK;
}

// ---- candidate passes --------------------------------------------------------------------------------

int check_state_box(const float* box4) {
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(box4[k])) return set_err(VT_ERR_INVALID_ARG, "state box: non-finite value");
    if (!(box4[2] >= 1.0f) || !(box4[3] >= 1.0f) || box4[2] > 32768.0f || box4[3] > 32768.0f ||
        fabsf(box4[0]) > 65536.0f || fabsf(box4[1]) > 65536.0f)
        return set_err(VT_ERR_INVALID_ARG, "state box %g,%g %gx%g out of range", box4[0], box4[1],
                       box4[2], box4[3]);
    return VT_OK;
}

int Engine::ensure_candidate_buffers() {
    if (h_winner) return VT_OK;
    if (!d_cand_states) HIPCHK(dalloc0(&d_cand_states, (size_t)B, stream));
    if (!d_cands) HIPCHK(dalloc0(&d_cands, (size_t)B, stream));
    if (!d_winner) HIPCHK(dalloc0(&d_winner, (size_t)B, stream));
    if (!h_cands) HIPCHK(hipHostMalloc((void**)&h_cands, sizeof(vt_candidate) * (size_t)B * RING));
    HIPCHK(hipHostMalloc((void**)&h_winner, sizeof(int32_t) * (size_t)B));
    memset(h_winner, 0, sizeof(int32_t) * (size_t)B);
    return VT_OK;
}

int Engine::check_candidates(const vt_candidate* cands, int n) const {
    if (!cands) return set_err(VT_ERR_INVALID_ARG, "null candidate list");
    if (n < 1 || n > B) return set_err(VT_ERR_INVALID_ARG, "pass over %d candidate slots: need 1..%d", n, B);
    for (int i = 0; i < n; ++i) {
        const int s = cands[i].stream;
        if (s < 0 || s >= B) return set_err(VT_ERR_INVALID_ARG, "cands[%d].stream = %d out of range (0..%d)", i, s, B - 1);
        if (cands[i].has_box)
            if (int rc = check_state_box(cands[i].box)) return rc;
    }
    for (int i = 0; i < n; ++i)
        if (!h_initialized[cands[i].stream])
            return set_err(VT_ERR_NOT_INITIALIZED, "stream %d: update before init", cands[i].stream);
    return VT_OK;
}

// every stream once and no slot with a box: the list is a subset pass over `streams`
bool Engine::plain_list(const vt_candidate* cands, int n, std::vector<int32_t>* streams) {
    streams->assign((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        if (cands[i].has_box) return false;
        for (int j = 0; j < i; ++j)
            if (cands[j].stream == cands[i].stream) return false;
        (*streams)[(size_t)i] = cands[i].stream;
    }
    return true;
}

int Engine::enqueue_candidates(const vt_candidate* cands, const vt_frame* frames, int n) {
    if (int rc = check_candidates(cands, n)) return rc;
    if (!frames) return set_err(VT_ERR_INVALID_ARG, "null frames");
    for (int i = 0; i < n; ++i)
        if (int rc = check_frame(frames[i])) return rc;
    std::vector<int32_t> streams;
    if (plain_list(cands, n, &streams)) return enqueue(streams.data(), frames, n);
    for (int i = 0; i < n; ++i) streams[(size_t)i] = cands[i].stream;
    DEVICE_SCOPE(device);
    if (int rc = ensure_candidate_buffers()) return rc;
    // the template gather keeps the slot -> stream map; the decode stores results by slot and NO state to the host:
    // only the commit kernel writes by-stream copies
    const int slot = ring_pos;      // the ring position build_block takes and waits for: the list's copy shares it
    PassShape ps;
    if (int rc = build_block(streams.data(), frames, n, nullptr, false, &ps)) return rc;
    vt_candidate* hc = h_cands + (size_t)slot * B;
    std::copy(cands, cands + n, hc);
    HIPCHK(hipMemcpyAsync(d_cands, hc, sizeof(vt_candidate) * (size_t)n, hipMemcpyHostToDevice, stream));
    HIPCHK(hipEventRecord(ring_ev[slot], stream));      // the position's event again: now behind the list's copy too
    const CandArgs ca{d_cands, d_states, d_cand_states, d_results, d_winner, h_states_all, h_winner, n};
    ps.cand = &ca;
    segments_moved = true;          // the next full pass restores every stream's template rows
    cand_pending = true;
    ps.tier = pick_crop_tier(cands, n);
    return run_pass(nullptr, ps);
}

int Engine::wait_candidates(vt_result* out, int32_t* winner, int n) {
    if (int rc = wait(out, n)) return rc;
    if (cand_pending) {             // the winner table of the commit kernel; slot_of reads a stream's winning slot from now on
        pass_winner.assign(h_winner, h_winner + pass_n);
        cand_pending = false;
    }
    if (winner)
        for (int i = 0; i < std::min(n, pass_n); ++i) winner[i] = pass_winner.empty() ? i : pass_winner[(size_t)i];
    return VT_OK;
}

// ---- construction ----------------------------------------------------------------------------------

size_t nv12_bytes_read(size_t w, size_t h) {      // bytes the full-frame converter reads of a packed NV12 buffer
    if (!w || !h) return 0;
    const size_t uv_rows = (h + 1) / 2;
    const size_t last = (uv_rows - 1) * w + ((w & 1) ? w : w - 1);
    return w * h + last + 1;
}

int read_file(const char* path, std::vector<uint8_t>* out) {
    FILE* f = fopen(path, "rb");
    if (!f) return set_err(VT_ERR_IO, "cannot open weights file '%s'", path);
    fseek(f, 0, SEEK_END);
    long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (sz <= 0) { fclose(f); return set_err(VT_ERR_IO, "weights file '%s' is empty", path); }
    out->resize((size_t)sz);
    size_t got = fread(out->data(), 1, (size_t)sz, f);
    fclose(f);
    if (got != (size_t)sz) return set_err(VT_ERR_IO, "short read on '%s'", path);
    return VT_OK;
}

int check_device(int device_id) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return set_err(VT_ERR_NO_DEVICE, "no HIP device visible (%s); this library has no CPU path",
                       e == hipSuccess ? "count 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= n)
        return set_err(VT_ERR_NO_DEVICE, "device %d out of range (have %d)", device_id, n);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess)
        return set_err(VT_ERR_NO_DEVICE, "cannot query device %d", device_id);
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_err(VT_ERR_NO_DEVICE, "device %d is %s; kernels are built for gfx950 only",
                       device_id, prop.gcnArchName);
    return VT_OK;
}

int make_engine(const char* path, const void* d_src, size_t bytes, int device_id,
                       const vt_config* cfg, int B, Engine** out) {
    if (!out) return set_err(VT_ERR_INVALID_ARG, "null output handle");
    *out = nullptr;
    if (B < 1 || B > VT_MAX_STREAMS)
        return set_err(VT_ERR_INVALID_ARG, "n_streams %d out of range (1..%d)", B, VT_MAX_STREAMS);
    if (int rc = check_device(device_id)) return rc;
    DEVICE_SCOPE(device_id);
    HIPCHK(gemm_prepare()); HIPCHK(attention_prepare()); HIPCHK(headconv_prepare());
    Engine* e = new (std::nothrow) Engine();
    if (!e) return set_err(VT_ERR_OOM, "out of host memory");
    e->device = device_id;
    e->B = B;
    int rc = VT_OK;
    do {
        hipError_t he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
        if (he != hipSuccess) { rc = set_err(VT_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(he)); break; }
        if (path) {
            std::vector<uint8_t> blob;
            if ((rc = read_file(path, &blob))) break;
            if ((rc = e->load_blob_host(blob))) break;
        } else {
            if ((rc = e->load_blob_device(d_src, bytes))) break;
        }
        e->success_threshold = e->d.success_threshold;
        if (cfg && cfg->struct_size >= sizeof(vt_config)) {
            if (cfg->success_threshold >= 0.0f) e->success_threshold = cfg->success_threshold;
            e->use_graph = cfg->use_graph != 0;
            if (cfg->max_frame_width > 0) e->max_w = cfg->max_frame_width;
            if (cfg->max_frame_height > 0) e->max_h = cfg->max_frame_height;
            if (cfg->max_device_mib > 0) e->max_device_bytes = (size_t)cfg->max_device_mib << 20;
            if (cfg->host_window_margin_pct > 0) e->margin = std::min(cfg->host_window_margin_pct, 400) / 100.0f;
            else if (cfg->host_window_margin_pct < 0) e->margin = 0.0f;
            e->host_zero_copy = cfg->host_zero_copy;
        }
        if ((rc = e->alloc_buffers())) break;
        // which head: the band kernel only where the planner finds a band height for all three layer kinds
        e->head_band_ok = headconv_plannable(e->d.gs, e->d.C, e->d.C, e->d.D, false, false) &&
                          headconv_plannable(e->d.gs, e->d.C, e->d.C, 9 * e->d.C, true, false) &&
                          headconv_plannable(e->d.gs, e->d.C, e->d.C, 9 * e->d.C, true, true);
        if ((rc = e->capture_all_graphs())) break;
    } while (0);
    if (rc != VT_OK) {
        char keep[512];
        memcpy(keep, g_err, sizeof(keep));
        delete e;
        memcpy(g_err, keep, sizeof(keep));
        return rc;
    }
    *out = e;
    return VT_OK;
}

void fill_info(const Engine* e, vt_model_info* o) {
    memset(o, 0, sizeof(*o));
    const ModelDims& d = e->d;
    o->patch = d.patch; o->template_size = d.T; o->search_size = d.S; o->dim = d.D;
    o->heads = d.H; o->layers = d.L; o->mlp_dim = d.mlp; o->head_channels = d.C;
    o->tokens_template = d.nt; o->tokens_search = d.ns; o->kpad = d.kpad; o->score_grid = d.gs;
    o->encoder_flops_per_frame = e->flops_encoder();
    o->flops_per_frame = e->flops_encoder() + e->flops_head();
    o->weight_bytes = e->blob_bytes;
}
