// vt_features.hip — host side of the ten optional in-the-pass features of an Engine
#include "vt_engine.hpp"

// ---- the first enable of an optional feature -------------------------------------------------------------

// The one transaction (vt_engine.hpp: Feature). The captured passes are those of an engine without the feature: they
// are dropped and captured again, as vt_group_set_tuning does.
int Engine::enable_feature(const Feature& f) {
    DEVICE_SCOPE(device);
    HIPCHK(hipStreamSynchronize(stream));
    const double mib = f.extra / 1048576.0;
    if (max_device_bytes && activation_bytes() + blob_bytes + feature_bytes() + f.extra > max_device_bytes)
        return set_err(VT_ERR_OOM, "%s: needs %.3f MiB more HBM; vt_config.max_device_mib allows %.1f in all", f.name, mib,
                       max_device_bytes / 1048576.0);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && f.extra > free_b)
        return set_err(VT_ERR_OOM, "%s: needs %.3f MiB more HBM; %.1f MiB are free", f.name, mib, free_b / 1048576.0);
    hipError_t he = f.alloc();
    if (he == hipSuccess) he = hipStreamSynchronize(stream);    // the fills and copies have landed
    if (he != hipSuccess) {
        f.uninstall();
        return set_err(he == hipErrorOutOfMemory ? VT_ERR_OOM : VT_ERR_HIP, "%s: %s", f.name, hipGetErrorString(he));
    }
    f.install();
    drop_graphs();
    if (int rc = capture_all_graphs()) {
        char keep[512];
        memcpy(keep, vt_err_text(), sizeof(keep));
        drop_graphs();
        f.uninstall();
        (void)capture_all_graphs();     // the passes the engine had; should that fail too, enqueue() captures on demand
        memcpy(vt_err_text(), keep, sizeof(keep));
        return rc;
    }
    if (f.commit) f.commit();
    return VT_OK;
}

// ---- the optional sinks: ONE list --------------------------------------------------------------------
// A row per optional member of PassOut: bit, element size, by stream (peak records: by slot - adopt_peaks, peaks_n), where
// it is in a record and in the engine (its own mirror), the feature's capable flag. By stream, behind the brace: the device
// records [B] (the feature's store, their offset in it), the events that zero them (the table of DESIGN.md section 3, cell by
// cell - proposals are not reset by an import) and, for motion, the host's second copy beside `known`.
struct Sink {
    unsigned bit; size_t elem; bool by_stream; void* PassOut::*in; void* Engine::*own; bool Engine::*capable;
    struct Recs { uint8_t* Engine::*store; size_t (Engine::*off)() const; unsigned resets; std::vector<MotionRec> Engine::*known; } recs;
};
static const Sink kSinks[] = {      // the casts: every member is a pointer to records of elem bytes
    {Engine::SINK_PEAKS, sizeof(vt_peaks), false, (void* PassOut::*)&PassOut::host_peaks, (void* Engine::*)&Engine::h_peaks, &Engine::peaks_capable},
    {Engine::SINK_MOTION, sizeof(MotionRec), true, (void* PassOut::*)&PassOut::host_motion, (void* Engine::*)&Engine::h_motion_all, &Engine::motion_capable,
     {&Engine::d_motion, &Engine::motion_off_recs, Engine::RESET_INIT | Engine::RESET_IMPORT | Engine::RESET_BOX | Engine::RESET_OFF, &Engine::known_motion}},
    {Engine::SINK_APPEAR, sizeof(AppearRec), true, (void* PassOut::*)&PassOut::host_appearance, (void* Engine::*)&Engine::h_appear_all, &Engine::appear_capable,
     {&Engine::d_appear, &Engine::appear_off_recs, Engine::RESET_INIT | Engine::RESET_IMPORT | Engine::RESET_ACTION}},
    {Engine::SINK_PROP, sizeof(PropRec), true, (void* PassOut::*)&PassOut::host_proposals, (void* Engine::*)&Engine::h_prop_all, &Engine::prop_capable,
     {&Engine::d_prop, &Engine::prop_off_recs, Engine::RESET_INIT}},
    {Engine::SINK_CONFLICT, sizeof(ConflictRec), true, (void* PassOut::*)&PassOut::host_conflicts, (void* Engine::*)&Engine::h_conflict_all, &Engine::conflict_capable,
     {&Engine::d_conflict, &Engine::conflict_off_recs, Engine::RESET_INIT | Engine::RESET_IMPORT | Engine::RESET_BOX | Engine::RESET_ACTION}},
    {Engine::SINK_HEALTH, sizeof(HealthRec), true, (void* PassOut::*)&PassOut::host_health, (void* Engine::*)&Engine::h_health_all, &Engine::health_capable,
     {&Engine::d_health, &Engine::health_off_recs, Engine::RESET_INIT | Engine::RESET_IMPORT | Engine::RESET_OFF}},       // the record holds has_prev and still: no previous thumbnail
    {Engine::SINK_ARB, sizeof(ArbRec), true, (void* PassOut::*)&PassOut::host_arbitrate, (void* Engine::*)&Engine::h_arb_all, &Engine::arb_capable,
     {&Engine::d_arb, &Engine::arb_off_recs, Engine::RESET_INIT | Engine::RESET_IMPORT | Engine::RESET_OFF}},
};

int Engine::reset_records(unsigned event, int first, int last, unsigned of) {
    const size_t n = (size_t)(last - first);
    for (const Sink& s : kSinks) {
        if (!(s.bit & of) || !(s.recs.resets & event) || !(this->*s.capable)) continue;
        HIPCHK(hipMemsetAsync(this->*s.recs.store + (this->*s.recs.off)() + s.elem * (size_t)first, 0, s.elem * n, stream));
        memset((char*)(this->*s.own) + s.elem * (size_t)first, 0, s.elem * n);
        if (s.recs.known) std::fill_n((this->*s.recs.known).begin() + first, n, MotionRec{});
    }
    return VT_OK;
}

static hipError_t pinned0(void** p, size_t bytes) {
    if (*p) return hipSuccess;
    hipError_t e = hipHostMalloc(p, bytes);
    if (e == hipSuccess) memset(*p, 0, bytes);
    return e;
}
static void unpin(void** p) { if (*p) (void)hipHostFree(*p); *p = nullptr; }

hipError_t Engine::sinks_alloc(PassOut* o, unsigned members) const {
    hipError_t e = hipSuccess;
    if (members & SINK_BASE) e = pinned0((void**)&o->host_results, sizeof(vt_result) * (size_t)B);
    if (e == hipSuccess && (members & SINK_BASE)) e = pinned0((void**)&o->host_states, sizeof(StreamState) * (size_t)B);
    for (const Sink& s : kSinks)
        if (e == hipSuccess && (members & s.bit)) e = pinned0(&(o->*s.in), s.elem * (size_t)B);
    return e;
}

void Engine::sinks_free(PassOut* o, unsigned members) const {
    if (members & SINK_BASE) { unpin((void**)&o->host_results); unpin((void**)&o->host_states); }
    for (const Sink& s : kSinks)
        if (members & s.bit) unpin(&(o->*s.in));
}

unsigned Engine::sink_members() const {
    unsigned m = SINK_BASE;
    for (const Sink& s : kSinks) m |= this->*s.capable ? s.bit : 0u;
    return m;
}

PassOut Engine::pass_sinks(const PassOut* to, bool by_stream_states) const {
    PassOut o{to ? to->host_results : h_results, !by_stream_states ? nullptr : to ? to->host_states : h_states_all, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (const Sink& s : kSinks)
        if (this->*s.capable) o.*s.in = to ? to->*s.in : this->*s.own;
    return o;
}

void Engine::adopt_stream_sinks(PassOut from, int stream) {
    for (const Sink& s : kSinks)
        if (s.by_stream && this->*s.capable && from.*s.in)
            memcpy((char*)(this->*s.own) + s.elem * (size_t)stream, (const char*)(from.*s.in) + s.elem * (size_t)stream, s.elem);
}

int Engine::enable_store(const char* name, size_t bytes, size_t zeroed, const void* policy, size_t policy_bytes, unsigned sink,
                         hipError_t (*fill)(Engine*, uint8_t*), const std::function<void(uint8_t*)>& wire) {
    uint8_t* store = nullptr; PassOut own{};        // own: the engine's own mirror
    auto alloc = [&] {
        hipError_t he = hipMalloc((void**)&store, bytes);
        if (he == hipSuccess) he = hipMemsetAsync(store, 0, zeroed, stream);
        if (he == hipSuccess && policy) he = hipMemcpyAsync(store, policy, policy_bytes, hipMemcpyHostToDevice, stream);
        if (he == hipSuccess && fill) he = fill(this, store);
        if (he == hipSuccess) he = sinks_alloc(&own, sink);
        for (HostSlot& sl : hs)     // pipelined slots that exist already: here, so that no pass allocates pinned memory for them
            if (he == hipSuccess && sl.out.host_results) he = sinks_alloc(&sl.out, sink);
        return he;
    };
    auto mirrors = [&] {
        for (const Sink& s : kSinks)
            if (s.bit & sink) this->*s.own = own.*s.in;
    };
    auto install = [&] { mirrors(); wire(store); };
    auto uninstall = [&] {
        (void)hipFree(store);       // null: no operation
        sinks_free(&own, sink);
        mirrors();                  // null again
        for (HostSlot& sl : hs) sinks_free(&sl.out, sink);
        wire(nullptr);
    };
    return enable_feature({name, bytes, alloc, install, uninstall, nullptr});
}

// ---- template refresh --------------------------------------------------------------------------------

int Engine::reset_refresh_tickets() {
    if (d_tickets) HIPCHK(hipMemsetAsync(d_tickets, 0, sizeof(unsigned) * (size_t)B, stream));
    if (appear_capable) HIPCHK(hipMemsetAsync(d_appear_tickets(), 0, sizeof(unsigned) * (size_t)B, stream));
    if (arb_capable) HIPCHK(hipMemsetAsync(d_arb_tickets(), 0, sizeof(unsigned) * VT_ARB_MAX * (size_t)B, stream));
    return VT_OK;
}

// The first enabled policy: the store grows to two buffers per stream (buffer tpl_gen & 1 = the stream's rows), policy
// array and tickets are allocated. The old store is kept until the new passes exist: a failed capture puts it back.
int Engine::enable_refresh() {
    if (refresh_capable) return VT_OK;
    const size_t rows = (size_t)d.nt * d.kpad;
    bf16_t *tpl2 = nullptr, *const tpl1 = d_tpl;
    RefreshPolicy* pol = nullptr;
    unsigned* tick = nullptr;
    const bool moved = segments_moved;
    auto alloc = [&] {
        std::vector<StreamState> sts((size_t)B);     // before the device allocations: may throw
        hipError_t he = dalloc0(&tpl2, 2 * rows * (size_t)B, stream);
        if (he == hipSuccess) he = dalloc0(&pol, (size_t)B, stream);
        if (he == hipSuccess) he = dalloc0(&tick, (size_t)B, stream);
        if (he == hipSuccess)
            he = hipMemcpy2DAsync(tpl2, 2 * rows * sizeof(bf16_t), tpl1, rows * sizeof(bf16_t), rows * sizeof(bf16_t),
                                  (size_t)B, hipMemcpyDeviceToDevice, stream);
        // a stream that was imported (vt_snapshot.hip) may carry an odd tpl_gen in this single-buffer engine: its current rows
        // belong into buffer tpl_gen & 1 of the new store, where every reader will look for them (buffer 0 keeps a copy)
        if (he == hipSuccess) he = hipMemcpyAsync(sts.data(), d_states, sizeof(StreamState) * (size_t)B, hipMemcpyDeviceToHost, stream);
        if (he == hipSuccess) he = hipStreamSynchronize(stream);
        for (int b = 0; b < B && he == hipSuccess; ++b)
            if (sts[(size_t)b].tpl_gen & 1)
                he = hipMemcpyAsync(tpl2 + ((size_t)b * 2 + 1) * rows, tpl1 + (size_t)b * rows, rows * sizeof(bf16_t),
                                    hipMemcpyDeviceToDevice, stream);
        return he;
    };
    auto install = [&] {
        d_tpl = tpl2; d_policy = pol; d_tickets = tick;
        refresh_capable = true;
        segments_moved = false;
    };
    auto uninstall = [&] {
        d_tpl = tpl1; d_policy = nullptr; d_tickets = nullptr;
        refresh_capable = false;
        segments_moved = moved;
        (void)hipFree(tpl2); (void)hipFree(pol); (void)hipFree(tick);     // null: no operation
    };
    return enable_feature({"template refresh", refresh_bytes(), alloc, install, uninstall, [&] { (void)hipFree(tpl1); }});
}

int Engine::set_refresh(int s, int period, float min_score) {
    if (s < -1 || s >= B) return set_err(VT_ERR_INVALID_ARG, "template refresh: stream %d out of range (-1..%d)", s, B - 1);
    if (period < 0 || period == 1 || period > VT_REFRESH_MAX_PERIOD)
        return set_err(VT_ERR_INVALID_ARG, "template refresh: period %d (0 = off, else 2..%d)", period, VT_REFRESH_MAX_PERIOD);
    if (!std::isfinite(min_score) || min_score < 0.0f || min_score > 1.0f)
        return set_err(VT_ERR_INVALID_ARG, "template refresh: min_score must be finite and in 0..1");
    if (period > 0)
        if (int rc = enable_refresh()) return rc;
    const int s0 = s < 0 ? 0 : s, s1 = s < 0 ? B : s + 1;
    if (refresh_capable) {      // period and min_score only: the diagnostic counter behind them is the device's
        DEVICE_SCOPE(device);
        HIPCHK(hipStreamSynchronize(stream));
        for (int b = s0; b < s1; ++b) {
            const RefreshPolicy p{period, min_score, 0, 0};
            HIPCHK(hipMemcpy(d_policy + b, &p, 2 * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        if (int rc = reset_refresh_tickets()) return rc;
        HIPCHK(hipStreamSynchronize(stream));
    }
    for (int b = s0; b < s1; ++b) { h_policy[(size_t)b].period = period; h_policy[(size_t)b].min_score = min_score; }
    return VT_OK;
}

int Engine::refresh_stats(int s, vt_refresh_stats* out) {
    if (!out) return set_err(VT_ERR_INVALID_ARG, "null argument");
    if (s < 0 || s >= B) return set_err(VT_ERR_INVALID_ARG, "template refresh: stream %d out of range (0..%d)", s, B - 1);
    DEVICE_SCOPE(device);
    HIPCHK(hipStreamSynchronize(stream));
    memset(out, 0, sizeof(*out));
    out->period = h_policy[(size_t)s].period;
    out->min_score = h_policy[(size_t)s].min_score;
    if (refresh_capable) {
        RefreshPolicy p{};
        HIPCHK(hipMemcpy(&p, d_policy + s, sizeof(p), hipMemcpyDeviceToHost));
        out->skipped_geometry = p.skipped_geometry;
    }
    StreamState st{};
    HIPCHK(hipMemcpy(&st, d_states + s, sizeof(st), hipMemcpyDeviceToHost));
    out->generation = st.tpl_gen;
    out->last_frame = st.tpl_frame;
    return VT_OK;
}

// ---- target chips ------------------------------------------------------------------------------------

// The first enable allocates the store (enable_feature). A second enable with the same parameters is a no-op.
int Engine::enable_chips(int size, int kind, const float* na, const float* nb) {
    if (size < 32 || size > 512 || size % 8 != 0)
        return set_err(VT_ERR_INVALID_ARG, "chips: size %d (a multiple of 8 in 32..512)", size);
    if (kind != VT_CHIP_NORM_BF16 && kind != VT_CHIP_RGB8) return set_err(VT_ERR_INVALID_ARG, "chips: unknown kind %d", kind);
    float a3[3] = {1.0f, 1.0f, 1.0f}, b3[3] = {0.0f, 0.0f, 0.0f};
    if (kind == VT_CHIP_NORM_BF16) {
        if (!na || !nb) return set_err(VT_ERR_INVALID_ARG, "chips: the bf16 kind needs norm_a and norm_b");
        for (int c = 0; c < 3; ++c) {
            if (!std::isfinite(na[c]) || !std::isfinite(nb[c])) return set_err(VT_ERR_INVALID_ARG, "chips: norms must be finite");
            a3[c] = na[c]; b3[c] = nb[c];
        }
    }
    if (chip_capable) {
        if (size != chip_size || kind != chip_kind || memcmp(a3, chip_na, sizeof(a3)) != 0 || memcmp(b3, chip_nb, sizeof(b3)) != 0)
            return set_err(VT_ERR_INVALID_ARG, "chips: the engine's chips are fixed at size %d, kind %d and the norms of the "
                           "first enable", chip_size, chip_kind);
        return VT_OK;
    }
    const size_t cb = chip_bytes_of(size, kind);
    uint8_t* chips = nullptr;       // one allocation: [B][cb] chips | [B] infos (cb is a multiple of 192: the infos are aligned)
    ChipPolicy* pol = nullptr;
    auto alloc = [&] {
        hipError_t he = dalloc0(&chips, (cb + sizeof(vt_chip_info)) * (size_t)B, stream);
        return he == hipSuccess ? dalloc0(&pol, (size_t)B, stream) : he;
    };
    auto install = [&] {
        d_chips = chips; d_chip_infos = reinterpret_cast<vt_chip_info*>(chips + cb * (size_t)B); d_chip_policy = pol;
        chip_size = size; chip_kind = kind;
        memcpy(chip_na, a3, sizeof(a3)); memcpy(chip_nb, b3, sizeof(b3));
        chip_capable = true;
    };
    auto uninstall = [&] {
        (void)hipFree(chips); (void)hipFree(pol);       // null: no operation
        d_chips = nullptr; d_chip_infos = nullptr; d_chip_policy = nullptr;
        chip_capable = false;
        chip_size = chip_kind = 0;
    };
    return enable_feature({"chips", chip_store_bytes_of(B, size, kind), alloc, install, uninstall});
}

int Engine::set_chips(int s, float factor, int period, int phase) {
    if (!chip_capable) return set_err(VT_ERR_INVALID_ARG, "chips: not enabled on this engine (vt_group_enable_chips)");
    if (s < -1 || s >= B) return set_err(VT_ERR_INVALID_ARG, "chips: stream %d out of range (-1..%d)", s, B - 1);
    if (!(factor == 0.0f || (factor >= 0.5f && factor <= 4.0f)))     // a NaN fails both
        return set_err(VT_ERR_INVALID_ARG, "chips: factor must be 0 (off) or in 0.5..4");
    if (period < 1 || period > VT_CHIP_MAX_PERIOD)
        return set_err(VT_ERR_INVALID_ARG, "chips: period %d (1..%d)", period, VT_CHIP_MAX_PERIOD);
    if (phase < 0 || phase >= period) return set_err(VT_ERR_INVALID_ARG, "chips: phase %d (0..period-1 = %d)", phase, period - 1);
    DEVICE_SCOPE(device);
    HIPCHK(hipStreamSynchronize(stream));
    const ChipPolicy p{factor == 0.0f ? 0.0f : factor, period, phase, 0};
    for (int b = s < 0 ? 0 : s; b < (s < 0 ? B : s + 1); ++b)
        HIPCHK(hipMemcpy(d_chip_policy + b, &p, sizeof(p), hipMemcpyHostToDevice));
    return VT_OK;
}

// behind every queued pass on the group's stream: ONE device-to-host copy of the store's bytes from the first listed
// stream's chip (infos only: info) to the last listed stream's info (chips only: chip) into the pinned mirror, then handed out
int Engine::read_chips(const int* streams, int n, void* out, size_t out_stride, vt_chip_info* infos) {
    if (!chip_capable) return set_err(VT_ERR_INVALID_ARG, "chips: not enabled on this engine (vt_group_enable_chips)");
    const size_t cb = chip_bytes(), ib = sizeof(vt_chip_info), info0 = (size_t)B * cb;
    if (n < 1 || n > B || (out && out_stride < cb) || (!out && !infos))
        return set_err(VT_ERR_INVALID_ARG, "read_chips: bad count, stride or no output");
    int lo = B, hi = -1;
    for (int i = 0; i < n; ++i) {
        const int s = streams ? streams[i] : i;
        if (s < 0 || s >= B) return set_err(VT_ERR_INVALID_ARG, "read_chips: stream %d out of range (0..%d)", s, B - 1);
        lo = std::min(lo, s); hi = std::max(hi, s);
    }
    DEVICE_SCOPE(device);
    if (!h_chip_stage) HIPCHK(hipHostMalloc((void**)&h_chip_stage, (size_t)B * (cb + ib), hipHostMallocDefault));
    const size_t from = out ? (size_t)lo * cb : info0 + (size_t)lo * ib;
    const size_t to = infos ? info0 + (size_t)(hi + 1) * ib : (size_t)(hi + 1) * cb;
    HIPCHK(hipMemcpyAsync(h_chip_stage + from, d_chips + from, to - from, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (int i = 0; i < n; ++i) {
        const int s = streams ? streams[i] : i;
        if (out) memcpy((uint8_t*)out + (size_t)i * out_stride, h_chip_stage + (size_t)s * cb, cb);
        if (infos) memcpy(infos + i, h_chip_stage + info0 + (size_t)s * ib, ib);
    }
    return VT_OK;
}

// ---- response peaks ----------------------------------------------------------------------------------

// The policy of stream s (-1: all). The first policy with max_peaks > 0 allocates the records, the policies and the
// pinned mirrors (enable_feature).
int Engine::set_peaks(int s, int max_peaks, int radius, float min_resp) {
    if (s < -1 || s >= B) return set_err(VT_ERR_INVALID_ARG, "peaks: stream %d out of range (-1..%d)", s, B - 1);
    if (max_peaks < 0 || max_peaks > VT_PEAKS_MAX)
        return set_err(VT_ERR_INVALID_ARG, "peaks: max_peaks %d (0: off, else 1..%d)", max_peaks, VT_PEAKS_MAX);
    if (radius < 1 || radius > 4) return set_err(VT_ERR_INVALID_ARG, "peaks: radius %d (1..4)", radius);
    if (!(min_resp >= 0.0f && min_resp <= 1.0f))       // a NaN fails both
        return set_err(VT_ERR_INVALID_ARG, "peaks: min_resp must be finite in 0..1");
    if (!peaks_capable && max_peaks == 0)
        return set_err(VT_ERR_INVALID_ARG, "peaks: not enabled on this engine (a policy with max_peaks > 0 enables it)");
    DEVICE_SCOPE(device);
    HIPCHK(hipStreamSynchronize(stream));
    if (!peaks_capable) {
        peaks_policy.reserve((size_t)B);        // may throw: before anything is allocated on the device
        auto wire = [&](uint8_t* store) {       // the store: [B] records | [B] policies, all zero (every policy off)
            d_peaks = reinterpret_cast<vt_peaks*>(store);
            d_peaks_policy = store ? reinterpret_cast<PeaksPolicy*>(store + sizeof(vt_peaks) * (size_t)B) : nullptr;
            peaks_policy.assign(store ? (size_t)B : 0, PeaksPolicy{0, 0, 0.0f, 0});
            if (store) peaks_n = 0;
            peaks_capable = store != nullptr;
        };
        if (int rc = enable_store("peaks", peaks_bytes(), peaks_bytes(), nullptr, 0, SINK_PEAKS, nullptr, wire)) return rc;
    }
    const PeaksPolicy p{max_peaks, radius, min_resp == 0.0f ? 0.0f : min_resp, 0};
    for (int b = s < 0 ? 0 : s; b < (s < 0 ? B : s + 1); ++b) {
        HIPCHK(hipMemcpy(d_peaks_policy + b, &p, sizeof(p), hipMemcpyHostToDevice));
        peaks_policy[(size_t)b] = p;
    }
    return VT_OK;
}

int Engine::last_peaks(vt_peaks* out, int n) const {
    if (!peaks_capable) return set_err(VT_ERR_INVALID_ARG, "peaks: not enabled on this engine (vt_group_set_peaks)");
    if (!out || n < 1) return set_err(VT_ERR_INVALID_ARG, "last_peaks: null output or n < 1");
    for (int i = 0; i < std::min(n, peaks_n); ++i) out[i] = h_peaks[i];
    return VT_OK;
}

// ---- result overlay ----------------------------------------------------------------------------------

// [6]: flags, drawn by the stream's last pass, passes drawn / gated / on a format that is not drawable, N of the last label
int Engine::overlay_stats(int s, float* out6) {
    OverlayStats st{};
    HIPCHK(hipMemcpy(&st, d_overlay_stats() + s, sizeof(st), hipMemcpyDeviceToHost));
    out6[0] = (float)overlay_policy.flags; out6[1] = (float)st.drawn_last; out6[2] = (float)st.n_drawn;
    out6[3] = (float)st.n_gated; out6[4] = (float)st.n_unsupported; out6[5] = (float)st.last_n;
    return VT_OK;
}

// ---- motion prior ------------------------------------------------------------------------------------

void Engine::predicted_box(int s, float* box4, int steps) const {
    const StreamState& k = known[(size_t)s];
    memcpy(box4, k.box, 4 * sizeof(float));
    for (int i = 0; i < steps && motion_capable; ++i) {
        float from[4];
        memcpy(from, box4, sizeof(from));
        if (!motion_predict(motion_policy.on, from, known_motion[(size_t)s].v, k.frame_w, k.frame_h, box4)) break;
    }
}

// [8]: the engine flag, vx, vy, live, the shift of the stream's last pass, passes with a shift, failed updates that advanced
int Engine::motion_stats(int s, float* out8) {
    MotionRec r{};
    HIPCHK(hipMemcpy(&r, d_motion_recs() + s, sizeof(r), hipMemcpyDeviceToHost));
    out8[0] = (float)motion_policy.on; out8[1] = r.v[0]; out8[2] = r.v[1]; out8[3] = (float)r.live;
    out8[4] = r.shift[0]; out8[5] = r.shift[1]; out8[6] = (float)r.n_shift; out8[7] = (float)r.n_coast;
    return VT_OK;
}

// ---- appearance check ---------------------------------------------------------------------------------

hipError_t Engine::anchor_from_template(int b, int gen) {
    if (!appear_capable) return hipSuccess;
    const bf16_t* rows = tpl_init_rows(b) + (refresh_capable ? (size_t)(gen & 1) * appear_rows() : 0);
    return hipMemcpyAsync(d_anchor(b), rows, sizeof(bf16_t) * appear_rows(), hipMemcpyDeviceToDevice, stream);
}

int Engine::appearance_anchor(int value) {
    if (!appear_capable)
        return set_err(VT_ERR_INVALID_ARG, "appearance_anchor: the check is not enabled on this engine (vt_group_set_tuning \"appearance\")");
    if (value < -1 || value >= B) return set_err(VT_ERR_INVALID_ARG, "appearance_anchor: stream %d (-1: all, else 0..%d)", value, B - 1);
    if (value >= 0 && !h_initialized[(size_t)value]) return set_err(VT_ERR_NOT_INITIALIZED, "appearance_anchor: stream %d not initialised", value);
    DEVICE_SCOPE(device);
    HIPCHK(hipStreamSynchronize(stream));
    std::vector<StreamState> sts((size_t)B);
    HIPCHK(hipMemcpy(sts.data(), d_states, sizeof(StreamState) * (size_t)B, hipMemcpyDeviceToHost));
    for (int b = value < 0 ? 0 : value; b < (value < 0 ? B : value + 1); ++b)
        if (h_initialized[(size_t)b]) {
            HIPCHK(anchor_from_template(b, sts[(size_t)b].tpl_gen));
            if (int rc = reset_records(RESET_ACTION, b, b + 1, SINK_APPEAR)) return rc;
        }
    HIPCHK(hipStreamSynchronize(stream));
    return VT_OK;
}

// the enable: the anchors of the streams that are initialised, from their current template rows
static hipError_t fill_anchors(Engine* e, uint8_t* store) {
    std::unique_ptr<StreamState[]> sts(new (std::nothrow) StreamState[(size_t)e->B]);     // no throw behind the device allocation
    if (!sts) return hipErrorOutOfMemory;
    hipError_t he = hipMemcpyAsync(sts.get(), e->d_states, sizeof(StreamState) * (size_t)e->B, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    bf16_t* anchors = reinterpret_cast<bf16_t*>(store + e->appear_off_anchor());
    const size_t rows = e->appear_rows();
    for (int b = 0; b < e->B && he == hipSuccess; ++b)
        if (e->h_initialized[(size_t)b])
            he = hipMemcpyAsync(anchors + (size_t)b * rows, e->tpl_init_rows(b) + (e->refresh_capable ? (size_t)(sts[(size_t)b].tpl_gen & 1) * rows : 0),
                                sizeof(bf16_t) * rows, hipMemcpyDeviceToDevice, e->stream);
    return he;
}

// [8]: the engine flag, the stream's record (status, similarity, frames_done), its counters (evaluated, gated), period, gate_pm
int Engine::appearance_stats(int s, float* out8) {
    // the record: the pinned mirror, i.e. that of the stream's last pass the HOST has collected (a pipelined pass still
    // running has written the device record already, and may yet be redone); the counters: the device's
    const AppearRec r = h_appear_all[s];
    AppearCount c{};
    HIPCHK(hipMemcpy(&c, d_appear_counts() + s, sizeof(c), hipMemcpyDeviceToHost));
    out8[0] = (float)appear_policy.on; out8[1] = (float)r.status; out8[2] = r.similarity; out8[3] = (float)r.frames_done;
    out8[4] = (float)c.evaluated; out8[5] = (float)c.gated; out8[6] = (float)appear_policy.period; out8[7] = (float)appear_policy.gate_pm;
    return VT_OK;
}

// ---- reacquire proposals ------------------------------------------------------------------------------

// [VT_PROP_STATS]: mode, status, frames_done, n, c, Wg, Hg, evaluated, period, max, min_sim_pm, max_cells, then per
// proposal sim, box[4], position
int Engine::proposals_stats(int s, float* out) {
    // the record: the pinned mirror, i.e. that of the stream's last pass the HOST has collected; the counter: the device's
    const PropRec r = h_prop_all[s];
    int32_t ev = 0;
    HIPCHK(hipMemcpy(&ev, d_prop_counts() + s, sizeof(ev), hipMemcpyDeviceToHost));
    out[0] = (float)prop_policy.mode; out[1] = (float)r.status; out[2] = (float)r.frames_done; out[3] = (float)r.n;
    out[4] = r.c; out[5] = (float)r.Wg; out[6] = (float)r.Hg; out[7] = (float)ev;
    out[8] = (float)prop_policy.period; out[9] = (float)prop_policy.max_n; out[10] = (float)prop_policy.min_sim_pm;
    out[11] = (float)prop_policy.max_cells;
    for (int k = 0; k < VT_PROP_MAX; ++k) {
        float* o = out + 12 + 6 * k;
        o[0] = r.p[k].sim; o[1] = r.p[k].box[0]; o[2] = r.p[k].box[1]; o[3] = r.p[k].box[2]; o[4] = r.p[k].box[3];
        o[5] = (float)r.p[k].pos;
    }
    return VT_OK;
}

// ---- stream conflicts ----------------------------------------------------------------------------------

int Engine::conflicts_scene(int value) {
    if (!conflict_capable)
        return set_err(VT_ERR_INVALID_ARG, "conflicts_scene: stream conflicts are not enabled on this engine (vt_group_set_tuning \"conflicts\")");
    int first = 0, last = 0;
    int32_t scene = 0;
    char text[256];
    if (vtkeys::decode_scene(value, B, &first, &last, &scene, text, sizeof(text)) != vtkeys::ACCEPTED)
        return set_err(VT_ERR_INVALID_ARG, "%s", text);
    std::vector<int32_t> now = conflict_scenes;     // may throw: before anything changes
    now.resize((size_t)B, 0);
    std::fill(now.begin() + first, now.begin() + last, scene);
    DEVICE_SCOPE(device);
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipMemcpy(d_conflict_scenes() + first, now.data() + first, sizeof(int32_t) * (size_t)(last - first), hipMemcpyHostToDevice));
    if (int rc = reset_records(RESET_ACTION, first, last, SINK_CONFLICT)) return rc;
    conflict_scenes.swap(now);
    return VT_OK;
}

// [16]: the engine flag, the stream's record (status, frames_done, n_over, partner[4], iou[4]), its counters (evaluated,
// conflicting, gated), its scene
int Engine::conflicts_stats(int s, float* out16) {
    // the record: the pinned mirror, i.e. that of the stream's last pass the HOST has collected; the counters: the device's
    const ConflictRec r = h_conflict_all[s];
    ConflictCount c{};
    HIPCHK(hipMemcpy(&c, d_conflict_counts() + s, sizeof(c), hipMemcpyDeviceToHost));
    out16[0] = (float)conflict_policy.on; out16[1] = (float)r.status; out16[2] = (float)r.frames_done; out16[3] = (float)r.n_over;
    for (int k = 0; k < VT_CONFLICT_MAX; ++k) { out16[4 + k] = (float)r.partner[k]; out16[8 + k] = r.iou[k]; }
    out16[12] = (float)c.evaluated; out16[13] = (float)c.conflicting; out16[14] = (float)c.gated;
    out16[15] = (float)(conflict_scenes.empty() ? 0 : conflict_scenes[(size_t)s]);
    return VT_OK;
}

// ---- frame health ------------------------------------------------------------------------------------

// [24], for people: mode, status, frames_done, flags, c, Wg, Hg, still, S1 / n, the standard deviation, D / n,
// HD * 1000 / (2 n), G * 1000 / G_ref, evaluated, flagged, gated, then period, cell, still_run, flat_q, cut_pm, gate, and two
// zeros. The exact integers: "health_words"
int Engine::health_stats(int s, float* out) {
    // the record: the pinned mirror, i.e. that of the stream's last pass the HOST has collected; the counters: the device's
    const HealthRec r = h_health_all[s];
    HealthCount c{};
    HIPCHK(hipMemcpy(&c, d_health_counts() + s, sizeof(c), hipMemcpyDeviceToHost));
    const double n = (double)r.Wg * r.Hg, mean = n > 0 ? r.S1 / n : 0.0, var = n > 0 ? r.S2 / n - mean * mean : 0.0;
    const float v[VT_HEALTH_STATS] = {(float)health_policy.on, (float)r.status, (float)r.frames_done, (float)r.flags, (float)r.c, (float)r.Wg,
                                      (float)r.Hg, (float)r.still, (float)mean, (float)sqrt(var > 0 ? var : 0.0), n > 0 ? (float)(r.D / n) : 0.0f,
                                      n > 0 ? (float)(r.HD * 1000.0 / (2.0 * n)) : 0.0f, r.G_ref > 0 ? (float)(r.G * 1000.0 / (double)r.G_ref) : 0.0f,
                                      (float)c.evaluated, (float)c.flagged, (float)c.gated, (float)health_policy.period, (float)health_policy.cell,
                                      (float)health_policy.still_run, (float)health_policy.flat_q, (float)health_policy.cut_pm, (float)health_policy.gate,
                                      0.0f, 0.0f};
    memcpy(out, v, sizeof(v));
    return VT_OK;
}

int Engine::health_words(int s, float* out) {
    uint32_t w[sizeof(HealthRec) / 4];
    memcpy(w, h_health_all + s, sizeof(w));
    for (size_t k = 0; k < sizeof(HealthRec) / 4; ++k) { out[2 * k] = (float)(w[k] & 0xFFFFu); out[2 * k + 1] = (float)(w[k] >> 16); }
    return VT_OK;
}

// ---- peak arbitration -----------------------------------------------------------------------------------

// [48]: the flag, status, frames_done, n, chosen, evaluated, switched, 0; then four peaks of cell, status, score, response,
// similarity, the float box x, y, w, h, 0. Every value is exact in binary32 (cells, counts and statuses are small integers)
int Engine::arbitrate_stats(int s, float* out) {
    // the record: the pinned mirror, i.e. that of the stream's last pass the HOST has collected; the counters: the device's
    const ArbRec r = h_arb_all[s];
    ArbCount c{};
    HIPCHK(hipMemcpy(&c, d_arb_counts() + s, sizeof(c), hipMemcpyDeviceToHost));
    float v[VT_ARB_STATS] = {(float)arb_policy.on, (float)r.status, (float)r.frames_done, (float)r.n, (float)r.chosen, (float)c.evaluated,
                             (float)c.switched, 0.0f};
    for (int k = 0; k < VT_ARB_MAX; ++k) {
        const ArbPeak& p = r.peak[k];
        const float w[10] = {(float)p.cell, (float)p.status, p.score, p.resp, p.similarity, p.box[0], p.box[1], p.box[2], p.box[3], 0.0f};
        memcpy(v + 8 + 10 * k, w, sizeof(w));
    }
    memcpy(out, v, sizeof(v));
    return VT_OK;
}

// ---- the keyed features: ONE list, ONE setter -----------------------------------------------------------
using namespace vtkeys;

// the key tables address the policies by word: the kernels' structs have their members there, their limits are the bounds
constexpr bool at(size_t offset, int word) { return offset == sizeof(int32_t) * (size_t)word; }
static_assert(sizeof(OverlayPolicy) == 4 * OV_WORDS && at(offsetof(OverlayPolicy, flags), OV_FLAGS) && at(offsetof(OverlayPolicy, thickness), OV_THICKNESS) &&
              at(offsetof(OverlayPolicy, size), OV_SIZE) && at(offsetof(OverlayPolicy, scale), OV_SCALE) && at(offsetof(OverlayPolicy, luma), OV_LUMA) &&
              at(offsetof(OverlayPolicy, rgb), OV_RGB) && at(offsetof(OverlayPolicy, min_score_pct), OV_MIN_SCORE_PCT), "OverlayPolicy");
static_assert(sizeof(MotionPolicy) == 4 * MO_WORDS && at(offsetof(MotionPolicy, on), MO_ON) && at(offsetof(MotionPolicy, gain_pct), MO_GAIN_PCT) &&
              at(offsetof(MotionPolicy, coast), MO_COAST) && at(offsetof(MotionPolicy, max_pct), MO_MAX_PCT), "MotionPolicy");
static_assert(sizeof(AppearPolicy) == 4 * AP_WORDS && at(offsetof(AppearPolicy, on), AP_ON) && at(offsetof(AppearPolicy, period), AP_PERIOD) &&
              at(offsetof(AppearPolicy, gate_pm), AP_GATE_PM) && at(offsetof(AppearPolicy, tau), AP_TAU) && kAppearKeys[1].hi == VT_APPEAR_MAX_PERIOD, "AppearPolicy");
static_assert(sizeof(PropPolicy) == 4 * PR_WORDS && at(offsetof(PropPolicy, mode), PR_MODE) && at(offsetof(PropPolicy, period), PR_PERIOD) &&
              at(offsetof(PropPolicy, max_n), PR_MAX_N) && at(offsetof(PropPolicy, min_sim_pm), PR_MIN_SIM_PM) && at(offsetof(PropPolicy, tau), PR_TAU) &&
              at(offsetof(PropPolicy, max_cells), PR_MAX_CELLS) && kPropKeys[1].hi == VT_PROP_MAX_PERIOD && kPropKeys[2].hi == VT_PROP_MAX &&
              kPropKeys[4].lo == VT_PROP_MIN_CELLS && kPropKeys[4].hi == VT_PROP_MAX_CELLS && OV_WORDS <= kMaxWords && PR_WORDS <= kMaxWords, "PropPolicy");
static_assert(sizeof(ConflictPolicy) == 4 * CF_WORDS && at(offsetof(ConflictPolicy, on), CF_ON) && at(offsetof(ConflictPolicy, iou_pm), CF_IOU_PM) &&
              at(offsetof(ConflictPolicy, gate), CF_GATE) && at(offsetof(ConflictPolicy, tau), CF_TAU) && CF_WORDS <= kMaxWords, "ConflictPolicy");
static_assert(sizeof(HealthPolicy) == 4 * HL_WORDS && at(offsetof(HealthPolicy, on), HL_ON) && at(offsetof(HealthPolicy, period), HL_PERIOD) &&
              at(offsetof(HealthPolicy, cell), HL_CELL) && at(offsetof(HealthPolicy, still_run), HL_STILL_RUN) && at(offsetof(HealthPolicy, flat_q), HL_FLAT_Q) &&
              at(offsetof(HealthPolicy, cut_pm), HL_CUT_PM) && at(offsetof(HealthPolicy, gate), HL_GATE) && at(offsetof(HealthPolicy, max_cells), HL_MAX_CELLS) &&
              kHealthKeys[HL_PERIOD].hi == VT_HEALTH_MAX_PERIOD && kHealthKeys[HL_MAX_CELLS].lo == VT_HEALTH_MIN_CELLS &&
              kHealthKeys[HL_MAX_CELLS].hi == VT_HEALTH_MAX_CELLS && HL_WORDS <= kMaxWords, "HealthPolicy");

static_assert(sizeof(ArbPolicy) == 4 * AR_WORDS && at(offsetof(ArbPolicy, on), AR_ON) && at(offsetof(ArbPolicy, max_peaks), AR_MAX) &&
              at(offsetof(ArbPolicy, radius), AR_RADIUS) && at(offsetof(ArbPolicy, min_resp_pm), AR_MIN_RESP_PM) && at(offsetof(ArbPolicy, low_pm), AR_LOW_PM) &&
              at(offsetof(ArbPolicy, high_pm), AR_HIGH_PM) && kArbKeys[AR_MAX].hi == VT_ARB_MAX && AR_WORDS <= kMaxWords, "ArbPolicy");
// the anchors are the appearance store's
static int arb_refuse(Engine* e) {
    return e->appear_capable ? VT_OK
                             : set_err(VT_ERR_INVALID_ARG, "arbitrate: the engine is not appearance-capable (vt_group_set_tuning \"appearance\" first: the anchors are the appearance store's)");
}
static int proposals_refuse(Engine* e) {
    return prop_pattern_side(e->d.T) ? VT_OK : set_err(VT_ERR_INVALID_ARG, "proposals: template size %d is a multiple of neither 16 nor 14", e->d.T);
}

// The stores: overlay the policy | [B] counters; motion the policy | [B] records (zero like known_motion, which nothing
// writes before the engine is capable); appearance all zero but the policy and the anchors of the initialised streams;
// proposals sized by the max_cells of the enable and zero up to the thumbnails; conflicts all zero but the policy (every
// stream in scene 0); health sized by the max_cells of the enable and zero up to the thumbnails; arbitration all zero but
// the policy up to the probes. The casts: a policy is words from its first member on.
const std::array<KeyedFeature, 7>& keyed_features() {
    static const std::array<KeyedFeature, 7> list = {{
        {"result overlay", "result_overlay", apply_overlay, (int32_t Engine::*)&Engine::overlay_policy, OV_WORDS, OV_FLAGS, "result_overlay", &Engine::overlay_capable,
         &Engine::d_overlay, &Engine::overlay_bytes, nullptr, 0, "result_overlay", 6, &Engine::overlay_stats},
        {"motion prior", "motion_", apply_motion, (int32_t Engine::*)&Engine::motion_policy, MO_WORDS, MO_ON, "motion_prior", &Engine::motion_capable,
         &Engine::d_motion, &Engine::motion_bytes, nullptr, Engine::SINK_MOTION, "motion", 8, &Engine::motion_stats},
        {"appearance check", "appearance", apply_appearance, (int32_t Engine::*)&Engine::appear_policy, AP_WORDS, AP_ON, "appearance", &Engine::appear_capable,
         &Engine::d_appear, &Engine::appear_bytes, nullptr, Engine::SINK_APPEAR, "appearance", 8, &Engine::appearance_stats,
         fill_anchors, "appearance_anchor", &Engine::appearance_anchor},
        {"reacquire proposals", "proposals", apply_proposals, (int32_t Engine::*)&Engine::prop_policy, PR_WORDS, PR_MODE, "proposals", &Engine::prop_capable,
         &Engine::d_prop, &Engine::prop_bytes, &Engine::prop_off_thumb, Engine::SINK_PROP, "proposals", VT_PROP_STATS, &Engine::proposals_stats,
         nullptr, nullptr, nullptr, proposals_refuse},
        {"stream conflicts", "conflicts", apply_conflicts, (int32_t Engine::*)&Engine::conflict_policy, CF_WORDS, CF_ON, "conflicts", &Engine::conflict_capable,
         &Engine::d_conflict, &Engine::conflict_bytes, nullptr, Engine::SINK_CONFLICT, "conflicts", 16, &Engine::conflicts_stats,
         nullptr, "conflicts_scene", &Engine::conflicts_scene},
        {"frame health", "health", apply_health, (int32_t Engine::*)&Engine::health_policy, HL_WORDS, HL_ON, "health", &Engine::health_capable,
         &Engine::d_health, &Engine::health_bytes, &Engine::health_off_thumbs, Engine::SINK_HEALTH, "health", VT_HEALTH_STATS, &Engine::health_stats},
        {"peak arbitration", "arbitrate", apply_arbitrate, (int32_t Engine::*)&Engine::arb_policy, AR_WORDS, AR_ON, "arbitrate", &Engine::arb_capable,
         &Engine::d_arb, &Engine::arb_bytes, &Engine::arb_off_probe, Engine::SINK_ARB, "arbitrate", VT_ARB_STATS, &Engine::arbitrate_stats,
         nullptr, nullptr, nullptr, arb_refuse},
    }};
    return list;
}

int not_enabled(const KeyedFeature& f) {
    return set_err(VT_ERR_INVALID_ARG, "%s: not enabled on this engine (vt_group_set_tuning \"%s\")", f.name, f.on_key);
}

int Engine::set_keyed(const KeyedFeature& f, const std::string& key, int value) {
    if (f.action_key && key == f.action_key) return (this->*f.action)(value);
    static const Engine fresh;      // its policies are the defaults
    int32_t* const host = &(this->*f.policy);
    const size_t bytes = sizeof(int32_t) * (size_t)f.words;
    int32_t p[kMaxWords], before[kMaxWords];
    memcpy(p, host, bytes); memcpy(before, host, bytes);
    char text[256];
    const Answer a = f.apply(key.c_str(), value, &(fresh.*f.policy), p, this->*f.capable, text, sizeof(text));
    if (a == REFUSED) return set_err(VT_ERR_INVALID_ARG, "%s", text);
    if (a == UNKNOWN) return set_err(VT_ERR_INVALID_ARG, "unknown tuning key '%s'", key.c_str());
    DEVICE_SCOPE(device);
    HIPCHK(hipStreamSynchronize(stream));
    if (!(this->*f.capable) && p[f.on_word] != 0) {
        if (int rc = f.refuse_enable ? f.refuse_enable(this) : VT_OK) return rc;
        memcpy(host, p, bytes);     // the store is sized and the passes are captured from the host's copy (proposals: max_cells)
        const size_t size = (this->*f.store_bytes)(), zeroed = f.zeroed_bytes ? (this->*f.zeroed_bytes)() : size;
        auto wire = [&](uint8_t* store) { this->*f.store = store; this->*f.capable = store != nullptr; };
        if (int rc = enable_store(f.name, size, zeroed, p, bytes, f.sink, f.fill, wire)) { memcpy(host, before, bytes); return rc; }
    } else if (this->*f.capable) {
        HIPCHK(hipMemcpy(this->*f.store, p, bytes, hipMemcpyHostToDevice));
        if (key == f.on_key && p[f.on_word] == 0)       // that key, value 0: every stream's records (kSinks: RESET_OFF)
            if (int rc = reset_records(RESET_OFF, 0, B, f.sink)) return rc;
    }
    memcpy(host, p, bytes);
    return VT_OK;
}

// HBM of the optional features this engine has enabled, beside activation_bytes() under max_device_mib
size_t Engine::feature_bytes() const {
    size_t n = (refresh_capable ? refresh_bytes() : 0) + (chip_capable ? chip_store_bytes_of(B, chip_size, chip_kind) : 0) +
               (peaks_capable ? peaks_bytes() : 0);
    for (const KeyedFeature& f : keyed_features())
        if (this->*f.capable) n += (this->*f.store_bytes)();
    return n;
}
