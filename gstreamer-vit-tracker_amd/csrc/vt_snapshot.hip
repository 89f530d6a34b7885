// vt_snapshot.hip — stream snapshots: one stream's state record, refresh policy and current template rows as a
// self-contained byte string (layout and contract: include/vittrack_hip.h; DESIGN.md section 3, "Stream snapshots").
//   - the format's validation, on the host, with no GPU (snapshots arrive from disk and from the network: they get the
//     treatment Engine::index_blob gives weight blobs - every size bounded before anything is derived from it);
//   - export: pack (k_snapshot.hip) on the group's stream into device staging, one copy to its pinned twin, header and
//     checksum on the host;
//   - import: pinned twin -> device staging -> unpack on the group's stream; synchronous with nothing outstanding,
//     queued behind the pipelined passes like vt_group_enqueue_init_host otherwise;
//   - copy: both without a caller buffer, device to device on one GPU.
#include "vt_engine.hpp"
#include "k_snapshot.hpp"
#include <cstddef>

struct SnapHeader {     // bytes [0, VT_SNAP_HEADER_BYTES) of a snapshot, little-endian
    char magic[4], version[4];
    uint32_t total_bytes, header_bytes, state_bytes, policy_bytes, rows_bytes, flags;
    int32_t patch, template_size, search_size, kpad, tokens_template;
    float norm_a[3], norm_b[3];
    uint32_t reserved0;
    uint64_t checksum;
    uint32_t reserved[16];
};
static_assert(sizeof(SnapHeader) == VT_SNAP_HEADER_BYTES && offsetof(SnapHeader, checksum) == 80 &&
              offsetof(SnapHeader, patch) == 32 && offsetof(SnapHeader, norm_a) == 52, "snapshot header layout");
static const char kSnapMagic[4] = {'V', 'T', 'S', 'S'}, kSnapVersion[4] = {'0', '0', '0', '1'};
#define VT_SNAP_FLAG_ANY_GRAPHS 1u

// FNV-1a-64 over the whole string with the checksum field read as zero (at most ~250 KB per stream: well under a
// millisecond on the host; the device has nothing to add to it)
static uint64_t snap_checksum(const uint8_t* p, size_t bytes) {
    uint64_t h = 0xcbf29ce484222325ull;
    const size_t c0 = offsetof(SnapHeader, checksum), c1 = c0 + 8;
    for (size_t i = 0; i < bytes; ++i) {
        h ^= (i >= c0 && i < c1) ? 0u : p[i];
        h *= 0x100000001b3ull;
    }
    return h;
}

static size_t snap_bytes_for(long long nt, long long kpad) {
    if (nt < 1 || nt > 65536 || kpad < 64 || kpad > 16384 || kpad % 64) return 0;
    return (size_t)VT_SNAP_ROWS_OFF + (size_t)(2 * nt * kpad);
}

// the header of a snapshot of e's model
static void snap_fill_header(const Engine* e, SnapHeader* h) {
    memset(h, 0, sizeof(*h));
    memcpy(h->magic, kSnapMagic, 4);
    memcpy(h->version, kSnapVersion, 4);
    h->header_bytes = VT_SNAP_HEADER_BYTES;
    h->state_bytes = sizeof(StreamState);
    h->policy_bytes = sizeof(RefreshPolicy);
    h->rows_bytes = (uint32_t)(sizeof(bf16_t) * (size_t)e->d.nt * e->d.kpad);
    h->total_bytes = (uint32_t)e->snapshot_bytes();
    h->flags = e->want_levels ? VT_SNAP_FLAG_ANY_GRAPHS : 0u;
    h->patch = e->d.patch; h->template_size = e->d.T; h->search_size = e->d.S; h->kpad = e->d.kpad;
    h->tokens_template = e->d.nt;
    memcpy(h->norm_a, e->d.norm_a, sizeof(h->norm_a));
    memcpy(h->norm_b, e->d.norm_b, sizeof(h->norm_b));
}

// ---- validation (no GPU) ------------------------------------------------------------------------------------------------

// sizes, magic, reserved words and the geometry as such; *h is the header on success
static int snap_check_header(const uint8_t* p, size_t bytes, SnapHeader* h) {
    if (bytes < sizeof(SnapHeader)) return set_err(VT_ERR_FORMAT, "snapshot: %zu bytes is shorter than the header", bytes);
    memcpy(h, p, sizeof(*h));
    if (memcmp(h->magic, kSnapMagic, 4) != 0) return set_err(VT_ERR_FORMAT, "snapshot: bad magic");
    if (memcmp(h->version, kSnapVersion, 4) != 0) return set_err(VT_ERR_FORMAT, "snapshot: unsupported version");
    if (h->header_bytes != sizeof(SnapHeader) || h->state_bytes != sizeof(StreamState) || h->policy_bytes != sizeof(RefreshPolicy))
        return set_err(VT_ERR_FORMAT, "snapshot: section sizes %u / %u / %u, expected %zu / %zu / %zu", h->header_bytes,
                       h->state_bytes, h->policy_bytes, sizeof(SnapHeader), sizeof(StreamState), sizeof(RefreshPolicy));
    const uint64_t sum = (uint64_t)h->header_bytes + h->state_bytes + h->policy_bytes + h->rows_bytes;
    if (sum != h->total_bytes || (uint64_t)bytes != sum)
        return set_err(VT_ERR_FORMAT, "snapshot: sizes do not add up (sections %llu, stored total %u, given %zu bytes)",
                       (unsigned long long)sum, h->total_bytes, bytes);
    if ((h->flags & ~VT_SNAP_FLAG_ANY_GRAPHS) != 0 || h->reserved0 != 0)
        return set_err(VT_ERR_FORMAT, "snapshot: non-zero reserved flag bits or word");
    for (uint32_t r : h->reserved)
        if (r != 0) return set_err(VT_ERR_FORMAT, "snapshot: non-zero reserved word");
    // the bounds Engine::index_blob puts on the same numbers, before anything is derived from them
    if (h->patch < 2 || h->patch > 64 || h->template_size < h->patch || h->search_size < h->patch ||
        h->template_size > 4096 || h->search_size > 4096 || h->template_size % h->patch || h->search_size % h->patch ||
        h->kpad < 64 || h->kpad > 16384 || h->kpad % 64 || h->kpad < 3 * h->patch * h->patch)
        return set_err(VT_ERR_FORMAT, "snapshot: geometry out of range (patch %d, template %d, search %d, kpad %d)", h->patch,
                       h->template_size, h->search_size, h->kpad);
    const int gt = h->template_size / h->patch;
    if (h->tokens_template != gt * gt || (uint64_t)h->rows_bytes != 2ull * (uint64_t)h->tokens_template * (uint64_t)h->kpad)
        return set_err(VT_ERR_FORMAT, "snapshot: %d template tokens / %u bytes of rows do not match the geometry",
                       h->tokens_template, h->rows_bytes);
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(h->norm_a[i]) || !std::isfinite(h->norm_b[i]))
            return set_err(VT_ERR_FORMAT, "snapshot: non-finite normalisation constant");
    return VT_OK;
}

// the snapshot's input geometry is the engine's: the five integers and the six floats, compared as bits
static int snap_check_geometry(const SnapHeader& h, const ModelDims& d) {
    if (h.patch != d.patch || h.template_size != d.T || h.search_size != d.S || h.kpad != d.kpad || h.tokens_template != d.nt)
        return set_err(VT_ERR_FORMAT, "snapshot: geometry patch %d template %d search %d kpad %d tokens %d differs from the "
                       "engine's %d / %d / %d / %d / %d", h.patch, h.template_size, h.search_size, h.kpad, h.tokens_template,
                       d.patch, d.T, d.S, d.kpad, d.nt);
    if (memcmp(h.norm_a, d.norm_a, sizeof(h.norm_a)) != 0 || memcmp(h.norm_b, d.norm_b, sizeof(h.norm_b)) != 0)
        return set_err(VT_ERR_FORMAT, "snapshot: pixel normalisation differs from the engine's");
    return VT_OK;
}

// a state some pass could have left; cells: the score grid's size
static int snap_check_state(const StreamState& st, int cells) {
    if (st.initialized != 1) return set_err(VT_ERR_FORMAT, "snapshot: state is not that of an initialised stream");
    if (check_state_box(st.box) != VT_OK) {
        char why[256];
        snprintf(why, sizeof(why), "%s", vt_err_text());
        return set_err(VT_ERR_FORMAT, "snapshot: %s", why);
    }
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(st.geo[k]) || !std::isfinite(st.last_fbox[k]))
            return set_err(VT_ERR_FORMAT, "snapshot: non-finite crop geometry or last box");
    if (!std::isfinite(st.last_score)) return set_err(VT_ERR_FORMAT, "snapshot: non-finite last score");
    if (st.frame_w < 16 || st.frame_h < 16 || st.frame_w > 65536 || st.frame_h > 65536)
        return set_err(VT_ERR_FORMAT, "snapshot: frame size %dx%d out of range", st.frame_w, st.frame_h);
    if (st.frames_done < 0 || st.success_count < 0 || st.success_count > st.frames_done)
        return set_err(VT_ERR_FORMAT, "snapshot: counters out of range (frames_done %d, success_count %d)", st.frames_done,
                       st.success_count);
    if (st.last_idx < 0 || st.last_idx >= cells)
        return set_err(VT_ERR_FORMAT, "snapshot: last_idx %d outside the score grid of %d cells", st.last_idx, cells);
    if (st.tpl_gen < 0 || st.tpl_frame < 0 || st.tpl_frame > st.frames_done)
        return set_err(VT_ERR_FORMAT, "snapshot: refresh words out of range (generation %d, last_frame %d of %d)", st.tpl_gen,
                       st.tpl_frame, st.frames_done);
    if (st.window_miss < 0 || (long long)st.window_miss > (long long)st.frames_done + 1)
        return set_err(VT_ERR_FORMAT, "snapshot: window_miss %d out of range", st.window_miss);
    return VT_OK;
}

// a policy Engine::set_refresh would take
static int snap_check_policy(const RefreshPolicy& p) {
    if (p.period < 0 || p.period == 1 || p.period > VT_REFRESH_MAX_PERIOD)
        return set_err(VT_ERR_FORMAT, "snapshot: refresh period %d (0 = off, else 2..%d)", p.period, VT_REFRESH_MAX_PERIOD);
    if (!std::isfinite(p.min_score) || p.min_score < 0.0f || p.min_score > 1.0f)
        return set_err(VT_ERR_FORMAT, "snapshot: refresh min_score must be finite and in 0..1");
    if (p.skipped_geometry < 0 || p.reserved != 0)
        return set_err(VT_ERR_FORMAT, "snapshot: refresh policy counter negative or reserved word non-zero");
    return VT_OK;
}

// the whole string; d: the engine it is meant for, or null (vt_snapshot_info)
static int snap_validate(const uint8_t* p, size_t bytes, const ModelDims* d, SnapHeader* h, StreamState* st, RefreshPolicy* pol) {
    if (int rc = snap_check_header(p, bytes, h)) return rc;
    if (snap_checksum(p, bytes) != h->checksum) return set_err(VT_ERR_FORMAT, "snapshot: checksum mismatch");
    if (d)
        if (int rc = snap_check_geometry(*h, *d)) return rc;
    memcpy(st, p + VT_SNAP_STATE_OFF, sizeof(*st));
    memcpy(pol, p + VT_SNAP_POLICY_OFF, sizeof(*pol));
    const int gs = h->search_size / h->patch;
    if (int rc = snap_check_state(*st, gs * gs)) return rc;
    if (int rc = snap_check_policy(*pol)) return rc;
    const size_t n = h->rows_bytes / 2;
    for (size_t i = 0; i < n; ++i) {
        bf16_t v;
        memcpy(&v, p + VT_SNAP_ROWS_OFF + 2 * i, 2);
        if ((v & 0x7f80u) == 0x7f80u) return set_err(VT_ERR_FORMAT, "snapshot: non-finite template element %zu", i);
    }
    return VT_OK;
}

// ---- staging ------------------------------------------------------------------------------------------------------------

// a record pair nothing is using: one whose last work has passed, else a new one. Never freed before the engine is:
// freeing device memory waits for the device, and a queued import waits for nothing.
int Engine::snap_staging(SnapStage** out) {
    for (SnapStage* sg : snaps)
        if (sg && sg->done_ev && hipEventQuery(sg->done_ev) == hipSuccess) { *out = sg; return VT_OK; }
    (void)hipGetLastError();                 // hipErrorNotReady of the queries above is no error
    snaps.push_back(nullptr);
    SnapStage* sg = snaps.back() = new SnapStage();     // the engine's from here on, whatever fails below
    HIPCHK(hipMalloc((void**)&sg->d, snapshot_bytes()));
    HIPCHK(hipHostMalloc((void**)&sg->h, snapshot_bytes()));
    HIPCHK(hipEventCreateWithFlags(&sg->up_ev, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&sg->done_ev, hipEventDisableTiming));   // last: a half-built one is never picked
    *out = sg;
    return VT_OK;
}

static SnapArgs snap_args(Engine* e, int stream, uint8_t* d_rec) {
    return SnapArgs{e->d_states + stream, e->refresh_capable ? e->d_policy + stream : nullptr, e->tpl_init_rows(stream),
                    e->tpl_bufs(), e->d.nt * e->d.kpad, d_rec};
}

// ---- export ---------------------------------------------------------------------------------------------------------------

static int snap_check_source(const Engine* e, int s, const char* what) {
    if (s < 0 || s >= e->B) return set_err(VT_ERR_INVALID_ARG, "%s: stream %d out of range (0..%d)", what, s, e->B - 1);
    if (!e->h_initialized[(size_t)s]) return set_err(VT_ERR_NOT_INITIALIZED, "%s: stream %d was never initialised", what, s);
    if (e->in_outstanding_pass(s))
        return set_err(VT_ERR_INVALID_ARG, "%s: stream %d is in an outstanding pass, collect it first (vt_group_wait_next)", what, s);
    return VT_OK;
}

// Stream s (checked by the caller) packed behind whatever e's stream holds into a staging record; its pinned twin gets
// the header and, of the payload, everything (whole) or state and policy only (the rows then stay on the device for a
// copy on the same GPU). Waits for the stream: collects nothing, changes nothing.
static int snap_pack_stream(Engine* e, int s, bool whole, Engine::SnapStage** out) {
    DEVICE_SCOPE(e->device);
    Engine::SnapStage* sg = nullptr;
    if (int rc = e->snap_staging(&sg)) return rc;
    const size_t total = e->snapshot_bytes();
    hipError_t he = launch_snapshot_pack(snap_args(e, s, sg->d), e->stream);
    if (he == hipSuccess)
        he = hipMemcpyAsync(sg->h + VT_SNAP_STATE_OFF, sg->d + VT_SNAP_STATE_OFF, (whole ? total : (size_t)VT_SNAP_ROWS_OFF) - VT_SNAP_STATE_OFF,
                            hipMemcpyDeviceToHost, e->stream);
    (void)hipEventRecord(sg->done_ev, e->stream);       // also after a failed launch: the staging is busy until then
    if (he != hipSuccess) return set_err(VT_ERR_HIP, "snapshot pack: %s", hipGetErrorString(he));
    HIPCHK(hipStreamSynchronize(e->stream));
    SnapHeader h;
    snap_fill_header(e, &h);
    memcpy(sg->h, &h, sizeof(h));
    if (whole) {
        h.checksum = snap_checksum(sg->h, total);
        memcpy(sg->h, &h, sizeof(h));
    }
    *out = sg;
    return VT_OK;
}

static int snap_export(Engine* e, int s, void* buf, size_t cap, size_t* written) {
    if (written) *written = 0;
    if (int rc = snap_check_source(e, s, "export_stream")) return rc;
    const size_t total = e->snapshot_bytes();
    if (written) *written = total;
    if (cap < total) return set_err(VT_ERR_SHORT_BUFFER, "export_stream: the snapshot needs %zu bytes, the buffer has %zu", total, cap);
    if (!buf) return set_err(VT_ERR_INVALID_ARG, "export_stream: null buffer");
    Engine::SnapStage* sg = nullptr;
    if (int rc = snap_pack_stream(e, s, true, &sg)) { if (written) *written = 0; return rc; }
    memcpy(buf, sg->h, total);
    return VT_OK;
}

// ---- import ---------------------------------------------------------------------------------------------------------------

// Stream t of e becomes the validated record (st, pol, flags). The payload comes from host bytes `rec` (the whole
// string: staged and uploaded here) or, with d_owner, from that staging record's device half, which some stream of this
// GPU finishes writing at d_owner->up_ev. Everything that can fail for want of memory comes first, the staging in
// front of the enabling: when an error is returned before the unpack is launched nothing has changed - but for a second
// graph set whose capture failed half-way, whose finished tiers stay (Engine::capture_graphs_for).
static int snap_import(Engine* e, int t, const StreamState& st, const RefreshPolicy& pol, uint32_t flags, const uint8_t* rec,
                       Engine::SnapStage* d_owner) {
    const bool pipelined = e->host_seq != e->host_collected;
    if (pipelined && e->in_outstanding_pass(t))
        return set_err(VT_ERR_INVALID_ARG, "import_stream: stream %d is in an outstanding pass, collect it first (vt_group_wait_next)", t);
    const bool enable = pol.period >= 2 && !e->refresh_capable;
    if (enable && pipelined)        // as vt_group_set_template_refresh: the first enabling recaptures the graphs
        return set_err(VT_ERR_INVALID_ARG, "import_stream: the snapshot's refresh policy would enable template refresh on this "
                       "engine; collect the pipelined host passes first (vt_group_wait_next)");
    DEVICE_SCOPE(e->device);
    Engine::SnapStage* sg = d_owner;
    if (!sg)
        if (int rc = e->snap_staging(&sg)) return rc;
    if (enable)
        if (int rc = e->enable_refresh()) return rc;    // VT_ERR_OOM: nothing changed
    // like an init on such a format: the second graph set, once; needs the stream idle, so with passes outstanding this
    // one call waits for them (they stay uncollected), as vt_group_enqueue_init_host documents
    if (flags & VT_SNAP_FLAG_ANY_GRAPHS)
        if (int rc = e->capture_graphs_for(VT_PIX_BGR8)) return rc;
    if (!d_owner) {
        const size_t total = e->snapshot_bytes();
        memcpy(sg->h, rec, total);                      // the caller's bytes are free on return
        // with passes outstanding the upload runs beside them on the copy stream; the unpack waits for it alone
        hipStream_t up = pipelined && e->copy_stream ? e->copy_stream : e->stream;
        HIPCHK(hipMemcpyAsync(sg->d, sg->h, total, hipMemcpyHostToDevice, up));
        if (up != e->stream) {
            HIPCHK(hipEventRecord(sg->up_ev, up));
            HIPCHK(hipStreamWaitEvent(e->stream, sg->up_ev, 0));
        }
    } else {
        HIPCHK(hipStreamWaitEvent(e->stream, sg->up_ev, 0));
    }
    const hipError_t he = launch_snapshot_unpack(snap_args(e, t, sg->d), e->stream);
    (void)hipEventRecord(sg->done_ev, e->stream);       // also after a failed launch: the staging is busy until then
    if (he != hipSuccess) return set_err(VT_ERR_HIP, "snapshot unpack: %s", hipGetErrorString(he));
    // no part of a snapshot: the imported stream starts without a velocity, a previous thumbnail or a record of the target
    // it had (its scene stays: policy, not state), and the imported rows become its appearance anchor
    if (int rc = e->reset_records(Engine::RESET_IMPORT, t, t + 1)) return rc;
    HIPCHK(e->anchor_from_template(t, st.tpl_gen));
    if (!pipelined) HIPCHK(hipStreamSynchronize(e->stream));    // synchronous, like vt_group_init_device
    // what the host knows of this stream is the imported state from now on: the next window is cut around its box,
    // exact, and a rewind behind a queued import restores it (the template store is not rewound)
    e->known[(size_t)t] = st;
    e->h_states_all[t] = st;
    e->h_initialized[(size_t)t] = 1;
    e->h_policy[(size_t)t].period = pol.period;
    e->h_policy[(size_t)t].min_score = pol.min_score;
    if (!e->refresh_capable) e->segments_moved = true;  // the next full pass puts every stream's rows in place from the store
    return VT_OK;
}

static int snap_import_bytes(Engine* e, int t, const void* buf, size_t bytes) {
    if (t < 0 || t >= e->B) return set_err(VT_ERR_INVALID_ARG, "import_stream: stream %d out of range (0..%d)", t, e->B - 1);
    SnapHeader h;
    StreamState st;
    RefreshPolicy pol;
    if (int rc = snap_validate((const uint8_t*)buf, bytes, &e->d, &h, &st, &pol)) return rc;
    return snap_import(e, t, st, pol, h.flags, (const uint8_t*)buf, nullptr);
}

extern "C" {

size_t vt_snapshot_bytes(const vt_model_info* info) try {
    return info ? snap_bytes_for(info->tokens_template, info->kpad) : 0;
} catch (...) { return 0; }

size_t vt_group_snapshot_bytes(const vt_group* g) try {
    return g ? g->e->snapshot_bytes() : 0;
} catch (...) { return 0; }

int vt_snapshot_info(const void* buf, size_t bytes, vt_snapshot_desc* out) try {
    if (!buf || !out) return set_err(VT_ERR_INVALID_ARG, "null argument");
    SnapHeader h;
    StreamState st;
    RefreshPolicy pol;
    if (int rc = snap_validate((const uint8_t*)buf, bytes, nullptr, &h, &st, &pol)) return rc;
    memset(out, 0, sizeof(*out));
    out->total_bytes = h.total_bytes; out->header_bytes = h.header_bytes; out->state_bytes = h.state_bytes;
    out->policy_bytes = h.policy_bytes; out->rows_bytes = h.rows_bytes; out->flags = h.flags;
    out->patch = h.patch; out->template_size = h.template_size; out->search_size = h.search_size; out->kpad = h.kpad;
    out->tokens_template = h.tokens_template;
    memcpy(out->norm_a, h.norm_a, sizeof(out->norm_a));
    memcpy(out->norm_b, h.norm_b, sizeof(out->norm_b));
    memcpy(out->box, st.box, sizeof(out->box));
    out->frame_width = st.frame_w; out->frame_height = st.frame_h;
    out->frames_done = st.frames_done; out->success_count = st.success_count; out->last_score = st.last_score;
    out->period = pol.period; out->min_score = pol.min_score; out->skipped_geometry = pol.skipped_geometry;
    out->generation = st.tpl_gen; out->last_frame = st.tpl_frame;
    return VT_OK;
} VT_NOTHROW_INT

int vt_group_export_stream(vt_group* g, int stream, void* buf, size_t cap, size_t* written) try {
    if (!g) return set_err(VT_ERR_INVALID_ARG, "null group");
    return snap_export(g->e, stream, buf, cap, written);
} VT_NOTHROW_INT

int vt_group_import_stream(vt_group* g, int stream, const void* buf, size_t bytes) try {
    if (!g || !buf) return set_err(VT_ERR_INVALID_ARG, "null argument");
    return snap_import_bytes(g->e, stream, buf, bytes);
} VT_NOTHROW_INT

int vt_export_state(vt_tracker* t, void* buf, size_t cap, size_t* written) try {
    if (!t) return set_err(VT_ERR_INVALID_ARG, "null tracker");
    return snap_export(t->e, 0, buf, cap, written);
} VT_NOTHROW_INT

int vt_import_state(vt_tracker* t, const void* buf, size_t bytes) try {
    if (!t || !buf) return set_err(VT_ERR_INVALID_ARG, "null argument");
    return snap_import_bytes(t->e, 0, buf, bytes);
} VT_NOTHROW_INT

int vt_group_copy_stream(vt_group* src, int s, vt_group* dst, int t) try {
    if (!src || !dst) return set_err(VT_ERR_INVALID_ARG, "null group");
    Engine *a = src->e, *b = dst->e;
    if (int rc = snap_check_source(a, s, "copy_stream")) return rc;
    if (t < 0 || t >= b->B) return set_err(VT_ERR_INVALID_ARG, "copy_stream: destination stream %d out of range (0..%d)", t, b->B - 1);
    if (a == b && s == t) return set_err(VT_ERR_INVALID_ARG, "copy_stream: source and destination are the same stream");
    SnapHeader h;
    snap_fill_header(a, &h);
    if (int rc = snap_check_geometry(h, b->d)) return rc;       // before anything is launched
    const bool same_gpu = a->device == b->device;
    Engine::SnapStage* sg = nullptr;
    if (int rc = snap_pack_stream(a, s, !same_gpu, &sg)) return rc;
    StreamState st;
    RefreshPolicy pol;
    memcpy(&st, sg->h + VT_SNAP_STATE_OFF, sizeof(st));
    memcpy(&pol, sg->h + VT_SNAP_POLICY_OFF, sizeof(pol));
    if (!same_gpu) {    // the bytes of vt_group_export_stream into vt_group_import_stream, through both engines' pinned staging
        if (int rc = snap_validate(sg->h, a->snapshot_bytes(), &b->d, &h, &st, &pol)) return rc;
        return snap_import(b, t, st, pol, h.flags, sg->h, nullptr);
    }
    // one GPU: the record stays in a's device staging. The pack is done (snap_pack_stream waited for the 104 bytes
    // the host needs); the event is the general form of the hand-over, and b's unpack marks the staging busy until it ran
    const int gs = b->d.S / b->d.patch;
    if (int rc = snap_check_state(st, gs * gs)) return rc;
    if (int rc = snap_check_policy(pol)) return rc;
    {
        DEVICE_SCOPE(a->device);
        HIPCHK(hipEventRecord(sg->up_ev, a->stream));
    }
    return snap_import(b, t, st, pol, h.flags, nullptr, sg);
} VT_NOTHROW_INT

}  // extern "C"
