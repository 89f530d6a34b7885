// vt_ingest.hip — host-frame ingest behind the C ABI: only the window of a frame that the pass can sample crosses
// PCIe; the pipelined form uploads frame t+1 on a copy stream while pass t runs.
#include "vt_engine.hpp"

// ---- host-frame ingest: only the windows that the pass can sample cross PCIe ----------------------
// The reference hands over whole frames (6.2 MB of RGB8 at 1080p, src/pipeline.rs:105-112) although
// the tracker reads a window of side 4*sqrt(w*h) around the last box. The windows of all the frames
// of a call are packed back to back into one pinned arena and moved with ONE async H2D copy; the
// frame descriptors handed to the kernels point into the device copy and carry the window origin.
// The caller's buffer of a synchronous call is no longer referenced when the call returns (src/pipeline.rs:125
// draws into it).
struct HostWin {
    int fmt, w, h, s0, s1;
    const uint8_t *p0, *p1;
    int x_lo, y_lo, ww, wh;
    size_t bytes, uv_off;
};

// row pitch of a packed format's window in the arena: 4-byte pixels and grey bytes on 16-byte boundaries (the crop kernel
// then fetches 4 / 8 pixels per load), the others back to back
static size_t packed_row_bytes(int fmt, int ww) {
    const size_t rb = (size_t)ww * pix_row_bpp(fmt);
    return pix_row_bpp(fmt) == 4 || pix_row_bpp(fmt) == 1 ? (rb + 15) & ~(size_t)15 : rb;
}

// PIXF_420SP: row pitches of a packed window's luma plane and of its chroma plane(s), and the chroma planes' rows. Every
// plane's bytes are packed as they are - 16-bit samples stay 16-bit, two chroma planes stay two, the second one
// pitch * rows behind the first, which is where a windowed frame has it (vittrack_hip.h: vt_pixfmt2)
static void packed_planes(int fmt, int ww, int wh, size_t* ys, size_t* cs, int* crows) {
    *ys = ((size_t)ww * pix_row_bpp(fmt) + 15) & ~(size_t)15;
    *cs = ((size_t)pix_chroma_row_bytes(fmt, ww) + 15) & ~(size_t)15;
    *crows = pix_chroma_rows(fmt, wh);
}

// bytes of a window's packed form in the arena, from its extent
static void size_window(HostWin* win) {
    if (pix_family(win->fmt) == PIXF_420SP) {
        // rows of the packed window start on 16-byte boundaries: the pixel kernel then fetches 8 pixels per load
        size_t ys, cs;
        int crows;
        packed_planes(win->fmt, win->ww, win->wh, &ys, &cs, &crows);
        win->uv_off = (ys * win->wh + 255) & ~(size_t)255;
        win->bytes = win->uv_off + cs * crows * (pix_planar(win->fmt) ? 2 : 1);
    } else {
        win->uv_off = 0;
        win->bytes = packed_row_bytes(win->fmt, win->ww) * win->wh;
    }
    win->bytes = (win->bytes + 255) & ~(size_t)255;
}

// `grow`: enlargement of the crop side for a SPECULATIVE window (the box of the pass that is still
// running is not known): 0 = the exact crop
static int plan_window(const Engine* e, const vt_frame& hf, const float* box, float grow, HostWin* win) {
    const int fmt = hf.format, w = hf.width, h = hf.height, s0 = hf.stride0, s1 = hf.stride1;
    const uint8_t *p0 = (const uint8_t*)hf.plane0, *p1 = (const uint8_t*)hf.plane1;
    if (!p0 || w < 16 || h < 16) return set_err(VT_ERR_INVALID_ARG, "null frame or size < 16");
    if (w > e->max_w || h > e->max_h)
        return set_err(VT_ERR_INVALID_ARG, "frame %dx%d exceeds configured max %dx%d", w, h, e->max_w, e->max_h);
    // by family (vt_frame.hpp: PixFamily); the messages name the format
    const int fam = pix_family(fmt), bpp = pix_row_bpp(fmt);
    if (fam == PIXF_RGB) {
        if (s0 < bpp * w) return set_err(VT_ERR_INVALID_ARG, "%s stride < %d*width", pix_name(fmt), bpp);
    } else if (fam == PIXF_422) {
        if ((w & 1) || s0 < 2 * w) return set_err(VT_ERR_INVALID_ARG, "%s: odd width or stride < 2*width", pix_name(fmt));
    } else if (fam == PIXF_420SP) {
        if (!p1 || s0 < w * bpp || s1 < pix_chroma_row_bytes(fmt, w))
            return set_err(VT_ERR_INVALID_ARG, "%s: bad plane or stride", pix_name(fmt));
        if (pix_rows422(fmt) && (w & 1)) return set_err(VT_ERR_INVALID_ARG, "%s: odd width", pix_name(fmt));
    } else {
        if (const char* why = pix_refusal(fmt))     // as check_frame
            return set_err(VT_ERR_INVALID_ARG, "%s frame format 0x%x: %s", pix_name(fmt), (unsigned)fmt, why);
        return set_err(VT_ERR_INVALID_ARG, "unknown pixel format %d", fmt);
    }
    // window = search crop (factor 4; it contains the factor-2 template crop) + bilinear margin
    const float side = 4.0f * sqrtf(fmaxf(box[2] * box[3], 1.0f)) * (1.0f + grow);
    const float cx = box[0] + 0.5f * box[2], cy = box[1] + 0.5f * box[3];
    long x_lo = (long)floorf(cx - 0.5f * side) - 4, x_hi = (long)ceilf(cx + 0.5f * side) + 4;
    long y_lo = (long)floorf(cy - 0.5f * side) - 4, y_hi = (long)ceilf(cy + 0.5f * side) + 4;
    x_lo = std::max(0L, std::min((long)w, x_lo)) & ~1L;
    y_lo = std::max(0L, std::min((long)h, y_lo)) & ~1L;
    x_hi = std::max(x_lo, std::min((long)w, (x_hi + 1) & ~1L));
    y_hi = std::max(y_lo, std::min((long)h, (y_hi + 1) & ~1L));
    if (x_hi - x_lo < 2 || y_hi - y_lo < 2) {   // window misses the frame: nothing can be sampled
        x_lo = 0; y_lo = 0; x_hi = 2; y_hi = 2;
    }
    win->fmt = fmt; win->w = w; win->h = h; win->s0 = s0; win->s1 = s1; win->p0 = p0; win->p1 = p1;
    win->x_lo = (int)x_lo; win->y_lo = (int)y_lo;
    win->ww = (int)(x_hi - x_lo); win->wh = (int)(y_hi - y_lo);
    size_window(win);
    return VT_OK;
}

static bool same_host_frame(const vt_frame& a, const vt_frame& b) {
    return a.plane0 == b.plane0 && a.plane1 == b.plane1 && a.width == b.width && a.height == b.height &&
           a.stride0 == b.stride0 && a.stride1 == b.stride1 && a.format == b.format;
}

// The one growth rule of a staging arena: half as much again as asked for. The old pair is freed here - hipFree waits
// for the device - so a caller that must not wait (queued_init_staging) only ever calls this on a fresh arena.
int StageArena::ensure(size_t need) {
    if (need <= cap) return VT_OK;
    release();
    const size_t want = need + need / 2 + 4096;
    HIPCHK(hipMalloc((void**)&d, want));
    HIPCHK(hipHostMalloc((void**)&h, want));
    cap = want;
    return VT_OK;
}
void StageArena::release() {
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
    *this = StageArena();
}

static void pack_window(const StageArena& a, const HostWin& wn, size_t off, vt_frame* f) {
    uint8_t* dst = a.h + off;
    memset(f, 0, sizeof(*f));
    f->width = wn.w; f->height = wn.h; f->format = wn.fmt;
    f->origin_x = wn.x_lo; f->origin_y = wn.y_lo;
    f->windowed = 1;   // strides describe the packed window
    f->window_w = wn.ww; f->window_h = wn.wh;
    if (pix_family(wn.fmt) != PIXF_420SP) {
        const size_t bpp = (size_t)pix_row_bpp(wn.fmt);
        const size_t rb = (size_t)wn.ww * bpp, rs = packed_row_bytes(wn.fmt, wn.ww);   // as plan_window
        for (int r = 0; r < wn.wh; ++r)
            memcpy(dst + r * rs, wn.p0 + (size_t)(wn.y_lo + r) * wn.s0 + (size_t)wn.x_lo * bpp, rb);
        f->plane0 = a.d + off; f->stride0 = (int)rs;
    } else {
        size_t ys, uvs;                                                                     // as size_window
        int uvh;
        packed_planes(wn.fmt, wn.ww, wn.wh, &ys, &uvs, &uvh);
        const size_t bpp = (size_t)pix_row_bpp(wn.fmt);
        const bool planar = pix_planar(wn.fmt);
        for (int r = 0; r < wn.wh; ++r)
            memcpy(dst + (size_t)r * ys, wn.p0 + (size_t)(wn.y_lo + r) * wn.s0 + (size_t)wn.x_lo * bpp, (size_t)wn.ww * bpp);
        // chroma bytes of the window's columns (x_lo is even): pairs of samples, or one byte per pair in each of two planes.
        // Odd frame width: the last pixel's V byte lies one past the row's last full pair
        const long c_lo = planar ? wn.x_lo / 2 : (long)wn.x_lo * (long)bpp;
        const int uv_avail = (int)std::min<long>(pix_chroma_row_bytes(wn.fmt, wn.ww), (long)wn.s1 - c_lo);
        const int r_lo = pix_rows422(wn.fmt) ? wn.y_lo : wn.y_lo / 2;
        // the caller's second chroma plane lies behind the rows of the whole frame's first, the packed one behind uvh rows
        const size_t second_src = (size_t)wn.s1 * (size_t)pix_chroma_rows(wn.fmt, wn.h), second_dst = uvs * (size_t)uvh;
        for (int pl = 0; pl < (planar ? 2 : 1); ++pl)
            for (int r = 0; r < uvh; ++r)
                memcpy(dst + wn.uv_off + pl * second_dst + (size_t)r * uvs,
                       wn.p1 + pl * second_src + (size_t)(r_lo + r) * wn.s1 + c_lo, (size_t)uv_avail);
        f->plane0 = a.d + off; f->plane1 = a.d + off + wn.uv_off;
        f->stride0 = (int)ys; f->stride1 = (int)uvs;
    }
}

// n host frames -> n device frame descriptors (windows packed into `a`, ONE H2D copy enqueued on copy_on).
// boxes[i]: the box that decides frame i's window (the new box at init, the last state at update);
// grow[i]: its enlargement (plan_window), null: every window exact. pack_all: no zero-copy route, whatever the
// configuration says (the kernels must not read the caller's memory after the call has returned).
// share (candidate passes): slots that name the same host frame are staged ONCE, as the bounding rectangle of their
// windows, and all take that one descriptor - every slot's own window lies inside it, so each still samples exactly
// the pixels it would from a window of its own.
static int stage_host_frames_to(Engine* e, StageArena& a, hipStream_t copy_on, const vt_frame* host, int n,
                                const float (*boxes)[4], const float* grow, vt_frame* dev, size_t* bytes_out,
                                bool pack_all = false, bool share = false) {
    std::vector<HostWin> wins((size_t)n);
    std::vector<char> mapped((size_t)n, 0);
    std::vector<int> first((size_t)n);          // the first slot with the same frame (itself: staged on its own)
    for (int i = 0; i < n; ++i) {
        first[(size_t)i] = i;
        for (int j = 0; share && j < i; ++j)
            if (first[(size_t)j] == j && same_host_frame(host[i], host[j])) { first[(size_t)i] = j; break; }
    }
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
        const vt_frame& hf = host[i];
        if (int rc = plan_window(e, hf, boxes[i], grow ? grow[i] : 0.0f, &wins[i])) return rc;
        // a frame inside a range mapped by vt_host_register goes to the kernels as it lies (zero copy) - on
        // single-stream engines, or where the caller asked for it: for a batched engine the packed upload beside
        // the previous pass is faster than PCIe reads inside the pass (vt_config.host_zero_copy, vittrack_hip.h)
        const bool zc = !pack_all && (e->host_zero_copy > 0 || (e->host_zero_copy == 0 && e->B == 1));
        if (!zc) continue;
        // bytes the kernels may touch: every row of the frame, the last one only as far as it is wide
        const bool sp = pix_family(hf.format) == PIXF_420SP;
        const size_t rowb = (size_t)hf.width * pix_row_bpp(hf.format);
        const size_t ext0 = (size_t)(hf.height - 1) * (size_t)hf.stride0 + rowb;
        const size_t crows = (size_t)pix_chroma_rows(hf.format, hf.height) * (pix_planar(hf.format) ? 2 : 1);
        const size_t ext1 = sp ? (crows - 1) * (size_t)hf.stride1 + (size_t)pix_chroma_row_bytes(hf.format, hf.width) : 0;
        const uint8_t* d0 = mapped_device_ptr(e->device, (const uint8_t*)hf.plane0, ext0);
        const uint8_t* d1 = sp ? mapped_device_ptr(e->device, (const uint8_t*)hf.plane1, ext1) : nullptr;
        if (d0 && (!sp || d1)) {
            mapped[(size_t)i] = 1;
            memset(&dev[i], 0, sizeof(vt_frame));
            dev[i].plane0 = d0; dev[i].plane1 = d1; dev[i].width = hf.width; dev[i].height = hf.height;
            dev[i].stride0 = hf.stride0; dev[i].stride1 = hf.stride1; dev[i].format = hf.format;
        }
    }
    for (int i = 0; i < n; ++i) {               // a shared frame's window grows to hold every slot's
        const int f = first[(size_t)i];
        if (f == i || mapped[(size_t)i]) continue;
        HostWin& u = wins[(size_t)f];
        const HostWin& w = wins[(size_t)i];
        const int x_hi = std::max(u.x_lo + u.ww, w.x_lo + w.ww), y_hi = std::max(u.y_lo + u.wh, w.y_lo + w.wh);
        u.x_lo = std::min(u.x_lo, w.x_lo); u.y_lo = std::min(u.y_lo, w.y_lo);
        u.ww = x_hi - u.x_lo; u.wh = y_hi - u.y_lo;
        size_window(&u);
    }
    for (int i = 0; i < n; ++i)
        if (!mapped[(size_t)i] && first[(size_t)i] == i) total += wins[(size_t)i].bytes;
    if (bytes_out) *bytes_out = total;
    if (total == 0) return VT_OK;            // every frame mapped: nothing to pack, nothing to copy
    DEVICE_SCOPE(e->device);
    if (total > a.cap) {        // grown only while nothing uses it
        HIPCHK(hipStreamSynchronize(e->stream));
        if (copy_on != e->stream) HIPCHK(hipStreamSynchronize(copy_on));
        if (int rc = a.ensure(total)) return rc;
    }
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        if (mapped[(size_t)i]) continue;
        if (first[(size_t)i] != i) { dev[i] = dev[first[(size_t)i]]; continue; }    // packed already: first[i] < i
        pack_window(a, wins[i], off, &dev[i]);
        off += wins[i].bytes;
    }
    HIPCHK(hipMemcpyAsync(a.d, a.h, total, hipMemcpyHostToDevice, copy_on));
    return VT_OK;
}

// the synchronous entry points: one arena, copy on the engine's own stream (every such call waits
// for its pass before returning, so the arena is free again at the next call)
int stage_host_frames(Engine* e, const vt_frame* host, int n, const float (*boxes)[4], vt_frame* dev, bool share) {
    return stage_host_frames_to(e, e->stage, e->stream, host, n, boxes, nullptr, dev, nullptr, false, share);
}

// ---- pipelined host passes -------------------------------------------------------------------------

static int host_slot_prepare(Engine* e, Engine::HostSlot& sl) {
    DEVICE_SCOPE(e->device);
    // whatever of the slot's sinks is missing: all of them at its first use, an optional feature's records at its first use
    // after that feature's enable (the enable itself covers the slots that exist, so no pass allocates for them)
    HIPCHK(e->sinks_alloc(&sl.out, e->sink_members()));
    if (sl.done_ev) return VT_OK;
    // HIP multiplexes a process's streams onto a few hardware queues (four by default): with more
    // streams than that alive - e.g. four engines, each with a compute and a copy stream - an upload
    // can share a queue with some engine's compute stream and is then ordered behind that engine's
    // whole pass (measured: pipelined = synchronous throughput; a high-priority copy stream did not
    // change that). Two engines per process (2 + 2 streams) keep the overlap: 99.5 % of the
    // HBM-resident rate.
    if (!e->copy_stream) HIPCHK(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
    if (!sl.up_ev) HIPCHK(hipEventCreateWithFlags(&sl.up_ev, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&sl.done_ev, hipEventDisableTiming));
    return VT_OK;
}

// the boxes the windows of a pass over streams[0..n) (null: all streams in order) are planned around: the last the
// host knows - on a motion-capable engine moved as the pass's place launch will move them (Engine::predicted_box: the
// same binary32 operations on the mirrored record, so an exact window stays exact)
// spec (per listed stream, may be null): the stream is in the pass still running, so what the host knows is one pass
// old - its box is moved by the known velocity for that pass as well
static std::vector<float> known_boxes(const Engine* e, const int32_t* streams, int n, const char* spec = nullptr) {
    std::vector<float> boxes((size_t)n * 4);
    for (int i = 0; i < n; ++i) e->predicted_box(streams ? streams[i] : i, &boxes[(size_t)i * 4], spec && spec[i] ? 2 : 1);
    return boxes;
}

// One synchronous host pass over streams[0..n) (null: all streams in order): every window cut around its stream's own
// last box, the pass enqueued and waited for. vt_group_update_host is the null list.
static int update_host_pass(Engine* e, const int32_t* streams, const vt_frame* host_frames, int n, vt_result* out,
                            const char* what) {
    if (int rc = refuse_while_pipelined(e, what)) return rc;
    if (int rc = e->check_streams(streams, n)) return rc;
    DEVICE_SCOPE(e->device);
    if (int rc = e->wait(nullptr, 0)) return rc;   // last pass done: its boxes are in `known`
    std::vector<vt_frame> dev((size_t)n);
    const std::vector<float> boxes = known_boxes(e, streams, n);
    if (int rc = stage_host_frames(e, host_frames, n, reinterpret_cast<const float(*)[4]>(boxes.data()), dev.data()))
        return rc;
    if (int rc = e->enqueue(streams, dev.data(), n)) return rc;
    return e->wait(out, n);
}

// a collected (or redone) pass becomes what the host knows: the entries of ITS streams move, no others. The
// decode kernel stores a slot's results by slot and its states by stream (k_head.hip: decode_box).
static void adopt_peaks(Engine* e, const Engine::HostSlot& sl) {
    if (!e->peaks_capable || !sl.out.host_peaks) return;
    for (size_t i = 0; i < sl.list.size(); ++i) e->h_peaks[i] = sl.out.host_peaks[i];
    e->peaks_n = (int)sl.list.size();
}
static void adopt_slot(Engine* e, const Engine::HostSlot& sl) {
    for (size_t i = 0; i < sl.list.size(); ++i) {
        const int s = sl.list[i];
        e->known[s] = sl.out.host_states[s];
        e->h_states_all[s] = sl.out.host_states[s];        // the engine's own mirrors follow
        e->adopt_stream_sinks(sl.out, s);                  // ... and those of the optional by-stream records
        if (e->motion_capable && sl.out.host_motion) e->known_motion[(size_t)s] = sl.out.host_motion[s];
        e->h_results[i] = sl.out.host_results[i];
    }
    adopt_peaks(e, sl);                         // the peak records are by slot, like the results
}

// exact (non-speculative) synchronous pass over the slot's frames and list with the states the device holds
// now; results and states land in the slot's buffers
static int host_pass_exact_sync(Engine* e, Engine::HostSlot& sl) {
    const int n = (int)sl.list.size();
    std::vector<vt_frame> dev((size_t)n);
    const std::vector<float> boxes = known_boxes(e, sl.list.data(), n);
    if (int rc = stage_host_frames(e, sl.host.data(), n, reinterpret_cast<const float(*)[4]>(boxes.data()), dev.data()))
        return rc;
    if (int rc = e->enqueue(sl.list.data(), dev.data(), n, &sl.out)) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    adopt_slot(e, sl);
    sl.redone = true;
    return VT_OK;
}

// One pipelined pass over streams[0..n) (checked by the caller): windows packed into the free slot's arena and
// uploaded on the copy stream, the pass enqueued behind that upload. vt_group_enqueue_host is the identity list.
static int enqueue_host_pass(Engine* e, const int32_t* streams, const vt_frame* host_frames, int n, const char* what) {
    const unsigned outstanding = e->host_seq - e->host_collected;
    if (outstanding >= 2)
        return set_err(VT_ERR_INVALID_ARG, "%s: two passes outstanding, call vt_group_wait_next first", what);
    DEVICE_SCOPE(e->device);
    Engine::HostSlot& sl = e->hs[e->host_seq & 1];
    if (int rc = host_slot_prepare(e, sl)) return rc;
    if (outstanding == 0) {
        // nothing of ours is running: make sure nothing else is either, then the boxes are exact
        if (int rc = e->wait(nullptr, 0)) return rc;
    }
    // a stream that is in the pass still outstanding has a box nobody knows yet: its window is cut around the last
    // known one, enlarged; every other stream's known box is exact, and so is its window - it cannot cause a redo
    const Engine::HostSlot& older = e->hs[(e->host_seq + 1) & 1];
    std::vector<char> spec((size_t)n, 0);
    std::vector<float> grow((size_t)n, 0.0f);
    for (int i = 0; i < n; ++i)
        if (outstanding == 1 && older.lists(streams[i])) { spec[(size_t)i] = 1; grow[(size_t)i] = e->margin; }
    std::vector<vt_frame> dev((size_t)n);
    const std::vector<float> boxes = known_boxes(e, streams, n, spec.data());
    if (int rc = stage_host_frames_to(e, sl.arena, e->copy_stream, host_frames, n,
                                      reinterpret_cast<const float(*)[4]>(boxes.data()), grow.data(), dev.data(), nullptr))
        return rc;
    HIPCHK(hipEventRecord(sl.up_ev, e->copy_stream));
    HIPCHK(hipStreamWaitEvent(e->stream, sl.up_ev, 0));          // the pass starts behind ITS upload only
    if (int rc = e->enqueue(streams, dev.data(), n, &sl.out)) return rc;   // results land in THIS slot's buffers
    HIPCHK(hipEventRecord(sl.done_ev, e->stream));
    sl.host.assign(host_frames, host_frames + n);
    sl.list.assign(streams, streams + n);
    sl.spec.swap(spec);
    sl.redone = false;
    sl.pending = true;
    e->host_seq += 1;
    return VT_OK;
}

// staging for one queued init with an arena of `need` bytes: one whose work on the group's stream is done, else a
// new one. Never grown in place: freeing device memory waits for the device, and a queued init waits for nothing.
static int queued_init_staging(Engine* e, size_t need, Engine::QueuedInit** out) {
    for (Engine::QueuedInit* q : e->qinits)
        if (q && q->arena.cap >= need && q->done_ev && hipEventQuery(q->done_ev) == hipSuccess) { *out = q; return VT_OK; }
    (void)hipGetLastError();                 // hipErrorNotReady of the queries above is no error
    e->qinits.push_back(nullptr);
    Engine::QueuedInit* q = e->qinits.back() = new Engine::QueuedInit();   // the engine's from here on, whatever fails below
    HIPCHK(hipHostMalloc((void**)&q->h_state, sizeof(StreamState)));
    HIPCHK(hipHostMalloc((void**)&q->h_desc, sizeof(FrameDesc)));
    HIPCHK(hipEventCreateWithFlags(&q->up_ev, hipEventDisableTiming));
    if (int rc = q->arena.ensure(need)) return rc;        // fresh: nothing is freed, nothing waits
    HIPCHK(hipEventCreateWithFlags(&q->done_ev, hipEventDisableTiming));   // last: a half-built one is never picked
    *out = q;
    return VT_OK;
}

extern "C" {

int vt_group_init_host(vt_group* g, int stream, const vt_frame* host_frame, vt_bbox box) try {
    if (!g || !host_frame) return set_err(VT_ERR_INVALID_ARG, "null argument");
    Engine* e = g->e;
    if (stream < 0 || stream >= e->B) return set_err(VT_ERR_INVALID_ARG, "bad stream index");
    if (int rc = refuse_while_pipelined(e, "init_host")) return rc;
    DEVICE_SCOPE(e->device);
    HIPCHK(hipStreamSynchronize(e->stream));     // the staging arena is shared by the group's passes
    const float fb[1][4] = {{(float)box.x, (float)box.y, (float)box.width, (float)box.height}};
    vt_frame f;
    if (int rc = stage_host_frames(e, host_frame, 1, fb, &f)) return rc;
    return e->init_stream(stream, &f, box);
} VT_NOTHROW_INT

int vt_group_update_host(vt_group* g, const vt_frame* host_frames, int n, vt_result* out) try {
    if (!g || !host_frames || !out) return set_err(VT_ERR_INVALID_ARG, "null argument");
    Engine* e = g->e;
    if (n != e->B) return set_err(VT_ERR_INVALID_ARG, "update_host: need exactly %d frames", e->B);
    for (int b = 0; b < n; ++b)
        if (!e->h_initialized[b]) return set_err(VT_ERR_NOT_INITIALIZED, "stream %d not initialised", b);
    return update_host_pass(e, nullptr, host_frames, n, out, "update_host");
} VT_NOTHROW_INT

// the same window logic on the n streams of a subset pass: stream streams[i]'s window is cut around its own last box
int vt_group_update_host_streams(vt_group* g, const int32_t* streams, const vt_frame* host_frames, int n,
                                 vt_result* out) try {
    if (!g || !streams || !host_frames || !out) return set_err(VT_ERR_INVALID_ARG, "null argument");
    return update_host_pass(g->e, streams, host_frames, n, out, "update_host_streams");
} VT_NOTHROW_INT

// A candidate pass on host frames: every slot's window is cut around the slot's own box (exact: nothing is
// speculative, no redo), slots on one host frame share one staged rectangle; then the device form.
int vt_group_update_host_candidates(vt_group* g, const vt_candidate* cands, const vt_frame* host_frames, int n,
                                    vt_result* out, int32_t* winner) try {
    if (!g || !cands || !host_frames || !out) return set_err(VT_ERR_INVALID_ARG, "null argument");
    Engine* e = g->e;
    if (int rc = refuse_while_pipelined(e, "update_host_candidates")) return rc;
    if (int rc = e->check_candidates(cands, n)) return rc;
    DEVICE_SCOPE(e->device);
    if (int rc = e->wait(nullptr, 0)) return rc;   // last pass done: its boxes are in `known`
    std::vector<float> boxes((size_t)n * 4);
    for (int i = 0; i < n; ++i) {       // a slot without a box is cut around its stream's (predicted) box
        if (cands[i].has_box) memcpy(&boxes[(size_t)i * 4], cands[i].box, 4 * sizeof(float));
        else e->predicted_box(cands[i].stream, &boxes[(size_t)i * 4]);
    }
    std::vector<vt_frame> dev((size_t)n);
    if (int rc = stage_host_frames(e, host_frames, n, reinterpret_cast<const float(*)[4]>(boxes.data()), dev.data(), true))
        return rc;
    if (int rc = e->enqueue_candidates(cands, dev.data(), n)) return rc;
    return e->wait_candidates(out, winner, n);
} VT_NOTHROW_INT

int vt_group_enqueue_host(vt_group* g, const vt_frame* host_frames, int n) try {
    if (!g || !host_frames) return set_err(VT_ERR_INVALID_ARG, "null argument");
    Engine* e = g->e;
    if (n != e->B) return set_err(VT_ERR_INVALID_ARG, "enqueue_host: need exactly %d frames", e->B);
    for (int b = 0; b < n; ++b)
        if (!e->h_initialized[b]) return set_err(VT_ERR_NOT_INITIALIZED, "stream %d not initialised", b);
    std::vector<int32_t> all((size_t)n);
    for (int b = 0; b < n; ++b) all[(size_t)b] = b;
    return enqueue_host_pass(e, all.data(), host_frames, n, "enqueue_host");
} VT_NOTHROW_INT

int vt_group_enqueue_host_streams(vt_group* g, const int32_t* streams, const vt_frame* host_frames, int n) try {
    if (!g || !streams || !host_frames) return set_err(VT_ERR_INVALID_ARG, "null argument");
    Engine* e = g->e;
    if (int rc = e->check_streams(streams, n)) return rc;
    return enqueue_host_pass(e, streams, host_frames, n, "enqueue_host_streams");
} VT_NOTHROW_INT

int vt_group_enqueue_init_host(vt_group* g, int stream, const vt_frame* host_frame, vt_bbox box) try {
    if (!g || !host_frame) return set_err(VT_ERR_INVALID_ARG, "null argument");
    Engine* e = g->e;
    if (stream < 0 || stream >= e->B) return set_err(VT_ERR_INVALID_ARG, "bad stream index");
    if (e->host_seq == e->host_collected) return vt_group_init_host(g, stream, host_frame, box);
    for (const Engine::HostSlot& sl : e->hs)
        if (sl.pending && sl.lists(stream))
            return set_err(VT_ERR_INVALID_ARG, "enqueue_init_host: stream %d is in an outstanding pass, collect it "
                           "first (vt_group_wait_next)", stream);
    if (int rc = e->check_init_box(box)) return rc;
    // the frame's own checks, before anything is allocated or changed
    const float fb[1][4] = {{(float)box.x, (float)box.y, (float)box.width, (float)box.height}};
    HostWin probe;
    if (int rc = plan_window(e, *host_frame, fb[0], 0.0f, &probe)) return rc;
    DEVICE_SCOPE(e->device);
    // the first stream on a format other than RGB8 / NV12 / YUY2 has the second graph set captured; a capture needs
    // the group's stream idle, so this one call waits for the outstanding passes (they stay uncollected): never a
    // capture beside a running pass
    if (int rc = e->capture_graphs_for(host_frame->format)) return rc;
    Engine::QueuedInit* q = nullptr;
    if (int rc = queued_init_staging(e, probe.bytes, &q)) return rc;
    // window packed into the init's own pinned arena now (the caller's buffer is free on return), uploaded on the
    // copy stream; the state write and the template crop go on the group's stream behind the passes already queued
    // and behind that upload. Nothing here waits for the group's stream.
    vt_frame f;
    size_t up_bytes = 0;
    // packed also from registered memory: the crop runs after this call has returned
    if (int rc = stage_host_frames_to(e, q->arena, e->copy_stream, host_frame, 1, fb, nullptr, &f, &up_bytes, true)) return rc;
    if (int rc = check_frame(f)) return rc;
    if (up_bytes) {
        HIPCHK(hipEventRecord(q->up_ev, e->copy_stream));
        HIPCHK(hipStreamWaitEvent(e->stream, q->up_ev, 0));
    }
    const int rc = e->launch_init(stream, &f, box, q->h_state, q->h_desc);
    HIPCHK(hipEventRecord(q->done_ev, e->stream));   // also after a failed launch: the staging is busy until then
    if (rc) return rc;
    // what the host knows of this stream is its init state from now on: the next window is cut around the init box,
    // exact, and a rewind behind this init restores the initialised state (the template rows are not rewound)
    e->known[stream] = *q->h_state;
    e->h_states_all[stream] = *q->h_state;
    e->h_initialized[stream] = 1;
    return VT_OK;
} VT_NOTHROW_INT

int vt_group_wait_next(vt_group* g, vt_result* out, int n) try {
    if (!g) return set_err(VT_ERR_INVALID_ARG, "null group");
    Engine* e = g->e;
    if (e->host_seq == e->host_collected) return set_err(VT_ERR_INVALID_ARG, "wait_next: no pass outstanding");
    DEVICE_SCOPE(e->device);
    Engine::HostSlot& sl = e->hs[e->host_collected & 1];
    Engine::HostSlot& younger = e->hs[(e->host_collected + 1) & 1];
    const bool has_younger = e->host_seq - e->host_collected == 2;
    const int pass_n = (int)sl.list.size();
    if (!sl.redone) {
        HIPCHK(hipEventSynchronize(sl.done_ev));
        bool miss = false;
        for (int i = 0; i < pass_n; ++i) {
            const StreamState& st = sl.out.host_states[sl.list[(size_t)i]];
            miss = miss || (sl.spec[(size_t)i] && st.window_miss != 0 && st.window_miss == st.frames_done);
        }
        if (miss) {
            // a stream moved out of its speculative window: rewind the streams of this pass and of the one queued
            // behind it to the states they started from - `known`, the host's copy of the states the last collected
            // pass (or a queued init) left each of them - and redo this pass over its list, then the younger one,
            // which may have consumed its wrong states, over its own, with exact windows. The same lists: a stream's
            // bits depend on the pass size. Streams in neither pass are not touched.
            e->host_redos += 1;
            HIPCHK(hipStreamSynchronize(e->stream));
            if (int rc = e->reset_refresh_tickets()) return rc;      // nothing is running: no half-counted refresh survives
            // (a rewound tpl_gen names the stream's old template buffer again: a span holds at most one refresh of a stream)
            std::vector<char> rewind((size_t)e->B, 0);
            for (int s : sl.list) rewind[(size_t)s] = 1;
            if (has_younger)
                for (int s : younger.list) rewind[(size_t)s] = 1;
            for (int b = 0; b < e->B; ++b)
                if (rewind[(size_t)b]) {
                    HIPCHK(hipMemcpy(e->d_states + b, &e->known[(size_t)b], sizeof(StreamState), hipMemcpyHostToDevice));
                    if (e->motion_capable)      // the records rewind with the states they belong to
                        HIPCHK(hipMemcpy(e->d_motion_recs() + b, &e->known_motion[(size_t)b], sizeof(MotionRec), hipMemcpyHostToDevice));
                }
            if (int rc = host_pass_exact_sync(e, sl)) return rc;
            if (has_younger)
                if (int rc = host_pass_exact_sync(e, younger)) return rc;
        }
    }
    if (out)
        for (int i = 0; i < std::min(n, pass_n); ++i) out[i] = sl.out.host_results[i];
    // boxes the next window is planned around: this pass's - unless a younger pass was redone just
    // now, whose states are newer (host_pass_exact_sync adopted both already, in order)
    if (!(has_younger && younger.redone)) adopt_slot(e, sl);
    else adopt_peaks(e, sl);                    // last_peaks follows the results handed out above, whichever states are newer
    sl.pending = false;
    e->host_collected += 1;
    return VT_OK;
} VT_NOTHROW_INT


}  // extern "C"
