// vt_ops_util.hpp — what the operator entry points (vt_ops.hip) share on the device side: buffers that know their size,
// guard bands, the timing loop, the operand set of a GEMM launch and, for the in-the-pass launches, the slot maps, the frame
// list, the pinned mirrors and the policy words through a key table.
#pragma once
#include <initializer_list>
#include <utility>

#include "vt_engine.hpp"
#include "vt_ops_host.hpp"

static_assert(kLoShiftMin == VT_LO_SHIFT_MIN && kLoShiftMax == VT_LO_SHIFT_MAX, "vt_ops_host.hpp restates the range of lo_shift");

// A device buffer that takes its byte count once: alloc / zeros / filled / upload set it, download copies that many back.
// upload of a null pointer (an optional operand) leaves the buffer empty, and as<T>() of an empty buffer is nullptr.
struct DevArr : DevBuf {
    size_t bytes = 0;
    hipError_t alloc(size_t n) { bytes = n; return DevBuf::alloc(n); }
    hipError_t filled(size_t n, int byte) {
        const hipError_t e = alloc(n);
        return e != hipSuccess ? e : hipMemset(p, byte, n);
    }
    hipError_t zeros(size_t n) { return filled(n, 0); }
    // pad: bytes allocated behind the n uploaded ones, for a kernel whose last vector load reaches past its operand
    hipError_t upload(const void* host, size_t n, size_t pad = 0) {
        if (!host) return hipSuccess;
        const hipError_t e = DevBuf::alloc(n + pad);
        bytes = n;
        return e != hipSuccess ? e : hipMemcpy(p, host, n, hipMemcpyHostToDevice);
    }
    hipError_t download(void* host) const { return hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// An optional pinned, device-visible mirror of a caller's host array (what PassOut points a launch at): from() copies the
// caller's bytes in, back() - after the guards are checked - copies them out. A null host pointer: as<T>() is null, no copy.
struct Mirror {
    void *p = nullptr, *host = nullptr;
    size_t bytes = 0;
    ~Mirror() { if (p) (void)hipHostFree(p); }
    hipError_t from(void* h, size_t n) {
        if (!h) return hipSuccess;
        host = h; bytes = n;
        const hipError_t e = hipHostMalloc(&p, n ? n : 4);
        if (e == hipSuccess) memcpy(p, h, n);
        return e;
    }
    void back() const { if (host) memcpy(host, p, bytes); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// The output buffer of a hook between two guard bands: the bands carry a byte pattern, the output 0xff (a
// bf16 NaN), so a row the kernel never stores arrives as NaN instead of whatever a reused allocation held, and a store
// just outside the buffer (a slip in a row or block index) is reported instead of landing in a neighbour's memory.
// A buffer whose start value is part of the kernel's contract takes that value instead: another byte (zeros for V^T and
// the counters) or the caller's bytes (upload: an addend updated in place, states, records).
struct GuardedOut {
    static constexpr size_t kGuard = 4096;      // bytes on each side; keeps out() 4 KiB aligned
    static constexpr int kPattern = 0xA5;
    DevBuf buf;
    size_t bytes = 0;
    hipError_t alloc(size_t n, int start = 0xff) {
        bytes = n;
        hipError_t e = buf.alloc(n + 2 * kGuard);
        if (e != hipSuccess) return e;
        e = hipMemset(buf.p, kPattern, n + 2 * kGuard);
        if (e != hipSuccess) return e;
        return hipMemset(out(), start, n);
    }
    hipError_t upload(const void* host, size_t n) {
        const hipError_t e = alloc(n);
        return e != hipSuccess ? e : hipMemcpy(out(), host, n, hipMemcpyHostToDevice);
    }
    void* out() const { return static_cast<char*>(buf.p) + kGuard; }
    template <class T> T* as() const { return static_cast<T*>(out()); }
    hipError_t download(void* host) const { return hipMemcpy(host, out(), bytes, hipMemcpyDeviceToHost); }
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

// after the synchronise: VT_OK when the bands of every listed output (one never allocated is passed over) are intact
static inline int guards_intact(const char* what, std::initializer_list<std::pair<const GuardedOut*, const char*>> outs) {
    for (const auto& o : outs) {
        if (!o.first->bytes) continue;
        long where = 0;
        HIPCHK(o.first->check(&where));
        if (where) return set_err(VT_ERR_HIP, "%s wrote outside its %s: guard byte %ld changed", what, o.second, where);
    }
    return VT_OK;
}

// `count` bf16 values of a device buffer, widened to float32
static inline hipError_t download_bf16(const void* dev, size_t count, float* out) {
    std::vector<bf16_t> tmp(count);
    const hipError_t e = hipMemcpy(tmp.data(), dev, count * 2, hipMemcpyDeviceToHost);
    if (e == hipSuccess) widen_bf16(tmp.data(), count, out);
    return e;
}

// Mean microseconds per launch on the null stream: three launches to warm up, then `iters` of them between two events.
// The events are destroyed on every way out.
template <class F>
static inline hipError_t time_launches(int iters, F launch, float* us_out) {
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    hipError_t e = hipSuccess;
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = launch();
    if (e == hipSuccess) e = hipEventCreate(&ev.e0);
    if (e == hipSuccess) e = hipEventCreate(&ev.e1);
    if (e == hipSuccess) e = hipEventRecord(ev.e0, nullptr);
    for (int i = 0; i < iters && e == hipSuccess; ++i) e = launch();
    if (e == hipSuccess) e = hipEventRecord(ev.e1, nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(ev.e1);
    float ms = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev.e0, ev.e1);
    if (e == hipSuccess) *us_out = ms * 1000.0f / iters;
    return e;
}

// The operands every GEMM-shaped hook gives its launch: a [M][lda] and w [N][K] (bf16 bits), bias [N] (null: zeros)
struct GemmOperands {
    DevArr a, w, bias;
    hipError_t upload(GemmArgs& g, const uint16_t* ha, const uint16_t* hw, const float* hbias, size_t M, int N, int K, int lda) {
        hipError_t e = a.upload(ha, M * lda * 2);
        if (e == hipSuccess) e = w.upload(hw, (size_t)N * K * 2);
        if (e == hipSuccess) e = hbias ? bias.upload(hbias, (size_t)N * 4) : bias.zeros((size_t)N * 4);
        g.A = a.as<const bf16_t>(); g.lda = lda; g.W = w.as<const bf16_t>(); g.ldw = K; g.bias = bias.as<const float>();
        g.M = (int)M; g.N = N; g.K = K;
        return e;
    }
};

// after the guards: every ticket of `per` per slot came back to zero by itself
static inline int tickets_returned(const char* hook, const GuardedOut& tickets, size_t per) {
    std::vector<unsigned> t(tickets.bytes / sizeof(unsigned));
    HIPCHK(tickets.download(t.data()));
    for (size_t i = 0; i < t.size(); ++i) {
        if (!t[i]) continue;
        char peak[32] = "";
        if (per > 1) snprintf(peak, sizeof(peak), ", peak %zu", i % per);
        return set_err(VT_ERR_HIP, "%s: slot %zu%s left its ticket at %u", hook, i / per, peak, t[i]);
    }
    return VT_OK;
}

// the dimensions the in-the-pass crops read: template T (search S), patch, padded patch columns, norm (a0, a1, a2, b0, b1, b2)
static inline ModelDims model_dims(int T, int S, int patch, int kpad, const float* norm) {
    ModelDims d{};
    d.T = T; d.S = S; d.patch = patch; d.gt = T / patch; d.nt = d.gt * d.gt; d.kpad = kpad;
    for (int c = 0; c < 3; ++c) { d.norm_a[c] = norm[c]; d.norm_b[c] = norm[3 + c]; }
    return d;
}

// A hook's policy words through its feature's key table (vt_feature_keys.hpp): VT_OK and *pol filled, or the refusal of the
// first word the table refuses, in the words every hook uses
template <class Pol, int N>
static inline int policy_from_words(const char* hook, const vtkeys::Key (&rows)[N], vtkeys::Apply apply, const Pol& def,
                                    const int32_t* policy, Pol* pol) {
    static_assert(sizeof(Pol) <= sizeof(int32_t) * vtkeys::kMaxWords, "a policy is at most kMaxWords words");
    int32_t words[vtkeys::kMaxWords] = {};
    const int bad = vtkeys::check_words(rows, apply, reinterpret_cast<const int32_t*>(&def), policy, words);
    if (bad >= 0)
        return set_err(VT_ERR_INVALID_ARG, "%s: policy word %d (%s) = %d refused", hook, rows[bad].word, rows[bad].key,
                       (int)policy[rows[bad].word]);
    memcpy(pol, words, sizeof(Pol));
    return VT_OK;
}

// The frames of an in-the-pass launch, one per slot: check() refuses what check_frame refuses and keeps the descriptors and
// the highest pixel level among the formats; upload() is the last step before the launches.
struct HookFrames {
    std::vector<FrameDesc> desc;
    int level = 0;
    DevArr dfr, dflag;
    int check(const vt_frame* frames, int n) {
        desc.resize((size_t)n);
        for (int b = 0; b < n; ++b) {
            if (int rc = check_frame(frames[b])) return rc;
            to_desc(frames[b], &desc[(size_t)b]);
            level = std::max(level, pix_level(frames[b].format));
        }
        return VT_OK;
    }
    hipError_t upload(int device_frames = 1) {
        const int32_t flag = device_frames != 0;
        hipError_t e = dfr.upload(desc.data(), desc.size() * sizeof(FrameDesc));
        if (e == hipSuccess) e = dflag.upload(&flag, 4);
        return e != hipSuccess ? e : hipDeviceSynchronize();    // the caller's frames may have been filled on another stream
    }
    const FrameDesc* dev() const { return dfr.as<const FrameDesc>(); }
    const int32_t* dev_flag() const { return dflag.as<const int32_t>(); }
};

// The two optional maps of an in-the-pass launch over n slots: slot_stream (slot -> stream < n_streams) and winner (a
// candidate pass's winner table, entries < n). check_all(hook) is VT_OK or the first refusal, under the hook's name.
struct SlotMaps {
    const int32_t *slot_stream, *winner;
    int n, n_streams;
    DevArr dmap, dwin;
    // noun: what the hook calls the records a stream indexes; without a map, slot b is stream b
    int check_all(const char* hook, const char* noun = "streams") const {
        if (!slot_stream && n_streams < n) return set_err(VT_ERR_INVALID_ARG, "%s: %d %s for %d slots", hook, n_streams, noun, n);
        for (int b = 0; b < n; ++b) {
            if (slot_stream && (slot_stream[b] < 0 || slot_stream[b] >= n_streams))
                return set_err(VT_ERR_INVALID_ARG, "%s: slot %d names stream %d of %d", hook, b, (int)slot_stream[b], n_streams);
            if (winner && (winner[b] < 0 || winner[b] >= n))
                return set_err(VT_ERR_INVALID_ARG, "%s: winner[%d] = %d of %d slots", hook, b, (int)winner[b], n);
        }
        return VT_OK;
    }
    // after check_all: outside a candidate pass (no winner table) no stream has two writers - two slots of one stream would
    // write the same record, state and counters from two workgroups. twice: the hook's words for it
    int check_unique(const char* hook, const char* twice) const {
        if (!slot_stream || winner) return VT_OK;
        std::vector<char> named((size_t)n_streams, 0);
        for (int b = 0; b < n; ++b) {
            if (named[(size_t)slot_stream[b]]) return set_err(VT_ERR_INVALID_ARG, "%s: stream %d %s", hook, (int)slot_stream[b], twice);
            named[(size_t)slot_stream[b]] = 1;
        }
        return VT_OK;
    }
    hipError_t upload() {
        const hipError_t e = dmap.upload(slot_stream, (size_t)n * 4);
        return e != hipSuccess ? e : dwin.upload(winner, (size_t)n * 4);
    }
    const int32_t* dev_slot_stream() const { return dmap.as<const int32_t>(); }
    const int32_t* dev_winner() const { return dwin.as<const int32_t>(); }
};
