// vt_ops_util.hpp — what the operator entry points (vt_ops.hip) share on the device side: buffers that know their size,
// guard bands, the timing loop, the operand set of a GEMM launch and the slot maps of the in-the-pass launches.
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

// pinned, device-visible host memory (what PassOut points the decode at)
struct PinnedBuf {
    void* p = nullptr;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t n) { return hipHostMalloc(&p, n ? n : 4); }
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

// The two optional maps of an in-the-pass launch over n slots: slot_stream (slot -> stream < n_streams) and winner (a
// candidate pass's winner table, entries < n). check(hook, b) is VT_OK or the refusal of slot b, under the hook's name.
struct SlotMaps {
    const int32_t *slot_stream, *winner;
    int n, n_streams;
    DevArr dmap, dwin;
    int check(const char* hook, int b) const {
        if (slot_stream && (slot_stream[b] < 0 || slot_stream[b] >= n_streams))
            return set_err(VT_ERR_INVALID_ARG, "%s: slot %d names stream %d of %d", hook, b, (int)slot_stream[b], n_streams);
        if (winner && (winner[b] < 0 || winner[b] >= n))
            return set_err(VT_ERR_INVALID_ARG, "%s: winner[%d] = %d of %d slots", hook, b, (int)winner[b], n);
        return VT_OK;
    }
    hipError_t upload() {
        const hipError_t e = dmap.upload(slot_stream, (size_t)n * 4);
        return e != hipSuccess ? e : dwin.upload(winner, (size_t)n * 4);
    }
    const int32_t* dev_slot_stream() const { return dmap.as<const int32_t>(); }
    const int32_t* dev_winner() const { return dwin.as<const int32_t>(); }
};
