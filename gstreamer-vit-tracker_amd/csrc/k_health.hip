// k_health.hip — frame health ("Frame health"; the rule to the bit: include/vittrack_hip_ops.h,
// vt_op_frame_health): is the picture of a stream frozen, flat, or cut to another scene.
//
// Four launches, built to sit behind the decode (the commit) and ahead of everything that cuts or draws - the thumbnail is
// taken from undrawn pixels -, directly behind conflicts_check; refresh rule 10 (k_refresh.hip) reads the record:
//
// health_prepare, one workgroup per slot: the workgroup looks through the slots ahead for the stream's first slot (up to
// 1023 entries: four coalesced loads per thread, not a thousand dependent ones), then thread 0 evaluates the due rule, the whole-frame test, the geometry and the
// previous thumbnail's from wave-uniform loads and writes the slot's header, which the three launches behind obey, and the
// thumbnails' bookkeeping of the stream's record; where the stream is measured the workgroup zeroes the stream's four
// accumulators and its current histogram.
//
// health_thumb, grid (max_cells / 256, slots): one thread per thumbnail cell, the sixteen taps of camera motion's cell
// (k_thumb_dev.hpp), one uint16 store. Folded in, while the thread holds its cell: S1 = sum t, S2 = sum t * t, D = sum
// |t - p| against the previous thumbnail at the same index (status 1), and the histogram of t >> 7. The sums go thread ->
// wave (64-lane shuffles, 32 bits: 64 * 4080^2 < 2^32) -> LDS -> one 64-bit integer atomic per quantity and workgroup; the
// histogram is counted in LDS and leaves with at most 32 32-bit atomics per workgroup (empty bins send none).
//
// health_measure, same grid: G. A thread reads its cell and the cells right of and below it from the thumbnail the launch
// ahead stored: at most 512 KiB per stream, written microseconds earlier, so the reads are L2-resident and coalesced
// (cell + 1, cell + Wg); no halo is staged in LDS - every cell would be staged to be read twice. The sum leaves like the others.
//
// health_decide, one workgroup per slot: HD over the 32 bins, still, the flags, G_ref, the record to the device array and
// the pass's pinned mirror (PassOut.host_health), the counters.
//
// Integers only: nothing in this file is a floating-point operation, and no sum depends on the order of its additions. (A
// tap reaches the cell function as the pixel fetch's three float values, exact integers 0..255, and is an int from its
// first use on: k_thumb_dev.hpp.) Launch dimensions depend on max_cells and
// the slot count alone; workgroups of slots that are not measured, and those beyond Wg * Hg, leave at once from wave-uniform
// loads of the header. Only the feature's own buffers are written.
#include "k_health.hpp"
#include "k_camera_motion.hpp"  // cam_auto_cell: the automatic cell is the camera motion's
#include "k_thumb_dev.hpp"

static constexpr int kHealthRecWords = sizeof(HealthRec) / 4;

__device__ __forceinline__ bool health_measured(int status) { return status == 1 || status == 5; }

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;       // lane 0 holds the wave's sum
}

__global__ __launch_bounds__(256) void health_prepare_kernel(HealthArgs a) {
    __shared__ int s_zero;
    __shared__ int s_cur;
    __shared__ int s_later;
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int stream = a.slot_stream ? a.slot_stream[slot] : slot;
    // the first slot naming the stream works for it: the slots ahead are looked through by the whole workgroup, coalesced
    if (tid == 0) s_later = 0;
    __syncthreads();
    if (a.slot_stream)
        for (int j = tid; j < slot; j += 256)
            if (a.slot_stream[j] == stream) s_later = 1;    // every writer stores the same value
    __syncthreads();
    if (tid == 0) {
        const HealthPolicy pol = *a.policy;
        HealthHead h{};
        h.stream = stream;
        if (s_later) {
            h.status = -1;
        } else {
            const StreamState& st = a.states[stream];
            const FrameDesc& f = a.frames[slot];
            HealthRec* r = a.recs + stream;
            h.frames_done = st.frames_done;
            int status = (pol.on != 0 && st.initialized && st.frames_done % pol.period == 0) ? 1 : 0;
            // a whole frame in device memory
            if (status == 1 && (*a.devflag == 0 || f.x0 != 0 || f.y0 != 0 || f.ww != f.w || f.wh != f.h)) status = 4;
            if (status == 1) {  // the geometry
                const int c = pol.cell ? pol.cell : cam_auto_cell(f.w, f.h, a.max_cells);
                status = 2;
                if (c > 0) {
                    h.c = c; h.Wg = f.w / c; h.Hg = f.h / c;
                    if ((long long)h.Wg * h.Hg <= (long long)a.max_cells && h.Wg >= 8 && h.Hg >= 8) status = 1;
                }
            }
            if (status == 1) {
                const bool prev = r->has_prev && r->pW == f.w && r->pH == f.h && r->pc == h.c;
                h.cur = r->has_prev ? (r->cur ^ 1) & 1 : 0;
                if (!prev) status = 5;
                r->has_prev = 1; r->cur = h.cur; r->pW = f.w; r->pH = f.h; r->pc = h.c;
            } else if (status != 0) {
                r->has_prev = 0;    // statuses 2 and 4; a pass that is not due keeps the previous thumbnail
            }
            h.status = status;
        }
        a.heads[slot] = h;
        s_zero = health_measured(h.status) ? 1 : 0;
        s_cur = h.cur;
    }
    __syncthreads();
    if (!s_zero) return;
    if (tid < HEALTH_ACCS) a.accs[(size_t)stream * HEALTH_ACCS + tid] = 0ull;
    if (tid >= 64 && tid < 64 + VT_HEALTH_BINS) a.hist[((size_t)stream * 2 + s_cur) * VT_HEALTH_BINS + (tid - 64)] = 0;
}

template <int ANY>
__global__ __launch_bounds__(256) void health_thumb_kernel(HealthArgs a) {
    __shared__ unsigned s_part[4][3];
    __shared__ int s_hist[VT_HEALTH_BINS];
    const int slot = blockIdx.y, tid = threadIdx.x;
    const HealthHead& h = a.heads[slot];
    const int status = h.status;
    if (!health_measured(status)) return;
    const int Wg = h.Wg, cells = Wg * h.Hg;
    if ((int)blockIdx.x * 256 >= cells) return;         // the whole workgroup
    if (tid < VT_HEALTH_BINS) s_hist[tid] = 0;
    __syncthreads();
    const int cell = blockIdx.x * 256 + tid;
    unsigned t = 0, d = 0;
    if (cell < cells) {
        const int j = cell / Wg, i = cell - j * Wg;
        t = (unsigned)thumb_cell<ANY>(a.frames[slot], i, j, h.c);
        uint16_t* cur = a.thumbs + ((size_t)h.stream * 2 + h.cur) * (size_t)a.max_cells;
        cur[cell] = (uint16_t)t;
        if (status == 1) {
            const uint16_t* prev = a.thumbs + ((size_t)h.stream * 2 + (h.cur ^ 1)) * (size_t)a.max_cells;
            d = (unsigned)abs((int)t - (int)prev[cell]);
        }
        atomicAdd(&s_hist[t >> 7], 1);      // LDS
    }
    const unsigned w1 = wave_sum(t), w2 = wave_sum(t * t), wd = wave_sum(d);
    if ((tid & 63) == 0) { s_part[tid >> 6][0] = w1; s_part[tid >> 6][1] = w2; s_part[tid >> 6][2] = wd; }
    __syncthreads();
    unsigned long long* acc = a.accs + (size_t)h.stream * HEALTH_ACCS;
    if (tid < 3) {      // S1, S2, D: one 64-bit atomic each
        const unsigned long long s = (unsigned long long)s_part[0][tid] + s_part[1][tid] + s_part[2][tid] + s_part[3][tid];
        if (tid < 2 || status == 1) atomicAdd(acc + (tid == 0 ? HEALTH_ACC_S1 : tid == 1 ? HEALTH_ACC_S2 : HEALTH_ACC_D), s);
    }
    if (tid >= 64 && tid < 64 + VT_HEALTH_BINS) {
        const int b = tid - 64, v = s_hist[b];
        if (v != 0) atomicAdd(a.hist + ((size_t)h.stream * 2 + h.cur) * VT_HEALTH_BINS + b, v);
    }
}

__global__ __launch_bounds__(256) void health_measure_kernel(HealthArgs a) {
    __shared__ unsigned s_part[4];
    const int slot = blockIdx.y, tid = threadIdx.x;
    const HealthHead& h = a.heads[slot];
    if (!health_measured(h.status)) return;
    const int Wg = h.Wg, Hg = h.Hg, cells = Wg * Hg;
    if ((int)blockIdx.x * 256 >= cells) return;         // the whole workgroup
    const uint16_t* cur = a.thumbs + ((size_t)h.stream * 2 + h.cur) * (size_t)a.max_cells;
    const int cell = blockIdx.x * 256 + tid;
    unsigned g = 0;
    if (cell < cells) {
        const int j = cell / Wg, i = cell - j * Wg;
        const int t = cur[cell];
        if (i < Wg - 1) g += (unsigned)abs((int)cur[cell + 1] - t);
        if (j < Hg - 1) g += (unsigned)abs((int)cur[cell + Wg] - t);
    }
    const unsigned w = wave_sum(g);
    if ((tid & 63) == 0) s_part[tid >> 6] = w;
    __syncthreads();
    if (tid == 0)
        atomicAdd(a.accs + (size_t)h.stream * HEALTH_ACCS + HEALTH_ACC_G,
                  (unsigned long long)s_part[0] + s_part[1] + s_part[2] + s_part[3]);
}

__global__ __launch_bounds__(64) void health_decide_kernel(HealthArgs a) {
    __shared__ uint32_t s_rec[kHealthRecWords];
    const int slot = blockIdx.x, tid = threadIdx.x;
    const HealthHead h = a.heads[slot];
    if (h.status <= 0) return;      // another slot's stream, or not due: record, bookkeeping and counters stay
    const int stream = h.stream;
    unsigned hd = 0;
    if (h.status == 1 && tid < VT_HEALTH_BINS) {
        const int32_t* hc = a.hist + ((size_t)stream * 2 + h.cur) * VT_HEALTH_BINS;
        const int32_t* hp = a.hist + ((size_t)stream * 2 + (h.cur ^ 1)) * VT_HEALTH_BINS;
        hd = (unsigned)abs(hc[tid] - hp[tid]);
    }
    hd = wave_sum(hd);
    if (tid < kHealthRecWords) s_rec[tid] = reinterpret_cast<const uint32_t*>(a.recs + stream)[tid];
    __syncthreads();
    if (tid == 0) {
        const HealthPolicy pol = *a.policy;
        HealthRec r;
        memcpy(&r, s_rec, sizeof(r));       // still, G_ref and the bookkeeping of the prepare launch
        const int still_prev = r.still;
        r.status = h.status; r.frames_done = h.frames_done; r.flags = 0; r.c = h.c; r.Wg = h.Wg; r.Hg = h.Hg;
        r.still = 0; r.S1 = 0; r.S2 = 0; r.G = 0; r.D = 0; r.HD = 0;
        if (health_measured(h.status)) {
            const long long* acc = reinterpret_cast<const long long*>(a.accs) + (size_t)stream * HEALTH_ACCS;
            const long long n = (long long)h.Wg * h.Hg;
            r.S1 = acc[HEALTH_ACC_S1]; r.S2 = acc[HEALTH_ACC_S2]; r.G = acc[HEALTH_ACC_G];
            int flags = 0;
            if (n * r.S2 - r.S1 * r.S1 <= (long long)pol.flat_q * pol.flat_q * n * n) flags |= VT_HEALTH_FLAT;
            if (h.status == 1) {
                r.D = acc[HEALTH_ACC_D]; r.HD = (long long)hd;
                r.still = r.D == 0 ? min(still_prev + 1, VT_HEALTH_STILL_CAP) : 0;
                if (r.still >= pol.still_run) flags |= VT_HEALTH_FROZEN;
                if (pol.cut_pm > 0 && r.HD * 1000ll >= (long long)pol.cut_pm * 2ll * n) flags |= VT_HEALTH_CUT;
            }
            if (h.status == 5 || (flags & VT_HEALTH_CUT)) r.G_ref = r.G;
            r.flags = flags;
            HealthCount c = a.counts[stream];
            c.evaluated += 1;
            c.flagged += flags != 0 ? 1 : 0;
            a.counts[stream] = c;
        } else {
            r.G_ref = 0; r.has_prev = 0;    // statuses 2 and 4: nothing measured, no previous thumbnail
        }
        memcpy(s_rec, &r, sizeof(r));
    }
    __syncthreads();
    HealthRec* host = a.out ? a.out->host_health : nullptr;
    if (tid < kHealthRecWords) {
        const uint32_t v = s_rec[tid];
        reinterpret_cast<uint32_t*>(a.recs + stream)[tid] = v;
        if (host) reinterpret_cast<uint32_t*>(host + stream)[tid] = v;
    }
    __threadfence_system();     // the host's copy is visible once the stream synchronises
}
static_assert(kHealthRecWords <= 64, "one wave moves a record");

static bool health_args_ok(const HealthArgs& a) {
    return a.n >= 1 && a.n <= VT_MAX_STREAMS && a.max_cells >= VT_HEALTH_MIN_CELLS && a.max_cells <= VT_HEALTH_MAX_CELLS &&
           a.frames && a.states && a.policy && a.devflag && a.recs && a.counts && a.heads && a.accs && a.hist && a.thumbs;
}

hipError_t launch_health_prepare(const HealthArgs& a, hipStream_t st) {
    if (!health_args_ok(a)) return hipErrorInvalidValue;
    vt_launch(health_prepare_kernel, dim3(a.n), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_health_thumb(const HealthArgs& a, int any_layout, hipStream_t st) {
    if (!health_args_ok(a)) return hipErrorInvalidValue;
    const dim3 grid((a.max_cells + 255) / 256, a.n);
    if (any_layout >= 3) vt_launch(health_thumb_kernel<3>, grid, dim3(256), 0, st, a);
    else if (any_layout == 2) vt_launch(health_thumb_kernel<2>, grid, dim3(256), 0, st, a);
    else if (any_layout == 1) vt_launch(health_thumb_kernel<1>, grid, dim3(256), 0, st, a);
    else vt_launch(health_thumb_kernel<0>, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_health_measure(const HealthArgs& a, hipStream_t st) {
    if (!health_args_ok(a)) return hipErrorInvalidValue;
    vt_launch(health_measure_kernel, dim3((a.max_cells + 255) / 256, a.n), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_health_decide(const HealthArgs& a, hipStream_t st) {
    if (!health_args_ok(a)) return hipErrorInvalidValue;
    vt_launch(health_decide_kernel, dim3(a.n), dim3(64), 0, st, a);
    return hipGetLastError();
}
