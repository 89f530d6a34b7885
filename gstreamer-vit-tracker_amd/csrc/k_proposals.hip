// k_proposals.hip — reacquire proposals ("Reacquire proposals"; the rule to the bit:
// include/vittrack_hip.h, the "proposals*" keys).
//
// Four launches behind the decode of every pass of an engine that enabled the option (behind the candidate commit,
// motion_settle and the appearance launches; ahead of the refresh, chip, peaks and overlay launches: the pattern is
// pooled from the template the pass ran on and the thumbnail from undrawn pixels):
//
// proposals_prepare, one workgroup per slot: thread 0 evaluates the due rule and the geometry from wave-uniform loads;
// one thread per pattern cell pools the cell's (T/M)^2 x 3 template values in binary64, ascending (y, x, channel); the
// workgroup adds Sa and Saa (integers) and thread 0 writes the slot's header, which the three launches behind obey.
//
// proposals_thumb, grid (max_cells / 256, slots): one thread per thumbnail cell, sixteen fetch_rgb sub-taps, binary32
// sums in (v, u) order, one int16 store: the value, or VT_PROP_OUTSIDE where a sub-tap left the frame. Workgroups beyond Wg * Hg and those of slots whose header does not say
// "evaluate" leave at once: the launch dimensions never change, so a captured pass stays valid.
//
// proposals_match, grid (max_cells / 256, slots): a workgroup takes tiles of 32 x 8 positions (a stride loop over the
// slot's tiles); the tile's (32 + M - 1) x (8 + M - 1) thumbnail cells and the pattern sit in LDS; every thread owns
// one position and accumulates, over the window's cells that lie INSIDE the frame (the thumbnail marks the others), their
// count, Sa and Sp (int32: at most 256 * 32767), Saa, Spp and Sap (int64: one 32 x 32 + 64 multiply-add per cell and sum -
// a packed 16-bit dot product into a 32-bit accumulator would overflow at two saturated cells, and the map has to be
// exact for every input). The similarity is one binary64 divide and square root per position.
//
// proposals_list, one workgroup of 1024 threads per slot: the iterated argmax of k_peaks.hip over the map in global memory; the
// listed positions are kept in LDS and a position inside a listed one's square is skipped, so the map itself stays
// what the match launch wrote. The record leaves as 56 dwords to the device array and the pass's pinned mirror.
//
// Nothing but the option's own buffers is written: no word of StreamState, no result, no template row, no pixel. No
// atomics, no tickets. Compiled like k_refresh.hip (-ffp-contract=off): one IEEE operation per source operation.
#include "k_proposals.hpp"
#include "k_preproc_dev.hpp"

static constexpr int kPropRecWords = sizeof(PropRec) / 4;
static constexpr int kTileW = 32, kTileH = 8;       // positions per match tile: 256 threads

__device__ __forceinline__ int prop_clamp16(double v) {     // v is integral (rint): the clamp is exact
    return (int)fmin(fmax(v, -32767.0), 32767.0);
}

__global__ __launch_bounds__(256) void proposals_prepare_kernel(PropArgs a, int T, int patch, int gt, int kpad) {
    __shared__ PropHead s_h;
    __shared__ long long s_sa[4], s_saa[4];
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int stream = a.slot_stream ? a.slot_stream[slot] : slot;
    const int M = prop_pattern_side(T);
    if (tid == 0) {
        const PropPolicy pol = *a.policy;
        const vt_result r = a.results[slot];
        const StreamState& st = a.states[stream];
        const FrameDesc& f = a.frames[slot];
        PropHead h{};
        h.frames_done = st.frames_done; h.M = M;
        h.box[0] = st.box[0]; h.box[1] = st.box[1]; h.box[2] = st.box[2]; h.box[3] = st.box[3];
        // ---- due: (a) - (d) ----
        bool due = pol.mode != 0 && (!a.winner || a.winner[slot] == slot);
        if (due && pol.mode == 1) due = r.success == 0;
        if (due) due = st.frames_done % max(pol.period, 1) == 0;
        int status = due ? 1 : 0;
        // ---- (e), (f): a whole frame in device memory ----
        if (status == 1 && (*a.devflag == 0 || f.x0 != 0 || f.y0 != 0 || f.ww != f.w || f.wh != f.h)) status = 4;
        // ---- geometry ----
        if (status == 1) {
            const float s = sqrtf(st.box[2] * st.box[3]);
            const float c = 2.0f * s / (float)M;
            const float qw = (float)f.w / c, qh = (float)f.h / c;
            status = 2;
            if (c > 0.0f && qw <= (float)VT_PROP_MAX_CELLS && qh <= (float)VT_PROP_MAX_CELLS) {     // a NaN fails
                const int Wg = (int)ceilf(qw) + M / 2, Hg = (int)ceilf(qh) + M / 2;
                h.c = c; h.X0 = -(float)(M / 4) * c; h.Wg = Wg; h.Hg = Hg;
                if ((long long)Wg * Hg <= (long long)pol.max_cells && Wg >= M && Hg >= M) status = 1;
            }
        }
        h.status = status;
        s_h = h;
    }
    __syncthreads();
    if (s_h.status != 1) {
        if (tid == 0) a.heads[slot] = s_h;
        return;
    }
    // ---- the pattern: the stream's current rows, the template this pass ran on ----
    const int gen = a.tpl_bufs == 2 ? (a.states[stream].tpl_gen & 1) : 0;
    const size_t rows = (size_t)gt * gt * kpad;
    const bf16_t* tp = a.tpl + ((size_t)stream * a.tpl_bufs + gen) * rows;
    const int blk = T / M;
    long long q = 0;
    if (tid < M * M) {
        const int cy = tid / M, cx = tid - cy * M;
        double sum = 0.0;
        for (int y = cy * blk; y < (cy + 1) * blk; ++y)
#pragma unroll 4    // the loads of four pixels in flight; the additions keep their order
            for (int x = cx * blk; x < (cx + 1) * blk; ++x) {
                const bf16_t* row = tp + (size_t)((y / patch) * gt + x / patch) * kpad + (y % patch) * patch + x % patch;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) sum = sum + (double)bf16_to_f32(row[ch * patch * patch]);
            }
        q = prop_clamp16(rint(sum * (4096.0 / (double)(3 * blk * blk))));
        a.pattern[(size_t)slot * (VT_PROP_M_MAX * VT_PROP_M_MAX) + tid] = (int16_t)q;
    }
    long long sa = q, saa = q * q;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sa += __shfl_xor(sa, off, 64);
        saa += __shfl_xor(saa, off, 64);
    }
    if ((tid & 63) == 0) { s_sa[tid >> 6] = sa; s_saa[tid >> 6] = saa; }
    __syncthreads();
    if (tid == 0) {
        PropHead h = s_h;
        h.Sa = s_sa[0] + s_sa[1] + s_sa[2] + s_sa[3];
        h.Saa = s_saa[0] + s_saa[1] + s_saa[2] + s_saa[3];
        if ((long long)(M * M) * h.Saa - h.Sa * h.Sa == 0) h.status = 3;
        a.heads[slot] = h;
    }
}

template <int ANY>
__global__ __launch_bounds__(256) void proposals_thumb_kernel(PropArgs a, float na0, float na1, float na2, float nb0, float nb1,
                                                              float nb2) {
    const int slot = blockIdx.y;
    const PropHead& h = a.heads[slot];
    if (h.status != 1) return;
    const int Wg = h.Wg, cells = Wg * h.Hg;
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= cells) return;
    const int j = cell / Wg, i = cell - j * Wg;
    const float c = h.c, X0 = h.X0;
    const FrameDesc& f = a.frames[slot];
    float sum = 0.0f;
    int miss = 0;
    bool inside = true;     // every sub-tap lies in the frame
#pragma unroll 1
    for (int v = 0; v < 4; ++v) {
        const int py = (int)floorf(X0 + ((float)j + ((float)v + 0.5f) * 0.25f) * c);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int px = (int)floorf(X0 + ((float)i + ((float)u + 0.5f) * 0.25f) * c);
            inside = inside && px >= 0 && py >= 0 && px < f.w && py < f.h;
            float rgb[3];
            fetch_rgb<ANY>(f, px, py, rgb, miss);
            const float g = (rgb[0] * na0 + nb0) + (rgb[1] * na1 + nb1) + (rgb[2] * na2 + nb2);
            sum = sum + g;
        }
    }
    const float q = fminf(fmaxf(rintf(sum * (4096.0f / 48.0f)), -32767.0f), 32767.0f);
    a.thumb[(size_t)slot * a.max_cells + cell] = inside ? (int16_t)(int)q : (int16_t)VT_PROP_OUTSIDE;
}

__global__ __launch_bounds__(256) void proposals_match_kernel(PropArgs a) {
    __shared__ int16_t s_pat[VT_PROP_M_MAX * VT_PROP_M_MAX];
    __shared__ int16_t s_tile[(kTileH + VT_PROP_M_MAX - 1) * (kTileW + VT_PROP_M_MAX - 1)];
    const int slot = blockIdx.y, tid = threadIdx.x;
    const PropHead& h = a.heads[slot];
    if (h.status != 1) return;
    const int M = h.M, Wg = h.Wg, Hg = h.Hg;
    const int Pw = Wg - M + 1, Ph = Hg - M + 1;
    const int tx_n = (Pw + kTileW - 1) / kTileW, tiles = tx_n * ((Ph + kTileH - 1) / kTileH);
    if ((int)blockIdx.x >= tiles) return;
    const int16_t* thumb = a.thumb + (size_t)slot * a.max_cells;
    float* map = a.map + (size_t)slot * a.max_cells;
    if (tid < M * M) s_pat[tid] = a.pattern[(size_t)slot * (VT_PROP_M_MAX * VT_PROP_M_MAX) + tid];
    const int LW = kTileW + M - 1, LH = kTileH + M - 1;
    const int lx = tid % kTileW, ly = tid / kTileW;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int x0 = (t % tx_n) * kTileW, y0 = (t / tx_n) * kTileH;
        __syncthreads();        // the previous tile's reads are done (and the pattern is in place)
        for (int k = tid; k < LW * LH; k += 256) {
            const int yy = y0 + k / LW, xx = x0 + k % LW;
            s_tile[k] = (yy < Hg && xx < Wg) ? thumb[(size_t)yy * Wg + xx] : (int16_t)VT_PROP_OUTSIDE;
        }
        __syncthreads();
        const int px = x0 + lx, py = y0 + ly;
        if (px >= Pw || py >= Ph) continue;
        // the window's cells INSIDE the frame only: their count, the pattern's sums over them, the thumbnail's
        int n = 0, sa = 0, sp = 0;
        long long saa = 0, spp = 0, sap = 0;
        for (int y = 0; y < M; ++y) {
            const int16_t* trow = s_tile + (ly + y) * LW + lx;
            const int16_t* prow = s_pat + y * M;
            for (int x = 0; x < M; ++x) {
                const int raw = trow[x], in = raw != VT_PROP_OUTSIDE;
                const int p = in ? raw : 0, q = in ? prow[x] : 0;
                n += in;
                sa += q;
                sp += p;
                saa += (long long)q * q;
                spp += (long long)p * p;
                sap += (long long)q * p;
            }
        }
        const long long cov = (long long)n * sap - (long long)sa * sp;
        const long long va = (long long)n * saa - (long long)sa * sa;
        const long long vp = (long long)n * spp - (long long)sp * sp;
        double sim = (va > 0 && vp > 0) ? (double)cov / sqrt((double)va * (double)vp) : 0.0;
        sim = sim > 1.0 ? 1.0 : (sim < -1.0 ? -1.0 : sim);
        map[(size_t)py * Pw + px] = (float)sim;
    }
}

// candidate a = (similarity, position) beats b: the greater similarity, the lower position on a tie
__device__ __forceinline__ bool prop_better(float sa, int ia, float sb, int ib) { return sa > sb || (sa == sb && ia < ib); }
#define PROP_NO_POS 0x7fffffff

static constexpr int kListThreads = 1024;     // the scan of the map is bound by load latency: sixteen waves, four loads each in flight

__global__ __launch_bounds__(kListThreads) void proposals_list_kernel(PropArgs a) {
    __shared__ float s_wb[kListThreads / 64];
    __shared__ int s_wi[kListThreads / 64];
    __shared__ int s_lx[VT_PROP_MAX], s_ly[VT_PROP_MAX];
    __shared__ uint32_t s_rec[kPropRecWords];
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int stream = a.slot_stream ? a.slot_stream[slot] : slot;
    if (a.winner && a.winner[slot] != slot) return;     // a stream's record is its winning slot's
    const PropHead h = a.heads[slot];
    const PropPolicy pol = *a.policy;
    if (tid < kPropRecWords) s_rec[tid] = 0u;
    __syncthreads();
    int n = 0;
    if (h.status == 1) {
        const int M = h.M, Pw = h.Wg - M + 1, P = Pw * (h.Hg - M + 1), R = M / 2;
        const int K = min(max(pol.max_n, 1), VT_PROP_MAX);
        const float* map = a.map + (size_t)slot * a.max_cells;
        const int lane = tid & 63, wave = tid >> 6;
        for (int k = 0; k < K; ++k) {
            float best = -2.0f;
            int bidx = PROP_NO_POS;
#pragma unroll 4
            for (int i = tid; i < P; i += kListThreads) {
                const int py = i / Pw, px = i - py * Pw;
                bool open = true;
                for (int j = 0; j < k; ++j) open = open && (abs(px - s_lx[j]) > R || abs(py - s_ly[j]) > R);
                const float s = map[i];
                if (open && prop_better(s, i, best, bidx)) { best = s; bidx = i; }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const float ob = __shfl_xor(best, off, 64);
                const int oi = __shfl_xor(bidx, off, 64);
                if (prop_better(ob, oi, best, bidx)) { best = ob; bidx = oi; }
            }
            if (lane == 0) { s_wb[wave] = best; s_wi[wave] = bidx; }
            __syncthreads();
            best = s_wb[0]; bidx = s_wi[0];
#pragma unroll
            for (int w = 1; w < kListThreads / 64; ++w)
                if (prop_better(s_wb[w], s_wi[w], best, bidx)) { best = s_wb[w]; bidx = s_wi[w]; }
            // similarities do not increase from round to round: the first failure ends the list
            if (bidx == PROP_NO_POS || !(best >= pol.tau && best > 0.0f)) break;
            const int py = bidx / Pw, px = bidx - py * Pw;
            if (tid == 0) {
                const float cx = h.X0 + (float)(px + R) * h.c, cy = h.X0 + (float)(py + R) * h.c;
                uint32_t* p = s_rec + 8 + k * 6;
                p[0] = __float_as_uint(best);
                p[1] = __float_as_uint(cx - 0.5f * h.box[2]); p[2] = __float_as_uint(cy - 0.5f * h.box[3]);
                p[3] = __float_as_uint(h.box[2]); p[4] = __float_as_uint(h.box[3]);
                p[5] = (uint32_t)bidx;
                s_lx[k] = px; s_ly[k] = py;
            }
            n = k + 1;
            __syncthreads();
        }
    }
    if (tid == 0) {
        s_rec[0] = (uint32_t)h.status; s_rec[1] = (uint32_t)h.frames_done; s_rec[2] = (uint32_t)n;
        s_rec[3] = __float_as_uint(h.c); s_rec[4] = (uint32_t)h.Wg; s_rec[5] = (uint32_t)h.Hg;
        if (h.status == 1 || h.status == 3) a.evaluated[stream] += 1;
    }
    __syncthreads();
    if (tid < kPropRecWords) {
        const uint32_t v = s_rec[tid];
        reinterpret_cast<uint32_t*>(a.recs + stream)[tid] = v;
        PropRec* hp = a.out ? a.out->host_proposals : nullptr;
        if (hp) reinterpret_cast<uint32_t*>(hp + stream)[tid] = v;
        __threadfence_system();     // the host's copy is visible once the pass's event or the stream synchronises
    }
}

static bool prop_args_ok(const PropArgs& a) {
    return a.n >= 1 && a.max_cells >= VT_PROP_M_MAX * VT_PROP_M_MAX && a.frames && a.states && a.results && a.policy &&
           a.devflag && a.tpl && a.recs && a.evaluated && a.heads && a.pattern && a.thumb && a.map;
}

hipError_t launch_proposals_prepare(const PropArgs& a, const ModelDims& d, hipStream_t st) {
    if (!prop_args_ok(a) || prop_pattern_side(d.T) == 0 || d.gt * d.patch != d.T || (a.tpl_bufs != 1 && a.tpl_bufs != 2))
        return hipErrorInvalidValue;
    vt_launch(proposals_prepare_kernel, dim3(a.n), dim3(256), 0, st, a, d.T, d.patch, d.gt, d.kpad);
    return hipGetLastError();
}

hipError_t launch_proposals_thumb(const PropArgs& a, const ModelDims& d, int any_layout, hipStream_t st) {
    if (!prop_args_ok(a)) return hipErrorInvalidValue;
    const dim3 grid((a.max_cells + 255) / 256, a.n);
#define PROP_THUMB(ANY) vt_launch(proposals_thumb_kernel<ANY>, grid, dim3(256), 0, st, a, d.norm_a[0], d.norm_a[1], d.norm_a[2], \
                                  d.norm_b[0], d.norm_b[1], d.norm_b[2])
    if (any_layout >= 3) PROP_THUMB(3);
    else if (any_layout == 2) PROP_THUMB(2);
    else if (any_layout == 1) PROP_THUMB(1);
    else PROP_THUMB(0);
#undef PROP_THUMB
    return hipGetLastError();
}

hipError_t launch_proposals_match(const PropArgs& a, hipStream_t st) {
    if (!prop_args_ok(a)) return hipErrorInvalidValue;
    vt_launch(proposals_match_kernel, dim3((a.max_cells + 255) / 256, a.n), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_proposals_list(const PropArgs& a, hipStream_t st) {
    if (!prop_args_ok(a)) return hipErrorInvalidValue;
    vt_launch(proposals_list_kernel, dim3(a.n), dim3(kListThreads), 0, st, a);
    return hipGetLastError();
}
