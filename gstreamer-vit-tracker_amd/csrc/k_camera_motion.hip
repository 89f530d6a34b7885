// k_camera_motion.hip — camera motion ("Camera motion"; the rule to the bit:
// include/vittrack_hip_ops.h, vt_op_camera_motion).
//
// Four launches, built to be the first of a pass (ahead of motion_place, the template gather, cand_fill and the crop: the
// thumbnail is taken from undrawn pixels, and everything behind reads the box as the decision left it); today they run
// through the operator hook only:
//
// camera_prepare, one workgroup per slot: thread 0 evaluates the due rule, the geometry and the previous thumbnail's from
// wave-uniform loads and writes the slot's header, which the three launches behind obey, and the thumbnails' bookkeeping of
// the stream's record; where the search will run the workgroup zeroes the stream's SAD table.
//
// camera_thumb, grid (max_cells / 256, slots): one thread per thumbnail cell, sixteen fetch_rgb taps, an integer luma each,
// one uint16 store. Every tap lies inside the frame by construction. Workgroups beyond Wg * Hg and those of slots whose
// header does not say "evaluate" leave at once: the launch dimensions never change, so a captured pass stays valid.
//
// camera_search, grid (min(max_cells / 256, 64), slots): a workgroup takes tiles of 32 x 8 central cells (a stride loop
// over the slot's tiles); the tile's current cells and the previous thumbnail's (32 + 2R) x (8 + 2R) cells sit in LDS;
// every thread owns up to five displacements and adds |cur - prev| over the tile's cells (uint32: at most 256 * 4080),
// then over its tiles (64 bits), and leaves with one 64-bit integer atomic per displacement: consecutive lanes add to
// consecutive entries of the table. Integer sums: the order of the adds does not matter, nothing is a floating-point atomic.
//
// camera_decide, one workgroup per slot: the least (S, dx^2 + dy^2, index) and the least S at Chebyshev distance > 1 from
// it, the status, the three binary32 operations per axis of the sub-cell shift, the box (mode 2), the record to the
// device array and the pinned mirror, the box to the pinned state mirror.
//
// Only the option's own buffers and (mode 2) box[0], box[1] of the stream's state are written. Compiled like k_motion.hip
// (-ffp-contract=off, correctly rounded division): one IEEE operation per source operation.
#include "k_camera_motion.hpp"
#include "k_thumb_dev.hpp"

#pragma clang fp contract(off)

static constexpr int kCamRecWords = sizeof(CamRec) / 4;
static constexpr int kTileW = 32, kTileH = 8;       // central cells per search tile: 256 threads
static constexpr int kSearchBlocks = 64;            // workgroups per slot at most: each adds its tiles up before the atomics
static constexpr int kPerThread = (VT_CAM_TABLE + 255) / 256;       // displacements a thread owns at most

__device__ __forceinline__ bool cam_searched(int status) { return status == 1 || status == 3 || status == 6 || status == 7; }

__global__ __launch_bounds__(256) void camera_prepare_kernel(CamArgs a) {
    __shared__ int s_search;
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int stream = a.slot_stream ? a.slot_stream[slot] : slot;
    if (tid == 0) {
        const CamPolicy pol = *a.policy;
        CamHead h{};
        h.stream = stream; h.R = pol.range;
        bool first = true;      // (b): the first slot naming the stream works for it
        if (a.slot_stream)
            for (int j = 0; j < slot; ++j) first = first && a.slot_stream[j] != stream;
        if (!first) {
            h.status = -1;
        } else {
            const StreamState& st = a.states[stream];
            const FrameDesc& f = a.frames[slot];
            CamRec* r = a.recs + stream;
            h.frames_done = st.frames_done;
            int status = (pol.mode != 0 && st.initialized) ? 1 : 0;      // (a), (c)
            // (d), (e): a whole frame in device memory
            if (status == 1 && (*a.devflag == 0 || f.x0 != 0 || f.y0 != 0 || f.ww != f.w || f.wh != f.h)) status = 4;
            if (status == 1) {  // the geometry
                const int c = pol.cell ? pol.cell : cam_auto_cell(f.w, f.h, a.max_cells);
                status = 2;
                if (c > 0) {
                    h.c = c; h.Wg = f.w / c; h.Hg = f.h / c;
                    if ((long long)h.Wg * h.Hg <= (long long)a.max_cells && h.Wg - 2 * h.R >= 8 && h.Hg - 2 * h.R >= 8) status = 1;
                }
            }
            if (status == 1) {
                const bool prev = r->has_prev && r->pW == f.w && r->pH == f.h && r->pc == h.c;
                h.cur = r->has_prev ? (r->cur ^ 1) & 1 : 0;
                if (!prev) status = 5;
                r->has_prev = 1; r->cur = h.cur; r->pW = f.w; r->pH = f.h; r->pc = h.c;
            } else {
                r->has_prev = 0;    // the tracker moves the box in this pass: a shift measured over the gap would be applied twice
            }
            h.status = status;
        }
        a.heads[slot] = h;
        s_search = h.status == 1 ? (2 * h.R + 1) * (2 * h.R + 1) : 0;
    }
    __syncthreads();
    unsigned long long* tab = a.sad + (size_t)stream * VT_CAM_TABLE;
    for (int k = tid; k < s_search; k += 256) tab[k] = 0ull;
}

template <int ANY>
__global__ __launch_bounds__(256) void camera_thumb_kernel(CamArgs a) {
    const int slot = blockIdx.y;
    const CamHead& h = a.heads[slot];
    if (h.status != 1 && h.status != 5) return;
    const int Wg = h.Wg, cells = Wg * h.Hg;
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= cells) return;
    const int j = cell / Wg, i = cell - j * Wg;
    const int sum = thumb_cell<ANY>(a.frames[slot], i, j, h.c);     // k_thumb_dev.hpp
    a.thumbs[((size_t)h.stream * 2 + h.cur) * (size_t)a.max_cells + cell] = (uint16_t)sum;
}

__global__ __launch_bounds__(256) void camera_search_kernel(CamArgs a) {
    __shared__ uint16_t s_cur[kTileW * kTileH];
    __shared__ uint16_t s_prev[(kTileH + 2 * VT_CAM_R_MAX) * (kTileW + 2 * VT_CAM_R_MAX)];
    const int slot = blockIdx.y, tid = threadIdx.x;
    const CamHead& h = a.heads[slot];
    if (h.status != 1) return;
    const int R = h.R, Wg = h.Wg, Hg = h.Hg, side = 2 * R + 1, D = side * side;
    const int Cw = Wg - 2 * R, Ch = Hg - 2 * R;                 // the central cells every displacement sums
    const int tx_n = (Cw + kTileW - 1) / kTileW, tiles = tx_n * ((Ch + kTileH - 1) / kTileH);
    if ((int)blockIdx.x >= tiles) return;
    const uint16_t* cur = a.thumbs + ((size_t)h.stream * 2 + h.cur) * (size_t)a.max_cells;
    const uint16_t* prev = a.thumbs + ((size_t)h.stream * 2 + (h.cur ^ 1)) * (size_t)a.max_cells;
    const int LW = kTileW + 2 * R;
    int off[kPerThread];        // where in the halo the thread's displacement k finds the cell of tile position (0, 0)
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int d = tid + 256 * k, dy = d / side - R, dx = d % side - R;
        off[k] = d < D ? (R - dy) * LW + (R - dx) : -1;
    }
    unsigned long long acc[kPerThread] = {};
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int x0 = (t % tx_n) * kTileW, y0 = (t / tx_n) * kTileH;           // central coordinates: cell (R + x0, R + y0)
        const int tw = min(kTileW, Cw - x0), th = min(kTileH, Ch - y0);
        __syncthreads();        // the previous tile's reads are done
        {
            const int x = tid % kTileW, y = tid / kTileW;
            s_cur[tid] = (x < tw && y < th) ? cur[(size_t)(R + y0 + y) * Wg + (R + x0 + x)] : (uint16_t)0;
        }
        const int LH = th + 2 * R, lw = tw + 2 * R;     // previous cells (x0 .. x0 + tw + 2R) x (y0 .. y0 + th + 2R): all inside the grid
        for (int k = tid; k < LH * LW; k += 256) {
            const int yy = k / LW, xx = k - yy * LW;
            s_prev[k] = xx < lw ? prev[(size_t)(y0 + yy) * Wg + (x0 + xx)] : (uint16_t)0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            if (off[k] < 0) continue;
            unsigned s = 0;
            for (int y = 0; y < th; ++y) {
                const uint16_t* crow = s_cur + y * kTileW;
                const uint16_t* prow = s_prev + off[k] + y * LW;
                for (int x = 0; x < tw; ++x) s += (unsigned)abs((int)crow[x] - (int)prow[x]);
            }
            acc[k] += s;
        }
    }
    unsigned long long* tab = a.sad + (size_t)h.stream * VT_CAM_TABLE;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k)
        if (off[k] >= 0) atomicAdd(tab + tid + 256 * k, acc[k]);
}

// displacement a = (S, index) beats b: the lesser sum, then the lesser squared length, then the lesser index
__device__ __forceinline__ bool cam_better(long long sa, int ia, long long sb, int ib, int side, int R) {
    if (ib < 0) return ia >= 0;
    if (ia < 0) return false;
    if (sa != sb) return sa < sb;
    const int ax = ia % side - R, ay = ia / side - R, bx = ib % side - R, by = ib / side - R;
    const int ra = ax * ax + ay * ay, rb = bx * bx + by * by;
    return ra != rb ? ra < rb : ia < ib;
}

__global__ __launch_bounds__(256) void camera_decide_kernel(CamArgs a) {
    __shared__ long long s_s[256];
    __shared__ int s_i[256];
    __shared__ long long s_bs;
    __shared__ int s_bi;
    __shared__ uint32_t s_rec[kCamRecWords];
    const int slot = blockIdx.x, tid = threadIdx.x;
    const CamHead h = a.heads[slot];
    if (h.status < 0) return;       // the stream's record is its first slot's
    const int stream = h.stream, R = h.R, side = 2 * R + 1, D = side * side;
    const long long* tab = reinterpret_cast<const long long*>(a.sad) + (size_t)stream * VT_CAM_TABLE;
    long long S2 = 0;
    if (h.status == 1) {
        // ---- the best displacement ----
        long long bs = 0;
        int bi = -1;
        for (int d = tid; d < D; d += 256) {
            const long long s = tab[d];
            if (cam_better(s, d, bs, bi, side, R)) { bs = s; bi = d; }
        }
        s_s[tid] = bs; s_i[tid] = bi;
        __syncthreads();
        if (tid == 0) {
            for (int t = 1; t < 256; ++t)
                if (cam_better(s_s[t], s_i[t], bs, bi, side, R)) { bs = s_s[t]; bi = s_i[t]; }
            s_bs = bs; s_bi = bi;
        }
        __syncthreads();
        // ---- the runner-up outside the best one's 3 x 3 neighbourhood (R >= 2: there is one) ----
        const int bx = s_bi % side, by = s_bi / side;
        long long m = 0;
        int mi = -1;
        for (int d = tid; d < D; d += 256) {
            const int x = d % side, y = d / side;
            if (abs(x - bx) <= 1 && abs(y - by) <= 1) continue;
            const long long s = tab[d];
            if (mi < 0 || s < m) { m = s; mi = d; }
        }
        __syncthreads();        // thread 0 has read the first round's entries
        s_s[tid] = m; s_i[tid] = mi;
        __syncthreads();
        if (tid == 0) {
            for (int t = 1; t < 256; ++t)
                if (s_i[t] >= 0 && (mi < 0 || s_s[t] < m)) { m = s_s[t]; mi = s_i[t]; }
            S2 = m;
        }
    }
    if (tid < kCamRecWords) s_rec[tid] = reinterpret_cast<const uint32_t*>(a.recs + stream)[tid];
    __syncthreads();
    if (tid == 0) {
        const CamPolicy pol = *a.policy;
        CamRec r;
        memcpy(&r, s_rec, sizeof(r));       // the counters and the bookkeeping stay
        r.status = h.status; r.frames_done = h.frames_done; r.c = h.c; r.Wg = h.Wg; r.Hg = h.Hg; r.R = R;
        r.dx = 0; r.dy = 0; r.shift[0] = 0.0f; r.shift[1] = 0.0f; r.applied = 0; r.n = 0;
        r.S_best = 0; r.S0 = 0; r.S2 = 0;
        if (h.status == 1) {
            const int bi = s_bi, dx = bi % side - R, dy = bi / side - R;
            const long long Sb = s_bs;
            r.dx = dx; r.dy = dy; r.n = (h.Wg - 2 * R) * (h.Hg - 2 * R);
            r.S_best = Sb; r.S0 = tab[R * side + R]; r.S2 = S2;
            if (S2 == 0) r.status = 3;
            else if (abs(dx) == R || abs(dy) == R) r.status = 6;
            else if (Sb * 1000ll > (long long)pol.conf_pm * S2) r.status = 7;
            if (r.status == 1) {
                const long long nb[2][2] = {{tab[bi - 1], tab[bi + 1]}, {tab[bi - side], tab[bi + side]}};
                const int d2[2] = {dx, dy};
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const long long Sm = nb[k][0], Sp = nb[k][1];
                    const long long den = Sm - 2 * Sb + Sp;
                    const float num = 0.5f * (float)(Sm - Sp);
                    const float off = (den > 0 && Sb > 0) ? num / (float)den : 0.0f;      // an exact match is a whole-cell shift
                    const float cells = (float)d2[k] + off;
                    r.shift[k] = cells * (float)h.c;
                }
            }
            r.evaluated += 1;
        }
        StreamState* st = a.states + stream;
        if (pol.mode == 2 && r.status == 1 && (r.shift[0] != 0.0f || r.shift[1] != 0.0f)) {
            // the place rule of the motion prior (motion_predict): the moved centre stays inside the frame
            const float px = st->box[0] + r.shift[0], py = st->box[1] + r.shift[1];
            const float hw = 0.5f * st->box[2], hh = 0.5f * st->box[3];
            const float cx = px + hw, cy = py + hh;
            if (cx >= 0.0f && cx < (float)st->frame_w && cy >= 0.0f && cy < (float)st->frame_h) {
                st->box[0] = px; st->box[1] = py;
                r.applied = 1; r.moved += 1;
                if (a.host_states) { a.host_states[stream].box[0] = px; a.host_states[stream].box[1] = py; }
            }
        }
        memcpy(s_rec, &r, sizeof(r));
    }
    __syncthreads();
    if (tid < kCamRecWords) {
        const uint32_t v = s_rec[tid];
        reinterpret_cast<uint32_t*>(a.recs + stream)[tid] = v;
        if (a.host_recs) reinterpret_cast<uint32_t*>(a.host_recs + stream)[tid] = v;
    }
    __threadfence_system();     // the host's copies are visible once the stream synchronises
}

static bool cam_args_ok(const CamArgs& a) {
    return a.n >= 1 && a.n <= VT_MAX_STREAMS && a.max_cells >= VT_CAM_MIN_CELLS && a.max_cells <= VT_CAM_MAX_CELLS && a.frames &&
           a.states && a.policy && a.devflag && a.recs && a.heads && a.sad && a.thumbs;
}

hipError_t launch_camera_prepare(const CamArgs& a, hipStream_t st) {
    if (!cam_args_ok(a)) return hipErrorInvalidValue;
    vt_launch(camera_prepare_kernel, dim3(a.n), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_camera_thumb(const CamArgs& a, int any_layout, hipStream_t st) {
    if (!cam_args_ok(a)) return hipErrorInvalidValue;
    const dim3 grid((a.max_cells + 255) / 256, a.n);
    if (any_layout >= 3) vt_launch(camera_thumb_kernel<3>, grid, dim3(256), 0, st, a);
    else if (any_layout == 2) vt_launch(camera_thumb_kernel<2>, grid, dim3(256), 0, st, a);
    else if (any_layout == 1) vt_launch(camera_thumb_kernel<1>, grid, dim3(256), 0, st, a);
    else vt_launch(camera_thumb_kernel<0>, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_camera_search(const CamArgs& a, hipStream_t st) {
    if (!cam_args_ok(a)) return hipErrorInvalidValue;
    const int blocks = (a.max_cells + 255) / 256;
    vt_launch(camera_search_kernel, dim3(blocks < kSearchBlocks ? blocks : kSearchBlocks, a.n), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_camera_decide(const CamArgs& a, hipStream_t st) {
    if (!cam_args_ok(a)) return hipErrorInvalidValue;
    vt_launch(camera_decide_kernel, dim3(a.n), dim3(256), 0, st, a);
    return hipGetLastError();
}
