// k_movers.hip — moving regions ("Moving regions"; the rule to the bit: include/vittrack_hip_ops.h,
// vt_op_movers): where in a stream's picture something moves, as up to eight boxes per stream.
//
// Six launches behind four launchers (launch_movers_label is three of them), built to sit behind the decode (the commit)
// and ahead of everything that cuts or draws - the thumbnail is taken from undrawn pixels -, directly behind health_decide.
// No engine pass carries them yet: vt_op_movers runs them.
//
// movers_prepare, one workgroup per slot: frame health's prepare - the first slot naming a stream works for it, thread 0
// evaluates the due rule, the whole-frame test, the geometry and the background's from wave-uniform loads, writes the slot's
// header and the background's bookkeeping of the stream's record and zeroes the stream's accumulators.
//
// movers_thumb, grid (max_cells / 256, slots): one thread per cell, the sixteen taps of the thumbnail cell
// (k_thumb_dev.hpp) - health_thumb's memory behaviour: the one launch that reads whole frames -, then on the cell the thread
// holds: d = 16 t - bg, the moving bit from the background as it was, bg += d >> learn (status 5: bg = 16 t, no bit). One
// uint16 thumbnail store, one uint16 background store, one mask byte; the moving cells are counted wave (ballot) -> LDS ->
// one 32-bit integer atomic per workgroup.
//
// movers_label_start, same grid: the clean-up - a thread reads the mask bytes of its cell's 3x3 neighbourhood from the mask
// the launch ahead stored (L2-resident, the rows coalesced; no halo in LDS: a byte read nine times from L2 costs less than
// staging it) -, the kept byte (a store of 2 over 1: a neighbour that reads it meanwhile sees "moving" either way), the
// cell's first label (the left end of its run of kept cells within its row and workgroup, found in LDS; or -1), its
// extents' start, the kept count.
//
// movers_label_merge, same grid: union-find on the label array. A kept cell joins itself with its kept E, SW, S and SE
// neighbours (every 8-adjacency once). A join finds both roots, hangs the larger under the smaller with an integer atomicMin
// and, where the larger was no root any more, goes on with what the atomic found there. Every label only ever falls, and
// never below the least index of the cells it is joined with, so every find and every join ends: a find takes at most as
// many steps as its component has cells (a serpentine of k cells: at most k, not k sweeps of the grid), a join at most that
// many rounds, and the launch as a whole at most 4 * kept joins; a find hangs what it passes under its grandparent, so the
// paths halve as they are walked. No sweep count, no flag, no host round trip. The root of a
// finished component is its least row-major index whatever the order of the joins, because a root is only ever replaced by
// a smaller index of the same component. The loads of a find are relaxed device-scope atomics: they see the atomics of
// workgroups on other dies.
//
// movers_label_flatten, same grid, behind the merges (a launch boundary: every join has landed): label = find(cell), and at
// the root's index the area (atomicAdd), i0 (atomicMin), i1 and j1 (atomicMax); j0 is the root's row.
//
// movers_list, one workgroup per slot: the global-change test, up to max_n rounds over the labels - each picks the largest
// (area, then the smaller label) key below the round before's, a 64-bit integer atomicMax in LDS; the keys are distinct, so
// the list is the same whatever the scheduling -, the components' count, the kept cells under the stream's own box, still,
// the record to the device array and the optional pinned mirror, the counters.
//
// Integers only - no sum or merge depends on its order - with one exception, stated in the rule: the corners of the
// stream's own box are binary32 in the state and are scaled by the power of two 1 / c (exact) and floored or ceiled. (A tap
// reaches the cell function as the pixel fetch's three float values, exact integers 0..255: k_thumb_dev.hpp.) Launch
// dimensions depend on max_cells and the slot count alone; workgroups of slots that are not evaluated, and those beyond
// Wg * Hg, leave at once from wave-uniform loads of the header. Only the feature's own buffers are written.
#include "k_movers.hpp"
#include "k_camera_motion.hpp"  // cam_auto_cell: the automatic cell is the camera motion's
#include "k_thumb_dev.hpp"

static constexpr int kMoverRecWords = sizeof(MoverRec) / 4;
static_assert(kMoverRecWords == 64, "one wave moves a record");

__device__ __forceinline__ bool movers_measured(int status) { return status == 1 || status == 5; }
__device__ __forceinline__ bool movers_global(long long moving, long long cells, int global_pm) {
    return moving * 1000ll > (long long)global_pm * cells;
}
__device__ __forceinline__ int32_t* mover_ext(const MoverArgs& a, int stream, int which) {
    return a.exts + ((size_t)stream * MOVER_EXTS + which) * (size_t)a.max_cells;
}

__global__ __launch_bounds__(256) void movers_prepare_kernel(MoverArgs a) {
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
    if (tid != 0) return;
    const MoverPolicy pol = *a.policy;
    MoverHead h{};
    h.stream = stream;
    if (s_later) {
        h.status = -1;
    } else {
        const StreamState& st = a.states[stream];
        const FrameDesc& f = a.frames[slot];
        MoverRec* r = a.recs + stream;
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
            if (!(r->has_bg && r->pW == f.w && r->pH == f.h && r->pc == h.c)) status = 5;
            r->has_bg = 1; r->pW = f.w; r->pH = f.h; r->pc = h.c;
        } else if (status != 0) {
            r->has_bg = 0;      // statuses 2 and 4; a pass that is not due keeps the background
        }
        h.status = status;
        if (movers_measured(status)) {
            a.accs[(size_t)stream * MOVER_ACCS + MOVER_ACC_MOVING] = 0;
            a.accs[(size_t)stream * MOVER_ACCS + MOVER_ACC_KEPT] = 0;
        }
    }
    a.heads[slot] = h;
}

// the number of set flags of the workgroup, added to *acc by one atomic
__device__ __forceinline__ void movers_count(bool flag, int32_t* acc, int* s_part) {
    const int tid = threadIdx.x;
    const int w = __popcll(__ballot(flag));
    if ((tid & 63) == 0) s_part[tid >> 6] = w;
    __syncthreads();
    if (tid == 0) {
        const int s = s_part[0] + s_part[1] + s_part[2] + s_part[3];
        if (s) atomicAdd(acc, s);
    }
}

template <int ANY>
__global__ __launch_bounds__(256) void movers_thumb_kernel(MoverArgs a) {
    __shared__ int s_part[4];
    const int slot = blockIdx.y, tid = threadIdx.x;
    const MoverHead& h = a.heads[slot];
    const int status = h.status;
    if (!movers_measured(status)) return;
    const int Wg = h.Wg, cells = Wg * h.Hg;
    if ((int)blockIdx.x * 256 >= cells) return;         // the whole workgroup
    const int cell = blockIdx.x * 256 + tid;
    bool moving = false;
    if (cell < cells) {
        const MoverPolicy& pol = *a.policy;
        const int j = cell / Wg, i = cell - j * Wg;
        const int t = thumb_cell<ANY>(a.frames[slot], i, j, h.c);
        const size_t at = (size_t)h.stream * (size_t)a.max_cells + cell;
        a.thumbs[at] = (uint16_t)t;
        int b = 16 * t;
        if (status == 1) {
            const int was = a.bg[at], d = 16 * t - was;
            moving = abs(d) > 16 * pol.thr;
            b = was + (d >> mover_learn(pol.shape));    // an arithmetic shift: floor(d / 2^learn)
        }
        a.bg[at] = (uint16_t)b;
        a.mask[at] = moving ? 1 : 0;
    }
    if (status == 1) movers_count(moving, a.accs + (size_t)h.stream * MOVER_ACCS + MOVER_ACC_MOVING, s_part);
}

__global__ __launch_bounds__(256) void movers_label_start_kernel(MoverArgs a) {
    __shared__ int s_part[4];
    __shared__ uint8_t s_kept[256];
    const int slot = blockIdx.y, tid = threadIdx.x;
    const MoverHead& h = a.heads[slot];
    if (h.status != 1) return;
    const int Wg = h.Wg, Hg = h.Hg, cells = Wg * Hg;
    if ((int)blockIdx.x * 256 >= cells) return;         // the whole workgroup
    const int cell = blockIdx.x * 256 + tid;
    const int j = cell / Wg, i = cell - j * Wg;
    bool kept = false;
    if (cell < cells) {
        uint8_t* m = a.mask + (size_t)h.stream * (size_t)a.max_cells;
        if (m[cell]) {
            int nb = 0;
            for (int v = max(j - 1, 0); v <= min(j + 1, Hg - 1); ++v)
                for (int u = max(i - 1, 0); u <= min(i + 1, Wg - 1); ++u) nb += m[v * Wg + u] != 0;
            kept = nb >= mover_min_nb(a.policy->shape);
            if (kept) m[cell] = 2;
        }
        mover_ext(a, h.stream, MOVER_EXT_I0)[cell] = 0x7fffffff;
        mover_ext(a, h.stream, MOVER_EXT_I1)[cell] = -1;
        mover_ext(a, h.stream, MOVER_EXT_J1)[cell] = -1;
        mover_ext(a, h.stream, MOVER_EXT_AREA)[cell] = 0;
    }
    s_kept[tid] = kept;
    movers_count(kept, a.accs + (size_t)h.stream * MOVER_ACCS + MOVER_ACC_KEPT, s_part);       // a barrier: s_kept is whole
    if (cell >= cells) return;
    // the label starts at the left end of the cell's run of kept cells, as far as it lies in this row and this workgroup:
    // a smaller index of the same component, which is all a label ever has to be before the merges
    int first = tid;
    while (kept && first > 0 && first > tid - i && s_kept[first - 1]) --first;
    a.labels[(size_t)h.stream * (size_t)a.max_cells + cell] = kept ? cell - (tid - first) : -1;
}

// The root of x: labels fall towards it, so the walk ends after at most as many steps as the component has cells. On the way
// every cell passed is hung under its grandparent (an atomicMin like every other write to the labels: they only ever fall),
// which halves the path for whoever comes next
__device__ __forceinline__ int mover_find(int32_t* L, int x) {
    for (;;) {
        const int p = __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        const int g = __hip_atomic_load(L + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (g == p) return p;
        atomicMin(L + x, g);
        x = g;
    }
}
__device__ __forceinline__ void mover_join(int32_t* L, int x, int y) {
    for (;;) {
        x = mover_find(L, x); y = mover_find(L, y);
        if (x == y) return;
        if (x < y) { const int t = x; x = y; y = t; }      // x > y: x goes under y
        const int old = atomicMin(L + x, y);
        if (old == x) return;       // x was a root
        x = old;                    // it was not any more: what it hung under is joined with y next (old < x)
    }
}
// evaluated and not a global change: the slots whose labels are merged and flattened
__device__ __forceinline__ bool movers_labelled(const MoverArgs& a, const MoverHead& h) {
    return h.status == 1 && !movers_global(a.accs[(size_t)h.stream * MOVER_ACCS + MOVER_ACC_MOVING], (long long)h.Wg * h.Hg, a.policy->global_pm);
}

__global__ __launch_bounds__(256) void movers_label_merge_kernel(MoverArgs a) {
    const int slot = blockIdx.y;
    const MoverHead& h = a.heads[slot];
    if (!movers_labelled(a, h)) return;
    const int Wg = h.Wg, Hg = h.Hg, cells = Wg * Hg;
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= cells) return;
    const uint8_t* m = a.mask + (size_t)h.stream * (size_t)a.max_cells;
    if (m[cell] != 2) return;
    int32_t* L = a.labels + (size_t)h.stream * (size_t)a.max_cells;
    const int j = cell / Wg, i = cell - j * Wg;
    if (i + 1 < Wg && m[cell + 1] == 2) mover_join(L, cell, cell + 1);
    if (j + 1 < Hg) {
        if (i > 0 && m[cell + Wg - 1] == 2) mover_join(L, cell, cell + Wg - 1);
        if (m[cell + Wg] == 2) mover_join(L, cell, cell + Wg);
        if (i + 1 < Wg && m[cell + Wg + 1] == 2) mover_join(L, cell, cell + Wg + 1);
    }
}

__global__ __launch_bounds__(256) void movers_label_flatten_kernel(MoverArgs a) {
    const int slot = blockIdx.y;
    const MoverHead& h = a.heads[slot];
    if (!movers_labelled(a, h)) return;
    const int Wg = h.Wg, cells = Wg * h.Hg;
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= cells) return;
    int32_t* L = a.labels + (size_t)h.stream * (size_t)a.max_cells;
    if (a.mask[(size_t)h.stream * (size_t)a.max_cells + cell] != 2) return;
    const int root = mover_find(L, cell);
    atomicMin(L + cell, root);      // a finder that passes through this cell meanwhile reads an older label or the root: both lead there
    const int j = cell / Wg, i = cell - j * Wg;
    atomicAdd(mover_ext(a, h.stream, MOVER_EXT_AREA) + root, 1);
    atomicMin(mover_ext(a, h.stream, MOVER_EXT_I0) + root, i);
    atomicMax(mover_ext(a, h.stream, MOVER_EXT_I1) + root, i);
    atomicMax(mover_ext(a, h.stream, MOVER_EXT_J1) + root, j);
}

__global__ __launch_bounds__(256) void movers_list_kernel(MoverArgs a) {
    __shared__ __align__(8) uint32_t s_rec[kMoverRecWords];
    __shared__ unsigned long long s_best;
    __shared__ int s_roots, s_own;
    const int slot = blockIdx.x, tid = threadIdx.x;
    const MoverHead h = a.heads[slot];
    if (h.status <= 0) return;      // another slot's stream, or not due: record, bookkeeping and counters stay
    const int stream = h.stream;
    const MoverPolicy pol = *a.policy;
    const int cells = h.Wg * h.Hg, max_n = mover_max_n(pol.shape);
    const int moving = h.status == 1 ? a.accs[(size_t)stream * MOVER_ACCS + MOVER_ACC_MOVING] : 0;
    const int kept = h.status == 1 ? a.accs[(size_t)stream * MOVER_ACCS + MOVER_ACC_KEPT] : 0;
    const bool global = h.status == 1 && movers_global(moving, cells, pol.global_pm);
    const int32_t* L = a.labels + (size_t)stream * (size_t)a.max_cells;
    const int32_t* area = mover_ext(a, stream, MOVER_EXT_AREA);
    if (tid < kMoverRecWords) s_rec[tid] = reinterpret_cast<const uint32_t*>(a.recs + stream)[tid];
    if (tid == 0) { s_roots = 0; s_own = 0; }
    __syncthreads();
    // the own box: corners floored (left, top) and ceiled (right, bottom) to cells, clipped to the grid
    int ox0 = 0, oy0 = 0, ox1 = 0, oy1 = 0;
    if (h.status == 1) {
        const float* box = a.states[stream].box;
        const float inv = 1.0f / (float)h.c;        // a power of two: the products are exact
        ox0 = (int)fminf(fmaxf(floorf(box[0] * inv), 0.0f), (float)h.Wg);
        oy0 = (int)fminf(fmaxf(floorf(box[1] * inv), 0.0f), (float)h.Hg);
        ox1 = (int)fminf(fmaxf(ceilf((box[0] + box[2]) * inv), 0.0f), (float)h.Wg);
        oy1 = (int)fminf(fmaxf(ceilf((box[1] + box[3]) * inv), 0.0f), (float)h.Hg);
        if (ox1 < ox0) ox1 = ox0;
        if (oy1 < oy0) oy1 = oy0;
        const int ow = ox1 - ox0, on = ow * (oy1 - oy0);
        const uint8_t* m = a.mask + (size_t)stream * (size_t)a.max_cells;
        int own = 0;
        for (int k = tid; k < on; k += 256) own += m[(oy0 + k / ow) * h.Wg + ox0 + k % ow] == 2;
        if (own) atomicAdd(&s_own, own);    // LDS
    }
    MoverBox* boxes = reinterpret_cast<MoverBox*>(s_rec + offsetof(MoverRec, box) / 4);
    int n = 0;
    if (tid < (int)(sizeof(MoverBox) / 4) * VT_MOVER_MAX) s_rec[offsetof(MoverRec, box) / 4 + tid] = 0;
    unsigned long long below = ~0ull;
    if (h.status == 1 && !global) {
        for (int k = 0; k < max_n; ++k) {       // uniform: every thread sees the same s_best
            if (tid == 0) s_best = 0ull;
            __syncthreads();
            unsigned long long best = 0ull;
            int roots = 0;
            for (int cidx = tid; cidx < cells; cidx += 256) {
                if (L[cidx] != cidx) continue;
                ++roots;
                const int ar = area[cidx];
                const unsigned long long key = (unsigned long long)(unsigned)ar << 32 | (0xffffffffu - (unsigned)cidx);
                if (ar >= pol.min_area && key < below && key > best) best = key;
            }
            if (k == 0 && roots) atomicAdd(&s_roots, roots);
            if (best) atomicMax(&s_best, best);     // LDS, 64-bit integer
            __syncthreads();
            below = s_best;
            if (below == 0ull) break;
            if (tid == 0) {
                const int label = (int)(0xffffffffu - (unsigned)(below & 0xffffffffull));
                const int i0 = mover_ext(a, stream, MOVER_EXT_I0)[label], i1 = mover_ext(a, stream, MOVER_EXT_I1)[label];
                const int j0 = label / h.Wg, j1 = mover_ext(a, stream, MOVER_EXT_J1)[label];
                boxes[k] = MoverBox{i0 * h.c, j0 * h.c, (i1 - i0 + 1) * h.c, (j1 - j0 + 1) * h.c, (int)(below >> 32), label};
            }
            ++n;
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid == 0) {
        MoverRec& r = *reinterpret_cast<MoverRec*>(s_rec);       // in LDS: still, the bookkeeping of the prepare launch, the boxes
        const int still_prev = r.still;
        r.status = global ? 6 : h.status; r.frames_done = h.frames_done; r.c = h.c; r.Wg = h.Wg; r.Hg = h.Hg;
        r.n = n; r.moving = moving; r.kept = kept; r.components = s_roots;
        r.own_cells = (ox1 - ox0) * (oy1 - oy0); r.own_kept = s_own;
        r.still = (h.status == 1 && !global && s_own == 0 && kept > 0) ? min(still_prev + 1, VT_MOVER_STILL_CAP) : 0;
        if (h.status == 1) {
            MoverCount c = a.counts[stream];
            c.evaluated += 1;
            c.listed += n;
            a.counts[stream] = c;
        } else if (h.status != 5) {
            r.has_bg = 0; r.pW = 0; r.pH = 0; r.pc = 0;     // statuses 2 and 4: nothing measured, no background
        }
    }
    __syncthreads();
    MoverRec* host = a.host_recs;
    if (tid < kMoverRecWords) {
        const uint32_t v = s_rec[tid];
        reinterpret_cast<uint32_t*>(a.recs + stream)[tid] = v;
        if (host) reinterpret_cast<uint32_t*>(host + stream)[tid] = v;
    }
    __threadfence_system();     // the host's copy is visible once the stream synchronises
}

static bool movers_args_ok(const MoverArgs& a) {
    return a.n >= 1 && a.n <= VT_MAX_STREAMS && a.max_cells >= VT_MOVER_MIN_CELLS && a.max_cells <= VT_MOVER_MAX_CELLS &&
           a.frames && a.states && a.policy && a.devflag && a.recs && a.counts && a.heads && a.accs && a.labels && a.exts &&
           a.bg && a.thumbs && a.mask;
}

hipError_t launch_movers_prepare(const MoverArgs& a, hipStream_t st) {
    if (!movers_args_ok(a)) return hipErrorInvalidValue;
    vt_launch(movers_prepare_kernel, dim3(a.n), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_movers_thumb(const MoverArgs& a, int any_layout, hipStream_t st) {
    if (!movers_args_ok(a)) return hipErrorInvalidValue;
    const dim3 grid((a.max_cells + 255) / 256, a.n);
    if (any_layout >= 3) vt_launch(movers_thumb_kernel<3>, grid, dim3(256), 0, st, a);
    else if (any_layout == 2) vt_launch(movers_thumb_kernel<2>, grid, dim3(256), 0, st, a);
    else if (any_layout == 1) vt_launch(movers_thumb_kernel<1>, grid, dim3(256), 0, st, a);
    else vt_launch(movers_thumb_kernel<0>, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_movers_label(const MoverArgs& a, hipStream_t st) {
    if (!movers_args_ok(a)) return hipErrorInvalidValue;
    const dim3 grid((a.max_cells + 255) / 256, a.n);
    vt_launch(movers_label_start_kernel, grid, dim3(256), 0, st, a);
    vt_launch(movers_label_merge_kernel, grid, dim3(256), 0, st, a);
    vt_launch(movers_label_flatten_kernel, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_movers_list(const MoverArgs& a, hipStream_t st) {
    if (!movers_args_ok(a)) return hipErrorInvalidValue;
    vt_launch(movers_list_kernel, dim3(a.n), dim3(256), 0, st, a);
    return hipGetLastError();
}
