// k_snapshot.hip — pack a stream into a snapshot record and unpack one into a stream (vt_snapshot.hip).
//
// Pack is a launch of its own rather than three hipMemcpyAsync calls because WHICH template buffer holds a stream's rows
// is a word of its state (tpl_gen & 1) that only the device knows while work is queued on the stream: the copy's source
// address depends on a load. Reading that word on the host first would put a second stream synchronisation in front of
// the copy (vt_group_copy_stream packs behind whatever the source engine has queued). Unpack could be three copies - the
// record's tpl_gen is known to the host - and is the mirror image instead: one launch, one set of offsets to keep right.
// Both are ordered against the passes like any kernel of theirs.
//
// Off the hot path: no pass launches these, and the sizes are small (24 KiB to 216 KiB of rows), so the kernels are the
// plainest form that keeps every request 16 bytes wide: lane i moves 16-byte piece i of the rows; the first 26 lanes of
// workgroup 0 also move the 22 state words and the 4 policy words. Neither kernel reads anything it writes.
#include "k_snapshot.hpp"

static constexpr int SNAP_STATE_WORDS = sizeof(StreamState) / 4, SNAP_POLICY_WORDS = sizeof(RefreshPolicy) / 4;

__global__ __launch_bounds__(256) void snapshot_pack_kernel(SnapArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int gen = a.state->tpl_gen;                                   // wave-uniform
    const uint4* src = reinterpret_cast<const uint4*>(a.tpl + (size_t)(a.bufs == 2 ? (gen & 1) : 0) * a.row_elems);
    uint4* dst = reinterpret_cast<uint4*>(a.rec + VT_SNAP_ROWS_OFF);
    if (i < a.row_elems / 8) dst[i] = src[i];
    if (i < SNAP_STATE_WORDS)
        reinterpret_cast<uint32_t*>(a.rec + VT_SNAP_STATE_OFF)[i] = reinterpret_cast<const uint32_t*>(a.state)[i];
    else if (i < SNAP_STATE_WORDS + SNAP_POLICY_WORDS)
        reinterpret_cast<uint32_t*>(a.rec + VT_SNAP_POLICY_OFF)[i - SNAP_STATE_WORDS] =
            a.policy ? reinterpret_cast<const uint32_t*>(a.policy)[i - SNAP_STATE_WORDS] : 0u;
}

__global__ __launch_bounds__(256) void snapshot_unpack_kernel(SnapArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int gen = reinterpret_cast<const StreamState*>(a.rec + VT_SNAP_STATE_OFF)->tpl_gen;    // the record's, never the stream's
    const uint4* src = reinterpret_cast<const uint4*>(a.rec + VT_SNAP_ROWS_OFF);
    uint4* dst = reinterpret_cast<uint4*>(a.tpl + (size_t)(a.bufs == 2 ? (gen & 1) : 0) * a.row_elems);
    if (i < a.row_elems / 8) dst[i] = src[i];
    if (i < SNAP_STATE_WORDS)
        reinterpret_cast<uint32_t*>(a.state)[i] = reinterpret_cast<const uint32_t*>(a.rec + VT_SNAP_STATE_OFF)[i];
    else if (i < SNAP_STATE_WORDS + SNAP_POLICY_WORDS - 1 && a.policy)   // period, min_score, skipped_geometry; not the reserved word
        reinterpret_cast<uint32_t*>(a.policy)[i - SNAP_STATE_WORDS] =
            reinterpret_cast<const uint32_t*>(a.rec + VT_SNAP_POLICY_OFF)[i - SNAP_STATE_WORDS];
}

static bool snap_args_ok(const SnapArgs& a) {
    return a.state && a.tpl && a.rec && (a.bufs == 1 || a.bufs == 2) && a.row_elems >= 8 && a.row_elems % 8 == 0 &&
           (reinterpret_cast<uintptr_t>(a.rec) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.tpl) & 15) == 0;
}

hipError_t launch_snapshot_pack(const SnapArgs& a, hipStream_t st) {
    if (!snap_args_ok(a)) return hipErrorInvalidValue;
    vt_launch(snapshot_pack_kernel, dim3((a.row_elems / 8 + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_snapshot_unpack(const SnapArgs& a, hipStream_t st) {
    if (!snap_args_ok(a)) return hipErrorInvalidValue;
    vt_launch(snapshot_unpack_kernel, dim3((a.row_elems / 8 + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}
