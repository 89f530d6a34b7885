// k_snapshot.hpp — stream snapshots on the device (k_snapshot.hip; byte layout: include/vittrack_hip.h).
#pragma once
#include "vt_common.hpp"
#include "vt_frame.hpp"
#include "k_refresh.hpp"        // RefreshPolicy: part of the payload

// The payload of a snapshot record as it lies in device staging: state words, policy words, template rows, at the
// offsets of the byte string (whose header the host writes). rec is 16-byte aligned, so rec + VT_SNAP_ROWS_OFF is too.
#define VT_SNAP_HEADER_BYTES 152
#define VT_SNAP_STATE_OFF VT_SNAP_HEADER_BYTES
#define VT_SNAP_POLICY_OFF (VT_SNAP_STATE_OFF + 88)
#define VT_SNAP_ROWS_OFF (VT_SNAP_POLICY_OFF + 16)
static_assert(VT_SNAP_ROWS_OFF == 256 && sizeof(StreamState) == 88 && sizeof(RefreshPolicy) == 16, "snapshot layout");

struct SnapArgs {
    StreamState* state;         // the stream's record in the engine's state array
    RefreshPolicy* policy;      // the stream's policy; null on an engine that never enabled refresh (packs as zeros)
    bf16_t* tpl;                // the stream's rows in the template store: `bufs` buffers of row_elems elements each
    int bufs;                   // 2: the rows are those of buffer tpl_gen & 1; 1: the only buffer
    int row_elems;              // nt * kpad, a multiple of 8 (kpad % 64 == 0)
    uint8_t* rec;               // the record in device staging, VT_SNAP_ROWS_OFF + 2 * row_elems bytes
};
// pack: stream -> record (buffer chosen by the STREAM's tpl_gen); unpack: record -> stream (by the RECORD's tpl_gen).
// One launch each on `st`: 16 bytes per lane for the rows, one word per lane for state and policy.
hipError_t launch_snapshot_pack(const SnapArgs& a, hipStream_t st);
hipError_t launch_snapshot_unpack(const SnapArgs& a, hipStream_t st);
