// vt_engine.hpp — what the host-side translation units of libvittrack_hip.so share: error plumbing, the device
// scope, the Engine (one GPU's batch of tracked streams) and the handles of the C ABI.
//   vt_engine.hip   the Engine: weight blob, buffers, the per-frame launch plan (run_pass), graphs, the one way a pass is
//                   submitted (prepare_pass / enqueue; enqueue_candidates for a candidate pass - both put their block
//                   together in build_block), wait
//   vt_features.hip the optional in-the-pass features: the one transaction behind every first enable (enable_feature), the
//                   optional sinks, the keyed features' descriptors and their one setter (set_keyed), policies, statistics
//   vt_abi.hip      the extern "C" boundary of include/vittrack_hip.h (create / init / update, device-frame passes of a
//                   group, diagnostics, colour converter, overlays, dma-buf and host-mapping ingest)
//   vt_ingest.hip   host-frame ingest: the staging arena, window planning and packing, the host-frame passes of a group
//                   (synchronous, pipelined enqueue_host / wait_next, queued init, candidate passes on host frames)
//   vt_snapshot.hip stream snapshots: the byte format's validation, export / import / copy of a stream (k_snapshot.hip)
//   vt_rccl.hip     the start-up weight broadcast over a lazily loaded librccl
//   vt_ops.hip      operator-level entry points of include/vittrack_hip_ops.h - linked into
//                   libvittrack_hip_ops.so (tests, tuning tools) only, NOT into the product library
// The headers. A kernel file's host-visible ABI lives in the header of the same name; vt_common.hpp holds only what the
// math kernels also need.
//   vt_common.hpp   the core: vector types, vt_launch, bf16 helpers
//   vt_frame.hpp    pixel formats, FrameDesc, StreamState, ModelDims, PassOut
//   k_gemm.hpp      k_gemm.hip and k_gemm256.hip: the residual pair's specification, GemmArgs, the launch API
//   k_misc.hpp  k_attn.hpp  k_head.hpp  k_preproc.hpp  k_overlay.hpp  k_cand.hpp  k_snapshot.hpp   the launch APIs of those files
//   k_refresh.hpp  k_chip.hpp  k_peaks.hpp  k_motion.hpp  k_appearance.hpp  k_arbitrate.hpp  k_proposals.hpp
//   k_camera_motion.hpp  k_conflicts.hpp  k_health.hpp  k_result_overlay.hpp   one optional feature each: records, policy, launchers
//   k_ln_dev.hpp and the other *_dev.hpp, k_gemm_util.hpp   device code shared between kernel files; not included here
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <atomic>
#include <new>
#include <string>
#include <vector>

#include "vt_common.hpp"
#include "vt_frame.hpp"
#include "k_gemm.hpp"
#include "k_misc.hpp"
#include "k_attn.hpp"
#include "k_head.hpp"
#include "k_preproc.hpp"
#include "k_overlay.hpp"
#include "k_refresh.hpp"
#include "k_chip.hpp"
#include "k_peaks.hpp"
#include "k_motion.hpp"
#include "k_appearance.hpp"
#include "k_arbitrate.hpp"
#include "k_proposals.hpp"
#include "k_camera_motion.hpp"
#include "k_conflicts.hpp"
#include "k_health.hpp"
#include "k_cand.hpp"
#include "k_result_overlay.hpp"
#include "vt_feature_keys.hpp"

// ---- error plumbing ------------------------------------------------------------------------------

int set_err(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
char* vt_err_text();        // the calling thread's error text (512 bytes)
#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            return set_err(_e == hipErrorOutOfMemory ? VT_ERR_OOM : VT_ERR_HIP,            \
                           "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                           __LINE__);                                                      \
    } while (0)

// Nothing may unwind across the C boundary (the reference host is built with panic = "abort",
// /root/reference/Cargo.toml:37): every extern "C" entry is a function-try-block ending in one of
// these handlers. std::bad_alloc (vector / map / string / new inside the engine) -> VT_ERR_OOM.
#define VT_NOTHROW_INT                                                                      \
    catch (const std::bad_alloc&) { return set_err(VT_ERR_OOM, "out of host memory"); }     \
    catch (const std::exception& ex_) { return set_err(VT_ERR_HIP, "internal error: %s", ex_.what()); } \
    catch (...) { return set_err(VT_ERR_HIP, "internal error (unknown exception)"); }
#define VT_NOTHROW_VOID catch (...) { (void)set_err(VT_ERR_HIP, "internal error in a void entry point"); }
#define VT_NOTHROW_PTR catch (...) { (void)set_err(VT_ERR_HIP, "internal error"); return nullptr; }

// hipSetDevice for the duration of a call, restoring the caller's current device afterwards (a
// single-process multi-GPU host - or torch in the tests - keeps its own notion of "current").
struct DeviceScope {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) err = hipSetDevice(dev); else prev = -1;
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};
#define DEVICE_SCOPE(dev)                                                                   \
    DeviceScope dev_scope_(dev);                                                            \
    if (dev_scope_.err != hipSuccess)                                                       \
        return set_err(VT_ERR_HIP, "hipSetDevice(%d): %s", (int)(dev), hipGetErrorString(dev_scope_.err))


// ---- weight blob ---------------------------------------------------------------------------------

static const char kMagic[8] = {'V', 'T', 'W', 'B', '0', '0', '0', '1'};
static const size_t kHeaderBytes = 256, kEntryBytes = 64;

struct BlobEntry {
    char name[32];
    uint32_t dtype, rows, cols, pad;
    uint64_t offset, nbytes;
};
static_assert(sizeof(BlobEntry) == 64, "blob entry layout");

struct TensorRef {
    const void* ptr = nullptr;
    uint32_t dtype = 0, rows = 0, cols = 0;
};

struct LayerW {
    const float *ln1_g, *ln1_b, *qkv_b, *proj_b, *ln2_g, *ln2_b, *fc1_b, *fc2_b;
    const bf16_t *qkv_w, *proj_w, *fc1_w, *fc2_w;
    // LayerNorm 1 / 2 folded into the QKV / fc1 GEMM (launch_fold_layernorm, once per engine):
    // weights bf16(gamma * W), their column sums, and beta W^T + bias
    const bf16_t *qkv_wf = nullptr, *fc1_wf = nullptr;
    const float *qkv_cs = nullptr, *qkv_c = nullptr, *fc1_cs = nullptr, *fc1_c = nullptr;
};

struct KernelStat {
    std::string name;
    int launches = 0;
    double ms = 0, flops = 0, bytes = 0;
};

struct Profiler {
    // a, b: marker events around the entry's launches; k: the first launch's own begin / end (vt_launch), used when the
    // entry was exactly one launch
    struct Rec { hipEvent_t a, b; LaunchProbe k; int fam; };
    std::vector<Rec> recs;
    std::vector<KernelStat> fams;
    int family(const std::string& n) {
        for (size_t i = 0; i < fams.size(); ++i)
            if (fams[i].name == n) return (int)i;
        KernelStat k;
        k.name = n;
        fams.push_back(k);
        return (int)fams.size() - 1;
    }
};

// One pass as run_pass launches it and capture_graph captures it. Engine::prepare_pass builds it for a pass that is
// about to run; nothing of it is engine state.
struct PassShape {
    int n = 0;                              // slots (M = n * ntok)
    const int32_t* slot_stream = nullptr;   // device map slot -> stream of a subset pass; null: the full pass (n == B, slot b is stream b)
    int tier = 0;                           // crop-buffer tier (Engine::pick_crop_tier)
    int any_layout = 0;                     // the highest pix_level of the slots' formats (k_preproc.hip: fetch_rgb<level>)
    // a candidate pass (k_cand.hip): slot_stream says whose TEMPLATE a slot takes; its STATE is the slot's own candidate
    // state (cand->cand_states, identity map), filled ahead of the crop and committed behind the decode. Null: a
    // slot's state is its stream's.
    const CandArgs* cand = nullptr;
    // the last encoder block runs on the search rows only (Engine::last_block_compact: the ONE place that decides it)
    bool compact = false;
};

// Where the packed windows of host frames go: a pinned host arena and its device twin of the same capacity
// (vt_ingest.hip). The synchronous path, each pipelined slot and each queued init own one.
struct StageArena {
    uint8_t *d = nullptr, *h = nullptr;
    size_t cap = 0;
    int ensure(size_t need);    // at least `need` bytes; a larger pair replaces the old one, which nothing may be using
    void release();
};

struct KeyedFeature;
struct Engine {
    int device = 0, B = 1;
    bool use_graph = true, taps = false;
    ModelDims d{};
    hipStream_t stream = nullptr;
    // weights
    uint8_t* d_blob = nullptr;
    size_t blob_bytes = 0;
    std::map<std::string, TensorRef> tens;
    std::vector<LayerW> layers;
    // activations
    bf16_t *d_patches = nullptr, *d_qk = nullptr, *d_vt = nullptr,
           *d_attn = nullptr, *d_mlp = nullptr, *d_feat = nullptr, *d_ta = nullptr,
           *d_tb = nullptr, *d_zeros = nullptr;     // d_zeros: 256 B of zeros (out-of-map taps of the 3x3 convs)
    // residual stream as the 3-byte pair (x = xh + xl * 2^-s, s = the blob's lo_shift: lq), its chunk partial statistics and the row terms of the
    // folded LayerNorm (vt_common.hpp); folded weights of all layers
    bf16_t *d_xh = nullptr, *d_foldw = nullptr;
    uint8_t* d_xl = nullptr;                      // the low half of the pair: one signed byte per element (spec v3, vt_common.hpp)
    LoQuant lq;                                   // the pair's quantum, from header int 12 of the blob (index_blob); baked into the captured passes
    bool taps_filled = false;                     // a pass has written the tap copies since taps were last enabled
    unsigned* d_xrange = nullptr;                 // [L + 1][VT_XRANGE_WORDS] of the range report (vt_group_read_tensor "xrange"), allocated by the first read
    uint8_t* d_taps = nullptr;                    // [slot][hi: M*D bf16 | lo8: M*D bytes]
    size_t tap_slot_bytes() const { return (size_t)B * d.ntok * d.D * 3; }
    unsigned* d_band_cnt = nullptr;               // per stream: bands of the last head layer that have arrived (k_head.hip)
    float* d_band_best = nullptr;                 // per stream and band: the band's argmax candidate
    float2 *d_cstat = nullptr, *d_rstat = nullptr;
    unsigned* d_panel_cnt = nullptr;   // arrival counters of the 256-row panels (X-epilogues of the 256x256 kernel)
    float *d_foldv = nullptr, *d_headout = nullptr;
    StreamState* d_states = nullptr;
    FrameDesc* d_frames = nullptr;      // per-pass block: [B] frame descriptors (by slot) | PassOut | [B] slot -> stream | device-frames word
    // template rows of every stream as init wrote them, [B][nt][kpad]: a subset pass gathers its streams' rows into its
    // slots' segments of d_patches, and the next full pass puts every segment back from here
    bf16_t* d_tpl = nullptr;
    bool segments_moved = false;        // d_patches' template rows are not in stream order (a subset pass ran since)
    // The first enable of an optional in-the-pass feature, for every one below: on the idle stream,
    // never inside an update - `extra` bytes checked against max_device_mib (beside activation_bytes() and
    // feature_bytes()) and against free memory (VT_ERR_OOM), alloc(), install() (pointers, *_capable = true), every
    // graph dropped and captured again with the feature's launches in it, commit() if there is one. Should alloc() or
    // the capture fail, uninstall() frees and resets whatever alloc() and install() left - it runs after a partial
    // alloc() too -, the passes the engine had are captured again and the first error is the one reported: nothing
    // changes on failure. An engine is capable for good; engines that never enable launch what they always did.
    struct Feature {
        const char* name;                       // for the messages
        size_t extra;
        std::function<hipError_t()> alloc;
        std::function<void()> install, uninstall, commit;
    };
    int enable_feature(const Feature& f);
    // enable_feature for "one store of `bytes` with its first `zeroed` bytes zero-filled, `policy` (or null) uploaded to
    // its start and fill(store) run on it + the sinks `sink` on the engine's own mirror and on every HostSlot that already
    // has sinks (later ones: host_slot_prepare)". wire(store) at install, wire(null) at uninstall: the feature's own members.
    int enable_store(const char* name, size_t bytes, size_t zeroed, const void* policy, size_t policy_bytes, unsigned sink,
                     hipError_t (*fill)(Engine*, uint8_t* store), const std::function<void(uint8_t*)>& wire);
    // One key of vt_group_set_tuning that belongs to f. A bad value changes nothing. Before the enable a value is kept in
    // the host's copy; the first non-zero "on" word is the enable; every later change is one small copy to the record.
    int set_keyed(const KeyedFeature& f, const std::string& key, int value);
    // template refresh (k_refresh.hip). The first policy that is enabled makes the engine refresh-capable: d_tpl becomes
    // [B][2][nt][kpad] (a stream's rows: buffer tpl_gen & 1 of its state), every pass - full ones too - gathers its
    // template rows from there and runs the refresh launch behind its decode. restore_segments / segments_moved are
    // for engines that never enabled.
    bool refresh_capable = false;
    RefreshPolicy* d_policy = nullptr;            // [B] (capable engines)
    std::vector<RefreshPolicy> h_policy;          // what the host set: period, min_score
    unsigned* d_tickets = nullptr;                // [B] arrival counters of the refresh launch, zero between launches
    int tpl_bufs() const { return refresh_capable ? 2 : 1; }
    bf16_t* tpl_init_rows(int b) const { return d_tpl + (size_t)b * tpl_bufs() * d.nt * d.kpad; }   // buffer 0: init's
    size_t refresh_bytes() const { return (size_t)B * (sizeof(bf16_t) * d.nt * d.kpad + sizeof(RefreshPolicy) + sizeof(unsigned)); }
    int enable_refresh();                         // enable_feature: second buffer, policy, tickets
    int set_refresh(int stream, int period, float min_score);     // stream -1: all
    int refresh_stats(int stream, vt_refresh_stats* out);
    int reset_refresh_tickets();                  // wherever a pass may have been abandoned half-way (the appearance launches' tickets too)
    // target chips (k_chip.hip). The first enable fixes the chip side and kind and allocates the store [B][chip_bytes] +
    // [B] infos + [B] policies: every pass runs the chip launch behind its decode (and behind the refresh launch).
    bool chip_capable = false;
    int chip_size = 0, chip_kind = 0;
    float chip_na[3] = {1.0f, 1.0f, 1.0f}, chip_nb[3] = {0.0f, 0.0f, 0.0f};
    uint8_t* d_chips = nullptr;                   // ONE allocation: [B][chip_bytes()], then the [B] infos
    vt_chip_info* d_chip_infos = nullptr;         // [B], inside d_chips behind the chips
    ChipPolicy* d_chip_policy = nullptr;          // [B], written by set_chips only
    uint8_t* h_chip_stage = nullptr;              // pinned mirror of the store for read_chips, allocated by its first call
    static size_t chip_bytes_of(int size, int kind) { return (size_t)size * size * (kind == VT_CHIP_NORM_BF16 ? 6 : 3); }
    size_t chip_bytes() const { return chip_capable ? chip_bytes_of(chip_size, chip_kind) : 0; }
    static size_t chip_store_bytes_of(int B, int size, int kind) {
        return (size_t)B * (chip_bytes_of(size, kind) + sizeof(vt_chip_info) + sizeof(ChipPolicy));
    }
    // HBM of the optional features this engine has enabled, beside activation_bytes() under max_device_mib
    size_t feature_bytes() const;
    int enable_chips(int size, int kind, const float* na, const float* nb);   // enable_feature: the store
    int set_chips(int stream, float factor, int period, int phase);           // stream -1: all
    int read_chips(const int* streams, int n, void* out, size_t out_stride, vt_chip_info* infos);
    // response peaks (k_peaks.hip). The first policy with max_peaks > 0 allocates the records [B] by slot + the policies
    // [B] by stream and the pinned mirrors: every pass runs the peaks launch behind its decode (and behind the refresh
    // and chip launches).
    bool peaks_capable = false;
    vt_peaks* d_peaks = nullptr;                  // ONE allocation: [B] records by slot, then the [B] policies
    PeaksPolicy* d_peaks_policy = nullptr;        // [B] by stream, inside d_peaks; written by set_peaks only
    std::vector<PeaksPolicy> peaks_policy;        // the host's copy (what set_peaks wrote)
    vt_peaks* h_peaks = nullptr;                  // pinned [B]: the records of the last pass the host collected, by slot
    int peaks_n = 0;                              // ... and that pass's slot count
    size_t peaks_bytes() const { return (size_t)B * (sizeof(vt_peaks) + sizeof(PeaksPolicy)); }
    int set_peaks(int stream, int max_peaks, int radius, float min_resp);     // stream -1: all; the first enable is in here
    int last_peaks(vt_peaks* out, int n) const;
    // result overlay (k_result_overlay.hip). ONE policy per engine. The first non-zero flags allocate the policy record +
    // the [B] counters by stream: every pass ends with the overlay launch, behind the refresh, chip and peaks launches.
    bool overlay_capable = false;
    OverlayPolicy overlay_policy = VT_OVERLAY_DEFAULT_POLICY;     // the host's copy
    uint8_t* d_overlay = nullptr;                 // ONE allocation: the policy record, then the [B] OverlayStats
    OverlayPolicy* d_overlay_policy() const { return reinterpret_cast<OverlayPolicy*>(d_overlay); }
    OverlayStats* d_overlay_stats() const { return reinterpret_cast<OverlayStats*>(d_overlay + sizeof(OverlayPolicy)); }
    size_t overlay_bytes() const { return sizeof(OverlayPolicy) + (size_t)B * sizeof(OverlayStats); }
    // 1 while a device entry point builds its pass (vt_abi.hip: DeviceFramesScope): build_block writes it into the
    // pass's block, where the overlay launch reads it. Host-pointer passes hand the kernels staging or mapped host
    // memory: they never draw.
    int frames_on_device = 0;
    int overlay_stats(int stream, float* out6);
    // motion prior (k_motion.hip). ONE policy per engine, one record per stream. The first non-zero "motion_prior"
    // allocates the policy record + the [B] records and their pinned mirrors: every pass starts with the place launch and
    // runs the settle launch directly behind its decode (its commit).
    bool motion_capable = false;
    MotionPolicy motion_policy = VT_MOTION_DEFAULT_POLICY;       // the host's copy
    uint8_t* d_motion = nullptr;                  // ONE allocation: the policy record, then the [B] MotionRec by stream
    MotionPolicy* d_motion_policy() const { return reinterpret_cast<MotionPolicy*>(d_motion); }
    size_t motion_off_recs() const { return sizeof(MotionPolicy); }
    MotionRec* d_motion_recs() const { return reinterpret_cast<MotionRec*>(d_motion + motion_off_recs()); }
    size_t motion_bytes() const { return motion_off_recs() + (size_t)B * sizeof(MotionRec); }
    MotionRec* h_motion_all = nullptr;            // pinned [B] by stream: beside h_states_all, written by the settle launch
    std::vector<MotionRec> known_motion;          // beside `known`: the records after the last pass the HOST has collected
    int motion_stats(int stream, float* out8);
    // the box the next pass of `stream` is cut around, from what the host knows: the place rule on known / known_motion.
    // steps == 2: the stream is in the pass still running, whose outcome nobody knows - the rule applied twice, once for
    // that pass's own move and once for the next one's (a target at constant velocity lands there)
    void predicted_box(int stream, float* box4, int steps = 1) const;
    // appearance check (k_appearance.hip). ONE policy per engine; per stream an anchor and a probe of template rows, a
    // record and two counters. The first non-zero "appearance" allocates all of it, fills the anchors of the streams that
    // are initialised from their current template rows and makes the engine appearance-capable for good: every pass runs
    // the probe and the score launch behind its decode (its commit, motion_settle), ahead of the refresh launch, whose rule
    // 8 reads the records.
    bool appear_capable = false;
    AppearPolicy appear_policy = VT_APPEAR_DEFAULT_POLICY;      // the host's copy
    // ONE allocation: the policy | [B] counters | [B] records | [B] tickets | [B][chunks][5] partials (binary64) |
    // [B][nt][kpad] anchors | [B][nt][kpad] probes (bf16, by stream)
    uint8_t* d_appear = nullptr;
    size_t appear_rows() const { return (size_t)d.nt * d.kpad; }
    size_t appear_off_counts() const { return 64; }
    size_t appear_off_recs() const { return appear_off_counts() + sizeof(AppearCount) * (size_t)B; }
    size_t appear_off_tickets() const { return appear_off_recs() + sizeof(AppearRec) * (size_t)B; }
    size_t appear_off_partials() const { return (appear_off_tickets() + sizeof(unsigned) * (size_t)B + 63) & ~(size_t)63; }
    size_t appear_off_anchor() const { return (appear_off_partials() + sizeof(double) * 5 * (size_t)B * appear_chunks(d.nt) + 63) & ~(size_t)63; }
    size_t appear_bytes() const { return appear_off_anchor() + 2 * sizeof(bf16_t) * appear_rows() * (size_t)B; }
    AppearPolicy* d_appear_policy() const { return reinterpret_cast<AppearPolicy*>(d_appear); }
    AppearCount* d_appear_counts() const { return reinterpret_cast<AppearCount*>(d_appear + appear_off_counts()); }
    AppearRec* d_appear_recs() const { return reinterpret_cast<AppearRec*>(d_appear + appear_off_recs()); }
    unsigned* d_appear_tickets() const { return reinterpret_cast<unsigned*>(d_appear + appear_off_tickets()); }
    double* d_appear_partials() const { return reinterpret_cast<double*>(d_appear + appear_off_partials()); }
    bf16_t* d_anchor(int b = 0) const { return reinterpret_cast<bf16_t*>(d_appear + appear_off_anchor()) + (size_t)b * appear_rows(); }
    bf16_t* d_probe(int b = 0) const { return d_anchor(B) + (size_t)b * appear_rows(); }
    // pinned [B] by stream: the records of the last passes the host collected - what "appearance" of vt_group_read_tensor
    // reports (the kernels store to the pass's sink; adopt_slot copies a collected pipelined pass's entries here)
    AppearRec* h_appear_all = nullptr;
    int appearance_anchor(int stream);      // the "appearance_anchor" action: stream's (-1: every initialised stream's) anchor <- its CURRENT template rows
    int appearance_stats(int stream, float* out8);
    // stream b's anchor <- its current template rows (buffer gen & 1 of a refresh-capable engine's store); behind the
    // stream's work. init, queued init, import, copy, the "appearance_anchor" action
    hipError_t anchor_from_template(int b, int gen);
    // reacquire proposals (k_proposals.hip). ONE policy per engine; per stream a record and a counter, per slot the working
    // set of the four launches. The first non-zero "proposals" allocates all of it with the max_cells of that moment and
    // makes the engine proposals-capable for good: every pass runs the four launches behind its decode (its commit,
    // motion_settle, the appearance launches), ahead of the refresh launch.
    bool prop_capable = false;
    PropPolicy prop_policy = VT_PROP_DEFAULT_POLICY;            // the host's copy
    // ONE allocation: the policy | [B] counters | [B] records | [B] headers | [B] patterns | [B][max_cells] thumbnails
    // (int16) | [B][max_cells] maps (float)
    uint8_t* d_prop = nullptr;
    static size_t prop_off_counts() { return 64; }
    size_t prop_off_recs() const { return (prop_off_counts() + sizeof(int32_t) * (size_t)B + 63) & ~(size_t)63; }
    size_t prop_off_heads() const { return prop_off_recs() + sizeof(PropRec) * (size_t)B; }
    size_t prop_off_pattern() const { return (prop_off_heads() + sizeof(PropHead) * (size_t)B + 63) & ~(size_t)63; }
    size_t prop_off_thumb() const { return prop_off_pattern() + sizeof(int16_t) * VT_PROP_M_MAX * VT_PROP_M_MAX * (size_t)B; }
    size_t prop_off_map(int max_cells) const { return prop_off_thumb() + sizeof(int16_t) * (size_t)max_cells * (size_t)B; }
    size_t prop_bytes() const { return prop_off_map(prop_policy.max_cells) + sizeof(float) * (size_t)prop_policy.max_cells * (size_t)B; }
    PropPolicy* d_prop_policy() const { return reinterpret_cast<PropPolicy*>(d_prop); }
    int32_t* d_prop_counts() const { return reinterpret_cast<int32_t*>(d_prop + prop_off_counts()); }
    PropRec* d_prop_recs() const { return reinterpret_cast<PropRec*>(d_prop + prop_off_recs()); }
    PropHead* d_prop_heads() const { return reinterpret_cast<PropHead*>(d_prop + prop_off_heads()); }
    int16_t* d_prop_pattern() const { return reinterpret_cast<int16_t*>(d_prop + prop_off_pattern()); }
    int16_t* d_prop_thumb() const { return reinterpret_cast<int16_t*>(d_prop + prop_off_thumb()); }
    float* d_prop_map() const { return reinterpret_cast<float*>(d_prop + prop_off_map(prop_policy.max_cells)); }
    // pinned [B] by stream: the records of the last passes the host collected - what "proposals" of vt_group_read_tensor
    // reports (the list launch stores to the pass's sink; adopt_slot copies a collected pipelined pass's entries here)
    PropRec* h_prop_all = nullptr;
#define VT_PROP_STATS 60    // floats of "proposals": 12 + VT_PROP_MAX * 6
    int proposals_stats(int stream, float* out60);
    // stream conflicts (k_conflicts.hip). ONE policy per engine; per stream a scene, a record and three counters. The first
    // non-zero "conflicts" allocates all of it and makes the engine conflicts-capable for good: every pass runs the check
    // launch behind its decode (its commit, motion_settle), ahead of the appearance, proposals and refresh launches; refresh
    // rule 9 reads the records.
    bool conflict_capable = false;
    ConflictPolicy conflict_policy = VT_CONFLICT_DEFAULT_POLICY;     // the host's copy
    std::vector<int32_t> conflict_scenes;         // beside it: the host's copy of the scenes, [B] on a capable engine
    // ONE allocation: the policy | [B] scenes | [B] records | [B] counters, all zero but the policy
    uint8_t* d_conflict = nullptr;
    size_t conflict_off_scenes() const { return 64; }
    size_t conflict_off_recs() const { return (conflict_off_scenes() + sizeof(int32_t) * (size_t)B + 63) & ~(size_t)63; }
    size_t conflict_off_counts() const { return conflict_off_recs() + sizeof(ConflictRec) * (size_t)B; }
    size_t conflict_bytes() const { return conflict_off_counts() + sizeof(ConflictCount) * (size_t)B; }
    ConflictPolicy* d_conflict_policy() const { return reinterpret_cast<ConflictPolicy*>(d_conflict); }
    int32_t* d_conflict_scenes() const { return reinterpret_cast<int32_t*>(d_conflict + conflict_off_scenes()); }
    ConflictRec* d_conflict_recs() const { return reinterpret_cast<ConflictRec*>(d_conflict + conflict_off_recs()); }
    ConflictCount* d_conflict_counts() const { return reinterpret_cast<ConflictCount*>(d_conflict + conflict_off_counts()); }
    // pinned [B] by stream: the records of the last passes the host collected - what "conflicts" of vt_group_read_tensor reports
    ConflictRec* h_conflict_all = nullptr;
    // the "conflicts_scene" action: value >= 0: stream value & 0xFFFF (0xFFFF: every stream) goes to scene value >> 16; -1:
    // every stream back to scene 0. The records of the streams it names are zeroed.
    int conflicts_scene(int value);
    int conflicts_stats(int stream, float* out16);
    // frame health (k_health.hip). ONE policy per engine; per stream a record, three counters, four accumulators, two
    // histograms and two thumbnails of max_cells, per slot a header. The first non-zero "health" allocates all of it with the
    // max_cells of that moment and makes the engine health-capable for good: every pass runs the four launches directly behind
    // conflicts_check, ahead of the appearance, proposals and refresh launches; refresh rule 10 reads the records.
    bool health_capable = false;
    HealthPolicy health_policy = VT_HEALTH_DEFAULT_POLICY;      // the host's copy
    // ONE allocation: the policy | [B] records | [B] counters | [B] headers | [B] accumulators | [B][2][32] histograms |
    // [B][2][max_cells] thumbnails, zero up to the thumbnails
    uint8_t* d_health = nullptr;
    size_t health_off_recs() const { return 64; }
    size_t health_off_counts() const { return health_off_recs() + sizeof(HealthRec) * (size_t)B; }
    size_t health_off_heads() const { return (health_off_counts() + sizeof(HealthCount) * (size_t)B + 63) & ~(size_t)63; }
    size_t health_off_accs() const { return health_off_heads() + sizeof(HealthHead) * (size_t)B; }
    size_t health_off_hist() const { return health_off_accs() + sizeof(long long) * HEALTH_ACCS * (size_t)B; }
    size_t health_off_thumbs() const { return (health_off_hist() + sizeof(int32_t) * 2 * VT_HEALTH_BINS * (size_t)B + 63) & ~(size_t)63; }
    size_t health_bytes() const { return health_off_thumbs() + sizeof(uint16_t) * 2 * (size_t)health_policy.max_cells * (size_t)B; }
    HealthPolicy* d_health_policy() const { return reinterpret_cast<HealthPolicy*>(d_health); }
    HealthRec* d_health_recs() const { return reinterpret_cast<HealthRec*>(d_health + health_off_recs()); }
    HealthCount* d_health_counts() const { return reinterpret_cast<HealthCount*>(d_health + health_off_counts()); }
    HealthHead* d_health_heads() const { return reinterpret_cast<HealthHead*>(d_health + health_off_heads()); }
    unsigned long long* d_health_accs() const { return reinterpret_cast<unsigned long long*>(d_health + health_off_accs()); }
    int32_t* d_health_hist() const { return reinterpret_cast<int32_t*>(d_health + health_off_hist()); }
    uint16_t* d_health_thumbs() const { return reinterpret_cast<uint16_t*>(d_health + health_off_thumbs()); }
    // pinned [B] by stream: the records of the last passes the host collected - what "health" and "health_words" report
    HealthRec* h_health_all = nullptr;
#define VT_HEALTH_STATS 24
#define VT_HEALTH_WORDS (2 * (int)(sizeof(HealthRec) / 4))
    int health_stats(int stream, float* out24);
    int health_words(int stream, float* out);       // the record's 32-bit words, low half then high half: every float exact
    // peak arbitration (k_arbitrate.hip). ONE policy per engine; per stream a record, two counters and four probes of template
    // rows, per (slot, peak) a ticket and the score launch's chunk partials. The first non-zero "arbitrate" - refused unless the
    // engine is appearance-capable: the anchors are the appearance store's - allocates all of it and makes the engine
    // arbitration-capable for good: every pass runs the four launches directly behind decode / cand_commit, ahead of
    // motion_settle, so that everything that reads the new box reads the final one.
    bool arb_capable = false;
    ArbPolicy arb_policy = VT_ARB_DEFAULT_POLICY;       // the host's copy
    // ONE allocation: the policy | [B] records | [B] counters | [4B] tickets | [4B][chunks][5] partials | [B][4][nt][kpad] probes,
    // zero up to the probes
    uint8_t* d_arb = nullptr;
    size_t arb_off_recs() const { return 64; }
    size_t arb_off_counts() const { return arb_off_recs() + sizeof(ArbRec) * (size_t)B; }
    size_t arb_off_tickets() const { return arb_off_counts() + sizeof(ArbCount) * (size_t)B; }
    size_t arb_off_partials() const { return (arb_off_tickets() + sizeof(unsigned) * VT_ARB_MAX * (size_t)B + 63) & ~(size_t)63; }
    size_t arb_off_probe() const { return (arb_off_partials() + sizeof(double) * 5 * VT_ARB_MAX * (size_t)B * appear_chunks(d.nt) + 63) & ~(size_t)63; }
    size_t arb_bytes() const { return arb_off_probe() + sizeof(bf16_t) * VT_ARB_MAX * appear_rows() * (size_t)B; }
    ArbPolicy* d_arb_policy() const { return reinterpret_cast<ArbPolicy*>(d_arb); }
    ArbRec* d_arb_recs() const { return reinterpret_cast<ArbRec*>(d_arb + arb_off_recs()); }
    ArbCount* d_arb_counts() const { return reinterpret_cast<ArbCount*>(d_arb + arb_off_counts()); }
    unsigned* d_arb_tickets() const { return reinterpret_cast<unsigned*>(d_arb + arb_off_tickets()); }
    double* d_arb_partials() const { return reinterpret_cast<double*>(d_arb + arb_off_partials()); }
    bf16_t* d_arb_probe() const { return reinterpret_cast<bf16_t*>(d_arb + arb_off_probe()); }
    // pinned [B] by stream: the records of the last passes the host collected - what "arbitrate" of vt_group_read_tensor reports
    ArbRec* h_arb_all = nullptr;
#define VT_ARB_STATS 48
    int arbitrate_stats(int stream, float* out48);
    vt_result* d_results = nullptr;
    // candidate passes (allocated by the first one): per slot a candidate state, the slot's vt_candidate and the winner
    // table; the pinned ring of candidate lists runs beside h_frames (same ring position, same event)
    StreamState* d_cand_states = nullptr;
    vt_candidate *d_cands = nullptr, *h_cands = nullptr;
    int32_t *d_winner = nullptr, *h_winner = nullptr;
    int ensure_candidate_buffers();
    // pinned host
    static const int RING = 8;
    FrameDesc* h_frames = nullptr;  // [RING] blocks of B descriptors + PassOut + the slot map (16-B multiples)
    size_t frames_block_bytes() const { return (sizeof(FrameDesc) * (size_t)B + sizeof(PassOut) + 4 * (size_t)B + 4 + 15) & ~(size_t)15; }
    size_t map_offset() const { return sizeof(FrameDesc) * (size_t)B + sizeof(PassOut); }
    size_t devflag_offset() const { return map_offset() + 4 * (size_t)B; }     // the pass's device-frames word (result overlay)
    const int32_t* d_devflag() const { return (const int32_t*)((const char*)d_frames + devflag_offset()); }
    const int32_t* d_map() const { return (const int32_t*)((const char*)d_frames + map_offset()); }
    // the last pass (written by build_block only): its slot count and, for a subset pass, the stream of every slot
    // (empty: all B streams in order); feat_in_head: it did not write d_feat (recomputed when read)
    int pass_n = 1;
    std::vector<int32_t> pass_streams;
    bool feat_in_head = false;
    // The last block on search rows only. Behind the last attention nobody reads the template rows:
    // where the pass is eligible its last attention writes the search queries' rows compactly ([n * ns][D] in d_attn),
    // proj reads its residual addend from the whole-layout pair through the row remap of the 256x256 kernel
    // (GemmArgs.seg_rows) and writes a compact pair, and fc1, fc2, the final LayerNorm and the head run on n * ns rows.
    // The compact pair lives in d_qk, which is dead behind the last attention: hi at its start, lo8 behind B * ns * D
    // bf16 elements (3 B * ns * D bytes of the 4 B * ntok * D the buffer has).
    int last_rows = 1;                  // vt_group_set_tuning "last_rows": 0 = every pass runs all rows
    bool pass_compact = false;          // the last pass's last block ran on the search rows only (written by build_block)
    bf16_t* xc_hi() const { return d_qk; }
    uint8_t* xc_lo() const { return reinterpret_cast<uint8_t*>(d_qk + (size_t)B * d.ns * d.D); }
    // a pass over n slots runs its last block on the search rows only: "last_rows" is on, no taps (they copy whole-layout
    // rows of every block), attention mode 3, and the compact proj (M = n * ns) still takes the 256x256 kernel, the only
    // one with the remapped addend read. with_taps false for the captured passes: they are never replayed under taps.
    bool last_block_compact(int n, bool with_taps) const;
    // reads of the whole-layout residual ("x", untapped "xrange") after a compacted pass: the compact search rows are
    // copied to their places in d_xh / d_xl, whose template rows still hold what block L-2 left. Idempotent.
    int expand_last_block();
    // after a candidate pass: pass_streams[i] is slot i's stream (streams may repeat) and pass_winner[i] the winning slot
    // of that stream; empty after every other pass
    std::vector<int32_t> pass_winner;
    bool cand_pending = false;          // the last pass enqueued was a candidate pass whose winners have not been collected
    int slot_of(int stream) const;      // slot of `stream` in the last pass (a candidate pass: its winning slot), -1 if it was not in it
    FrameDesc* h_block(int slot) const { return (FrameDesc*)((char*)h_frames + (size_t)slot * frames_block_bytes()); }
    hipEvent_t ring_ev[RING]{};
    int ring_pos = 0;
    vt_result* h_results = nullptr;
    StreamState* h_state = nullptr;
    // A pass's sinks: the PassOut (vt_common.hpp) of pinned buffers its outputs land in - results and peak records by
    // slot, states and every optional feature's records [B] by stream. The engine's own are h_results, h_states_all, h_peaks
    // and the h_*_all above; every pipelined slot has a record of its own. sinks_alloc gives a record the members asked for
    // that it lacks, [B] each and zero-filled (a member that exists stays: idempotent); sinks_free frees and nulls them. The
    // optional ones are the rows of ONE list (vt_features.hip: kSinks), which everything below walks.
    enum : unsigned { SINK_BASE = 1 /* results, states */, SINK_PEAKS = 2, SINK_MOTION = 4, SINK_APPEAR = 8, SINK_PROP = 16, SINK_CONFLICT = 32, SINK_HEALTH = 64, SINK_ARB = 128, SINK_ALL = 255 };
    unsigned sink_members() const;      // SINK_BASE and the sinks of the features the engine is capable of
    // what a pass's block carries of `to` (null: of the engine's own): host_states only with by_stream_states, an optional member only on a capable engine
    PassOut pass_sinks(const PassOut* to, bool by_stream_states) const;
    void adopt_stream_sinks(PassOut from, int stream);      // a collected pass's optional by-stream records of `stream` into the engine's own
    hipError_t sinks_alloc(PassOut* o, unsigned members) const;
    void sinks_free(PassOut* o, unsigned members) const;
    // What zeroes a by-stream record (the table's columns): an init, synchronous or queued; an import or
    // being the destination of a copy; vt_group_set_state_box; the feature's on-key set to 0; the feature's action key. Which
    // of them zeroes which record is the mask of its row of kSinks, and nowhere else.
    enum : unsigned { RESET_INIT = 1, RESET_IMPORT = 2, RESET_BOX = 4, RESET_OFF = 8, RESET_ACTION = 16 };
    // The records of streams [first, last) that `event` zeroes, among the sinks `of` (the last two events are one feature's),
    // on a capable engine: on the device behind the work on the engine's stream, and in the host's copies - the streams are
    // in no outstanding pass, nothing else writes their entries. The caller synchronises where it has to.
    int reset_records(unsigned event, int first, int last, unsigned of = SINK_ALL);
    // graph
    // one captured pass per crop-buffer tier (k_preproc.hip: 16 / 32 / 64 KiB of LDS per tile), all captured at creation
    static constexpr int TIERS = 3;
    // graphs[1], graphs[2], graphs[3]: the same passes with the crop kernels that read any vt_pixfmt / any vt_pixfmt2 as
    // well / any of those with a colour code other than BT.601 limited range
    // (k_preproc.hip: fetch_rgb<level>, vt_frame.hpp: pix_level), for passes that carry a format other than RGB8 / NV12 /
    // YUY2: all tiers of a level captured together (capture_all_graphs) when the first stream is initialised on a format
    // of that level - never inside an update
    struct PassGraph { hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; };
    PassGraph graphs[PIX_LEVELS][TIERS];          // [pix_level][tier]
    unsigned want_levels = 0;                     // bit l: a stream was initialised on a format of level l > 0: capture_all_graphs takes that set too
    int crop_tier_forced = -1;                    // >= 0: tests / A-B runs (vt_group_set_tuning "crop_tier")
    int graph_captures = 0;                       // hipGraph captures since creation (vt_group_graph_captures)
    long graph_replays[TIERS] = {0, 0, 0};        // passes replayed per tier (vt_group_read_tensor "graph_replays")
    bool head_band_ok = false;                    // the head's band kernel takes this model's shapes (planner consulted at creation)
    StageArena stage;               // host-frame staging of the synchronous entry points
    StreamState* h_states_all = nullptr;  // pinned mirror of d_states after the last pass
    int max_w = 3840, max_h = 2160;
    size_t max_device_bytes = 0;    // vt_config.max_device_mib (0: no limit but free memory)
    // host-side copy of the stream states after the last pass the HOST has collected (window planning
    // reads this, never a pinned buffer a running pass may still write)
    std::vector<StreamState> known;
    // pipelined host passes (vt_group_enqueue_host[_streams] / vt_group_wait_next): two slots, each with its own
    // pinned + device arena, result buffers, state snapshot and events; uploads go on copy_stream
    struct HostSlot {
        StageArena arena;
        // the pass's sinks (sinks_alloc): results and peak records by SLOT (list order); states and motion records [B]
        // by STREAM, valid at the listed streams' indices only
        PassOut out{};
        hipEvent_t up_ev = nullptr, done_ev = nullptr;
        std::vector<vt_frame> host;     // the caller's frames, valid until the pass is collected
        std::vector<int32_t> list;      // the pass's streams (the identity list: the full pass)
        std::vector<char> spec;         // per listed stream: its window was speculative (it was in the pass then outstanding)
        bool pending = false, redone = false;
        bool lists(int stream) const { return std::find(list.begin(), list.end(), stream) != list.end(); }
    } hs[2];
    // staging of the queued inits (vt_group_enqueue_init_host): each owns its pinned state + descriptor, its window
    // arena and the event behind its work on the group's stream; one is reused once that event has passed
    struct QueuedInit {
        StageArena arena;
        StreamState* h_state = nullptr;
        FrameDesc* h_desc = nullptr;
        hipEvent_t up_ev = nullptr, done_ev = nullptr;
    };
    std::vector<QueuedInit*> qinits;
    // staging of the stream snapshots (vt_snapshot.hip): a device record and its pinned twin, vt_group_snapshot_bytes
    // each, and the event behind the last work that reads or writes them. Allocated by the first export / import / copy
    // (an engine that never calls one has none); one is reused once its event has passed, so the synchronous calls
    // share one and every queued import has its own
    struct SnapStage {
        uint8_t *d = nullptr, *h = nullptr;
        hipEvent_t up_ev = nullptr, done_ev = nullptr;
    };
    std::vector<SnapStage*> snaps;
    size_t snapshot_bytes() const { return 256 + sizeof(bf16_t) * (size_t)d.nt * d.kpad; }
    int snap_staging(SnapStage** out);
    bool in_outstanding_pass(int stream) const {
        for (const HostSlot& sl : hs)
            if (sl.pending && sl.lists(stream)) return true;
        return false;
    }
    int check_init_box(vt_bbox box) const;
    // the state write, the template crop and its copy to d_tpl, on the group's stream; h_st / h_desc: pinned staging
    // that stays untouched until that work is done
    int launch_init(int b, const vt_frame* f, vt_bbox box, StreamState* h_st, FrameDesc* h_desc);
    hipStream_t copy_stream = nullptr;
    unsigned host_seq = 0, host_collected = 0;   // pipelined passes enqueued / collected
    unsigned host_redos = 0;                      // passes redone because a speculative window missed
    float margin = 0.75f;                         // speculative enlargement of the crop side
    int head_band_kernel = 2;                     // 0: the head as implicit GEMMs + head_out + decode (A/B, tests);
                                                  // 1: band kernels behind the LayerNorm kernel; 2: + the final LayerNorm
                                                  // inside the 1x1 layer's kernel where the shape allows it (default)
    bool head_band() const { return head_band_kernel && head_band_ok; }
    // the head's first kernel normalises its rows itself: the passes run no final LayerNorm and write no d_feat
    bool head_ln_fused() const { return head_band() && head_band_kernel >= 2 && headconv_ln_supported(d.gs, d.C, d.D); }
    hipError_t final_layernorm(int n, bool compact);     // compact: from the compact pair of a compacted pass
    int host_zero_copy = 0;                       // vt_config.host_zero_copy: 0 auto (single-stream engines), 1 always, -1 never
    float success_threshold = 0.2f;
    std::vector<int> h_initialized;

    ~Engine() { destroy(); }
    void destroy();
    int load_blob_host(const std::vector<uint8_t>& blob);
    int load_blob_device(const void* d_src, size_t bytes);
    int index_blob(const uint8_t* host_copy, size_t bytes);
    size_t activation_bytes() const;
    int alloc_buffers();
    int run_pass(Profiler* prof, const PassShape& ps);
    int restore_segments();             // every stream's template rows back into its own segment (after a subset pass)
    int capture_graph(int tier, int any_layout);      // the full pass of that shape into graphs[any_layout][tier]
    int capture_all_graphs();
    int capture_graphs_for(int format);           // the graph set of the format's level, once, when a stream starts on a format that needs it
    int pick_crop_tier(const int32_t* streams = nullptr, int n = 0) const;   // streams == null: all B
    int pick_crop_tier(const vt_candidate* cands, int n) const;              // a candidate pass: from the slots' boxes
    void drop_graphs();
    // One pass over streams[0..n), frames[i] for streams[i]; streams == null: all B streams in order (n == B), and no
    // list is built for it. VT_ERR_INVALID_ARG / VT_ERR_NOT_INITIALIZED with nothing enqueued on bad input (checked in
    // the order list, initialisation, frames). sinks: where the pass's outputs land (null: the engine's own buffers).
    int check_streams(const int32_t* streams, int n) const;
    // The one place a pass's block is put together, for n checked frames: a block of the pinned ring once the copy that
    // last used it is done - descriptors, PassOut (host_states only with by_stream_states; peak and motion records only
    // on engines capable of them), the slot map (map: slot -> stream; null: the full pass) and the device-frames word -
    // uploaded behind the stream's work, its event recorded, and the last-pass record written. *ps: n, slot_stream,
    // any_layout and compact filled; tier and cand are the caller's. The engine's device is current.
    int build_block(const int32_t* map, const vt_frame* frames, int n, const PassOut* sinks, bool by_stream_states, PassShape* ps);
    // checks + build_block + the template rows' bookkeeping + the tier; the engine's device is current
    int prepare_pass(const int32_t* streams, const vt_frame* frames, int n, const PassOut* sinks, PassShape* ps);
    int enqueue(const int32_t* streams, const vt_frame* frames, int n, const PassOut* sinks = nullptr);
    int wait(vt_result* out, int n);
    // A candidate pass over cands[0..n) (k_cand.hip): checked (list, boxes, initialisation, frames - nothing enqueued
    // on bad input), built and launched eagerly. A list that is a plain subset pass - every stream once, no box - goes
    // through enqueue() as that pass. wait_candidates collects results and winners and gives slot_of the winner's meaning.
    int check_candidates(const vt_candidate* cands, int n) const;
    static bool plain_list(const vt_candidate* cands, int n, std::vector<int32_t>* streams);
    int enqueue_candidates(const vt_candidate* cands, const vt_frame* frames, int n);
    int wait_candidates(vt_result* out, int32_t* winner, int n);
    int init_stream(int b, const vt_frame* f, vt_bbox box);
    const TensorRef* find(const std::string& n) const {
        auto it = tens.find(n);
        return it == tens.end() ? nullptr : &it->second;
    }
    double flops_encoder() const;
    double flops_head() const;
};

// A keyed feature: ONE engine-wide policy of int32_t words set through keys of vt_group_set_tuning (vt_feature_keys.hpp),
// a device store with that policy at its start, at most one by-stream sink, one statistics tensor of vt_group_read_tensor.
// keyed_features() (vt_features.hip) is the ONE place a new one registers: everything else walks that list.
struct KeyedFeature {
    const char *name, *prefix;                  // for the messages; a key is the feature's iff it starts with prefix
    vtkeys::Apply apply;                        // the key table and its specials
    int32_t Engine::*policy; int words, on_word;        // the host's copy as words (a new Engine's: the defaults); the first non-zero value of word on_word enables
    const char* on_key;                         // that word's key: set to 0 on a capable engine it is the RESET_OFF of the feature's records
    bool Engine::*capable; uint8_t* Engine::*store;
    size_t (Engine::*store_bytes)() const;      // of an engine with the host's copy as it is
    size_t (Engine::*zeroed_bytes)() const;     // leading bytes the enable zero-fills; null: all
    unsigned sink; const char* tensor; int stats_len;   // SINK_* or 0: none; the name of vt_group_read_tensor that answers stats_len floats from stats
    int (Engine::*stats)(int stream, float* out);       // of a capable engine. The rest: null if not needed
    hipError_t (*fill)(Engine*, uint8_t* store) = nullptr;      // more than zeros and the policy in the new store
    const char* action_key = nullptr; int (Engine::*action)(int value) = nullptr;       // a key that is an action, not a field, and what it does
    int (*refuse_enable)(Engine*) = nullptr;    // a reason this engine cannot enable at all
};
const std::array<KeyedFeature, 7>& keyed_features();
int not_enabled(const KeyedFeature& f);         // the ONE error of a tensor of f's on an engine that is not capable of f

// zero-filled device buffer. The fill is ordered on the ENGINE's stream: that stream is non-blocking, so a
// hipMemset on the null stream (asynchronous for device memory) is not ordered against the kernels the
// engine launches next - the LayerNorm fold at construction raced with the fill of its own output when
// the null stream was busy zeroing the gigabytes of a several-hundred-stream engine.
template <typename T>
static hipError_t dalloc0(T** p, size_t count, hipStream_t s) {
    hipError_t e = hipMalloc((void**)p, count * sizeof(T));
    if (e != hipSuccess) return e;
    return hipMemsetAsync(*p, 0, count * sizeof(T), s);
}

int read_file(const char* path, std::vector<uint8_t>* out);
int check_device(int device_id);
int make_engine(const char* path, const void* d_src, size_t bytes, int device_id, const vt_config* cfg, int B, Engine** out);
void fill_info(const Engine* e, vt_model_info* o);
int check_frame(const vt_frame& f);
int check_state_box(const float* box4);     // the one check of a caller's state box (vt_group_set_state_box, candidate slots)
void to_desc(const vt_frame& f, FrameDesc* o);

// ---- handles of the C ABI --------------------------------------------------------------------------
struct vt_group { Engine* e; };
struct vt_tracker {                 // view: the tracker as a group of one
    Engine* e;
    vt_group view;
    explicit vt_tracker(Engine* en) : e(en), view{en} {}
};

// A pipelined host pass (vt_group_enqueue_host) that has not been collected owns the stream states
int refuse_while_pipelined(const Engine* e, const char* what);

// ---- host-frame ingest (vt_ingest.hip) ---------------------------------------------------------------
// share: slots that name the same host frame are staged once, as the bounding rectangle of their windows
int stage_host_frames(Engine* e, const vt_frame* host, int n, const float (*boxes)[4], vt_frame* dev, bool share = false);
const uint8_t* mapped_device_ptr(int device, const uint8_t* p, size_t bytes);

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 4); }
};
size_t nv12_bytes_read(size_t w, size_t h);
