// vt_feature_keys.hpp — the vt_group_set_tuning keys of the keyed optional features as tables: the word of the policy a key
// writes, what it accepts, what it says when it refuses. Pure C++17 - no HIP, nothing of vt_engine.hpp - so
// tests/feature_keys_main.cpp runs all of it on the CPU. vt_features.hip asserts the word indices against the structs.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace vtkeys {
// a value < 0 stands for the default's word, anything else must lie in lo..hi; refusal: a printf format for the caller's value
// bits > 0: the key is the field of `bits` bits at bit `shift` of its word (several small keys share a word); 0: the whole word
struct Key {
    const char* key; int word; int32_t lo, hi; const char* refusal; int shift = 0, bits = 0;
    constexpr int32_t get(int32_t w) const { return bits ? (int32_t)(((uint32_t)w >> shift) & ((1u << bits) - 1u)) : w; }
    constexpr int32_t put(int32_t w, int32_t v) const {
        return bits ? (int32_t)(((uint32_t)w & ~(((1u << bits) - 1u) << shift)) | ((uint32_t)v << shift)) : v;
    }
};
enum Answer { ACCEPTED, REFUSED, UNKNOWN };     // REFUSED: words untouched, text written; UNKNOWN: not a key of the table
constexpr int kMaxWords = 8;                    // of the longest policy
template <int N>
inline Answer apply(const Key (&rows)[N], const char* key, int value, const int32_t* def, int32_t* words, char* text, size_t cap) {
    for (const Key& k : rows) {
        if (strcmp(key, k.key) != 0) continue;
        const int32_t v = value < 0 ? k.get(def[k.word]) : value;
        if (v < k.lo || v > k.hi) { snprintf(text, cap, k.refusal, value); return REFUSED; }
        words[k.word] = k.put(words[k.word], v);
        return ACCEPTED;
    }
    return UNKNOWN;
}
inline float tau_of(int32_t pm) { return (float)pm / 1000.0f; }
inline void put_tau(int32_t* word, int32_t pm) { const float tau = tau_of(pm); memcpy(word, &tau, sizeof(tau)); }    // one binary32 divide
// a feature's keys from outside, table and specials: one (key, value) applied to `words`; capable: the engine has enabled it
typedef Answer (*Apply)(const char* key, int value, const int32_t* def, int32_t* words, bool capable, char* text, size_t cap);
// An operator hook's policy words through a feature's table, row by row: -1 and `words` filled, or the index of the first row
// refused. A hook takes no "default" value: a negative word is refused here
template <int N>
inline int check_words(const Key (&rows)[N], Apply apply, const int32_t* def, const int32_t* policy, int32_t* words) {
    char text[256];
    for (int i = 0; i < N; ++i) {
        const int32_t v = policy[rows[i].word] < 0 ? -1 : rows[i].get(policy[rows[i].word]);
        if (v < 0 || apply(rows[i].key, v, def, words, false, text, sizeof(text)) != ACCEPTED) return i;
    }
    // a word shared by bit-field keys holds nothing but their fields: a bit beside them is refused at the word's first row
    for (int i = 0; i < N; ++i)
        if (rows[i].bits && words[rows[i].word] != policy[rows[i].word]) {
            for (int j = 0; j < N; ++j)
                if (rows[j].word == rows[i].word) return j;
        }
    return -1;
}

enum { OV_FLAGS, OV_THICKNESS, OV_SIZE, OV_SCALE, OV_LUMA, OV_RGB, OV_MIN_SCORE_PCT, OV_WORDS = 8 };      // OverlayPolicy
static constexpr Key kOverlayKeys[] = {
    {"result_overlay", OV_FLAGS, 0, 7, "result_overlay: flags %d (1 rectangle | 2 crosshair | 4 label, 0: off)"},
    {"result_overlay_luma", OV_LUMA, 0, 255, "result_overlay_luma: %d (0..255)"},
    {"result_overlay_rgb", OV_RGB, 0, 0xFFFFFF, "result_overlay_rgb: 0x%x (0..0xFFFFFF)"},
    {"result_overlay_min_score_pct", OV_MIN_SCORE_PCT, 0, 100, "result_overlay_min_score_pct: %d (0..100)"},
};
// "result_overlay_style": thickness | size << 8 | scale << 16; a negative value restores all three
inline Answer apply_overlay(const char* key, int value, const int32_t* def, int32_t* words, bool, char* text, size_t cap) {
    if (strcmp(key, "result_overlay_style") != 0) return apply(kOverlayKeys, key, value, def, words, text, cap);
    const int th = value & 255, size = (value >> 8) & 255, scale = value >> 16;
    if (value >= 0 && (th < 1 || th > 16 || size < 1 || size > 64 || scale < 1 || scale > 4)) {
        snprintf(text, cap, "result_overlay_style: thickness %d (1..16), size %d (1..64), scale %d (1..4)", th, size, scale);
        return REFUSED;
    }
    words[OV_THICKNESS] = value < 0 ? def[OV_THICKNESS] : th;
    words[OV_SIZE] = value < 0 ? def[OV_SIZE] : size;
    words[OV_SCALE] = value < 0 ? def[OV_SCALE] : scale;
    return ACCEPTED;
}

enum { MO_ON, MO_GAIN_PCT, MO_COAST, MO_MAX_PCT, MO_WORDS };      // MotionPolicy
static constexpr Key kMotionKeys[] = {
    {"motion_prior", MO_ON, 0, 1, "motion_prior: %d (0: off, 1: on)"},
    {"motion_gain_pct", MO_GAIN_PCT, 1, 100, "motion_gain_pct: %d (1..100)"},
    {"motion_coast", MO_COAST, 0, 60, "motion_coast: %d (0..60)"},
    {"motion_max_pct", MO_MAX_PCT, 0, 200, "motion_max_pct: %d (0..200)"},
};
inline Answer apply_motion(const char* key, int value, const int32_t* def, int32_t* words, bool, char* text, size_t cap) {
    return apply(kMotionKeys, key, value, def, words, text, cap);
}

enum { AP_ON, AP_PERIOD, AP_GATE_PM, AP_TAU, AP_WORDS };          // AppearPolicy
static constexpr Key kAppearKeys[] = {
    {"appearance", AP_ON, 0, 1, "appearance: %d (0: off, 1: on)"},
    {"appearance_period", AP_PERIOD, 1, 1000000, "appearance_period: %d (1..1000000)"},
    {"appearance_gate_pm", AP_GATE_PM, 0, 1000, "appearance_gate_pm: %d (0..1000)"},
};
inline Answer apply_appearance(const char* key, int value, const int32_t* def, int32_t* words, bool, char* text, size_t cap) {
    const Answer a = apply(kAppearKeys, key, value, def, words, text, cap);
    if (a == ACCEPTED && strcmp(key, "appearance_gate_pm") == 0) put_tau(words + AP_TAU, words[AP_GATE_PM]);
    return a;
}

enum { PR_MODE, PR_PERIOD, PR_MAX_N, PR_MIN_SIM_PM, PR_TAU, PR_MAX_CELLS, PR_WORDS = 8 };     // PropPolicy
static constexpr Key kPropKeys[] = {
    {"proposals", PR_MODE, 0, 2, "proposals: %d (0: off, 1: failed updates, 2: every update)"},
    {"proposals_period", PR_PERIOD, 1, 1000000, "proposals_period: %d (1..1000000)"},
    {"proposals_max", PR_MAX_N, 1, 8, "proposals_max: %d (1..8)"},
    {"proposals_min_sim_pm", PR_MIN_SIM_PM, 0, 1000, "proposals_min_sim_pm: %d (0..1000)"},
    {"proposals_max_cells", PR_MAX_CELLS, 16384, 4194304, "proposals_max_cells: %d (16384..4194304)"},
};
// "proposals_max_cells" sizes the store: frozen once the engine is capable, whatever the value
inline Answer apply_proposals(const char* key, int value, const int32_t* def, int32_t* words, bool capable, char* text, size_t cap) {
    if (capable && strcmp(key, "proposals_max_cells") == 0) {
        snprintf(text, cap, "proposals_max_cells: fixed by the first enable of \"proposals\" (%d)", (int)words[PR_MAX_CELLS]);
        return REFUSED;
    }
    const Answer a = apply(kPropKeys, key, value, def, words, text, cap);
    if (a == ACCEPTED && strcmp(key, "proposals_min_sim_pm") == 0) put_tau(words + PR_TAU, words[PR_MIN_SIM_PM]);
    return a;
}

enum { CF_ON, CF_IOU_PM, CF_GATE, CF_TAU, CF_WORDS = 8 };         // ConflictPolicy
static constexpr Key kConflictKeys[] = {
    {"conflicts", CF_ON, 0, 1, "conflicts: %d (0: off, 1: on)"},
    {"conflicts_iou_pm", CF_IOU_PM, 1, 1000, "conflicts_iou_pm: %d (1..1000)"},
    {"conflicts_gate", CF_GATE, 0, 1, "conflicts_gate: %d (0: report only, 1: refresh rule 9)"},
};
inline Answer apply_conflicts(const char* key, int value, const int32_t* def, int32_t* words, bool, char* text, size_t cap) {
    const Answer a = apply(kConflictKeys, key, value, def, words, text, cap);
    if (a == ACCEPTED && strcmp(key, "conflicts_iou_pm") == 0) put_tau(words + CF_TAU, words[CF_IOU_PM]);
    return a;
}
// The value of the "conflicts_scene" action on an engine of B streams: stream | scene << 16. Stream 0xFFFF: every stream;
// -1: every stream back to scene 0. ACCEPTED: streams [*first, *last) go to *scene; REFUSED: text written, nothing else.
constexpr int kSceneAllStreams = 0xFFFF;
inline Answer decode_scene(int value, int B, int* first, int* last, int32_t* scene, char* text, size_t cap) {
    const int stream = value & 0xFFFF, sc = value >> 16;
    if (value < -1 || (value >= 0 && stream != kSceneAllStreams && stream >= B)) {
        if (value < -1) snprintf(text, cap, "conflicts_scene: %d (stream | scene << 16, stream 0xFFFF: all; -1: every stream to scene 0)", value);
        else snprintf(text, cap, "conflicts_scene: stream %d (0..%d, 0xFFFF: all) of scene %d", stream, B - 1, sc);
        return REFUSED;
    }
    const bool all = value < 0 || stream == kSceneAllStreams;
    *first = all ? 0 : stream; *last = all ? B : stream + 1;
    *scene = value < 0 ? 0 : sc;
    return ACCEPTED;
}

// camera motion (k_camera_motion.hip): the policy words of vt_op_camera_motion, which validates them with this table; no
// engine key reaches it yet
enum { CM_MODE, CM_CELL, CM_RANGE, CM_CONF_PM, CM_MAX_CELLS, CM_WORDS = 8 };      // CamPolicy
static constexpr Key kCameraKeys[] = {
    {"camera_motion", CM_MODE, 0, 2, "camera_motion: %d (0: off, 1: measure, 2: measure and move the box)"},
    {"camera_motion_cell", CM_CELL, 0, 32, "camera_motion_cell: %d (0: automatic, 4, 8, 16 or 32)"},
    {"camera_motion_range", CM_RANGE, 2, 16, "camera_motion_range: %d (2..16)"},
    {"camera_motion_conf_pm", CM_CONF_PM, 0, 1000, "camera_motion_conf_pm: %d (0..1000)"},
    {"camera_motion_max_cells", CM_MAX_CELLS, 4096, 1048576, "camera_motion_max_cells: %d (4096..1048576)"},
};
// "camera_motion_cell": 0 or a power of two in 4..32; "camera_motion_max_cells" sizes the store: frozen once the engine is capable
inline Answer apply_camera_motion(const char* key, int value, const int32_t* def, int32_t* words, bool capable, char* text, size_t cap) {
    if (capable && strcmp(key, "camera_motion_max_cells") == 0) {
        snprintf(text, cap, "camera_motion_max_cells: fixed by the first enable of \"camera_motion\" (%d)", (int)words[CM_MAX_CELLS]);
        return REFUSED;
    }
    if (strcmp(key, "camera_motion_cell") == 0 && value > 0 && (value < 4 || (value & (value - 1)) != 0)) {
        snprintf(text, cap, kCameraKeys[CM_CELL].refusal, value);
        return REFUSED;
    }
    return apply(kCameraKeys, key, value, def, words, text, cap);
}

// frame health (k_health.hip): the "health*" keys; vt_op_frame_health validates its policy words with the same table
enum { HL_ON, HL_PERIOD, HL_CELL, HL_STILL_RUN, HL_FLAT_Q, HL_CUT_PM, HL_GATE, HL_MAX_CELLS, HL_WORDS = 8 };     // HealthPolicy
static constexpr Key kHealthKeys[] = {
    {"health", HL_ON, 0, 1, "health: %d (0: off, 1: on)"},
    {"health_period", HL_PERIOD, 1, 1000000, "health_period: %d (1..1000000)"},
    {"health_cell", HL_CELL, 0, 32, "health_cell: %d (0: automatic, 4, 8, 16 or 32)"},
    {"health_still_run", HL_STILL_RUN, 1, 1000, "health_still_run: %d (1..1000)"},
    {"health_flat_q", HL_FLAT_Q, 0, 4080, "health_flat_q: %d (0..4080)"},
    {"health_cut_pm", HL_CUT_PM, 0, 1000, "health_cut_pm: %d (0..1000, 0: never)"},
    {"health_gate", HL_GATE, 0, 1, "health_gate: %d (0: report only, 1: refresh rule 10)"},
    {"health_max_cells", HL_MAX_CELLS, 4096, 262144, "health_max_cells: %d (4096..262144)"},
};
// "health_cell": 0 or a power of two in 4..32; "health_max_cells" sizes the store: frozen once the engine is capable
inline Answer apply_health(const char* key, int value, const int32_t* def, int32_t* words, bool capable, char* text, size_t cap) {
    if (capable && strcmp(key, "health_max_cells") == 0) {
        snprintf(text, cap, "health_max_cells: fixed by the first enable of \"health\" (%d)", (int)words[HL_MAX_CELLS]);
        return REFUSED;
    }
    if (strcmp(key, "health_cell") == 0 && value > 0 && (value < 4 || (value & (value - 1)) != 0)) {
        snprintf(text, cap, kHealthKeys[HL_CELL].refusal, value);
        return REFUSED;
    }
    return apply(kHealthKeys, key, value, def, words, text, cap);
}

// peak arbitration (k_arbitrate.hip): the "arbitrate*" keys; vt_op_arbitrate validates its policy words with the same table.
// Six keys and two reserved words; the kernels form each threshold as (float)pm / 1000.0f - the text of tau_of -
// so no derived word is stored
enum { AR_ON, AR_MAX, AR_RADIUS, AR_MIN_RESP_PM, AR_LOW_PM, AR_HIGH_PM, AR_WORDS = 8 };      // ArbPolicy
static constexpr Key kArbKeys[] = {
    {"arbitrate", AR_ON, 0, 1, "arbitrate: %d (0: off, 1: on)"},
    {"arbitrate_max", AR_MAX, 2, 4, "arbitrate_max: %d (2..4)"},
    {"arbitrate_radius", AR_RADIUS, 1, 4, "arbitrate_radius: %d (1..4)"},
    {"arbitrate_min_resp_pm", AR_MIN_RESP_PM, 0, 1000, "arbitrate_min_resp_pm: %d (0..1000)"},
    {"arbitrate_low_pm", AR_LOW_PM, 0, 1000, "arbitrate_low_pm: %d (0..1000)"},
    {"arbitrate_high_pm", AR_HIGH_PM, 0, 1000, "arbitrate_high_pm: %d (0..1000)"},
};
inline Answer apply_arbitrate(const char* key, int value, const int32_t* def, int32_t* words, bool, char* text, size_t cap) {
    return apply(kArbKeys, key, value, def, words, text, cap);
}

// moving regions (k_movers.hip): the policy words of vt_op_movers, which validates them with this table; no engine key
// reaches it yet. Ten keys in
// eight words - kMaxWords stays 8 -: "movers_learn", "movers_min_nb" and "movers_max" are four-bit fields of word MV_SHAPE
enum { MV_ON, MV_PERIOD, MV_CELL, MV_THR, MV_MIN_AREA, MV_GLOBAL_PM, MV_SHAPE, MV_MAX_CELLS, MV_WORDS = 8 };     // MoverPolicy
static constexpr Key kMoverKeys[] = {
    {"movers", MV_ON, 0, 1, "movers: %d (0: off, 1: on)"},
    {"movers_period", MV_PERIOD, 1, 1000000, "movers_period: %d (1..1000000)"},
    {"movers_cell", MV_CELL, 0, 32, "movers_cell: %d (0: automatic, 4, 8, 16 or 32)"},
    {"movers_thr", MV_THR, 0, 4080, "movers_thr: %d (0..4080)"},
    {"movers_min_area", MV_MIN_AREA, 1, 262144, "movers_min_area: %d (1..262144)"},
    {"movers_global_pm", MV_GLOBAL_PM, 0, 1000, "movers_global_pm: %d (0..1000, 1000: never)"},
    {"movers_learn", MV_SHAPE, 0, 8, "movers_learn: %d (0..8)", 0, 4},
    {"movers_min_nb", MV_SHAPE, 1, 9, "movers_min_nb: %d (1..9)", 4, 4},
    {"movers_max", MV_SHAPE, 1, 8, "movers_max: %d (1..8)", 8, 4},
    {"movers_max_cells", MV_MAX_CELLS, 4096, 262144, "movers_max_cells: %d (4096..262144)"},
};
// "movers_cell": 0 or a power of two in 4..32; "movers_max_cells" sizes the store: frozen once the engine is capable
inline Answer apply_movers(const char* key, int value, const int32_t* def, int32_t* words, bool capable, char* text, size_t cap) {
    if (capable && strcmp(key, "movers_max_cells") == 0) {
        snprintf(text, cap, "movers_max_cells: fixed by the first enable of \"movers\" (%d)", (int)words[MV_MAX_CELLS]);
        return REFUSED;
    }
    if (strcmp(key, "movers_cell") == 0 && value > 0 && (value < 4 || (value & (value - 1)) != 0)) {
        for (const Key& k : kMoverKeys)         // the row of that key, wherever it stands in the table
            if (strcmp(k.key, key) == 0) snprintf(text, cap, k.refusal, value);
        return REFUSED;
    }
    return apply(kMoverKeys, key, value, def, words, text, cap);
}
}   // namespace vtkeys
