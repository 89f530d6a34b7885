// The key tables of the keyed optional features (csrc/vt_feature_keys.hpp) on the CPU: tests/test_feature_keys_host.py compiles
// this with -fsanitize=address,undefined and runs it. Prints one line per failed check; the exit status is their number (0: all
// hold). The refusal texts are written out here: they are what callers have seen since the features exist.
#include <cstdio>
#include <string>

#include "vt_feature_keys.hpp"

using namespace vtkeys;

static int failures = 0;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) { ++failures; printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

static int32_t bits_of(float f) { int32_t u; memcpy(&u, &f, 4); return u; }

// the default policies as words (VT_*_DEFAULT_POLICY of the engine's headers)
static const int32_t kOverlayDef[8] = {0, 3, 15, 2, 255, 0x00FF00, 25, 0};
static const int32_t kMotionDef[8] = {0, 50, 5, 100, 0, 0, 0, 0};
static const int32_t kAppearDef[8] = {0, 1, 0, 0 /* 0.0f */, 0, 0, 0, 0};
static const int32_t kPropDef[8] = {0, 1, 4, 500, 0x3F000000 /* 0.5f */, 262144, 0, 0};
static const int32_t kConflictDef[8] = {0, 300, 0, 0x3E99999A /* 0.3f */, 0, 0, 0, 0};
static const int32_t kCameraDef[8] = {0, 0, 8, 800, 65536, 0, 0, 0};
static const int32_t kHealthDef[8] = {0, 1, 0, 3, 32, 500, 0, 65536};
static const int32_t kArbDef[8] = {0, 3, 2, 50, 300, 500, 0, 0};

// one key as the engine's callers know it: bounds, and the texts one past each bound (null: a value below is the default)
struct Want { const char* key; int32_t lo, hi; const char* below; const char* above; };
static const Want kOverlayWant[] = {
    {"result_overlay", 0, 7, nullptr, "result_overlay: flags 8 (1 rectangle | 2 crosshair | 4 label, 0: off)"},
    {"result_overlay_luma", 0, 255, nullptr, "result_overlay_luma: 256 (0..255)"},
    {"result_overlay_rgb", 0, 0xFFFFFF, nullptr, "result_overlay_rgb: 0x1000000 (0..0xFFFFFF)"},
    {"result_overlay_min_score_pct", 0, 100, nullptr, "result_overlay_min_score_pct: 101 (0..100)"},
};
static const Want kMotionWant[] = {
    {"motion_prior", 0, 1, nullptr, "motion_prior: 2 (0: off, 1: on)"},
    {"motion_gain_pct", 1, 100, "motion_gain_pct: 0 (1..100)", "motion_gain_pct: 101 (1..100)"},
    {"motion_coast", 0, 60, nullptr, "motion_coast: 61 (0..60)"},
    {"motion_max_pct", 0, 200, nullptr, "motion_max_pct: 201 (0..200)"},
};
static const Want kAppearWant[] = {
    {"appearance", 0, 1, nullptr, "appearance: 2 (0: off, 1: on)"},
    {"appearance_period", 1, 1000000, "appearance_period: 0 (1..1000000)", "appearance_period: 1000001 (1..1000000)"},
    {"appearance_gate_pm", 0, 1000, nullptr, "appearance_gate_pm: 1001 (0..1000)"},
};
static const Want kPropWant[] = {
    {"proposals", 0, 2, nullptr, "proposals: 3 (0: off, 1: failed updates, 2: every update)"},
    {"proposals_period", 1, 1000000, "proposals_period: 0 (1..1000000)", "proposals_period: 1000001 (1..1000000)"},
    {"proposals_max", 1, 8, "proposals_max: 0 (1..8)", "proposals_max: 9 (1..8)"},
    {"proposals_min_sim_pm", 0, 1000, nullptr, "proposals_min_sim_pm: 1001 (0..1000)"},
    {"proposals_max_cells", 16384, 4194304, "proposals_max_cells: 16383 (16384..4194304)", "proposals_max_cells: 4194305 (16384..4194304)"},
};

// the words a refusal or an unknown key must leave alone: no default among them
static void scramble(int32_t* w) { for (int i = 0; i < kMaxWords; ++i) w[i] = 0x5A5A0000 + i; }
static bool same(const int32_t* a, const int32_t* b) { return memcmp(a, b, sizeof(int32_t) * kMaxWords) == 0; }

template <int N, int M>
static void table(const char* name, const Key (&rows)[N], const Want (&want)[M], Apply apply, const int32_t* def, const char* unknown) {
    CHECK(N == M, "%s: %d rows, %d written out here", name, N, M);
    int32_t w[kMaxWords], before[kMaxWords];
    char text[256];
    for (int i = 0; i < N && i < M; ++i) {
        const Key& k = rows[i];
        const Want& x = want[i];
        CHECK(std::string(k.key) == x.key && k.lo == x.lo && k.hi == x.hi, "%s row %d: %s %d..%d", name, i, k.key, (int)k.lo, (int)k.hi);
        CHECK(k.word >= 0 && k.word < kMaxWords, "%s: word %d", k.key, k.word);
        CHECK(def[k.word] >= k.lo && def[k.word] <= k.hi, "%s: the default %d is not a legal value", k.key, (int)def[k.word]);
        const struct { int value; int32_t lands; } ok[] = {{-1, def[k.word]}, {-7, def[k.word]}, {k.lo, k.lo}, {k.hi, k.hi}};
        for (const auto& c : ok) {
            scramble(w); scramble(before);
            CHECK(apply(k.key, c.value, def, w, false, text, sizeof(text)) == ACCEPTED, "%s %d not accepted", k.key, c.value);
            CHECK(w[k.word] == c.lands, "%s %d wrote %d", k.key, c.value, (int)w[k.word]);
            for (int j = 0; j < kMaxWords; ++j)     // its own word, and for the two per-mille keys the derived one behind it
                if (j != k.word && w[j] != before[j])
                    CHECK(j == k.word + 1 && w[j] == bits_of((float)w[k.word] / 1000.0f) && std::string(k.key).find("_pm") != std::string::npos,
                          "%s %d also wrote word %d", k.key, c.value, j);
        }
        const struct { int value; const char* text; } bad[] = {{k.lo - 1, x.below}, {k.hi + 1, x.above}};
        for (const auto& c : bad) {
            if (!c.text) { CHECK(c.value == -1, "%s: no text for %d", k.key, c.value); continue; }
            scramble(w); scramble(before);
            text[0] = 0;
            CHECK(apply(k.key, c.value, def, w, false, text, sizeof(text)) == REFUSED, "%s %d not refused", k.key, c.value);
            CHECK(same(w, before), "%s %d: a refusal changed the words", k.key, c.value);
            CHECK(std::string(text) == c.text, "%s %d says '%s', not '%s'", k.key, c.value, text, c.text);
        }
    }
    scramble(w); scramble(before);
    CHECK(apply(unknown, 1, def, w, false, text, sizeof(text)) == UNKNOWN && same(w, before), "%s: '%s' is not unknown", name, unknown);
    CHECK(apply("", 1, def, w, true, text, sizeof(text)) == UNKNOWN && same(w, before), "%s: the empty key is not unknown", name);
}

// check_words: the policy words of an operator hook through a table. Every row's lo and hi are legal values of these five
// tables (the cell keys: 0 and 32). pm, tau: the word of a per-mille key and the word its threshold lands in, or -1
template <int N>
static void hook_words(const char* name, const Key (&rows)[N], Apply apply, const int32_t* def, int pm, int tau) {
    int32_t pol[kMaxWords], w[kMaxWords], want[kMaxWords];
    for (const bool high : {false, true}) {
        memset(pol, 0, sizeof(pol));
        for (const Key& k : rows) pol[k.word] = high ? k.hi : k.lo;
        memcpy(want, pol, sizeof(want));
        if (pm >= 0) want[tau] = bits_of((float)pol[pm] / 1000.0f);
        memset(w, 0, sizeof(w));
        CHECK(check_words(rows, apply, def, pol, w) == -1 && same(w, want), "%s: the %s bounds are not taken as they are", name, high ? "upper" : "lower");
    }
    for (int i = 0; i < N; ++i) {
        for (const int32_t v : {rows[i].lo - 1, rows[i].hi + 1, -1, -7}) {      // a hook takes no "default": a negative word is refused
            for (const Key& k : rows) pol[k.word] = k.lo;
            pol[rows[i].word] = v;
            CHECK(check_words(rows, apply, def, pol, w) == i, "%s: %s = %d is not refused at row %d", name, rows[i].key, (int)v, i);
            pol[rows[N - 1].word] = rows[N - 1].hi + 1;     // a second bad word behind it: the lower row is named
            CHECK(check_words(rows, apply, def, pol, w) == i, "%s: %s = %d and a bad last word: not row %d", name, rows[i].key, (int)v, i);
        }
    }
}

static void hook_cells() {      // neither 0 nor a power of two in 4..32
    int32_t pol[kMaxWords], w[kMaxWords];
    for (const int32_t cell : {1, 2, 3, 5, 12, 31}) {
        memcpy(pol, kCameraDef, sizeof(pol)); pol[CM_CELL] = cell;
        CHECK(check_words(kCameraKeys, apply_camera_motion, kCameraDef, pol, w) == CM_CELL, "camera_motion_cell %d", (int)cell);
        memcpy(pol, kHealthDef, sizeof(pol)); pol[HL_CELL] = cell;
        CHECK(check_words(kHealthKeys, apply_health, kHealthDef, pol, w) == HL_CELL, "health_cell %d", (int)cell);
    }
    memcpy(pol, kHealthDef, sizeof(pol));       // the defaults themselves pass, as the words they are
    CHECK(check_words(kHealthKeys, apply_health, kHealthDef, pol, w) == -1 && same(w, kHealthDef), "the health defaults");
}

static void derived() {
    int32_t w[kMaxWords];
    char text[256];
    for (int pm = 0; pm <= 1000; ++pm) {
        const int32_t want = bits_of((float)pm / 1000.0f);
        CHECK(bits_of(tau_of(pm)) == want, "tau_of(%d)", pm);
        scramble(w);
        CHECK(apply_appearance("appearance_gate_pm", pm, kAppearDef, w, pm & 1, text, sizeof(text)) == ACCEPTED && w[AP_GATE_PM] == pm &&
              w[AP_TAU] == want, "appearance_gate_pm %d: tau bits 0x%08x, want 0x%08x", pm, (unsigned)w[AP_TAU], (unsigned)want);
        scramble(w);
        CHECK(apply_proposals("proposals_min_sim_pm", pm, kPropDef, w, pm & 1, text, sizeof(text)) == ACCEPTED && w[PR_MIN_SIM_PM] == pm &&
              w[PR_TAU] == want, "proposals_min_sim_pm %d: tau bits 0x%08x, want 0x%08x", pm, (unsigned)w[PR_TAU], (unsigned)want);
    }
    // the defaults are consistent with the derivation, and a default value derives too
    CHECK(kAppearDef[AP_TAU] == bits_of(tau_of(kAppearDef[AP_GATE_PM])) && kPropDef[PR_TAU] == bits_of(tau_of(kPropDef[PR_MIN_SIM_PM])), "default taus");
    scramble(w);
    CHECK(apply_proposals("proposals_min_sim_pm", -1, kPropDef, w, false, text, sizeof(text)) == ACCEPTED && w[PR_MIN_SIM_PM] == 500 &&
          w[PR_TAU] == bits_of(0.5f), "proposals_min_sim_pm -1");
    // a refused per-mille value derives nothing
    int32_t before[kMaxWords];
    scramble(w); scramble(before);
    CHECK(apply_appearance("appearance_gate_pm", 1001, kAppearDef, w, false, text, sizeof(text)) == REFUSED && same(w, before), "gate 1001");
}

static void style() {
    int32_t w[kMaxWords], before[kMaxWords];
    char text[256];
    const struct { int th, size, scale; bool ok; } cases[] = {
        {1, 1, 1, true}, {16, 64, 4, true}, {2, 9, 1, true}, {0, 9, 1, false}, {17, 9, 1, false}, {2, 0, 1, false}, {2, 65, 1, false},
        {2, 9, 0, false}, {2, 9, 5, false}, {2, 9, 4 + 256, false},
    };
    for (const auto& c : cases) {
        const int value = c.th | c.size << 8 | c.scale << 16;
        scramble(w); scramble(before);
        const Answer a = apply_overlay("result_overlay_style", value, kOverlayDef, w, false, text, sizeof(text));
        if (c.ok) {
            before[OV_THICKNESS] = c.th; before[OV_SIZE] = c.size; before[OV_SCALE] = c.scale;
            CHECK(a == ACCEPTED && same(w, before), "style %d/%d/%d", c.th, c.size, c.scale);
        } else {
            char want[256];
            snprintf(want, sizeof(want), "result_overlay_style: thickness %d (1..16), size %d (1..64), scale %d (1..4)", c.th, c.size, c.scale);
            CHECK(a == REFUSED && same(w, before) && std::string(text) == want, "style %d/%d/%d says '%s'", c.th, c.size, c.scale, text);
        }
    }
    scramble(w); scramble(before);
    CHECK(apply_overlay("result_overlay_style", 0, kOverlayDef, w, false, text, sizeof(text)) == REFUSED &&
          std::string(text) == "result_overlay_style: thickness 0 (1..16), size 0 (1..64), scale 0 (1..4)", "style 0 says '%s'", text);
    for (int value : {-1, -2, -0x7fffffff - 1}) {      // a negative value restores all three, and only them
        scramble(w); scramble(before);
        before[OV_THICKNESS] = 3; before[OV_SIZE] = 15; before[OV_SCALE] = 2;
        CHECK(apply_overlay("result_overlay_style", value, kOverlayDef, w, false, text, sizeof(text)) == ACCEPTED && same(w, before), "style %d", value);
    }
}

static void frozen_max_cells() {
    int32_t w[kMaxWords], before[kMaxWords];
    char text[256];
    for (int value : {-1, 16384, 65536, 4194305}) {     // whatever the value, once the engine is capable; the text names the frozen size
        memcpy(w, kPropDef, sizeof(w)); memcpy(before, kPropDef, sizeof(before));
        CHECK(apply_proposals("proposals_max_cells", value, kPropDef, w, true, text, sizeof(text)) == REFUSED && same(w, before) &&
              std::string(text) == "proposals_max_cells: fixed by the first enable of \"proposals\" (262144)", "max_cells %d says '%s'", value, text);
    }
    memcpy(w, kPropDef, sizeof(w));
    CHECK(apply_proposals("proposals_max_cells", 65536, kPropDef, w, false, text, sizeof(text)) == ACCEPTED && w[PR_MAX_CELLS] == 65536, "max_cells before the enable");
    CHECK(apply_proposals("proposals_max_cells", 1, kPropDef, w, true, text, sizeof(text)) == REFUSED &&
          std::string(text) == "proposals_max_cells: fixed by the first enable of \"proposals\" (65536)", "says '%s'", text);
    CHECK(apply_proposals("proposals_period", 7, kPropDef, w, true, text, sizeof(text)) == ACCEPTED && w[PR_PERIOD] == 7, "the other keys stay open");
}

int main() {
    table("result overlay", kOverlayKeys, kOverlayWant, apply_overlay, kOverlayDef, "result_overlay_colour");
    table("motion prior", kMotionKeys, kMotionWant, apply_motion, kMotionDef, "motion_blur");
    table("appearance check", kAppearKeys, kAppearWant, apply_appearance, kAppearDef, "appearance_gate");
    table("reacquire proposals", kPropKeys, kPropWant, apply_proposals, kPropDef, "proposals_min_sim");
    derived();
    style();
    frozen_max_cells();
    hook_words("motion prior", kMotionKeys, apply_motion, kMotionDef, -1, -1);
    hook_words("stream conflicts", kConflictKeys, apply_conflicts, kConflictDef, CF_IOU_PM, CF_TAU);
    hook_words("camera motion", kCameraKeys, apply_camera_motion, kCameraDef, -1, -1);
    hook_words("frame health", kHealthKeys, apply_health, kHealthDef, -1, -1);
    hook_words("peak arbitration", kArbKeys, apply_arbitrate, kArbDef, -1, -1);
    hook_cells();
    int32_t w[kMaxWords];
    char text[256];
    CHECK(apply_appearance("appearance_anchor", 0, kAppearDef, w, true, text, sizeof(text)) == UNKNOWN, "the anchor action is no field of the table");
    printf("%d checks failed\n", failures);
    return failures;
}
