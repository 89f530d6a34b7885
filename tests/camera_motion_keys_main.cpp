// The key table of the camera motion (csrc/vt_feature_keys.hpp: kCameraKeys, apply_camera_motion) on the CPU:
// tests/test_camera_motion_keys_host.py compiles this with -fsanitize=address,undefined and runs it. Prints one line per
// failed check; the exit status is their number (0: all hold). The refusal texts are written out here.
#include <cstdio>
#include <string>

#include "vt_feature_keys.hpp"

using namespace vtkeys;

static int failures = 0;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) { ++failures; printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

// the default policy as words (VT_CAM_DEFAULT_POLICY of the engine's headers)
static const int32_t kCamDef[8] = {0, 0, 8, 800, 65536, 0, 0, 0};

struct Want { const char* key; int word; int32_t lo, hi; const char* below; const char* above; };
static const Want kWant[] = {
    {"camera_motion", 0, 0, 2, nullptr, "camera_motion: 3 (0: off, 1: measure, 2: measure and move the box)"},
    {"camera_motion_cell", 1, 0, 32, nullptr, "camera_motion_cell: 33 (0: automatic, 4, 8, 16 or 32)"},
    {"camera_motion_range", 2, 2, 16, "camera_motion_range: 1 (2..16)", "camera_motion_range: 17 (2..16)"},
    {"camera_motion_conf_pm", 3, 0, 1000, nullptr, "camera_motion_conf_pm: 1001 (0..1000)"},
    {"camera_motion_max_cells", 4, 4096, 1048576, "camera_motion_max_cells: 4095 (4096..1048576)",
     "camera_motion_max_cells: 1048577 (4096..1048576)"},
};

static void scramble(int32_t* w) { for (int i = 0; i < kMaxWords; ++i) w[i] = 0x5A5A0000 + i; }
static bool same(const int32_t* a, const int32_t* b) { return memcmp(a, b, sizeof(int32_t) * kMaxWords) == 0; }

static void table() {
    const int N = (int)(sizeof(kCameraKeys) / sizeof(kCameraKeys[0])), M = (int)(sizeof(kWant) / sizeof(kWant[0]));
    CHECK(N == M, "%d rows, %d written out here", N, M);
    CHECK(CM_MODE == 0 && CM_CELL == 1 && CM_RANGE == 2 && CM_CONF_PM == 3 && CM_MAX_CELLS == 4 && CM_WORDS == 8 && CM_WORDS <= kMaxWords, "the words");
    int32_t w[kMaxWords], before[kMaxWords];
    char text[256];
    for (int i = 0; i < N && i < M; ++i) {
        const Key& k = kCameraKeys[i];
        const Want& x = kWant[i];
        CHECK(std::string(k.key) == x.key && k.word == x.word && k.lo == x.lo && k.hi == x.hi, "row %d: %s word %d %d..%d", i, k.key, k.word, (int)k.lo, (int)k.hi);
        CHECK(kCamDef[k.word] >= k.lo && kCamDef[k.word] <= k.hi, "%s: the default %d is not a legal value", k.key, (int)kCamDef[k.word]);
        const struct { int value; int32_t lands; } ok[] = {{-1, kCamDef[k.word]}, {-7, kCamDef[k.word]}, {k.lo, k.lo}, {k.hi, k.hi}};
        for (const auto& c : ok) {
            scramble(w); scramble(before);
            CHECK(apply_camera_motion(k.key, c.value, kCamDef, w, false, text, sizeof(text)) == ACCEPTED, "%s %d not accepted", k.key, c.value);
            before[k.word] = c.lands;
            CHECK(same(w, before), "%s %d wrote %d, or another word", k.key, c.value, (int)w[k.word]);
        }
        const struct { int value; const char* text; } bad[] = {{k.lo - 1, x.below}, {k.hi + 1, x.above}};
        for (const auto& c : bad) {
            if (!c.text) { CHECK(c.value == -1, "%s: no text for %d", k.key, c.value); continue; }
            scramble(w); scramble(before);
            text[0] = 0;
            CHECK(apply_camera_motion(k.key, c.value, kCamDef, w, false, text, sizeof(text)) == REFUSED, "%s %d not refused", k.key, c.value);
            CHECK(same(w, before), "%s %d: a refusal changed the words", k.key, c.value);
            CHECK(std::string(text) == c.text, "%s %d says '%s', not '%s'", k.key, c.value, text, c.text);
        }
    }
    for (const char* unknown : {"camera_motion_gain", "camera", "camera_motion_", ""}) {
        scramble(w); scramble(before);
        CHECK(apply_camera_motion(unknown, 1, kCamDef, w, false, text, sizeof(text)) == UNKNOWN && same(w, before), "'%s' is not unknown", unknown);
        CHECK(apply_camera_motion(unknown, 1, kCamDef, w, true, text, sizeof(text)) == UNKNOWN && same(w, before), "'%s' is not unknown (capable)", unknown);
    }
}

static void cells() {
    int32_t w[kMaxWords], before[kMaxWords];
    char text[256];
    for (int value : {0, 4, 8, 16, 32}) {
        for (bool capable : {false, true}) {
            scramble(w); scramble(before);
            before[CM_CELL] = value;
            CHECK(apply_camera_motion("camera_motion_cell", value, kCamDef, w, capable, text, sizeof(text)) == ACCEPTED && same(w, before), "cell %d", value);
        }
    }
    for (int value : {1, 2, 3, 5, 6, 7, 12, 24, 31, 33, 64, 128, 1 << 30}) {
        scramble(w); scramble(before);
        char want[256];
        snprintf(want, sizeof(want), "camera_motion_cell: %d (0: automatic, 4, 8, 16 or 32)", value);
        text[0] = 0;
        CHECK(apply_camera_motion("camera_motion_cell", value, kCamDef, w, false, text, sizeof(text)) == REFUSED && same(w, before) &&
              std::string(text) == want, "cell %d says '%s'", value, text);
    }
    scramble(w);
    CHECK(apply_camera_motion("camera_motion_cell", -1, kCamDef, w, true, text, sizeof(text)) == ACCEPTED && w[CM_CELL] == 0, "cell -1 is automatic");
    CHECK(apply_camera_motion("camera_motion_cell", -0x7fffffff - 1, kCamDef, w, true, text, sizeof(text)) == ACCEPTED && w[CM_CELL] == 0, "cell INT_MIN");
}

static void frozen_max_cells() {
    int32_t w[kMaxWords], before[kMaxWords];
    char text[256];
    for (int value : {-1, 4096, 65536, 1048577}) {      // whatever the value, once the engine is capable; the text names the frozen size
        memcpy(w, kCamDef, sizeof(w)); memcpy(before, kCamDef, sizeof(before));
        CHECK(apply_camera_motion("camera_motion_max_cells", value, kCamDef, w, true, text, sizeof(text)) == REFUSED && same(w, before) &&
              std::string(text) == "camera_motion_max_cells: fixed by the first enable of \"camera_motion\" (65536)", "max_cells %d says '%s'", value, text);
    }
    memcpy(w, kCamDef, sizeof(w));
    CHECK(apply_camera_motion("camera_motion_max_cells", 16384, kCamDef, w, false, text, sizeof(text)) == ACCEPTED && w[CM_MAX_CELLS] == 16384, "max_cells before the enable");
    CHECK(apply_camera_motion("camera_motion_max_cells", 1, kCamDef, w, true, text, sizeof(text)) == REFUSED &&
          std::string(text) == "camera_motion_max_cells: fixed by the first enable of \"camera_motion\" (16384)", "says '%s'", text);
    for (const Key& k : kCameraKeys)        // the other keys stay open
        if (k.word != CM_MAX_CELLS)
            CHECK(apply_camera_motion(k.key, k.hi, kCamDef, w, true, text, sizeof(text)) == ACCEPTED && w[k.word] == k.hi, "%s on a capable engine", k.key);
}

int main() {
    table();
    cells();
    frozen_max_cells();
    printf("%d checks failed\n", failures);
    return failures;
}
