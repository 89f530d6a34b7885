// The key table of the frame health (csrc/vt_feature_keys.hpp: kHealthKeys, apply_health) on the CPU:
// tests/test_frame_health_keys_host.py compiles this with -fsanitize=address,undefined and runs it. Prints one line per
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

// the default policy as words (VT_HEALTH_DEFAULT_POLICY of the engine's headers)
static const int32_t kHealthDef[8] = {0, 1, 0, 3, 32, 500, 0, 65536};

struct Want { const char* key; int word; int32_t lo, hi; const char* below; const char* above; };
static const Want kWant[] = {
    {"health", 0, 0, 1, nullptr, "health: 2 (0: off, 1: on)"},
    {"health_period", 1, 1, 1000000, "health_period: 0 (1..1000000)", "health_period: 1000001 (1..1000000)"},
    {"health_cell", 2, 0, 32, nullptr, "health_cell: 33 (0: automatic, 4, 8, 16 or 32)"},
    {"health_still_run", 3, 1, 1000, "health_still_run: 0 (1..1000)", "health_still_run: 1001 (1..1000)"},
    {"health_flat_q", 4, 0, 4080, nullptr, "health_flat_q: 4081 (0..4080)"},
    {"health_cut_pm", 5, 0, 1000, nullptr, "health_cut_pm: 1001 (0..1000, 0: never)"},
    {"health_gate", 6, 0, 1, nullptr, "health_gate: 2 (0: report only, 1: refresh rule 10)"},
    {"health_max_cells", 7, 4096, 262144, "health_max_cells: 4095 (4096..262144)", "health_max_cells: 262145 (4096..262144)"},
};

static void scramble(int32_t* w) { for (int i = 0; i < kMaxWords; ++i) w[i] = 0x5A5A0000 + i; }
static bool same(const int32_t* a, const int32_t* b) { return memcmp(a, b, sizeof(int32_t) * kMaxWords) == 0; }

static void table() {
    const int N = (int)(sizeof(kHealthKeys) / sizeof(kHealthKeys[0])), M = (int)(sizeof(kWant) / sizeof(kWant[0]));
    CHECK(N == M, "%d rows, %d written out here", N, M);
    CHECK(HL_ON == 0 && HL_PERIOD == 1 && HL_CELL == 2 && HL_STILL_RUN == 3 && HL_FLAT_Q == 4 && HL_CUT_PM == 5 && HL_GATE == 6 && HL_MAX_CELLS == 7 &&
          HL_WORDS == 8 && HL_WORDS <= kMaxWords, "the words");
    int32_t w[kMaxWords], before[kMaxWords];
    char text[256];
    for (int i = 0; i < N && i < M; ++i) {
        const Key& k = kHealthKeys[i];
        const Want& x = kWant[i];
        CHECK(std::string(k.key) == x.key && k.word == x.word && k.lo == x.lo && k.hi == x.hi, "row %d: %s word %d %d..%d", i, k.key, k.word, (int)k.lo, (int)k.hi);
        CHECK(kHealthDef[k.word] >= k.lo && kHealthDef[k.word] <= k.hi, "%s: the default %d is not a legal value", k.key, (int)kHealthDef[k.word]);
        const struct { int value; int32_t lands; } ok[] = {{-1, kHealthDef[k.word]}, {-7, kHealthDef[k.word]}, {k.lo, k.lo}, {k.hi, k.hi}};
        for (const auto& c : ok) {
            scramble(w); scramble(before);
            CHECK(apply_health(k.key, c.value, kHealthDef, w, false, text, sizeof(text)) == ACCEPTED, "%s %d not accepted", k.key, c.value);
            before[k.word] = c.lands;
            CHECK(same(w, before), "%s %d wrote %d, or another word", k.key, c.value, (int)w[k.word]);
        }
        const struct { int value; const char* text; } bad[] = {{k.lo - 1, x.below}, {k.hi + 1, x.above}};
        for (const auto& c : bad) {
            if (!c.text) { CHECK(c.value == -1, "%s: no text for %d", k.key, c.value); continue; }
            scramble(w); scramble(before);
            text[0] = 0;
            CHECK(apply_health(k.key, c.value, kHealthDef, w, false, text, sizeof(text)) == REFUSED, "%s %d not refused", k.key, c.value);
            CHECK(same(w, before), "%s %d: a refusal changed the words", k.key, c.value);
            CHECK(std::string(text) == c.text, "%s %d says '%s', not '%s'", k.key, c.value, text, c.text);
        }
    }
    for (const char* unknown : {"health_gain", "healt", "health_", "camera_motion_cell", "conflicts_gate", ""}) {
        scramble(w); scramble(before);
        CHECK(apply_health(unknown, 1, kHealthDef, w, false, text, sizeof(text)) == UNKNOWN && same(w, before), "'%s' is not unknown", unknown);
        CHECK(apply_health(unknown, 1, kHealthDef, w, true, text, sizeof(text)) == UNKNOWN && same(w, before), "'%s' is not unknown (capable)", unknown);
    }
}

static void cells() {
    int32_t w[kMaxWords], before[kMaxWords];
    char text[256];
    for (int value : {0, 4, 8, 16, 32}) {
        for (bool capable : {false, true}) {
            scramble(w); scramble(before);
            before[HL_CELL] = value;
            CHECK(apply_health("health_cell", value, kHealthDef, w, capable, text, sizeof(text)) == ACCEPTED && same(w, before), "cell %d", value);
        }
    }
    for (int value : {1, 2, 3, 5, 6, 7, 12, 24, 31, 33, 64, 128, 1 << 30}) {
        scramble(w); scramble(before);
        char want[256];
        snprintf(want, sizeof(want), "health_cell: %d (0: automatic, 4, 8, 16 or 32)", value);
        text[0] = 0;
        CHECK(apply_health("health_cell", value, kHealthDef, w, false, text, sizeof(text)) == REFUSED && same(w, before) &&
              std::string(text) == want, "cell %d says '%s'", value, text);
    }
    scramble(w);
    CHECK(apply_health("health_cell", -1, kHealthDef, w, true, text, sizeof(text)) == ACCEPTED && w[HL_CELL] == 0, "cell -1 is automatic");
    CHECK(apply_health("health_cell", -0x7fffffff - 1, kHealthDef, w, true, text, sizeof(text)) == ACCEPTED && w[HL_CELL] == 0, "cell INT_MIN");
}

static void frozen_max_cells() {
    int32_t w[kMaxWords], before[kMaxWords];
    char text[256];
    for (int value : {-1, 4096, 65536, 262145}) {      // whatever the value, once the engine is capable; the text names the frozen size
        memcpy(w, kHealthDef, sizeof(w)); memcpy(before, kHealthDef, sizeof(before));
        CHECK(apply_health("health_max_cells", value, kHealthDef, w, true, text, sizeof(text)) == REFUSED && same(w, before) &&
              std::string(text) == "health_max_cells: fixed by the first enable of \"health\" (65536)", "max_cells %d says '%s'", value, text);
    }
    memcpy(w, kHealthDef, sizeof(w));
    CHECK(apply_health("health_max_cells", 16384, kHealthDef, w, false, text, sizeof(text)) == ACCEPTED && w[HL_MAX_CELLS] == 16384, "max_cells before the enable");
    CHECK(apply_health("health_max_cells", 1, kHealthDef, w, true, text, sizeof(text)) == REFUSED &&
          std::string(text) == "health_max_cells: fixed by the first enable of \"health\" (16384)", "says '%s'", text);
    for (const Key& k : kHealthKeys)        // the other keys stay open
        if (k.word != HL_MAX_CELLS)
            CHECK(apply_health(k.key, k.hi, kHealthDef, w, true, text, sizeof(text)) == ACCEPTED && w[k.word] == k.hi, "%s on a capable engine", k.key);
}

int main() {
    table();
    cells();
    frozen_max_cells();
    printf("%d checks failed\n", failures);
    return failures;
}
