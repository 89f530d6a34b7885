// The key table of the peak arbitration (csrc/vt_feature_keys.hpp: kArbKeys, apply_arbitrate) on the CPU:
// tests/test_arbitrate_keys_host.py compiles this with -fsanitize=address,undefined and runs it. Prints one line per
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

// the default policy as words (VT_ARB_DEFAULT_POLICY of the engine's headers)
static const int32_t kArbDef[8] = {0, 3, 2, 50, 300, 500, 0, 0};

struct Want { const char* key; int word; int32_t lo, hi; const char* below; const char* above; };
static const Want kWant[] = {
    {"arbitrate", 0, 0, 1, nullptr, "arbitrate: 2 (0: off, 1: on)"},
    {"arbitrate_max", 1, 2, 4, "arbitrate_max: 1 (2..4)", "arbitrate_max: 5 (2..4)"},
    {"arbitrate_radius", 2, 1, 4, "arbitrate_radius: 0 (1..4)", "arbitrate_radius: 5 (1..4)"},
    {"arbitrate_min_resp_pm", 3, 0, 1000, nullptr, "arbitrate_min_resp_pm: 1001 (0..1000)"},
    {"arbitrate_low_pm", 4, 0, 1000, nullptr, "arbitrate_low_pm: 1001 (0..1000)"},
    {"arbitrate_high_pm", 5, 0, 1000, nullptr, "arbitrate_high_pm: 1001 (0..1000)"},
};

static void scramble(int32_t* w) { for (int i = 0; i < kMaxWords; ++i) w[i] = 0x5A5A0000 + i; }
static bool same(const int32_t* a, const int32_t* b) { return memcmp(a, b, sizeof(int32_t) * kMaxWords) == 0; }

static void table() {
    const int N = (int)(sizeof(kArbKeys) / sizeof(kArbKeys[0])), M = (int)(sizeof(kWant) / sizeof(kWant[0]));
    CHECK(N == M && N == 6, "%d rows, %d written out here", N, M);
    CHECK(AR_ON == 0 && AR_MAX == 1 && AR_RADIUS == 2 && AR_MIN_RESP_PM == 3 && AR_LOW_PM == 4 && AR_HIGH_PM == 5 && AR_WORDS == 8 &&
          AR_WORDS == kMaxWords, "the words: six keys and two reserved, kMaxWords stays 8");
    int32_t w[kMaxWords], before[kMaxWords];
    char text[256];
    for (int i = 0; i < N && i < M; ++i) {
        const Key& k = kArbKeys[i];
        const Want& x = kWant[i];
        CHECK(std::string(k.key) == x.key && k.word == x.word && k.lo == x.lo && k.hi == x.hi, "row %d: %s word %d %d..%d", i, k.key, k.word, (int)k.lo, (int)k.hi);
        CHECK(kArbDef[k.word] >= k.lo && kArbDef[k.word] <= k.hi, "%s: the default %d is not a legal value", k.key, (int)kArbDef[k.word]);
        const struct { int value; int32_t lands; } ok[] = {{-1, kArbDef[k.word]}, {-7, kArbDef[k.word]}, {-0x7fffffff - 1, kArbDef[k.word]},
                                                          {k.lo, k.lo}, {k.hi, k.hi}};
        for (const auto& c : ok) {
            for (bool capable : {false, true}) {
                scramble(w); scramble(before);
                CHECK(apply_arbitrate(k.key, c.value, kArbDef, w, capable, text, sizeof(text)) == ACCEPTED, "%s %d not accepted", k.key, c.value);
                before[k.word] = c.lands;
                CHECK(same(w, before), "%s %d wrote %d, or another word", k.key, c.value, (int)w[k.word]);
            }
        }
        const struct { int value; const char* text; } bad[] = {{k.lo - 1, x.below}, {k.hi + 1, x.above}, {0x7fffffff, ""}};
        for (const auto& c : bad) {
            if (!c.text) { CHECK(c.value == -1, "%s: no text for %d", k.key, c.value); continue; }
            scramble(w); scramble(before);
            text[0] = 0;
            CHECK(apply_arbitrate(k.key, c.value, kArbDef, w, false, text, sizeof(text)) == REFUSED, "%s %d not refused", k.key, c.value);
            CHECK(same(w, before), "%s %d: a refusal changed the words", k.key, c.value);
            if (c.text[0]) CHECK(std::string(text) == c.text, "%s %d says '%s', not '%s'", k.key, c.value, text, c.text);
            else CHECK(std::string(text).rfind(std::string(k.key) + ": 2147483647 (", 0) == 0, "%s INT_MAX says '%s'", k.key, text);
        }
    }
    for (const char* unknown : {"arbitrate_gain", "arbitrat", "arbitrate_", "arbitrate_low", "arbitrate_tau", "response_peaks", ""}) {
        scramble(w); scramble(before);
        CHECK(apply_arbitrate(unknown, 1, kArbDef, w, false, text, sizeof(text)) == UNKNOWN && same(w, before), "'%s' is not unknown", unknown);
        CHECK(apply_arbitrate(unknown, 1, kArbDef, w, true, text, sizeof(text)) == UNKNOWN && same(w, before), "'%s' is not unknown (capable)", unknown);
    }
}

// the thresholds the kernels form: one binary32 divide, the text of tau_of; no derived word is stored by any key
static void thresholds() {
    CHECK(tau_of(300) == 300.0f / 1000.0f && tau_of(500) == 0.5f && tau_of(0) == 0.0f && tau_of(1000) == 1.0f && tau_of(50) == 50.0f / 1000.0f, "tau_of");
    int32_t w[kMaxWords], before[kMaxWords];
    char text[256];
    for (const Key& k : kArbKeys) {
        memcpy(w, kArbDef, sizeof(w)); memcpy(before, kArbDef, sizeof(before));
        CHECK(apply_arbitrate(k.key, k.hi, kArbDef, w, true, text, sizeof(text)) == ACCEPTED, "%s", k.key);
        before[k.word] = k.hi;
        CHECK(same(w, before) && w[6] == 0 && w[7] == 0, "%s wrote a second word", k.key);
    }
}

int main() {
    table();
    thresholds();
    printf("%d checks failed\n", failures);
    return failures;
}
