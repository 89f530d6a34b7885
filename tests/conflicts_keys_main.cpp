// The key table of the stream conflicts (csrc/vt_feature_keys.hpp: kConflictKeys, apply_conflicts) and the decoding of the
// "conflicts_scene" action (decode_scene) on the CPU: tests/test_conflicts_keys_host.py compiles this with
// -fsanitize=address,undefined and runs it. Prints one line per failed check; the exit status is their number (0: all hold).
// The refusal texts are written out here.
#include <cstdio>
#include <string>

#include "vt_feature_keys.hpp"

using namespace vtkeys;

static int failures = 0;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) { ++failures; printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

static int32_t bits(float f) { int32_t u; memcpy(&u, &f, 4); return u; }
// the default policy as words (VT_CONFLICT_DEFAULT_POLICY of the engine's headers): off, 300 per mille, no gate, tau
static const int32_t kDef[8] = {0, 300, 0, bits(300.0f / 1000.0f), 0, 0, 0, 0};

struct Want { const char* key; int word; int32_t lo, hi; const char* below; const char* above; };
static const Want kWant[] = {
    {"conflicts", 0, 0, 1, nullptr, "conflicts: 2 (0: off, 1: on)"},
    {"conflicts_iou_pm", 1, 1, 1000, "conflicts_iou_pm: 0 (1..1000)", "conflicts_iou_pm: 1001 (1..1000)"},
    {"conflicts_gate", 2, 0, 1, nullptr, "conflicts_gate: 2 (0: report only, 1: refresh rule 9)"},
};

static void scramble(int32_t* w) { for (int i = 0; i < kMaxWords; ++i) w[i] = 0x5A5A0000 + i; }
static bool same(const int32_t* a, const int32_t* b) { return memcmp(a, b, sizeof(int32_t) * kMaxWords) == 0; }

static void table() {
    const int N = (int)(sizeof(kConflictKeys) / sizeof(kConflictKeys[0])), M = (int)(sizeof(kWant) / sizeof(kWant[0]));
    CHECK(N == M, "%d rows, %d written out here", N, M);
    CHECK(CF_ON == 0 && CF_IOU_PM == 1 && CF_GATE == 2 && CF_TAU == 3 && CF_WORDS == 8 && CF_WORDS <= kMaxWords, "the words");
    CHECK(kDef[CF_TAU] == bits(0.3f), "the default tau is 300 / 1000 in binary32");
    int32_t w[kMaxWords], before[kMaxWords];
    char text[256];
    for (int i = 0; i < N && i < M; ++i) {
        const Key& k = kConflictKeys[i];
        const Want& x = kWant[i];
        CHECK(std::string(k.key) == x.key && k.word == x.word && k.lo == x.lo && k.hi == x.hi, "row %d: %s word %d %d..%d", i, k.key, k.word, (int)k.lo, (int)k.hi);
        CHECK(kDef[k.word] >= k.lo && kDef[k.word] <= k.hi, "%s: the default %d is not a legal value", k.key, (int)kDef[k.word]);
        const struct { int value; int32_t lands; } ok[] = {{-1, kDef[k.word]}, {-7, kDef[k.word]}, {k.lo, k.lo}, {k.hi, k.hi}};
        for (const auto& c : ok) {
            scramble(w); scramble(before);
            CHECK(apply_conflicts(k.key, c.value, kDef, w, false, text, sizeof(text)) == ACCEPTED, "%s %d not accepted", k.key, c.value);
            before[k.word] = c.lands;
            if (k.word == CF_IOU_PM) before[CF_TAU] = bits((float)c.lands / 1000.0f);      // the one key that writes two words
            CHECK(same(w, before), "%s %d wrote %d, or another word", k.key, c.value, (int)w[k.word]);
        }
        const struct { int value; const char* text; } bad[] = {{k.lo - 1, x.below}, {k.hi + 1, x.above}};
        for (const auto& c : bad) {
            if (!c.text) { CHECK(c.value == -1, "%s: no text for %d", k.key, c.value); continue; }
            for (bool capable : {false, true}) {
                scramble(w); scramble(before);
                text[0] = 0;
                CHECK(apply_conflicts(k.key, c.value, kDef, w, capable, text, sizeof(text)) == REFUSED, "%s %d not refused", k.key, c.value);
                CHECK(same(w, before), "%s %d: a refusal changed the words", k.key, c.value);
                CHECK(std::string(text) == c.text, "%s %d says '%s', not '%s'", k.key, c.value, text, c.text);
            }
        }
    }
    // "conflicts_scene" is the action: no field of the table
    for (const char* unknown : {"conflicts_scene", "conflicts_iou", "conflict", "conflicts_", ""}) {
        scramble(w); scramble(before);
        CHECK(apply_conflicts(unknown, 1, kDef, w, false, text, sizeof(text)) == UNKNOWN && same(w, before), "'%s' is not unknown", unknown);
        CHECK(apply_conflicts(unknown, 1, kDef, w, true, text, sizeof(text)) == UNKNOWN && same(w, before), "'%s' is not unknown (capable)", unknown);
    }
}

static void tau() {
    int32_t w[kMaxWords];
    char text[256];
    for (int pm = 1; pm <= 1000; ++pm) {
        scramble(w);
        CHECK(apply_conflicts("conflicts_iou_pm", pm, kDef, w, true, text, sizeof(text)) == ACCEPTED && w[CF_IOU_PM] == pm &&
              w[CF_TAU] == bits((float)pm / 1000.0f), "pm %d", pm);
    }
    CHECK(bits(tau_of(500)) == bits(0.5f) && bits(tau_of(1000)) == bits(1.0f), "exact values");
}

static void scene(int value, int B, Answer want, int first, int last, int32_t sc, const char* says) {
    int f = -77, l = -77;
    int32_t s = -77;
    char text[256] = "untouched";
    const Answer a = decode_scene(value, B, &f, &l, &s, text, sizeof(text));
    CHECK(a == want, "scene value 0x%x of %d streams: answer %d", (unsigned)value, B, (int)a);
    if (want == ACCEPTED) {
        CHECK(f == first && l == last && s == sc, "scene value 0x%x of %d: streams [%d, %d) to scene %d", (unsigned)value, B, f, l, (int)s);
        CHECK(std::string(text) == "untouched", "an accepted value wrote a text");
    } else {
        CHECK(f == -77 && l == -77 && s == -77, "a refusal wrote its outputs");
        CHECK(std::string(text) == says, "scene value %d says '%s', not '%s'", value, text, says);
    }
}

static void scenes() {
    scene(0, 4, ACCEPTED, 0, 1, 0, nullptr);                        // stream 0 back to scene 0
    scene(3 | 7 << 16, 4, ACCEPTED, 3, 4, 7, nullptr);
    scene(0 | 32767 << 16, 1, ACCEPTED, 0, 1, 32767, nullptr);      // the largest scene a non-negative int32 packs
    scene(0x7FFFFFFF, 1024, ACCEPTED, 0, 1024, 32767, nullptr);     // ... with every stream
    scene(0xFFFF | 5 << 16, 4, ACCEPTED, 0, 4, 5, nullptr);         // 0xFFFF: every stream
    scene(0xFFFF, 1, ACCEPTED, 0, 1, 0, nullptr);
    scene(1023 | 1 << 16, 1024, ACCEPTED, 1023, 1024, 1, nullptr);
    scene(-1, 4, ACCEPTED, 0, 4, 0, nullptr);                       // every stream back to scene 0
    scene(-1, 1024, ACCEPTED, 0, 1024, 0, nullptr);
    scene(4 | 2 << 16, 4, REFUSED, 0, 0, 0, "conflicts_scene: stream 4 (0..3, 0xFFFF: all) of scene 2");
    scene(0xFFFE, 1024, REFUSED, 0, 0, 0, "conflicts_scene: stream 65534 (0..1023, 0xFFFF: all) of scene 0");
    scene(1, 1, REFUSED, 0, 0, 0, "conflicts_scene: stream 1 (0..0, 0xFFFF: all) of scene 0");
    scene(-2, 4, REFUSED, 0, 0, 0, "conflicts_scene: -2 (stream | scene << 16, stream 0xFFFF: all; -1: every stream to scene 0)");
    scene(-0x7fffffff - 1, 4, REFUSED, 0, 0, 0,
          "conflicts_scene: -2147483648 (stream | scene << 16, stream 0xFFFF: all; -1: every stream to scene 0)");
}

int main() {
    table();
    tau();
    scenes();
    printf("%d checks failed\n", failures);
    return failures;
}
