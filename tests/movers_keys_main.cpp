// The key table of the moving regions (csrc/vt_feature_keys.hpp: kMoverKeys, apply_movers, and the bit-field keys it
// brought: Key::get / Key::put, check_words) on the CPU: tests/test_movers_cases.py compiles this with
// -fsanitize=address,undefined and runs it. Prints one line per failed check; the exit status is their number (0: all
// hold). The refusal texts are written out here.
#include <cstdio>
#include <string>

#include "vt_feature_keys.hpp"

using namespace vtkeys;

static int failures = 0;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) { ++failures; printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

// the default policy as words (VT_MOVER_DEFAULT_POLICY of the engine's headers): shape = learn 4 | min_nb 3 << 4 | max 4 << 8
static const int32_t kShapeDef = 4 | 3 << 4 | 4 << 8;
static const int32_t kMoverDef[8] = {0, 1, 0, 96, 4, 400, kShapeDef, 65536};

struct Want { const char* key; int word, shift, bits; int32_t lo, hi, def; const char* below; const char* above; };
static const Want kWant[] = {
    {"movers", 0, 0, 0, 0, 1, 0, nullptr, "movers: 2 (0: off, 1: on)"},
    {"movers_period", 1, 0, 0, 1, 1000000, 1, "movers_period: 0 (1..1000000)", "movers_period: 1000001 (1..1000000)"},
    {"movers_cell", 2, 0, 0, 0, 32, 0, nullptr, "movers_cell: 33 (0: automatic, 4, 8, 16 or 32)"},
    {"movers_thr", 3, 0, 0, 0, 4080, 96, nullptr, "movers_thr: 4081 (0..4080)"},
    {"movers_min_area", 4, 0, 0, 1, 262144, 4, "movers_min_area: 0 (1..262144)", "movers_min_area: 262145 (1..262144)"},
    {"movers_global_pm", 5, 0, 0, 0, 1000, 400, nullptr, "movers_global_pm: 1001 (0..1000, 1000: never)"},
    {"movers_learn", 6, 0, 4, 0, 8, 4, nullptr, "movers_learn: 9 (0..8)"},
    {"movers_min_nb", 6, 4, 4, 1, 9, 3, "movers_min_nb: 0 (1..9)", "movers_min_nb: 10 (1..9)"},
    {"movers_max", 6, 8, 4, 1, 8, 4, "movers_max: 0 (1..8)", "movers_max: 9 (1..8)"},
    {"movers_max_cells", 7, 0, 0, 4096, 262144, 65536, "movers_max_cells: 4095 (4096..262144)", "movers_max_cells: 262145 (4096..262144)"},
};

// a legal start: the scrambled words of the other tests would put illegal values into the fields beside the one written
static void start(int32_t* w) { for (int i = 0; i < kMaxWords; ++i) w[i] = 0x5A5A0000 + i; w[MV_SHAPE] = 2 | 5 << 4 | 7 << 8 | 0x5A5A << 12; }
static bool same(const int32_t* a, const int32_t* b) { return memcmp(a, b, sizeof(int32_t) * kMaxWords) == 0; }
static int32_t field(const Want& x, int32_t w) { return x.bits ? (int32_t)(((uint32_t)w >> x.shift) & ((1u << x.bits) - 1u)) : w; }
static int32_t with(const Want& x, int32_t w, int32_t v) {
    if (!x.bits) return v;
    const uint32_t m = ((1u << x.bits) - 1u) << x.shift;
    return (int32_t)(((uint32_t)w & ~m) | ((uint32_t)v << x.shift));
}

static void table() {
    const int N = (int)(sizeof(kMoverKeys) / sizeof(kMoverKeys[0])), M = (int)(sizeof(kWant) / sizeof(kWant[0]));
    CHECK(N == M, "%d rows, %d written out here", N, M);
    CHECK(MV_ON == 0 && MV_PERIOD == 1 && MV_CELL == 2 && MV_THR == 3 && MV_MIN_AREA == 4 && MV_GLOBAL_PM == 5 && MV_SHAPE == 6 &&
          MV_MAX_CELLS == 7 && MV_WORDS == 8 && MV_WORDS <= kMaxWords && kMaxWords == 8, "the words: ten keys in eight");
    int32_t w[kMaxWords], before[kMaxWords];
    char text[256];
    for (int i = 0; i < N && i < M; ++i) {
        const Key& k = kMoverKeys[i];
        const Want& x = kWant[i];
        CHECK(std::string(k.key) == x.key && k.word == x.word && k.lo == x.lo && k.hi == x.hi && k.shift == x.shift && k.bits == x.bits,
              "row %d: %s word %d %d..%d at %d, %d bits", i, k.key, k.word, (int)k.lo, (int)k.hi, k.shift, k.bits);
        CHECK(field(x, kMoverDef[k.word]) == x.def && x.def >= k.lo && x.def <= k.hi, "%s: the default %d", k.key, (int)field(x, kMoverDef[k.word]));
        CHECK(!k.bits || k.hi < (1 << k.bits), "%s: %d does not fit %d bits", k.key, (int)k.hi, k.bits);
        const struct { int value; int32_t lands; } ok[] = {{-1, x.def}, {-7, x.def}, {k.lo, k.lo}, {k.hi, k.hi}};
        for (const auto& c : ok) {
            if (std::string(k.key) == "movers_cell" && c.value > 0 && (c.value & (c.value - 1))) continue;
            start(w); start(before);
            CHECK(apply_movers(k.key, c.value, kMoverDef, w, false, text, sizeof(text)) == ACCEPTED, "%s %d not accepted", k.key, c.value);
            before[k.word] = with(x, before[k.word], c.lands);
            CHECK(same(w, before), "%s %d wrote %d, or another word or field", k.key, c.value, (int)w[k.word]);
            CHECK(k.get(w[k.word]) == c.lands && k.put(before[k.word], c.lands) == before[k.word], "%s: get / put", k.key);
        }
        const struct { int value; const char* text; } bad[] = {{k.lo - 1, x.below}, {k.hi + 1, x.above}};
        for (const auto& c : bad) {
            if (!c.text) { CHECK(c.value == -1, "%s: no text for %d", k.key, c.value); continue; }
            start(w); start(before);
            text[0] = 0;
            CHECK(apply_movers(k.key, c.value, kMoverDef, w, false, text, sizeof(text)) == REFUSED, "%s %d not refused", k.key, c.value);
            CHECK(same(w, before), "%s %d: a refusal changed the words", k.key, c.value);
            CHECK(std::string(text) == c.text, "%s %d says '%s', not '%s'", k.key, c.value, text, c.text);
        }
    }
    for (const char* unknown : {"movers_gain", "mover", "movers_", "motion_prior", "health_cell", "movers_shape", ""}) {
        start(w); start(before);
        CHECK(apply_movers(unknown, 1, kMoverDef, w, false, text, sizeof(text)) == UNKNOWN && same(w, before), "'%s' is not unknown", unknown);
        CHECK(apply_movers(unknown, 1, kMoverDef, w, true, text, sizeof(text)) == UNKNOWN && same(w, before), "'%s' is not unknown (capable)", unknown);
    }
}

// the three fields of one word, every combination: each key moves its own four bits and nothing else
static void fields() {
    char text[256];
    int32_t w[kMaxWords];
    for (int learn = 0; learn <= 8; ++learn)
        for (int nb = 1; nb <= 9; ++nb)
            for (int mx = 1; mx <= 8; ++mx) {
                memcpy(w, kMoverDef, sizeof(w));
                const bool ok = apply_movers("movers_max", mx, kMoverDef, w, true, text, sizeof(text)) == ACCEPTED &&
                                apply_movers("movers_learn", learn, kMoverDef, w, true, text, sizeof(text)) == ACCEPTED &&
                                apply_movers("movers_min_nb", nb, kMoverDef, w, true, text, sizeof(text)) == ACCEPTED;
                CHECK(ok && w[MV_SHAPE] == (learn | nb << 4 | mx << 8), "learn %d min_nb %d max %d -> 0x%x", learn, nb, mx, (unsigned)w[MV_SHAPE]);
                for (int i = 0; i < kMaxWords; ++i)
                    if (i != MV_SHAPE) CHECK(w[i] == kMoverDef[i], "word %d moved", i);
            }
}

static void cells() {
    int32_t w[kMaxWords], before[kMaxWords];
    char text[256];
    for (int value : {0, 4, 8, 16, 32})
        for (bool capable : {false, true}) {
            start(w); start(before);
            before[MV_CELL] = value;
            CHECK(apply_movers("movers_cell", value, kMoverDef, w, capable, text, sizeof(text)) == ACCEPTED && same(w, before), "cell %d", value);
        }
    for (int value : {1, 2, 3, 5, 6, 7, 12, 24, 31, 33, 64, 128, 1 << 30}) {
        start(w); start(before);
        char want[256];
        snprintf(want, sizeof(want), "movers_cell: %d (0: automatic, 4, 8, 16 or 32)", value);
        text[0] = 0;
        CHECK(apply_movers("movers_cell", value, kMoverDef, w, false, text, sizeof(text)) == REFUSED && same(w, before) &&
              std::string(text) == want, "cell %d says '%s'", value, text);
    }
    start(w);
    CHECK(apply_movers("movers_cell", -0x7fffffff - 1, kMoverDef, w, true, text, sizeof(text)) == ACCEPTED && w[MV_CELL] == 0, "cell INT_MIN");
}

static void frozen_max_cells() {
    int32_t w[kMaxWords], before[kMaxWords];
    char text[256];
    for (int value : {-1, 4096, 65536, 262145}) {      // whatever the value, once the engine is capable; the text names the frozen size
        memcpy(w, kMoverDef, sizeof(w)); memcpy(before, kMoverDef, sizeof(before));
        CHECK(apply_movers("movers_max_cells", value, kMoverDef, w, true, text, sizeof(text)) == REFUSED && same(w, before) &&
              std::string(text) == "movers_max_cells: fixed by the first enable of \"movers\" (65536)", "max_cells %d says '%s'", value, text);
    }
    memcpy(w, kMoverDef, sizeof(w));
    CHECK(apply_movers("movers_max_cells", 16384, kMoverDef, w, false, text, sizeof(text)) == ACCEPTED && w[MV_MAX_CELLS] == 16384, "max_cells before the enable");
    for (const Key& k : kMoverKeys)         // the other keys stay open
        if (k.word != MV_MAX_CELLS)
            CHECK(apply_movers(k.key, k.hi, kMoverDef, w, true, text, sizeof(text)) == ACCEPTED && k.get(w[k.word]) == k.hi, "%s on a capable engine", k.key);
}

// an operator hook's eight words through the table: the fields are checked one by one, and a bit beside them is refused
static void hook_words() {
    int32_t pol[kMaxWords], w[kMaxWords];
    memcpy(pol, kMoverDef, sizeof(pol));
    pol[MV_ON] = 1; pol[MV_SHAPE] = 0 | 9 << 4 | 8 << 8;
    memset(w, 0, sizeof(w));
    CHECK(check_words(kMoverKeys, apply_movers, kMoverDef, pol, w) == -1 && same(w, pol), "a legal policy");
    const struct { int word; int32_t value; int row; } bad[] = {
        {MV_ON, 2, 0}, {MV_PERIOD, 0, 1}, {MV_CELL, 12, 2}, {MV_THR, 4081, 3}, {MV_MIN_AREA, 0, 4}, {MV_GLOBAL_PM, 1001, 5},
        {MV_SHAPE, 9 | 3 << 4 | 4 << 8, 6}, {MV_SHAPE, 4 | 0 << 4 | 4 << 8, 7}, {MV_SHAPE, 4 | 10 << 4 | 4 << 8, 7}, {MV_SHAPE, 4 | 3 << 4 | 0 << 8, 8},
        {MV_SHAPE, 4 | 3 << 4 | 9 << 8, 8}, {MV_SHAPE, -1, 6}, {MV_MAX_CELLS, 4095, 9}, {MV_THR, -1, 3},
    };
    for (const auto& c : bad) {
        memcpy(pol, kMoverDef, sizeof(pol));
        pol[c.word] = c.value;
        CHECK(check_words(kMoverKeys, apply_movers, kMoverDef, pol, w) == c.row, "word %d = %d: row %d", c.word, (int)c.value,
              check_words(kMoverKeys, apply_movers, kMoverDef, pol, w));
    }
    for (int bit : {12, 13, 20, 30}) {         // a bit beside the three fields: refused at the word's first row
        memcpy(pol, kMoverDef, sizeof(pol));
        pol[MV_SHAPE] |= 1 << bit;
        CHECK(check_words(kMoverKeys, apply_movers, kMoverDef, pol, w) == 6, "bit %d of the shape word: row %d", bit,
              check_words(kMoverKeys, apply_movers, kMoverDef, pol, w));
    }
    // the whole-word keys of the other tables go through get / put untouched
    CHECK(kHealthKeys[HL_FLAT_Q].get(0x12345678) == 0x12345678 && kHealthKeys[HL_FLAT_Q].put(7, -3) == -3, "a whole-word key");
}

int main() {
    table();
    fields();
    cells();
    frozen_max_cells();
    hook_words();
    printf("%d checks failed\n", failures);
    return failures;
}
