// The host arithmetic of the operator hooks (csrc/vt_ops_host.hpp) on the CPU: tests/test_ops_host_helpers.py compiles this
// with -fsanitize=address,undefined and runs it. Prints one line per failed check; the exit status is their number (0: all hold).
#include <cstdio>
#include <vector>

#include "vt_ops_host.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) { ++failures; printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static void rounding() {
    // exact ties go to the even bf16, upwards and downwards, for both signs; one ulp of float32 either side of a tie does not
    const struct { uint32_t in; uint16_t want; } cases[] = {
        {0x3F808000u, 0x3F80}, {0x3F818000u, 0x3F82}, {0xBF808000u, 0xBF80}, {0xBF818000u, 0xBF82},
        {0x3F808001u, 0x3F81}, {0x3F807FFFu, 0x3F80}, {0x3F817FFFu, 0x3F81}, {0x3F818001u, 0x3F82},
        {0x3F7FFFFFu, 0x3F80}, {0x3F7F8000u, 0x3F80}, {0xBF7FFFFFu, 0xBF80},       // the carry crosses the exponent
        {0x7F7FFFFFu, 0x7F80},                                                      // FLT_MAX rounds to infinity
        {0x00000000u, 0x0000}, {0x80000000u, 0x8000},
    };
    for (const auto& c : cases)
        CHECK(host_bf16(from_bits(c.in)) == c.want, "host_bf16(0x%08x) = 0x%04x, want 0x%04x", c.in, host_bf16(from_bits(c.in)), c.want);
    int checked = 0;
    for (uint32_t b = 0; b < 65536; ++b) {
        if ((b & 0x7F80u) == 0x7F80u && (b & 0x7Fu)) continue;      // a NaN
        ++checked;
        CHECK(bits_of(host_f32((uint16_t)b)) == b << 16, "host_f32(0x%04x) = 0x%08x", b, bits_of(host_f32((uint16_t)b)));
        CHECK(host_bf16(host_f32((uint16_t)b)) == b, "0x%04x comes back as 0x%04x", b, host_bf16(host_f32((uint16_t)b)));
    }
    CHECK(checked == 65536 - 2 * 127, "%d patterns", checked);
    const uint16_t in[3] = {0x3F80, 0x7FC1, 0xFF81};        // widening copies bits: NaN payloads survive
    float out[3];
    widen_bf16(in, 3, out);
    for (int i = 0; i < 3; ++i) CHECK(bits_of(out[i]) == (uint32_t)in[i] << 16, "widen_bf16(0x%04x) = 0x%08x", in[i], bits_of(out[i]));
}

// one value through the pair with shift s: the expected hi (as a float), lo8 and value
static void pair_case(int s, float x, float want_hi, int want_lo) {
    const float q = 1.0f / (float)(1 << s);
    uint16_t hi;
    int8_t lo;
    float back;
    pair_pack(&x, 1, s, &hi, &lo);
    pair_value(&hi, &lo, 1, q, &back);
    CHECK(host_f32(hi) == want_hi && lo == want_lo, "s %d x %.9g: hi %.9g lo %d, want hi %.9g lo %d", s, x, host_f32(hi), lo, want_hi, want_lo);
    CHECK(back == want_hi + (float)want_lo * q, "s %d x %.9g: value %.9g", s, x, back);
}

static void pair() {
    for (int s : {6, 12, 14}) {
        const float q = ldexpf(1.0f, -s);
        pair_case(s, 0.0f, 0.0f, 0);
        pair_case(s, q, q, 0);
        pair_case(s, -q, -q, 0);
        // around hi = 2^(10 - s), whose bf16 neighbours are 8 q above and 4 q below: remainders of exactly half a quantum go
        // to the even count
        const float h = ldexpf(1.0f, 10 - s);
        pair_case(s, h + 0.5f * q, h, 0);
        pair_case(s, h + 1.5f * q, h, 2);
        pair_case(s, h + 2.5f * q, h, 2);
        pair_case(s, h - 0.5f * q, h, 0);
        pair_case(s, h - 1.5f * q, h, -2);
        pair_case(s, h + 3.0f * q, h, 3);
        // around hi = 2^(17 - s) (neighbours 1024 q above, 512 q below) the remainder outgrows the byte: it stops at +-127,
        // it does not wrap
        const float g = ldexpf(1.0f, 17 - s);
        pair_case(s, g + 127.0f * q, g, 127);
        pair_case(s, g + 128.0f * q, g, 127);
        pair_case(s, g + 200.0f * q, g, 127);
        pair_case(s, g - 127.0f * q, g, -127);
        pair_case(s, g - 128.0f * q, g, -127);
        pair_case(s, g - 200.0f * q, g, -127);
    }
    CHECK(!lo_shift_ok(5) && lo_shift_ok(6) && lo_shift_ok(12) && lo_shift_ok(14) && !lo_shift_ok(15), "lo_shift range");
}

static void generators() {
    // what the timing hooks' own loops produced before the generators moved into the header
    const uint16_t lcg[8] = {0x3c8e, 0xbe3d, 0xbe21, 0x3c89, 0xbfd8, 0x3d24, 0x3d4d, 0x3c4b};
    const uint8_t xs[8] = {0x63, 0x7a, 0xa0, 0x7e, 0xe1, 0xea, 0xf2, 0x3d};
    std::vector<uint16_t> a(8), b(16);
    const uint32_t seed = fill_lcg_bf16(a.data(), 8, 12345u);
    for (int i = 0; i < 8; ++i) CHECK(a[i] == lcg[i], "lcg[%d] = 0x%04x, want 0x%04x", i, a[i], lcg[i]);
    CHECK(seed == 2355140353u, "seed after 8 values: %u", seed);
    fill_lcg_bf16(b.data(), 16, 12345u);        // one sequence over two arrays = the sequence in one
    fill_lcg_bf16(a.data(), 8, seed);
    for (int i = 0; i < 8; ++i) CHECK(b[8 + i] == a[i], "lcg continued [%d] = 0x%04x, want 0x%04x", i, a[i], b[8 + i]);
    std::vector<uint8_t> x(8);
    fill_xorshift_u8(x.data(), 8);
    for (int i = 0; i < 8; ++i) CHECK(x[i] == xs[i], "xorshift[%d] = 0x%02x, want 0x%02x", i, x[i], xs[i]);
    fill_xorshift_u8(x.data(), 0);              // nothing to fill: nothing touched
    CHECK(x[0] == xs[0], "an empty fill wrote");
}

static void cfg_split() {
    const struct { int in, cfg, order; } cases[] = {{-1, -1, 0}, {0, 0, 0}, {0x1ff, 0xff, 1}, {0x203, 3, 2}};
    for (const auto& c : cases) {
        const TileCfg t = split_cfg(c.in);
        CHECK(t.cfg == c.cfg && t.order == c.order, "split_cfg(%d) = (%d, %d), want (%d, %d)", c.in, t.cfg, t.order, c.cfg, c.order);
    }
}

int main() {
    rounding();
    pair();
    generators();
    cfg_split();
    printf("%d checks failed\n", failures);
    return failures > 255 ? 255 : failures;
}
