// colorimetry_frame_main.cpp — the format word of vt_frame.format (csrc/vt_frame.hpp alone): every word 0..65535, every word
// with one of the bits 16..31 set and -1. Compiled with AddressSanitizer and UndefinedBehaviorSanitizer and run as a child
// process by tests/test_colorimetry_frame_host.py. No GPU.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "vt_frame.hpp"

static int failed = 0, checks = 0;
#define CHECK(cond, ...) \
    do { \
        ++checks; \
        if (!(cond)) { \
            if (++failed <= 20) { printf("FAILED %s:%d %s ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        } \
    } while (0)

// what the helpers were before the word had colour bits, written out: the yardstick for "the base format's"
static const int kRgb[] = {VT_PIX_RGB8, VT_PIX_BGR8, VT_PIX_RGBX, VT_PIX_BGRX, VT_PIX2_GRAY8, VT_PIX2_XRGB, VT_PIX2_XBGR};
static const int k420[] = {VT_PIX_NV12, VT_PIX_NV21, VT_PIX2_I420, VT_PIX2_YV12, VT_PIX2_P010, VT_PIX2_NV16};
static const int k422[] = {VT_PIX_YUY2, VT_PIX_UYVY};
static int old_family(int fmt) {
    for (int v : kRgb) if (fmt == v) return PIXF_RGB;
    for (int v : k420) if (fmt == v) return PIXF_420SP;
    for (int v : k422) if (fmt == v) return PIXF_422;
    return -1;
}
static int old_level(int fmt) { return fmt >= VT_PIX2_I420 ? 2 : fmt != VT_PIX_RGB8 && fmt != VT_PIX_NV12 && fmt != VT_PIX_YUY2 ? 1 : 0; }

// section 1 of the rule: is the word refused?
static bool refused(long long word) {
    if (word < 0 || word > 0xffff) return true;
    const int base = (int)(word & 0xff), matrix = (int)((word >> 8) & 15), range = (int)((word >> 12) & 15);
    const int fam = old_family(base);
    if (fam < 0 || matrix > 2 || range > 1) return true;
    return fam == PIXF_RGB && (matrix != 0 || range != 0);
}

static void check_word(int word) {
    const bool bad = refused(word);
    const int fam = pix_family(word);
    CHECK((fam == -1) == bad, "word 0x%x family %d", (unsigned)word, fam);
    const int base = word & 0xff;
    const int code = ((word >> 8) & 15) * 2 + ((word >> 12) & 15);
    CHECK(pix_level(word) == (!bad && code != 0 ? 3 : old_level(word)), "word 0x%x level %d", (unsigned)word, pix_level(word));
    CHECK((pix_refusal(word) != nullptr) == (bad && word >= 0 && old_family(base) >= 0), "word 0x%x refusal text", (unsigned)word);
    if (bad) return;
    CHECK(fam == old_family(base), "word 0x%x", (unsigned)word);
    CHECK(pix_color_code(word) == code && code >= 0 && code <= 5, "word 0x%x code %d", (unsigned)word, pix_color_code(word));
    CHECK(pix_layout(word) == pix_layout(base), "word 0x%x", (unsigned)word);
    CHECK(strcmp(pix_name(word), pix_name(base)) == 0 && strcmp(pix_name(word), "?") != 0, "word 0x%x", (unsigned)word);
    CHECK(pix_row_bpp(word) == pix_row_bpp(base), "word 0x%x", (unsigned)word);
    CHECK(pix_planar(word) == pix_planar(base) && pix_rows422(word) == pix_rows422(base), "word 0x%x", (unsigned)word);
    for (int n : {1, 2, 17, 640, 1079, 16384}) {
        CHECK(pix_chroma_rows(word, n) == pix_chroma_rows(base, n), "word 0x%x rows %d", (unsigned)word, n);
        if (fam == PIXF_420SP)
            CHECK(pix_chroma_row_bytes(word, n) == pix_chroma_row_bytes(base, n), "word 0x%x row bytes %d", (unsigned)word, n);
    }
    // the code packed into the layout word (to_desc: lay | code << PIXL_CODE_SHIFT, | PIXL_FULLH for whole planar frames)
    // collides with no bit a kernel of level 2 reads: the masks of fetch_rgb<2>, of the tile body's groups and of the
    // result overlay, each evaluated on the word with and without the code
    if (fam == PIXF_RGB) return;        // never carries a code
    for (int fullh = 0; fullh < 2; ++fullh) {
        const int32_t plain = pix_layout(word) | (fullh ? PIXL_FULLH : 0);
        const int32_t lay = plain | (int32_t)((uint32_t)code << PIXL_CODE_SHIFT);
        CHECK(lay >= 0 && ((lay >> PIXL_CODE_SHIFT) & PIXL_CODE_MASK) == code, "word 0x%x lay 0x%x", (unsigned)word, (unsigned)lay);
        CHECK((plain & (PIXL_CODE_MASK << PIXL_CODE_SHIFT)) == 0, "word 0x%x: the layout word uses the code's bits", (unsigned)word);
        const int32_t masks[] = {3, 3 << 8, 3 << 16, 3 << 24, 1, 0x100, 255, 255 << 8, 255 << 16, PIXL_PLANAR, PIXL_S16, PIXL_HIBYTE,
                                 PIXL_ROWS422, PIXL_FULLH, PIXL_PLANAR | PIXL_S16};
        for (int32_t m : masks) CHECK((lay & m) == (plain & m), "word 0x%x mask 0x%x", (unsigned)word, (unsigned)m);
        const int shifts[] = {0, 8, 16, 20, 22, 24};
        const int ands[] = {1, 1, 3, 1, 1, 3};      // widest use of each shift below bit 26: (lay >> 24) & 3, (lay >> 20) & 1, ...
        for (int i = 0; i < 6; ++i)
            CHECK(((lay >> shifts[i]) & ands[i]) == ((plain >> shifts[i]) & ands[i]), "word 0x%x shift %d", (unsigned)word, shifts[i]);
        CHECK((((lay >> 24) & 1) ^ 1) == (((plain >> 24) & 1) ^ 1), "word 0x%x chroma row shift", (unsigned)word);
    }
}

int main() {
    static_assert(PIX_LEVELS == 4, "levels");
    static_assert(PIXL_CODE_SHIFT > 25 && PIXL_CODE_SHIFT + 3 <= 31, "the code lies above every layout bit and below the sign");
    static_assert(VT_FRAME_FORMAT(VT_PIX_NV12, VT_COLOR_BT601, VT_RANGE_LIMITED) == VT_PIX_NV12, "a plain format is itself");
    for (int word = 0; word <= 0xffff; ++word) check_word(word);
    for (int bit = 16; bit < 32; ++bit)
        for (int low : {0, (int)VT_PIX_NV12, (int)VT_PIX2_I420, VT_FRAME_FORMAT(VT_PIX_NV12, VT_COLOR_BT709, VT_RANGE_FULL), 0xffff})
            check_word((int)((uint32_t)low | (1u << bit)));
    check_word(-1);
    // the counts: 15 plain formats, 8 YUV formats x 5 further codes
    int valid = 0, level3 = 0;
    for (int word = 0; word <= 0xffff; ++word) {
        valid += pix_family(word) >= 0;
        level3 += pix_level(word) == 3;
    }
    CHECK(valid == 15 + 8 * 5 && level3 == 8 * 5, "valid %d level3 %d", valid, level3);
    // the refusal texts name what is wrong
    CHECK(strstr(pix_refusal(VT_FRAME_FORMAT(VT_PIX_RGB8, 1, 0)), "without chroma") != nullptr, "rgb8");
    CHECK(strstr(pix_refusal(VT_FRAME_FORMAT(VT_PIX_NV12, 3, 0)), "matrix") != nullptr, "matrix 3");
    CHECK(strstr(pix_refusal(VT_FRAME_FORMAT(VT_PIX_NV12, 0, 2)), "range") != nullptr, "range 2");
    CHECK(strstr(pix_refusal(VT_PIX_NV12 | 1 << 16), "above 15") != nullptr, "bit 16");
    CHECK(strcmp(pix_name(VT_FRAME_FORMAT(VT_PIX2_GRAY8, 1, 0)), "gray8") == 0, "name of a refused word");
    printf("%d checks, %d checks failed\n", checks, failed);
    return failed ? 1 : 0;
}
