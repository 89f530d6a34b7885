// k_preproc_body.inc — the bodies of the three crop kernels, as text: the ONE definition of the crop's arithmetic
// (geometry, tap order, float operation order, store shape). k_preproc.hip includes a body into each of its kernels;
// k_refresh.hip includes the same text into the template refresh, which therefore writes the bits init writes. Text and
// not a device function: inlined as a function, the tile body compiled to other code than it does in place (115 more
// instructions, other SGPR counts: profiles/template_refresh.txt), and those kernels are not to move.
// In scope at the include: ANY, f (the slot's FrameDesc), s (the stream's StreamState&), patches, b (the slot), size,
// patch, kpad, ntok, row_off, factor, na0..na2, nb0..nb2, is_template; bodies 2 and 3: PX; body 3: src (LDS) and LDSPX.
// A body may `return`. PRE_BODY: 1 one lane per pixel, 2 wide stores, 3 tiles of 64 x 32 staged in LDS.
// Preprocessor parameters of bodies 2 and 3 (k_chip.hip, the u8 chips; nobody else defines them, and undefined they
// expand to the text that stood here): PRE_OUT(v, c), what is kept of a channel's bilinear value v (default: the
// normalised bf16), and PRE_STORE_RGB8, the store of a lane's run as packed RGB bytes to chip8[size][size][3]
// (default: planar bf16 patch rows).
#ifndef PRE_OUT
#define PRE_OUT(v, c) f32_to_bf16(v * na[c] + nb[c])
#define PRE_OUT_DEFAULT
#endif
#if PRE_BODY == 1
    // crop geometry — same operations, same order as vto_crop_geometry (oracle/vt_oracle.c)
    const float bx = s.box[0], by = s.box[1], bw = s.box[2], bh = s.box[3];
    const float area = bw * bh;
    const float side = factor * sqrtf(area);
    const float scale = side / (float)size;
    const float cx = bx + 0.5f * bw;
    const float cy = by + 0.5f * bh;
    const float half = 0.5f * side;
    const float x0m = (cx - half) - 0.5f;
    const float y0m = (cy - half) - 0.5f;
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix == 0 && !is_template) {
        s.geo[0] = x0m; s.geo[1] = y0m; s.geo[2] = scale; s.geo[3] = side;
        s.frame_w = f.w; s.frame_h = f.h;
    }
    if (pix >= size * size) return;
    const int oy = pix / size, ox = pix % size;
    const float fy = ((float)oy + 0.5f) * scale + y0m;
    const float fx = ((float)ox + 0.5f) * scale + x0m;
    const float fy0 = floorf(fy), fx0 = floorf(fx);
    const float wy = fy - fy0, wx = fx - fx0;
    const int iy = (int)fy0, ix = (int)fx0;
    float p00[3], p01[3], p10[3], p11[3];
    int miss = 0;
    fetch_rgb<ANY>(f, ix, iy, p00, miss);
    fetch_rgb<ANY>(f, ix + 1, iy, p01, miss);
    fetch_rgb<ANY>(f, ix, iy + 1, p10, miss);
    fetch_rgb<ANY>(f, ix + 1, iy + 1, p11, miss);
    if (miss && !is_template) s.window_miss = s.frames_done + 1;   // every writer stores the same value
    const int grid = size / patch;
    const int token = (oy / patch) * grid + (ox / patch);
    const int kin = (oy % patch) * patch + (ox % patch);
    bf16_t* row = patches + ((size_t)b * ntok + row_off + token) * kpad;
    const float na[3] = {na0, na1, na2}, nb[3] = {nb0, nb1, nb2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = p00[c] + wx * (p01[c] - p00[c]);
        const float bot = p10[c] + wx * (p11[c] - p10[c]);
        const float v = top + wy * (bot - top);
        const float o = v * na[c] + nb[c];
        row[c * patch * patch + kin] = f32_to_bf16(o);
    }
#elif PRE_BODY == 2
    // crop geometry — same operations, same order as vto_crop_geometry (oracle/vt_oracle.c)
    const float bx = s.box[0], by = s.box[1], bw = s.box[2], bh = s.box[3];
    const float area = bw * bh;
    const float side = factor * sqrtf(area);
    const float scale = side / (float)size;
    const float cx = bx + 0.5f * bw;
    const float cy = by + 0.5f * bh;
    const float half = 0.5f * side;
    const float x0m = (cx - half) - 0.5f;
    const float y0m = (cy - half) - 0.5f;
    const int grp = blockIdx.x * blockDim.x + threadIdx.x;        // group of PX pixels
    if (grp == 0 && !is_template) {
        s.geo[0] = x0m; s.geo[1] = y0m; s.geo[2] = scale; s.geo[3] = side;
        s.frame_w = f.w; s.frame_h = f.h;
    }
    const int gpr = size / PX;                                     // groups per output row
    if (grp >= gpr * size) return;
    const int oy = grp / gpr, ox0 = (grp % gpr) * PX;
    const float fy = ((float)oy + 0.5f) * scale + y0m;
    const float fy0 = floorf(fy);
    const float wy = fy - fy0;
    const int iy = (int)fy0;
    const float na[3] = {na0, na1, na2}, nb[3] = {nb0, nb1, nb2};
    bf16_t o[3][PX];
    int miss = 0;
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        const float fx = ((float)(ox0 + k) + 0.5f) * scale + x0m;
        const float fx0 = floorf(fx);
        const float wx = fx - fx0;
        const int ix = (int)fx0;
        float p00[3], p01[3], p10[3], p11[3];
        fetch_rgb<ANY>(f, ix, iy, p00, miss);
        fetch_rgb<ANY>(f, ix + 1, iy, p01, miss);
        fetch_rgb<ANY>(f, ix, iy + 1, p10, miss);
        fetch_rgb<ANY>(f, ix + 1, iy + 1, p11, miss);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float top = p00[c] + wx * (p01[c] - p00[c]);
            const float bot = p10[c] + wx * (p11[c] - p10[c]);
            const float v = top + wy * (bot - top);
            o[c][k] = PRE_OUT(v, c);
        }
    }
    if (miss && !is_template) s.window_miss = s.frames_done + 1;   // every writer stores the same value
#ifdef PRE_STORE_RGB8
    PRE_STORE_RGB8_RUN(o, chip8 + ((size_t)oy * size + ox0) * 3);
    return;
#endif
    const int grid = size / patch;
    const int token = (oy / patch) * grid + (ox0 / patch);         // PX divides patch: one token per group
    const int kin = (oy % patch) * patch + (ox0 % patch);
    bf16_t* row = patches + ((size_t)b * ntok + row_off + token) * kpad;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        bf16_t* dst = row + c * patch * patch + kin;
        if constexpr (PX == 8) {
            uint4 v;
            v.x = o[c][0] | ((uint32_t)o[c][1] << 16); v.y = o[c][2] | ((uint32_t)o[c][3] << 16);
            v.z = o[c][4] | ((uint32_t)o[c][5] << 16); v.w = o[c][6] | ((uint32_t)o[c][7] << 16);
            *reinterpret_cast<uint4*>(dst) = v;
        } else {
            *reinterpret_cast<uint32_t*>(dst) = o[c][0] | ((uint32_t)o[c][1] << 16);
        }
    }
#elif PRE_BODY == 3
    // crop geometry — same operations, same order as vto_crop_geometry (oracle/vt_oracle.c)
    const float bx = s.box[0], by = s.box[1], bw = s.box[2], bh = s.box[3];
    const float area = bw * bh;
    const float side = factor * sqrtf(area);
    const float scale = side / (float)size;
    const float cx = bx + 0.5f * bw;
    const float cy = by + 0.5f * bh;
    const float half = 0.5f * side;
    const float x0m = (cx - half) - 0.5f;
    const float y0m = (cy - half) - 0.5f;
    if (blockIdx.x == 0 && threadIdx.x == 0 && !is_template) {
        s.geo[0] = x0m; s.geo[1] = y0m; s.geo[2] = scale; s.geo[3] = side;
        s.frame_w = f.w; s.frame_h = f.h;
    }
    const int tiles_x = size / PRE_TILE_W;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    // lane -> 8-pixel run of the tile. patch 16 (round 4): the tile is 4 x 2 tokens and a half-wave takes ONE
    // token - lane pair (2 py, 2 py + 1) of 16 patch rows - so that a channel's store instruction writes the
    // 512 contiguous bytes of that token's channel block instead of 16-B pieces of four different patch rows
    // (rows of the patch matrix lie kpad * 2 bytes apart); other patch sizes keep the row-major assignment.
    int oy, ox0;
    if (patch == 16) {
        const int tok = threadIdx.x >> 5, py = (threadIdx.x >> 1) & 15, hx = threadIdx.x & 1;
        oy = ty * PRE_TILE_H + (tok >> 2) * 16 + py;
        ox0 = tx * PRE_TILE_W + (tok & 3) * 16 + hx * PX;
    } else {
        oy = ty * PRE_TILE_H + (threadIdx.x >> 3);
        ox0 = tx * PRE_TILE_W + (threadIdx.x & 7) * PX;
    }
    // source rectangle of the tile: taps of its first and last output pixel (fx, fy grow with ox, oy)
    const int sx_lo = (int)floorf(((float)(tx * PRE_TILE_W) + 0.5f) * scale + x0m);
    const int sx_hi = (int)floorf(((float)(tx * PRE_TILE_W + PRE_TILE_W - 1) + 0.5f) * scale + x0m) + 1;
    const int sy_lo = (int)floorf(((float)(ty * PRE_TILE_H) + 0.5f) * scale + y0m);
    const int sy_hi = (int)floorf(((float)(ty * PRE_TILE_H + PRE_TILE_H - 1) + 0.5f) * scale + y0m) + 1;
    const long sw = (long)sx_hi - sx_lo + 1, sh = (long)sy_hi - sy_lo + 1;
    const bool staged = sw > 0 && sh > 0 && sw * sh <= LDSPX;      // block-uniform
    if (staged) {
        const int n = (int)(sw * sh), w_ = (int)sw;
        // NV12 planes whose rows start on 8-byte boundaries (the library's packed windows: pack_window; whole
        // frames with such strides): the rectangle is fetched in groups of 8 pixels - ONE 8-byte load of Y
        // and ONE of the interleaved UV row (4 pairs) per group, where the per-pixel path issues 24 byte
        // loads - and converted with the same integer formulas. A group that is not entirely inside the
        // frame and the stored window goes through fetch_rgb pixel by pixel (frame border: black; outside the
        // window: black + miss), so every entry of the LDS image is what the per-pixel loop writes.
        // NV21 takes the same path (ANY kernels): the descriptor says which byte of a pair is U
        // and so does NV16, with one chroma row per luma row; the planar and 16-bit layouts have groups of their own below
        // ANY = 3: every group converts with the frame's colour code (yuv_to_rgb_lay), as its per-pixel fallback does in fetch_rgb
        const bool fast = f.fmt == PIXF_420SP && (ANY < 2 || (f.lay & (PIXL_PLANAR | PIXL_S16)) == 0) && (((uintptr_t)f.p0 | (uintptr_t)f.p1 | (uintptr_t)f.s0 | (uintptr_t)f.s1) & 7) == 0;
        // ANY kernels, 4-byte RGB formats (RGBX, BGRX, XRGB, XBGR) whose rows start on 16-byte boundaries (the library's packed
        // windows; whole frames with such strides): ONE 16-byte load per 4 pixels, where the per-pixel path issues 12
        // byte loads; the same edge rule as the NV12 groups
        const bool fast4 = ANY && f.fmt == PIXF_RGB && (f.lay >> 24) == 4 && (((uintptr_t)f.p0 | (uintptr_t)f.s0) & 15) == 0;
        // ANY = 2 kernels, groups of 8 pixels for the other layouts with a luma / grey plane, under the same edge rule, each
        // on the alignment its loads need: 1 I420 / YV12 (8 B of Y + 4 B of U + 4 B of V), 2 P010 (16 B of Y + 16 B of
        // chroma, of which the high bytes), 3 GRAY8 (8 B)
        int xmode = 0;
        if constexpr (ANY >= 2) {
            if (f.fmt == PIXF_420SP && (f.lay & PIXL_PLANAR))
                xmode = ((((uintptr_t)f.p0 | (uintptr_t)f.s0) & 7) | (((uintptr_t)f.p1 | (uintptr_t)f.s1) & 3)) == 0 ? 1 : 0;
            else if (f.fmt == PIXF_420SP && (f.lay & PIXL_S16))
                xmode = (((uintptr_t)f.p0 | (uintptr_t)f.p1 | (uintptr_t)f.s0 | (uintptr_t)f.s1) & 15) == 0 ? 2 : 0;
            else if (f.fmt == PIXF_RGB && (f.lay >> 24) == 1)
                xmode = (((uintptr_t)f.p0 | (uintptr_t)f.s0) & 7) == 0 ? 3 : 0;
        }
        const int crs = ANY >= 2 ? ((f.lay >> 24) & 1) ^ 1 : 1;      // chroma row shift: 0 for NV16
        if (fast) {
            const int us = ANY ? (f.lay & 1) * 8 : 0, vs = ANY ? ((f.lay >> 8) & 1) * 8 : 8;   // bit offsets of U, V in a pair
            const int g_lo = (sx_lo - f.x0) >> 3, g_hi = (sx_hi - f.x0) >> 3;     // arithmetic shift: floor for negatives
            const int gpr = g_hi - g_lo + 1, ng = gpr * (int)sh;
            for (int i = threadIdx.x; i < ng; i += 256) {
                const int ry = i / gpr, wx0 = (g_lo + i % gpr) << 3;                // window column of the group
                const int py = sy_lo + ry, wy_ = py - f.y0, px0 = wx0 + f.x0;
                const bool inside = (unsigned)wy_ < (unsigned)f.wh && (unsigned)py < (unsigned)f.h && wx0 >= 0 &&
                                    wx0 + 7 < f.ww && px0 >= 0 && px0 + 7 < f.w;
                uint32_t* dst = src + ry * w_ + (px0 - sx_lo);
                if (inside) {
                    const uint2 y8 = *reinterpret_cast<const uint2*>(f.p0 + (size_t)wy_ * f.s0 + wx0);
                    const uint2 uv8 = *reinterpret_cast<const uint2*>(f.p1 + (size_t)(wy_ >> crs) * f.s1 + wx0);
                    const uint32_t yw[2] = {y8.x, y8.y}, uw[2] = {uv8.x, uv8.y};
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int col = px0 - sx_lo + k;
                        if (col < 0 || col >= w_) continue;
                        const uint32_t pair = uw[k >> 2] >> (((k >> 1) & 1) * 16);   // U, V of the pixel pair
                        int r, g, b;
                        yuv_to_rgb_lay<ANY>(f.lay, (int)((yw[k >> 2] >> ((k & 3) * 8)) & 255u), (int)((pair >> us) & 255u), (int)((pair >> vs) & 255u), r, g, b);
                        dst[k] = (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
                    }
                } else {
                    for (int k = 0; k < 8; ++k) {
                        const int col = px0 - sx_lo + k;
                        if (col < 0 || col >= w_) continue;
                        float p[3];
                        int miss = 0;
                        fetch_rgb<ANY>(f, px0 + k, py, p, miss);
                        dst[k] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)miss << 24);
                    }
                }
            }
        } else if (ANY >= 2 && xmode) {
            // the group's samples in NV12's form - 8 luma bytes, 4 (U, V) pairs - then NV12's conversion
            const int us = xmode == 2 ? (f.lay & 1) * 8 : 0, vs = xmode == 2 ? ((f.lay >> 8) & 1) * 8 : 8;
            const size_t second = (size_t)f.s1 * (size_t)((((f.lay & PIXL_FULLH) ? f.h : f.wh) + 1) >> 1);
            const uint8_t* pu = f.p1 + ((f.lay & 1) ? second : 0);
            const uint8_t* pv = f.p1 + ((f.lay & 0x100) ? second : 0);
            const int g_lo = (sx_lo - f.x0) >> 3, g_hi = (sx_hi - f.x0) >> 3;     // arithmetic shift: floor for negatives
            const int gpr = g_hi - g_lo + 1, ng = gpr * (int)sh;
            for (int i = threadIdx.x; i < ng; i += 256) {
                const int ry = i / gpr, wx0 = (g_lo + i % gpr) << 3;                // window column of the group
                const int py = sy_lo + ry, wy_ = py - f.y0, px0 = wx0 + f.x0;
                const bool inside = (unsigned)wy_ < (unsigned)f.wh && (unsigned)py < (unsigned)f.h && wx0 >= 0 &&
                                    wx0 + 7 < f.ww && px0 >= 0 && px0 + 7 < f.w;
                uint32_t* dst = src + ry * w_ + (px0 - sx_lo);
                if (inside) {
                    uint32_t yw[2], uw[2] = {0u, 0u};
                    if (xmode == 2) {
                        const u32x4_t y16 = *reinterpret_cast<const u32x4_t*>(f.p0 + (size_t)wy_ * f.s0 + (size_t)wx0 * 2);
                        const u32x4_t c16 = *reinterpret_cast<const u32x4_t*>(f.p1 + (size_t)(wy_ >> crs) * f.s1 + (size_t)wx0 * 2);
                        yw[0] = __builtin_amdgcn_perm(y16[1], y16[0], 0x07050301u);  // byte 1 of each of four samples
                        yw[1] = __builtin_amdgcn_perm(y16[3], y16[2], 0x07050301u);
                        uw[0] = __builtin_amdgcn_perm(c16[1], c16[0], 0x07050301u);
                        uw[1] = __builtin_amdgcn_perm(c16[3], c16[2], 0x07050301u);
                    } else {
                        const uint2 y8 = *reinterpret_cast<const uint2*>(f.p0 + (size_t)wy_ * f.s0 + wx0);
                        yw[0] = y8.x; yw[1] = y8.y;
                        if (xmode == 1) {
                            const size_t co = (size_t)(wy_ >> 1) * f.s1 + (wx0 >> 1);
                            const uint32_t u4 = *reinterpret_cast<const uint32_t*>(pu + co);
                            const uint32_t v4 = *reinterpret_cast<const uint32_t*>(pv + co);
                            uw[0] = __builtin_amdgcn_perm(v4, u4, 0x05010400u);     // u0 v0 u1 v1
                            uw[1] = __builtin_amdgcn_perm(v4, u4, 0x07030602u);     // u2 v2 u3 v3
                        }
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int col = px0 - sx_lo + k;
                        if (col < 0 || col >= w_) continue;
                        const uint32_t yk = (yw[k >> 2] >> ((k & 3) * 8)) & 255u;
                        if (xmode == 3) {
                            dst[k] = yk * 0x010101u;
                        } else {
                            const uint32_t pair = uw[k >> 2] >> (((k >> 1) & 1) * 16);   // U, V of the pixel pair
                            int r, g, b;
                            yuv_to_rgb_lay<ANY>(f.lay, (int)yk, (int)((pair >> us) & 255u), (int)((pair >> vs) & 255u), r, g, b);
                            dst[k] = (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
                        }
                    }
                } else {
                    for (int k = 0; k < 8; ++k) {
                        const int col = px0 - sx_lo + k;
                        if (col < 0 || col >= w_) continue;
                        float p[3];
                        int miss = 0;
                        fetch_rgb<ANY>(f, px0 + k, py, p, miss);
                        dst[k] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)miss << 24);
                    }
                }
            }
        } else if (fast4) {
            const uint32_t sel = ((uint32_t)f.lay & 0x00ffffffu) | 0x0c000000u;   // bytes R, G, B, zero of a pixel
            const int g_lo = (sx_lo - f.x0) >> 2, g_hi = (sx_hi - f.x0) >> 2;     // arithmetic shift: floor for negatives
            const int gpr = g_hi - g_lo + 1, ng = gpr * (int)sh;
            for (int i = threadIdx.x; i < ng; i += 256) {
                const int ry = i / gpr, wx0 = (g_lo + i % gpr) << 2;                // window column of the group
                const int py = sy_lo + ry, wy_ = py - f.y0, px0 = wx0 + f.x0;
                const bool inside = (unsigned)wy_ < (unsigned)f.wh && (unsigned)py < (unsigned)f.h && wx0 >= 0 &&
                                    wx0 + 3 < f.ww && px0 >= 0 && px0 + 3 < f.w;
                uint32_t* dst = src + ry * w_ + (px0 - sx_lo);
                if (inside) {
                    const u32x4_t q = *reinterpret_cast<const u32x4_t*>(f.p0 + (size_t)wy_ * f.s0 + (size_t)wx0 * 4);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int col = px0 - sx_lo + k;
                        if (col < 0 || col >= w_) continue;
                        dst[k] = __builtin_amdgcn_perm(0u, q[k], sel);              // r | g << 8 | b << 16
                    }
                } else {
                    for (int k = 0; k < 4; ++k) {
                        const int col = px0 - sx_lo + k;
                        if (col < 0 || col >= w_) continue;
                        float p[3];
                        int miss = 0;
                        fetch_rgb<ANY>(f, px0 + k, py, p, miss);
                        dst[k] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)miss << 24);
                    }
                }
            }
        } else {
            for (int i = threadIdx.x; i < n; i += 256) {
                float p[3];
                int miss = 0;
                fetch_rgb<ANY>(f, sx_lo + i % w_, sy_lo + i / w_, p, miss);
                src[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)miss << 24);
            }
        }
        __syncthreads();
    }
    const float fy = ((float)oy + 0.5f) * scale + y0m;
    const float fy0 = floorf(fy);
    const float wy = fy - fy0;
    const int iy = (int)fy0;
    const float na[3] = {na0, na1, na2}, nb[3] = {nb0, nb1, nb2};
    const int grid = size / patch;
    const int token = (oy / patch) * grid + (ox0 / patch);         // PX divides patch: one token per group
    const int kin = (oy % patch) * patch + (ox0 % patch);
    bf16_t* row = patches + ((size_t)b * ntok + row_off + token) * kpad;
    int miss = 0;
    if (!staged) {
        // rectangles over 4,096 source pixels (targets from ~130 px at search 384, ~90 px at search 256: see the
        // kernel's header): direct fetches, pixel by pixel, 2-byte stores. Kept out of
        // the staged path's code: inlined into its unrolled loop the 32 fetch_rgb bodies cost 70 VGPRs and
        // with them a block per CU.
#pragma unroll 1
        for (int k = 0; k < PX; ++k) {
            const float fx = ((float)(ox0 + k) + 0.5f) * scale + x0m;
            const float fx0 = floorf(fx);
            const float wx = fx - fx0;
            const int ix = (int)fx0;
            float p00[3], p01[3], p10[3], p11[3];
            fetch_rgb<ANY>(f, ix, iy, p00, miss);
            fetch_rgb<ANY>(f, ix + 1, iy, p01, miss);
            fetch_rgb<ANY>(f, ix, iy + 1, p10, miss);
            fetch_rgb<ANY>(f, ix + 1, iy + 1, p11, miss);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float top = p00[c] + wx * (p01[c] - p00[c]);
                const float bot = p10[c] + wx * (p11[c] - p10[c]);
                const float v = top + wy * (bot - top);
#ifdef PRE_STORE_RGB8
                chip8[((size_t)oy * size + ox0 + k) * 3 + c] = (uint8_t)PRE_OUT(v, c);
#else
                row[c * patch * patch + kin + k] = PRE_OUT(v, c);
#endif
            }
        }
        if (miss && !is_template) s.window_miss = s.frames_done + 1;
        return;
    }
    bf16_t o[3][PX];
    const int w_ = (int)sw;
    const uint32_t* r0base = src + (iy - sy_lo) * w_ - sx_lo;
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        const float fx = ((float)(ox0 + k) + 0.5f) * scale + x0m;
        const float fx0 = floorf(fx);
        const float wx = fx - fx0;
        const uint32_t* r0 = r0base + (int)fx0;
        const uint32_t t00 = r0[0], t01 = r0[1], t10 = r0[w_], t11 = r0[w_ + 1];
        miss |= (int)((t00 | t01 | t10 | t11) >> 24);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float p00 = (float)((t00 >> (8 * c)) & 255u), p01 = (float)((t01 >> (8 * c)) & 255u);
            const float p10 = (float)((t10 >> (8 * c)) & 255u), p11 = (float)((t11 >> (8 * c)) & 255u);
            const float top = p00 + wx * (p01 - p00);
            const float bot = p10 + wx * (p11 - p10);
            const float v = top + wy * (bot - top);
            o[c][k] = PRE_OUT(v, c);
        }
    }
    if (miss && !is_template) s.window_miss = s.frames_done + 1;   // every writer stores the same value
#ifdef PRE_STORE_RGB8
    PRE_STORE_RGB8_RUN(o, chip8 + ((size_t)oy * size + ox0) * 3);
    return;
#endif
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        uint4 v;
        v.x = o[c][0] | ((uint32_t)o[c][1] << 16); v.y = o[c][2] | ((uint32_t)o[c][3] << 16);
        v.z = o[c][4] | ((uint32_t)o[c][5] << 16); v.w = o[c][6] | ((uint32_t)o[c][7] << 16);
        *reinterpret_cast<uint4*>(row + c * patch * patch + kin) = v;
    }
#endif
#undef PRE_BODY
#ifdef PRE_OUT_DEFAULT
#undef PRE_OUT
#undef PRE_OUT_DEFAULT
#endif
