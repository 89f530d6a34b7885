// k_head.hpp — the decode launch and the head's band convolutions (k_head.hip).
#pragma once
#include "vt_common.hpp"
#include "vt_frame.hpp"

struct DecodeArgs {
    const bf16_t* t3;       // [B*ns][C]
    const float* w4;        // [8][C]
    const float* b4;        // [8]
    const float* hann;      // [ns]
    float* head_out;        // [B*ns][8]
    StreamState* states;    // [B]
    vt_result* results;     // [B] (device)
    const PassOut* out;     // device copy of this pass's PassOut
    // [B] slot -> stream of a subset pass (null: the identity, every full pass). head_out, results and
    // out->host_results are indexed by slot; states and out->host_states by stream.
    const int32_t* slot_stream;
    int B, ns, grid, C;     // B: slots of the pass
    float success_threshold;
};
hipError_t launch_decode(const DecodeArgs& a, hipStream_t st);     // head_out_kernel + decode_kernel (two launches)

// The head's convolutions on the band kernel of k_head.hip: out[B*grid*grid][N] bf16 = relu(conv(in) + bias).
// conv3x3: in [B*grid*grid][C] (ldin >= C), W [N][9*C] with column (ky*3+kx)*C + c, zero padding (zeros: >= 256 B
// of zeros in device memory), N == C; else a 1x1 layer: in [B*grid*grid][K], W [N][K].
struct HeadConvArgs {
    const bf16_t* in; int ldin;
    const bf16_t* W; int ldw;
    const float* bias;
    bf16_t* out; int ldout;
    const bf16_t* zeros;
    int B, grid, C, N, K;
    int conv3x3;
    int R, ncb;                 // rows per band / 16-column blocks per wave; <= 0: planned by the launcher
    unsigned* band_cnt;         // fused tail only: [B] arrival counters, zero between launches
    float* band_best;           // fused tail only: [B][bands][2] each band's argmax candidate (response, cell), bands <= grid
    int bands, mbe_max;         // filled in by the launcher
    unsigned long long* dbg;    // diagnostic builds only (VT_STAMPS): per-wave cycle sums [wgs][8][4]
    // 1x1 layer with the final LayerNorm inside (xh != nullptr; `in` is ignored): the layer's input row (b, cell) is
    // LayerNorm(xh + xl)[b * in_stride + in_off + cell][0..K) with gamma ln_g, beta ln_b
    const bf16_t* xh;
    const uint8_t* xl;
    const float *ln_g, *ln_b;
    float ln_eps;
    int in_stride, in_off;
    float lo_q = 1.0f / 4096.0f;    // the pair's quantum 2^-s (LoQuant.q)
};
bool headconv_supported(int grid, int C, int N, int K, bool conv3x3);
bool headconv_ln_supported(int grid, int N, int D);
bool headconv_plannable(int grid, int C, int N, int K, bool conv3x3, bool tail);   // supported and some band height fits LDS
hipError_t headconv_prepare();     // once per device, before the first launch / any stream capture
// dec != nullptr (3x3 layers only): the 5-logit layer, the score window, the argmax and the box decode run inside
// the same launch (dec->t3 is ignored: the logits are computed from the layer's own output tile)
hipError_t launch_headconv(HeadConvArgs a, const DecodeArgs* dec, hipStream_t st);
