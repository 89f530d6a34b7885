"""The six timing hooks of include/vittrack_hip_ops.h (vt_op_gemm_bench, vt_op_attention_bench, the two NV12 timers and the
timing forms of vt_op_headconv_bf16 / vt_op_headconv_ln_bf16_lo): each returns a finite, positive time, and each refuses
iters = 0 without touching us_out. Every shape is the smallest one tests/test_gpu_ops.py runs through the matching value
hook, so no kernel and no configuration runs here that does not run there. Nothing is asserted about speed."""
import ctypes
import math

import pytest

pytestmark = pytest.mark.gpu

ITERS = 2
EPI_F32, EPI_GELU, EPI_QKV = 5, 2, 4         # vt_op_gemm_bench takes the library's own numbering of the epilogues
HEADCONV = dict(B=2, grid=5, Cin=64, N=64, conv3x3=True, R=2, ncb=1)                     # test_head_band_kernel_conv3x3
HEADCONV_LN = dict(B=2, grid=15, D=768, N=128, ntok=230, off=5, R=2, ncb=2)              # ..._with_the_final_layernorm_inside


def _timed_ok(us):
    assert isinstance(us, float) and math.isfinite(us) and us > 0.0, us


@pytest.mark.parametrize("M,N,K,epi", [(64, 64, 64, EPI_F32),          # test_gemm_f32: an X-epilogue
                                       (336, 512, 768, EPI_GELU),      # test_gemm_activation_bf16
                                       (80, 384, 128, EPI_QKV)])       # test_qkv_epilogue_layout: B 1, tokens 80, D 128
def test_gemm_bench(gpu, M, N, K, epi):
    assert epi != EPI_QKV or (N % 192 == 0 and M % 4 == 0)
    _timed_ok(gpu.op_gemm_bench(M, N, K, epi, iters=ITERS))


def test_attention_bench(gpu):
    _timed_ok(gpu.op_attention_bench(1, 80, 2, mode=2, iters=ITERS))         # test_attention: B 1, N 80, H 2


def test_nv12_benches(gpu):
    _timed_ok(gpu.op_nv12_to_rgb8_bench(64, 48, iters=ITERS))
    _timed_ok(gpu.op_nv12_to_rgb8_batch_bench(64, 48, 2, iters=ITERS))


def test_headconv_bench(gpu):
    _timed_ok(gpu.op_headconv_bench(iters=ITERS, **HEADCONV))


@pytest.mark.parametrize("fused", [True, False])
def test_headconv_ln_bench(gpu, fused):
    _timed_ok(gpu.op_headconv_ln_bench(fused=fused, iters=ITERS, **HEADCONV_LN))


def test_every_timer_refuses_zero_iterations_and_leaves_the_time_alone(gpu):
    L = gpu.ops_lib()
    h, n = HEADCONV, HEADCONV_LN
    calls = {
        "gemm": lambda us: L.vt_op_gemm_bench(0, 64, 64, 64, EPI_F32, -1, 0, us),
        "attention": lambda us: L.vt_op_attention_bench(0, 1, 80, 2, 2, 0, us),
        "nv12": lambda us: L.vt_op_nv12_to_rgb8_bench(0, 64, 48, 0, us),
        "nv12 batch": lambda us: L.vt_op_nv12_to_rgb8_batch_bench(0, 64, 48, 2, 0, us),
        "headconv": lambda us: L.vt_op_headconv_bf16(0, None, None, None, None, h["B"], h["grid"], h["Cin"], h["N"], 1, h["R"],
                                                     h["ncb"], 0, us),
        "headconv_ln": lambda us: L.vt_op_headconv_ln_bf16_lo(0, None, None, None, None, ctypes.c_float(1e-6), n["ntok"], n["off"],
                                                              None, None, None, n["B"], n["grid"], n["D"], n["N"], 1, n["R"],
                                                              n["ncb"], 0, us, 12),
    }
    for name, call in calls.items():
        us = ctypes.c_float(-7.5)
        assert call(ctypes.byref(us)) == -1, name          # VT_ERR_INVALID_ARG
        assert us.value == -7.5, name
