"""Host side of the fp8-weight GEMM: the quantiser, and the bf16 decomposition policy unchanged by the weight-size parameter."""
import pytest
import torch

from sglang_amd import kernels as K


@pytest.mark.parametrize("block", [None, 128])
def test_quantize_fp8_weight_round_trips_within_half_a_step(block):
    g = torch.Generator().manual_seed(3)
    w = (torch.randn((200, 256), generator=g) * 0.02).to(torch.bfloat16)
    w[5] = 0                                        # an all-zero row
    w[128:, 128:] = 0                               # an all-zero block
    w8, s = K.quantize_fp8_weight(w, block)
    assert w8.dtype == torch.float8_e4m3fn and s.dtype == torch.float32
    assert tuple(s.shape) == ((200,) if block is None else (2, 2))
    full = s[:, None] if block is None else s.repeat_interleave(128, 0).repeat_interleave(128, 1)[:200]
    assert bool((s > 0).all()) and float(s[5] if block is None else s[1, 1]) == 1.0
    q = w.float() / full
    # e4m3 spacing at |q|: 2^(floor(log2 |q|) - 3), 2^-9 below the smallest normal 2^-6; round to nearest = half of it
    step = torch.exp2(torch.floor(torch.log2(q.abs().clamp_min(2.0 ** -6))) - 3)
    assert bool(((w8.float() - q).abs() <= step / 2 * (1 + 1e-6)).all())
    assert float(w8.float().abs().max()) <= 448.0 and bool((w8.float()[5] == 0).all())


def test_bf16_decomposition_ignores_the_weight_size_parameter():
    for M in (1, 16, 64, 96, 128):
        for N, Kd in ((6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336), (128256, 4096), (4864, 896), (1280, 8192)):
            for comb, silu in ((False, False), (True, False), (True, True)):
                assert K.choose_wstream_config(M, N, Kd, comb, silu) == K.choose_wstream_config(M, N, Kd, comb, silu, 2)
                assert K.choose_wstream_decomposition(M, N, Kd, comb, silu) == K.choose_wstream_decomposition(M, N, Kd, comb, silu, 2)
    # the figures the bf16 kernel's sweep fixed (tests/test_wstream_gemm_gpu.py): two-tile waves for the wide one-split launches
    assert K.choose_wstream_decomposition(64, 128256, 4096)[1] == 2 and K.choose_wstream_decomposition(64, 28672, 4096)[1] == 2
    assert K.wstream_preferred(128, 28672, 4096) is False and K.wstream_preferred(128, 28672, 4096, 1) is True
