"""GPU parity tests of the dense MFMA tile GEMM for 129..512-row decode batches (dense_tiled_gemm.hip) against an fp64
reference on the same bf16 inputs (F.linear, srt/layers/linear.py:1596-1660) and the oracle's silu_and_mul
(activation.py:141-143).  Bars as in test_wstream_gemm_gpu.py."""
import functools

import pytest
import torch

from oracle import ops as oo

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NARROW, WIDE = 64, 128


def _k():
    from sglang_amd import kernels

    return kernels


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """(x, w, fp64 x . w^T) on the host, computed once per shape and never modified."""
    g = torch.Generator().manual_seed(M * 131 + N + K)
    x = (torch.randn((M, K), generator=g) * 0.5).to(BF)
    w = (torch.randn((N, K), generator=g) * 0.05).to(BF)
    return x, w, x.double() @ w.double().t()


def _check(got, ref64):
    ref = ref64.float()
    err = (got.float() - ref).abs()
    tol = ref.abs() * 2.0 ** -8 + 1e-3
    assert bool((err <= tol).all()), f"max err {float(err.max())} (ref max {float(ref.abs().max())})"


@pytest.mark.parametrize("M", [129, 255, 256, 257, 400, 512])
@pytest.mark.parametrize("N,K", [(16, 128), (176, 384), (4096, 1024)])
@pytest.mark.parametrize("block_n,splits", [(None, None), (NARROW, 1), (WIDE, 1), (NARROW, 3), (WIDE, 2)])
def test_dense_tiled_gemm_matches_fp64_reference(device, M, N, K, block_n, splits):
    if splits is not None and splits > K // 128:
        pytest.skip("more splits than K chunks")
    x, w, ref = _case(M, N, K)
    got = _k().dense_tiled_gemm(x.to(device), w.to(device), block_n=block_n, splits=splits).cpu()
    _check(got, ref)


def test_dense_tiled_gemm_bias_strides_and_untouched_padding(device):
    g = torch.Generator().manual_seed(5)
    M, N, K = 300, 1136, 896
    xfull = torch.randn((M, K + 64), generator=g).to(BF).to(device)
    x = xfull[:, :K]
    w = (torch.randn((N, K), generator=g) * 0.05).to(BF).to(device)
    b = torch.randn(N, generator=g).to(BF).to(device)
    ref = x.cpu().double() @ w.cpu().double().t() + b.cpu().double()
    for splits in (1, 2):
        out_full = torch.zeros((M, N + 8), dtype=BF, device=device)
        _k().dense_tiled_gemm(x, w, bias=b, out=out_full[:, :N], splits=splits)
        _check(out_full[:, :N].cpu(), ref)
        assert float(out_full[:, N:].abs().max()) == 0.0


def test_dense_tiled_gemm_split_k_is_deterministic(device):
    x, w, _ = _case(400, 4096, 1024)
    x, w = x.to(device), w.to(device)
    a = _k().dense_tiled_gemm(x, w, block_n=NARROW, splits=3).clone()
    b = _k().dense_tiled_gemm(x, w, block_n=NARROW, splits=3)
    assert torch.equal(a, b)


@pytest.mark.parametrize("M", [129, 300, 512])
@pytest.mark.parametrize("I", [16, 176])
@pytest.mark.parametrize("splits", [1, 2])
def test_dense_tiled_silu_epilogue(device, M, I, splits):
    x, w, ref = _case(M, 2 * I, 256)
    want = oo.silu_and_mul(ref.to(BF))
    got = _k().dense_tiled_gemm(x.to(device), w.to(device), epilogue="silu_and_mul", splits=splits).cpu()
    assert got.shape == (M, I)
    d = (got.float() - want.float()).abs()
    # same rounding points; the fp32 accumulation differs from the rounded fp64 sum in the last place, so a few gate / up
    # values cross a bf16 rounding boundary (one ulp of a gate around -5 moves silu(gate) by 2.5 %)
    assert float((d > 0).float().mean()) < 0.02
    assert bool((d <= want.float().abs() * 2.0 ** -4 + 1e-3).all())


def test_dense_tiled_gemm_graph_replay_equals_eager(device):
    K_ = _k()
    x0, w, _ = _case(400, 4096, 1024)
    x1 = _case(257, 4096, 1024)[0]
    w = w.to(device)
    x = x0.to(device)
    out = torch.empty((400, 4096), dtype=BF, device=device)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        K_.dense_tiled_gemm(x, w, out=out, splits=2)           # warm-up: this stream's workspace exists before the capture
        s.synchronize()
        with torch.cuda.graph(graph, stream=s):
            K_.dense_tiled_gemm(x, w, out=out, splits=2)
    torch.cuda.current_stream().wait_stream(s)
    x[:257].copy_(x1.to(device))
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, K_.dense_tiled_gemm(x, w, splits=2))
