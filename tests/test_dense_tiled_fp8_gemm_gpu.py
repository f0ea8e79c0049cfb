"""GPU parity tests of the fp8-weight (e4m3, weight-only) MFMA tile GEMM for any row count (dense_tiled_fp8_gemm.hip) against
an fp64 reference on the same inputs: x . (w8 * s)^T + bias for the three scale shapes; the silu epilogue against oracle/ops.py.
Generators and tolerance: those of test_wstream_fp8_gemm_gpu.py (the decode kernel of the same contract)."""
import functools

import pytest
import torch

from oracle import ops as oo

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
E4M3 = torch.float8_e4m3fn
WIDE, NARROW = 256, 128
# (scale mode, tile, splits): the automatic choice, then each tile form at 1 split and at 2-3 (block scales: the narrow tile only)
FORMS = [(mode, None, None) for mode in ("tensor", "channel", "block128")]
FORMS += [(mode, tile, splits) for mode in ("tensor", "channel", "block128") for tile, splits in ((WIDE, 1), (NARROW, 1), (WIDE, 2), (NARROW, 3))
          if not (mode == "block128" and tile == WIDE)]


def _k():
    from sglang_amd import kernels

    return kernels


def _check(got, ref64):
    ref = ref64.float()
    err = (got.float() - ref).abs()
    tol = ref.abs() * 2.0 ** -8 + 1e-3
    assert bool((err <= tol).all()), f"max err {float(err.max())} (ref max {float(ref.abs().max())})"


def _w8(N, K, g):
    """Weights over the whole e4m3 code space (subnormals, +-448, -0), the two NaN codes replaced."""
    b = torch.randint(0, 256, (N, K), generator=g, dtype=torch.uint8)
    b[b == 0x7F] = 0x7E
    b[b == 0xFF] = 0x80
    return b.view(E4M3)


def _scale(mode, N, K, g):
    shape = {"tensor": (), "channel": (N,), "block128": ((N + 127) // 128, K // 128)}[mode]
    return (torch.rand(shape, generator=g) + 0.5) * 1e-2


def _deq64(w8, s):
    """fp64 w8 * s for any of the three scale shapes."""
    w = w8.double()
    if s.dim() == 2:
        s = s.repeat_interleave(128, 0).repeat_interleave(128, 1)[: w.shape[0]]
    elif s.dim() == 1:
        s = s[:, None]
    return w * s.double()


@functools.lru_cache(maxsize=None)
def _case(M, N, K, mode, bias=False):
    """(x, w8, scale, bias, fp64 reference), made once per shape."""
    g = torch.Generator().manual_seed(M * 131 + N + K + len(mode))
    x = (torch.randn((M, K), generator=g) * 0.5).to(BF)
    w8, s = _w8(N, K, g), _scale(mode, N, K, g)
    b = torch.randn(N, generator=g).to(BF) if bias else None
    ref = x.double() @ _deq64(w8, s).t()
    return x, w8, s, b, ref + b.double() if bias else ref


@pytest.mark.parametrize("M", [1, 129, 256, 257, 513, 700])
@pytest.mark.parametrize("N,K", [(16, 128), (176, 384), (4096, 1024)])
@pytest.mark.parametrize("mode,tile,splits", FORMS)
def test_dense_tiled_fp8_gemm_matches_fp64_reference(device, M, N, K, mode, tile, splits):
    if splits is not None and splits > K // 128:
        pytest.skip("more splits than K chunks")
    x, w8, s, _, ref = _case(M, N, K, mode)
    got = _k().dense_tiled_gemm(x.to(device), w8.to(device), w_scale=s.to(device), block_n=tile, splits=splits).cpu()
    _check(got, ref)


@pytest.mark.parametrize("mode", ["channel", "block128"])
def test_dense_tiled_fp8_gemm_bias_strides_and_untouched_padding(device, mode):
    M, N, K = 300, 1168, 896
    x, w8, s, b, ref = _case(M, N, K, mode, True)
    xfull = torch.zeros((M, K + 64), dtype=BF, device=device)
    xfull[:, :K] = x.to(device)
    wfull = torch.zeros((N, K + 32), dtype=torch.uint8, device=device).view(E4M3)
    wfull[:, :K] = w8.to(device)
    for splits in (1, 3):
        out_full = torch.zeros((M, N + 8), dtype=BF, device=device)
        _k().dense_tiled_gemm(xfull[:, :K], wfull[:, :K], bias=b.to(device), out=out_full[:, :N], splits=splits, w_scale=s.to(device))
        _check(out_full[:, :N].cpu(), ref)
        assert float(out_full[:, N:].abs().max()) == 0.0


@pytest.mark.parametrize("M", [129, 600])
@pytest.mark.parametrize("I", [16, 176])
@pytest.mark.parametrize("mode,tile", [("channel", WIDE), ("channel", NARROW), ("block128", NARROW)])
@pytest.mark.parametrize("splits", [1, 2])
def test_dense_tiled_fp8_silu_epilogue(device, M, I, mode, tile, splits):
    """silu_and_mul on the fp64 linear rounded to bf16: a value on a bf16 rounding boundary may land on the other side (one ulp of
    a gate around -5 moves silu by 2.5 %), as in the decode kernel's test."""
    x, w8, s, _, ref = _case(M, 2 * I, 384, mode)
    want = oo.silu_and_mul(ref.to(BF))
    got = _k().dense_tiled_gemm(x.to(device), w8.to(device), epilogue="silu_and_mul", block_n=tile, splits=splits, w_scale=s.to(device)).cpu()
    assert got.shape == (M, I)
    d = (got.float() - want.float()).abs()
    assert float((d > 0).float().mean()) < 0.03
    assert bool((d <= want.float().abs() * 2.0 ** -4 + 1e-3).all())


def test_dense_tiled_fp8_gemm_split_k_is_deterministic(device):
    x, w8, s, _, _ = _case(700, 4096, 1024, "block128")
    x, w8, s = x.to(device), w8.to(device), s.to(device)
    a = _k().dense_tiled_gemm(x, w8, w_scale=s, splits=3).clone()
    assert torch.equal(_k().dense_tiled_gemm(x, w8, w_scale=s, splits=3), a)


def test_dense_tiled_fp8_gemm_graph_replay_equals_eager(device):
    K_ = _k()
    x, w8, s, _, _ = _case(513, 4096, 1024, "channel")
    x, w8, s = x.to(device), w8.to(device), s.to(device)
    out = torch.empty((513, 4096), dtype=BF, device=device)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        K_.dense_tiled_gemm(x, w8, out=out, splits=2, w_scale=s)     # warm-up: this stream's workspace exists before the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            K_.dense_tiled_gemm(x, w8, out=out, splits=2, w_scale=s)
    torch.cuda.current_stream().wait_stream(stream)
    want = K_.dense_tiled_gemm(x, w8, splits=2, w_scale=s)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


def test_dense_tiled_fp8_gemm_rejections_raise_before_any_launch(device):
    K_ = _k()
    x = torch.zeros((300, 256), dtype=BF, device=device)
    w8 = torch.zeros((256, 256), dtype=E4M3, device=device)
    s = torch.ones(256, dtype=torch.float32, device=device)
    out = torch.full((300, 256), 7.0, dtype=BF, device=device)
    odd = torch.zeros((256, 264), dtype=torch.uint8, device=device).view(E4M3)[:, :256]      # rows 264 bytes apart
    bad = [dict(w=w8.view(torch.float8_e5m2), w_scale=s), dict(w=w8, w_scale=None),
           dict(w=w8, w_scale=torch.ones((2, 3), dtype=torch.float32, device=device)), dict(w=w8.to(BF), w_scale=s), dict(w=odd, w_scale=s)]
    for kw in bad:
        with pytest.raises((ValueError, RuntimeError)):
            K_.dense_tiled_gemm(x, kw.pop("w"), out=out, **kw)
    assert float((out.float() - 7.0).abs().max()) == 0.0
