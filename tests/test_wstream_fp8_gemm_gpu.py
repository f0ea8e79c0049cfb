"""GPU parity tests of the fp8-weight (e4m3, weight-only) weight-streaming decode GEMM (wstream_fp8_gemm.hip) against an fp64
reference on the same inputs: (x . w8^T) * s + bias, or the 128 x 128 block form; the fused epilogues against oracle/ops.py."""
import functools

import pytest
import torch

from oracle import ops as oo

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
E4M3 = torch.float8_e4m3fn


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


def _blocked(x):
    M, K = x.shape
    return x.view(M, K // 128, 128).permute(1, 0, 2).contiguous()


@pytest.mark.parametrize("M", [1, 16, 17, 64, 65, 128])
@pytest.mark.parametrize("N,K", [(16, 128), (112, 384), (4864, 896), (4096, 4096)])
@pytest.mark.parametrize("mode", ["tensor", "channel", "block128"])
@pytest.mark.parametrize("nw,splits", [(None, None), (4, 1), (5, 2), (8, 3)])
def test_fp8_gemm_matches_fp64_reference(device, M, N, K, mode, nw, splits):
    if splits is not None and splits > K // 128:
        pytest.skip("more splits than K chunks")
    if M > 64 and nw is not None and nw > 5:
        pytest.skip("beyond 64 rows only 4- and 5-wave groups are used")
    x, w8, s, _, ref = _case(M, N, K, mode)
    got = _k().wstream_gemm(x.to(device), w8.to(device), w_scale=s.to(device), waves_per_group=nw, splits=splits).cpu()
    _check(got, ref)


@pytest.mark.parametrize("M", [3, 64])
def test_fp8_gemm_bias_strides_and_untouched_padding(device, M):
    N, K = 1152, 896
    x, w8, s, b, ref = _case(M, N, K, "channel", True)
    xfull = torch.zeros((M, K + 64), dtype=BF, device=device)
    xfull[:, :K] = x.to(device)
    for splits in (1, 3):
        out_full = torch.zeros((M, N + 8), dtype=BF, device=device)
        _k().wstream_gemm(xfull[:, :K], w8.to(device), bias=b.to(device), out=out_full[:, :N], splits=splits, w_scale=s.to(device))
        _check(out_full[:, :N].cpu(), ref)
        assert float(out_full[:, N:].abs().max()) == 0.0


@pytest.mark.parametrize("M", [3, 64])
@pytest.mark.parametrize("mode", ["channel", "block128"])
def test_fp8_gemm_silu_and_add_rmsnorm_epilogues(device, M, mode):
    """The epilogues on the fp64 linear rounded to bf16, the way the bf16 tests compare against the unfused ops: a value on a bf16
    rounding boundary may land on the other side (one ulp of a gate around -5 moves silu by 2.5 %; one ulp of the normed output)."""
    K_ = _k()
    I, K = 896, 1024
    x, w8, s, _, ref = _case(M, 2 * I, K, mode)
    want = oo.silu_and_mul(ref.to(BF))
    for splits in (1, 2):
        got = K_.wstream_gemm(x.to(device), w8.to(device), epilogue="silu_and_mul", splits=splits, w_scale=s.to(device)).cpu()
        d = (got.float() - want.float()).abs()
        assert float((d > 0).float().mean()) < 0.03
        assert bool((d <= want.float().abs() * 2.0 ** -4 + 1e-3).all())
    g = torch.Generator().manual_seed(M)
    res = torch.randn((M, 2 * I), generator=g).to(BF)
    nrm = (torch.rand(2 * I, generator=g) + 0.5).to(BF)
    want_y, want_res = oo.fused_add_rmsnorm(ref.to(BF), res.clone(), nrm, 1e-5)
    res2 = res.to(device)
    got = K_.wstream_gemm(x.to(device), w8.to(device), epilogue="add_rmsnorm", residual=res2, norm_weight=nrm.to(device), eps=1e-5,
                          splits=2, w_scale=s.to(device)).cpu()
    # h = bf16(linear) may sit one bf16 ulp (<= 2^-7 |h|) from the reference's on a few elements; the sum and the output round once more
    h = ref.to(BF).float().abs()
    dt_max = h * 2.0 ** -7 + want_res.float().abs() * 2.0 ** -7
    dr = (res2.cpu().float() - want_res.float()).abs()
    assert float((dr > 0).float().mean()) < 0.02 and bool((dr <= dt_max + 1e-6).all())
    rs = torch.rsqrt(want_res.float().pow(2).mean(dim=1, keepdim=True) + 1e-5)
    d = (got.float() - want_y.float()).abs()
    assert bool((d <= dt_max * rs * nrm.float().abs() + want_y.float().abs() * 2.0 ** -6 + 1e-6).all())


@pytest.mark.parametrize("M", [3, 64])
@pytest.mark.parametrize("N,K,mode,splits", [(4096, 4096, "block128", None), (256, 384, "channel", 1), (1024, 896, "block128", 2)])
def test_fp8_gemm_chunk_major_activations_change_no_bit(device, M, N, K, mode, splits):
    K_ = _k()
    x, w8, s, _, _ = _case(M, N, K, mode)
    x, w8, s = x.to(device), w8.to(device), s.to(device)
    nw, s_auto = K_.choose_wstream_config(M, N, K, False, False, 1)
    sp = splits or s_auto
    want = K_.wstream_gemm(x, w8, w_scale=s, waves_per_group=nw, splits=sp)
    assert torch.equal(K_.wstream_gemm(_blocked(x), w8, w_scale=s, waves_per_group=nw, splits=sp), want)
    got_out = K_.wstream_gemm(x, w8, w_scale=s, waves_per_group=nw, splits=sp, out_blocked=True)
    assert got_out.shape == (N // 128, M, 128) and torch.equal(K_.unblock(got_out), want)


@pytest.mark.parametrize("M", [3, 64])
@pytest.mark.parametrize("N,K", [(64, 256), (4096, 4096)])
@pytest.mark.parametrize("mode", ["channel", "block128"])
def test_fp8_gemm_two_tiles_per_wave(device, M, N, K, mode):
    x, w8, s, _, ref = _case(M, N, K, mode)
    for nw, splits in ((2, 1), (4, 2)):
        got = _k().wstream_gemm(x.to(device), w8.to(device), w_scale=s.to(device), waves_per_group=nw, splits=splits, tiles_per_wave=2)
        _check(got.cpu(), ref)


def test_fp8_gemm_split_k_is_deterministic(device):
    x, w8, s, _, _ = _case(64, 4096, 4096, "block128")
    x, w8, s = x.to(device), w8.to(device), s.to(device)
    a = _k().wstream_gemm(x, w8, w_scale=s, splits=8, waves_per_group=8).clone()
    assert torch.equal(_k().wstream_gemm(x, w8, w_scale=s, splits=8, waves_per_group=8), a)


@pytest.mark.parametrize("M", [1, 17])
@pytest.mark.parametrize("Hq,Hkv,D,K", [(4, 2, 64, 256), (32, 8, 128, 4096)])
@pytest.mark.parametrize("fp8_pool", [False, True])
def test_fp8_qkv_rope_store_equals_unfused_ops(device, M, Hq, Hkv, D, K, fp8_pool):
    """fp8 qkv GEMM + combine(rope, KV store) == the GEMM's own bf16 output -> rotary_embedding (forward_native) -> store_kv_cache;
    that GEMM output is checked against the fp64 reference first."""
    K_ = _k()
    N = (Hq + 2 * Hkv) * D
    x, w8, s, b, ref = _case(M, N, K, "channel", True)
    x, w8, s, b = x.to(device), w8.to(device), s.to(device), b.to(device)
    g = torch.Generator().manual_seed(M + Hq)
    cache = oo.cos_sin_cache(oo.rope_inv_freq(D, 10000.0), 512).to(BF)
    positions = torch.randint(0, 512, (M,), generator=g)
    slots = 64
    loc = (torch.randperm(slots - 1, generator=g)[:M] + 1).to(device)
    splits = 2 if K >= 512 else 1
    qkv = K_.wstream_gemm(x, w8, bias=b, splits=splits, w_scale=s).cpu()             # same split count: same accumulators
    _check(qkv, ref)
    q_ref, k_ref, v_ref = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    q_ref, k_ref = oo.rotary_embedding(positions, q_ref.clone(), k_ref.clone(), D, cache, True)
    dt = torch.uint8 if fp8_pool else BF
    fmt = dict(kv_fp8=True, k_scale=0.75, v_scale=1.5) if fp8_pool else {}
    kc_ref, vc_ref = torch.zeros((slots, Hkv, D), dtype=dt, device=device), torch.zeros((slots, Hkv, D), dtype=dt, device=device)
    K_.store_kv_cache(k_ref.reshape(M, -1).contiguous().to(device), v_ref.contiguous().to(device), kc_ref, vc_ref, loc,
                      num_kv_heads=Hkv, head_dim=D, **fmt)
    kc, vc = torch.zeros_like(kc_ref), torch.zeros_like(vc_ref)
    q = K_.wstream_qkv_rope(x, w8, b, positions.to(device), cache.to(device), Hq, Hkv, D, kc, vc, loc, splits=splits, w_scale=s, **fmt)
    assert torch.equal(q.cpu(), q_ref.reshape(M, -1))
    assert torch.equal(kc.cpu(), kc_ref.cpu()) and torch.equal(vc.cpu(), vc_ref.cpu())
    assert int((kc.cpu().view(torch.uint8) != 0).sum()) > 0


def test_fp8_gemm_rejections_raise_before_any_launch(device):
    K_ = _k()
    x = torch.zeros((4, 256), dtype=BF, device=device)
    w8 = torch.zeros((256, 256), dtype=E4M3, device=device)
    s = torch.ones(256, dtype=torch.float32, device=device)
    out = torch.full((4, 256), 7.0, dtype=BF, device=device)
    bad = [dict(w=w8.view(torch.float8_e5m2), w_scale=s), dict(w=w8, w_scale=None), dict(w=w8, w_scale=s.to(BF)),
           dict(w=w8, w_scale=torch.ones((2, 3), dtype=torch.float32, device=device)),
           dict(w=w8.to(BF), w_scale=s), dict(x=x[:, :192], w=w8[:, :192], w_scale=s)]
    for kw in bad:
        with pytest.raises((ValueError, RuntimeError)):       # the wrapper's own checks, or the C side's (K = 192)
            K_.wstream_gemm(kw.pop("x", x), kw.pop("w"), out=out, **kw)
    assert float((out.float() - 7.0).abs().max()) == 0.0
