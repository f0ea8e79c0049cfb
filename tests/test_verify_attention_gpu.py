"""verify_attention.hip (split-KV tree-verify attention) against a plain fp64 attention.  Every case: scattered pool slots,
non-trivial req_pool_indices, q a strided view into a qkv row, mask bytes under the prefix columns ZERO (a kernel that read
them would mask the whole prefix).  Bar: atol = rtol = 4e-3, the bar of the project's random-case attention tests.
Achieved on an MI355X: see the printed maxima (recorded in DESIGN.md)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
BF, TOL = torch.bfloat16, 4e-3
POOLS = [5, 2, 7, 1]


def _tree_mask(e, g):
    """Ancestor matrix of a random tree (parents[j] < j): row j sees its ancestors and itself."""
    anc = torch.eye(e, dtype=torch.bool)
    for j in range(1, e):
        anc[j] |= anc[int(torch.randint(0, j, (1,), generator=g))]
    return anc


@functools.lru_cache(maxsize=None)
def _case(D, Hq, Hkv, prefixes, extends, masked=True, seed=0, planted=-1, ctx=None):
    """Inputs (CPU) for a ragged batch.  r2t rows are filled over the whole context so that lengths may change later."""
    g = torch.Generator().manual_seed(seed)
    B, T = len(prefixes), sum(extends)
    ctx = ctx or max(p + e for p, e in zip(prefixes, extends))
    slots = torch.randperm(B * ctx + 3, generator=g)
    r2t = torch.zeros((8, ctx), dtype=torch.int32)
    for b in range(B):
        r2t[POOLS[b]] = slots[b * ctx:(b + 1) * ctx].int()
    K = torch.randn((B * ctx + 3, Hkv, D), generator=g).to(BF)
    V = torch.randn((B * ctx + 3, Hkv, D), generator=g).to(BF)
    qkv = torch.randn((T, (Hq + 2 * Hkv) * D), generator=g).to(BF)
    if planted >= 0:       # one large logit late in the context: a K row parallel to q, scaled up
        K[r2t[POOLS[0], planted].long()] = (qkv[0, :D].float() * 3.0).to(BF)
    qo = torch.tensor([0] + list(extends)).cumsum(0).int()
    return dict(D=D, Hq=Hq, Hkv=Hkv, B=B, T=T, r2t=r2t, K=K, V=V, qkv=qkv, qo=qo, extends=extends, masked=masked,
                trees=[_tree_mask(e, g) for e in extends])


def _lens(c, prefixes):
    """Lengths, flat mask and its offsets for these prefixes (the mask bytes under the prefix stay zero)."""
    seq = [p + e for p, e in zip(prefixes, c["extends"])]
    blocks = []
    for p, e, s, tree in zip(prefixes, c["extends"], seq, c["trees"]):
        m = torch.zeros((e, s), dtype=torch.uint8)
        m[:, p:] = tree
        blocks.append(m.flatten())
    mip = torch.tensor([0] + [b.numel() for b in blocks]).cumsum(0)
    return torch.tensor(seq).int(), torch.tensor(prefixes).int(), torch.cat(blocks), mip


def _reference(c, prefixes):
    D, Hq, group = c["D"], c["Hq"], c["Hq"] // c["Hkv"]
    q = c["qkv"][:, :Hq * D].view(-1, Hq, D).double()
    out = torch.zeros((c["T"], Hq, D), dtype=torch.float64)
    for b, (p, e) in enumerate(zip(prefixes, c["extends"])):
        rows = c["r2t"][POOLS[b], :p + e].long()
        k, v = (x[rows].double().repeat_interleave(group, 1) for x in (c["K"], c["V"]))
        vis = torch.ones((e, p + e), dtype=torch.bool)
        vis[:, p:] = c["trees"][b] if c["masked"] else torch.tril(torch.ones((e, e), dtype=torch.bool))
        s = torch.einsum("ehd,shd->hes", q[c["qo"][b]:c["qo"][b + 1]], k) * D ** -0.5
        pr = torch.softmax(s.masked_fill(~vis, float("-inf")), -1)
        out[c["qo"][b]:c["qo"][b + 1]] = torch.einsum("hes,shd->ehd", pr, v)
    return out


def _device_args(c, prefixes, device, splits):
    from sglang_amd import kernels

    seq, pre, mask, mip = (x.to(device) for x in _lens(c, prefixes))
    q = c["qkv"].to(device)[:, :c["Hq"] * c["D"]].view(-1, c["Hq"], c["D"])
    ws = kernels.verify_workspace(c["T"], c["Hq"], c["D"], splits, device) if splits > 1 else (None, None)
    a = dict(q=q, out=torch.full((c["T"], c["Hq"], c["D"]), float("nan"), dtype=BF, device=device), K=c["K"].to(device),
             V=c["V"].to(device), r2t=c["r2t"].to(device), pools=torch.tensor(POOLS[:c["B"]], device=device), seq=seq, pre=pre,
             qo=c["qo"].to(device), mask=mask if c["masked"] else None, mip=mip if c["masked"] else None, ws=ws, splits=splits)
    return a


def _launch(c, a):
    from sglang_amd import kernels

    return kernels.verify_attention(a["q"], a["out"], a["K"], a["V"], a["r2t"], a["pools"], a["seq"], a["pre"], a["qo"], max(c["extends"]),
                                    c["D"] ** -0.5, custom_mask=a["mask"], mask_indptr=a["mip"], num_splits=a["splits"],
                                    ws_acc=a["ws"][0], ws_ml=a["ws"][1])


def _check(got, want, what):
    err = (got.double().cpu() - want).abs()
    print(f"{what}: max abs err {float(err.max()):.3e}")
    assert bool((err <= TOL + TOL * want.abs()).all()), (what, float(err.max()))


@pytest.mark.parametrize("splits", [1, 2, 5])
@pytest.mark.parametrize("nd", [1, 3, 8, "max"])
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (8, 2), (8, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_tree_mask_ragged_batch(device, D, Hq, Hkv, nd, splits):
    """Prefixes {0, 1, 63, 130}: the draft tokens sit inside one tile, straddle a tile boundary and a split boundary; five
    splits leave at least one split of every request without tiles."""
    nd = 64 // (Hq // Hkv) if nd == "max" else nd
    prefixes = (0, 1, 63, 130)
    c = _case(D, Hq, Hkv, prefixes, (nd,) * 4)
    out = _launch(c, _device_args(c, prefixes, device, splits))
    _check(out, _reference_cached(D, Hq, Hkv, prefixes, (nd,) * 4), (D, Hq, Hkv, nd, splits))


@functools.lru_cache(maxsize=None)
def _reference_cached(D, Hq, Hkv, prefixes, extends, masked=True, seed=0, planted=-1):
    return _reference(_case(D, Hq, Hkv, prefixes, extends, masked, seed, planted), prefixes)


@pytest.mark.parametrize("splits", [1, 3])
def test_causal_rule_without_a_mask(device, splits):
    prefixes, extends = (70, 0, 129), (1, 2, 5)
    c = _case(128, 8, 2, prefixes, extends, False, 1)
    out = _launch(c, _device_args(c, prefixes, device, splits))
    _check(out, _reference_cached(128, 8, 2, prefixes, extends, False, 1), ("causal", splits))


def test_long_context_running_maximum_rises_late(device):
    c = _case(128, 8, 2, (4099,), (6,), True, 2, 3500)
    out = _launch(c, _device_args(c, (4099,), device, 7))
    _check(out, _reference_cached(128, 8, 2, (4099,), (6,), True, 2, 3500), "long context, 7 splits")


def test_same_call_twice_is_bitwise_equal(device):
    c = _case(128, 8, 2, (0, 1, 63, 130), (8,) * 4)
    a, b = (_launch(c, _device_args(c, (0, 1, 63, 130), device, 5)) for _ in range(2))
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_graph_replay_follows_lengths_changed_in_place(device):
    """Captured at one set of lengths, replayed (three times) at a shorter AND a longer one inside the captured context."""
    first, second = (100, 40, 200), (37, 130, 260)
    c = _case(128, 8, 2, first, (4,) * 3, True, 3, -1, 300)
    a = _device_args(c, first, device, 3)
    buf = torch.zeros(c["T"] * 300, dtype=torch.uint8, device=device)          # the persistent mask buffer the graph reads
    buf[:a["mask"].numel()] = a["mask"]
    a["mask"] = buf
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _launch(c, a)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _launch(c, a)
    seq, pre, mask, mip = (x.to(device) for x in _lens(c, second))
    a["seq"].copy_(seq); a["pre"].copy_(pre); a["mip"].copy_(mip); a["mask"][:mask.numel()].copy_(mask)
    want = _reference(c, second)
    for i in range(3):
        a["out"].fill_(float("nan"))
        graph.replay()
        _check(a["out"], want, ("graph replay", i))


@pytest.mark.parametrize("kind,match", [("rows", "exceeds 64 rows"), ("dim", "head_dim=96"), ("ws", "needs the ws_acc")])
def test_argument_errors_raise_with_the_librarys_message(device, kind, match):
    D = 96 if kind == "dim" else 64
    nd = 9 if kind == "rows" else 2
    c = _case(D, 8, 1, (5,), (nd,))
    a = _device_args(c, (5,), device, 1)
    a["splits"] = 2 if kind == "ws" else 1
    with pytest.raises(RuntimeError, match=match):
        _launch(c, a)
