"""kernels.logprobs_from_logits (sampling_logprobs.hip) and the sampler's return_logprob route against plain torch in fp64:
z = logits.double() / T.double(), z - logsumexp(z); expected order = stable descending sort of the raw logits.

Bars: integer outputs bit-exact; finite values within 1e-4 absolute (derived: |z| <= 128, so the fp32 division and the
subtraction of lse contribute <= 128 * 2^-24 ~ 8e-6 each, expf and the tree sum ~1e-6 on log S: < 2e-5 in all); -inf exact.
Achieved maximum on an MI355X (printed by every case, `pytest -s`): 9.2e-6 over the direct cases, 2.4e-5 in
the sampler test at the logit 200 / 0.7 below the row maximum."""
import functools
import math

import pytest
import torch

from sglang_amd import kernels
from sglang_amd.layers import sampler as sampler_mod
from sglang_amd.layers.sampler import LogitsProcessorOutput, Sampler, SamplingBatchInfo

pytestmark = pytest.mark.gpu
TOL = 1e-4
SHAPES = [(1, 7), (3, 4099), (5, 32000), (64, 128256), (130, 151936)]


def _temps(B, lo=0.3):
    return torch.tensor([(lo, 1.0, 2.5)[b % 3] for b in range(B)], dtype=torch.float32, device="cuda")


def _reference(x, t):
    z = x.double() if t is None else x.double() / t.double()[:, None]
    order = torch.sort(x.double(), dim=-1, descending=True, stable=True).indices[:, :kernels.logprobs_max_top()]
    return z - torch.logsumexp(z, -1, keepdim=True), order


@functools.lru_cache(maxsize=2)
def _case(B, V, dtype, pad, with_t):
    g = torch.Generator(device="cuda").manual_seed(B * 1000003 + V)
    x = (4 * torch.randn((B, V + pad), generator=g, device="cuda")).to(dtype)[:, :V]      # pad > 0: a view into a wider buffer
    n = min(32, V)
    planted = [lambda r: r.__setitem__(slice(None), 1.5),                                  # (b) constant row
               lambda r: r.__setitem__(slice(V - n, V), 22 + 0.25 * torch.arange(n, device="cuda")),   # (a) winners in the tail
               lambda r: r.__setitem__(slice(0, V, 2), -math.inf),                         # (d) half the row -inf
               lambda r: r.__setitem__([0, V - 1, V // 2, V // 2 + 1], 25.0)]              # (c) equal maxima across ranges
    for b in range(B - 1, 0, -1):                    # rows B-1, B-2, .. while there is room; row 0 stays random
        if planted:
            planted.pop()(x[b])
    t = _temps(B) if with_t else None
    ids = torch.randint(0, V, (B,), generator=g, device="cuda", dtype=torch.int32 if with_t else torch.int64)   # sampled / greedy ids
    lists = [([0, V - 1, V // 3, V // 3], None, [])[b % 3] for b in range(B)]
    return x, t, ids, lists, _reference(x, t)


def _check_values(got, want, what):
    got, want = got.double(), want.double()
    inf = torch.isinf(want)
    assert not torch.isnan(got).any() and torch.equal(got[inf], want[inf]), what
    err = (got[~inf] - want[~inf]).abs().max().item() if (~inf).any() else 0.0
    print(f"{what}: max abs error {err:.3g}")
    assert err <= TOL, (what, err)


@pytest.mark.parametrize("n_top", [0, 1, 20, "max"])      # (the top one varies fastest: the cases of one input share its reference)
@pytest.mark.parametrize("with_t", [True, False])
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B,V", SHAPES)
def test_logprobs_match_fp64(B, V, dtype, pad, with_t, n_top):
    n_top = kernels.logprobs_max_top() if n_top == "max" else n_top
    x, t, ids, lists, (lp, order) = _case(B, V, dtype, pad, with_t)
    chosen, top_val, top_idx, req_val = kernels.logprobs_from_logits(x, t, ids, n_top, lists)
    k = min(n_top, V)
    assert top_idx.shape == (B, n_top) and top_idx.dtype == torch.int32
    assert torch.equal(top_idx[:, :k].long(), order[:, :k]) and (top_idx[:, k:] == -1).all()
    tag = f"[{B}, {V}] {dtype} pad {pad} T {with_t} n_top {n_top}"
    _check_values(top_val[:, :k], lp.gather(1, order[:, :k]), tag + " top")
    _check_values(chosen, lp.gather(1, ids.long()[:, None])[:, 0], tag + " chosen")
    rows = torch.tensor([b for b, l in enumerate(lists) for _ in (l or ())], device="cuda")
    cols = torch.tensor([i for l in lists for i in (l or ())], device="cuda")
    _check_values(req_val, lp[rows, cols], tag + " listed")
    again = kernels.logprobs_from_logits(x, t, ids, n_top, lists)
    assert all(torch.equal(a, b) for a, b in zip((chosen, top_val, top_idx, req_val), again))     # deterministic


def test_graph_replays_equal_eager():
    B, V, n_top = 5, 32000, 5
    x = torch.zeros((B, V), dtype=torch.bfloat16, device="cuda")
    ids = torch.zeros(B, dtype=torch.int32, device="cuda")
    t = _temps(B)
    kernels.logprobs_from_logits(x, t, ids, n_top)                    # (library load, allocator warm-up)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = kernels.logprobs_from_logits(x, t, ids, n_top)
    for seed in (1, 2, 3):
        g = torch.Generator(device="cuda").manual_seed(seed)
        x.copy_(4 * torch.randn((B, V), generator=g, device="cuda"))
        ids.copy_(torch.randint(0, V, (B,), generator=g, device="cuda"))
        graph.replay()
        eager = kernels.logprobs_from_logits(x, t, ids, n_top)
        assert all(torch.equal(a, b) for a, b in zip(out[:3], eager[:3]))


@pytest.mark.parametrize("B,V", [(8, 32000), (64, 128256)])
@pytest.mark.parametrize("greedy", [True, False])
def test_sampler_return_logprob(B, V, greedy):
    g = torch.Generator(device="cuda").manual_seed(B + V)
    x = (4 * torch.randn((B, V), generator=g, device="cuda")).to(torch.bfloat16)
    far = 6                                          # a logit 200 below the row maximum: its fp32 probability underflows
    x[:, far] = x.float().max(-1).values - 200
    t = _temps(B, lo=0.7)
    tops = [(0, 2, 5, 20)[b % 4] for b in range(B)]
    lists = [([far, 0, V - 1], None, [])[b % 3] for b in range(B)]
    info = SamplingBatchInfo.greedy(B, "cuda")
    if not greedy:
        info = SamplingBatchInfo(t[:, None].clone(), torch.ones(B, device="cuda"), torch.full((B,), 50, dtype=torch.int32, device="cuda"),
                                 torch.zeros(B, device="cuda"), False, need_top_k_sampling=True,
                                 sampling_seed=torch.arange(B, dtype=torch.int64, device="cuda"))
    lp, order = _reference(x, None if greedy else t)
    plain_ids = Sampler()(LogitsProcessorOutput(x.clone()), info)
    before = dict(sampler_mod.served)
    out = LogitsProcessorOutput(x.clone())
    ids = Sampler()(out, info, return_logprob=True, top_logprobs_nums=tops, token_ids_logprobs=lists)
    assert torch.equal(ids, plain_ids) and sampler_mod.served["logprobs_from_logits"] == before["logprobs_from_logits"] + 1
    if not greedy and B == 64:                       # (the one-call sampler takes decode batches of wide rows only)
        assert sampler_mod.served["one_call_from_logits"] == before["one_call_from_logits"] + 1
    _check_values(out.next_token_logprobs, lp.gather(1, ids.long()[:, None])[:, 0], "sampler chosen")
    assert out.next_token_logprobs.shape == (B,)
    for b in range(B):
        assert out.next_token_top_logprobs_idx[b] == order[b, :tops[b]].tolist()
        assert out.next_token_token_ids_logprobs_idx[b] == (lists[b] or [])
        for got, cols in ((out.next_token_top_logprobs_val[b], order[b, :tops[b]].tolist()), (out.next_token_token_ids_logprobs_val[b], lists[b] or [])):
            assert len(got) == len(cols)
            if cols:
                assert math.isfinite(min(got))       # the parent commit's log(probs) is -inf at the far logit
                _check_values(torch.tensor(got), lp[b, cols].cpu(), f"sampler row {b}")
