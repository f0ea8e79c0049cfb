"""kernels.tree_accept_from_logits (speculative_sampling.hip) against the algorithm written literally: a Python loop over a float64
softmax on the CPU.  Accept decisions are compared exactly -- the seeded coins keep every comparison of the reference >= 1e-4 away
from its threshold (asserted on the reference alone; fp32 softmax error on these rows is ~1e-6) --, the bonus token by the
bracket of the float64 residual CDF F:  F[t-1] - eps <= u F[-1] <= F[t] + eps  with eps = 1e-5 F[-1] (ten times the ~1e-6
relative error of an fp32 expf, a divide and a tree-ordered sum over 128k terms) and a non-zero residual at t.
Over the cases every request accepts none, some and all of a strong path (strong edges: p ~ 1; every other edge a moderate p that
the coins decide)."""
import pytest
import torch

from sglang_amd import kernels

pytestmark = pytest.mark.gpu
TREES = {"single": [-1], "seven": [-1, 0, 0, 1, 1, 2, 5],
         "sixteen": [-1, 0, 0, 0, 0, 0, 1, 6, 7, 8, 9, 2, 2, 11, 3, 6]}      # node 0 has 5 children; 0-1-6-7-8-9-10 is a chain of depth 6
TEMPS = [0.0, 0.7, 1.3]


def tables(parents):
    nd = len(parents)
    nt = [min((i for i in range(nd) if parents[i] == j), default=-1) for j in range(nd)]
    ns = [min((i for i in range(j + 1, nd) if j and parents[i] == parents[j]), default=-1) for j in range(nd)]
    return nt, ns


def reference(logits, temps, cand, parents, uniform, ufinal, ts=1.0, ta=1.0):
    """Per request (accept_index, accept_len, last_node, residual CDF | None, bonus of a greedy request, decision margin)."""
    B, nd = cand.shape
    x = logits.double().cpu().view(B, nd, -1)
    out = []
    for b in range(B):
        greedy = temps is None or temps[b] <= 0
        p = None if greedy else torch.softmax(x[b] / float(temps[b]), -1)
        cur, path, margin = 0, [0], float("inf")
        coin = float(uniform[b, 0])
        while True:
            acc, rejected, nxt = 0.0, [], -1
            for c in (i for i in range(nd) if parents[i] == cur):
                tok = int(cand[b, c])
                if greedy:
                    take = tok == int(torch.argmax(x[b, cur]))
                else:
                    q = float(p[cur, tok])
                    acc += q
                    by_coin, by_single = coin <= acc / ta, q >= ts
                    take = by_coin or by_single
                    ma, ms = abs(coin - acc / ta), abs(q - ts)
                    margin = min(margin, max(ma if by_coin else 0, ms if by_single else 0) if take else min(ma, ms))
                if take:
                    nxt = c
                    break
                rejected.append(tok)
            if nxt < 0:
                break
            cur, coin = nxt, float(uniform[b, nxt])
            path.append(cur)
        cdf = None
        if not greedy:
            res = p[cur].clone()
            res[rejected] = 0.0
            cdf = res.cumsum(0)
        out.append((path + [-1] * (nd - len(path)), len(path) - 1, cur, cdf, int(torch.argmax(x[b, cur])), margin))
    return out


def check(got, ref, ufinal, nd):
    idx, n, bonus, last = (t.cpu() for t in got)
    for b, (path, length, cur, cdf, top, margin) in enumerate(ref):
        assert idx[b].tolist() == path and int(n[b]) == length and int(last[b]) == cur, (b, idx[b].tolist(), path)
        t = int(bonus[b])
        if cdf is None:
            assert t == top, (b, t, top)
            continue
        total, eps = float(cdf[-1]), 1e-5 * float(cdf[-1])
        lo, hi, u = (float(cdf[t - 1]) if t else 0.0), float(cdf[t]), float(ufinal[b]) * total
        print(f"request {b}: accepted {length}, bonus {t}, u F = {u:.9g} in [{lo:.9g}, {hi:.9g}]")
        assert hi > lo and lo - eps <= u <= hi + eps, (b, t, lo, u, hi)


def case(V, pad, dtype, tree, seed):
    """CPU inputs + their reference: request b gets strong edges down the first strong[b] levels of the tree's longest chain."""
    parents = TREES[tree]
    nd, B = len(parents), 3
    g = torch.Generator().manual_seed(seed + V)
    x = (4 * torch.randn((B * nd, V + pad), generator=g)).to(dtype)[:, :V]     # pad > 0: a view into a wider buffer
    cand = torch.randint(0, V, (B, nd), generator=g)
    uniform, ufinal = torch.rand((B, nd), generator=g), torch.rand(B, generator=g)
    chain = {"single": [0], "seven": [0, 1, 3], "sixteen": [0, 1, 6, 7, 8, 9, 10]}[tree]
    strong = [(len(chain) - 1, 1, 0), (1, 0, len(chain) - 1), (0, len(chain) - 1, 1)][seed % 3]     # strong edges per request
    top = x.float().max(dim=1)
    x[torch.arange(nd), top.indices[:nd]] = (top.values[:nd] + 2).to(dtype)    # the greedy request's rows: a unique maximum
    for b in range(B):
        for j in range(1, nd):
            on_chain = j in chain and chain.index(j) <= strong[b]
            x[b * nd + parents[j], cand[b, j]] = 30.0 if on_chain else float(top.values[b * nd + parents[j]]) + (0.5 if b else -1.0)
    ref = reference(x, TEMPS, cand, parents, uniform, ufinal)
    assert min(r[-1] for r in ref) >= 1e-4, [r[-1] for r in ref]            # the input condition of the exact comparison
    nt, ns = tables(parents)
    return (x, torch.tensor(TEMPS), cand, torch.tensor([nt] * B, dtype=torch.int32), torch.tensor([ns] * B, dtype=torch.int32),
            uniform, ufinal), ref, nd


@pytest.mark.parametrize("tree", list(TREES))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V,pad", [(1000, 0), (1002, 2), (32003, 0), (128256, 0)])
def test_tree_accept_matches_the_float64_loop(V, pad, dtype, tree):
    seed = list(TREES).index(tree) + (dtype == torch.float32)
    cpu, ref, nd = case(V, pad, dtype, tree, seed)
    x, t, cand, nt, ns, uniform, ufinal = (v.cuda() for v in cpu)
    got = kernels.tree_accept_from_logits(x, t, cand, nt, ns, uniform, ufinal)
    check(got, ref, cpu[-1], nd)
    again = kernels.tree_accept_from_logits(x, t, cand.to(torch.int32), nt, ns, uniform, ufinal)      # deterministic; int32 ids
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("ts,ta", [(1.0, 1.0), (0.3, 1.0), (1.0, 0.5)])
def test_rejected_tokens_never_come_back_and_thresholds_move_the_path(ts, ta):
    """Three requests with the same rows and coins, different uniform_final: node 0's first child holds the row's largest
    probability (~0.6) and loses against the coin 0.95, the second child is negligible.  Default thresholds: both rejected, the bonus
    token is never the first child's; threshold_single = 0.3 or threshold_acc = 0.5 accept that child."""
    parents, V, B = TREES["seven"], 32003, 3
    nd = len(parents)
    g = torch.Generator().manual_seed(5)
    x = (4 * torch.randn((nd, V), generator=g)).to(torch.bfloat16).repeat(B, 1)
    cand = torch.randint(0, V, (1, nd), generator=g).repeat(B, 1)
    x[0::nd, cand[0, 1]] = 0.7 * (float(torch.logsumexp(x[0].double() / 0.7, 0)) + 0.4)        # p ~ e^0.4 / (1 + e^0.4) = 0.6
    temps = torch.full((B,), 0.7)
    uniform = torch.full((B, nd), 0.95)
    ufinal = torch.tensor([0.01, 0.5, 0.99])
    ref = reference(x, temps, cand, parents, uniform, ufinal, ts, ta)
    p_first = float(torch.softmax(x[0].double() / 0.7, -1)[cand[0, 1]])
    assert 0.4 < p_first < 0.9 and int(torch.argmax(x[0])) == int(cand[0, 1]) and min(r[-1] for r in ref) >= 1e-4, p_first
    assert all((r[1] == 0) == (ts == 1.0 and ta == 1.0) for r in ref), [r[0] for r in ref]
    nt, ns = tables(parents)
    got = kernels.tree_accept_from_logits(x.cuda(), temps.cuda(), cand.cuda(), torch.tensor([nt] * B, dtype=torch.int32).cuda(),
                                          torch.tensor([ns] * B, dtype=torch.int32).cuda(), uniform.cuda(), ufinal.cuda(), ts, ta)
    check(got, ref, ufinal, nd)
    if ts == 1.0 and ta == 1.0:
        assert int(cand[0, 1]) not in got[2].tolist() and int(cand[0, 2]) not in got[2].tolist()


def test_greedy_ties_go_to_the_lowest_column():
    parents, V = TREES["seven"], 32003
    nd = len(parents)
    x = torch.randn((nd, V), generator=torch.Generator().manual_seed(3))
    x[:, [5, V - 3]] = 40.0                                                 # the same maximum in the first and the last range
    cand = torch.tensor([[0, V - 3, 5, 7, 8, 5, V - 3]])
    nt, ns = tables(parents)
    got = kernels.tree_accept_from_logits(x.cuda(), None, cand.cuda(), torch.tensor([nt], dtype=torch.int32).cuda(),
                                          torch.tensor([ns], dtype=torch.int32).cuda())
    assert got[0].tolist() == [[0, 2, 5, -1, -1, -1, -1]] and got[1].tolist() == [2] and got[2].tolist() == [5] and got[3].tolist() == [5]
    check(got, reference(x, None, cand, parents, torch.zeros(1, nd), torch.zeros(1)), torch.zeros(1), nd)


def test_argument_errors_are_raised_before_any_launch():
    x = torch.zeros((3 * 65, 100), device="cuda")
    tb = torch.full((3, 65), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="nd"):
        kernels.tree_accept_from_logits(x, None, torch.zeros((3, 65), dtype=torch.int64, device="cuda"), tb, tb)
    with pytest.raises(ValueError, match="contiguous"):
        kernels.tree_accept_from_logits(x[:24], None, torch.zeros((8, 3), dtype=torch.int64, device="cuda").t(), tb[:, :8], tb[:, :8])
