"""ngram_draft.hip against the drafting rule of include/sglang_amd.h, restated below on host lists: tree_tokens, parents and num_real
must be EQUAL, for every split count, on rows whose lengths sit on both sides of every tile edge; ngram_commit against a Python loop;
the argument errors (host-side checks: no GPU needed)."""
import pytest
import torch

TILE = 1024                                                 # sgl_amd_ngram_draft_tile(), asserted below
LENS = [1, 2, 8, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 5000]
ROWS = [9, 3, 7, 0, 5, 2, 10, 4]                            # non-identity req_pool_indices into an 11-row table
WIDTH = 5004


def ngram_draft_reference(h, nd, max_n, min_n, branches, depth, window, pad_token):
    L = len(h)
    tokens, parents = [h[-1]], [-1]
    lo = max(0, L - 1 - window) if window > 0 else 0
    cand = []
    for p in range(lo, L - 1):
        m = 0
        while m < max_n and p - m >= 0 and h[p - m] == h[L - 1 - m]:
            m += 1
        if m >= min_n:
            cand.append((m, p))
    cand.sort(reverse=True)
    for m, p in cand[:branches]:
        cur = 0
        for tok in h[p + 1:min(p + 1 + depth, L)]:
            nxt = next((j for j in range(len(tokens)) if parents[j] == cur and tokens[j] == tok), -1)
            if nxt < 0:
                if len(tokens) == nd:
                    break
                tokens.append(tok); parents.append(cur); nxt = len(tokens) - 1
            cur = nxt
    num_real = len(tokens)
    while len(tokens) < nd:
        parents.append(len(tokens) - 1); tokens.append(pad_token)
    return tokens, parents, num_real


# (vocab, nd, max_n, min_n, branches, depth, window)
CASES = [(v, nd, 4, 1, 4, None, 0) for v in (1, 3, 50) for nd in (1, 8, 64)] + [
    (3, 64, 8, 3, 8, 5, 100),                               # the window cuts mid-tile, compares reach in front of it, min_n filters
    (3, 4, 4, 1, 4, 8, 0),                                  # the node budget cuts a continuation
]


@pytest.mark.gpu
@pytest.mark.parametrize("vocab,nd,max_n,min_n,branches,depth,window", CASES)
def test_draft_tree_equals_the_rule_for_every_split_count(device, vocab, nd, max_n, min_n, branches, depth, window):
    from sglang_amd import kernels as K

    assert K.ngram_draft_tile() == TILE and K.ngram_draft_max_ngram() == 8
    g = torch.Generator().manual_seed(vocab * 100 + nd)
    table = torch.randint(0, max(vocab, 2), (11, WIDTH), generator=g).to(torch.int32)     # garbage behind lens, in vocabulary
    hist = [torch.randint(0, vocab, (L,), generator=g).tolist() for L in LENS]
    for row, h in zip(ROWS, hist):
        table[row, :len(h)] = torch.tensor(h, dtype=torch.int32)
    d = nd - 1 if depth is None else depth
    want = [ngram_draft_reference(h, nd, max_n, min_n, branches, max(1, d), window, 77) for h in hist]
    if vocab == 3 and nd >= 8:
        assert any(w[1][:w[2]].count(0) > 1 for w in want), "no case with a branching tree"
    args = (table.to(device), torch.tensor(ROWS, device=device), torch.tensor(LENS, dtype=torch.int32, device=device), nd)
    for splits in (1, 3, 64):
        tt, par, nr = K.ngram_draft_tree(*args, max_ngram=max_n, min_ngram=min_n, branches=branches, depth=depth, window=window,
                                         pad_token=77, num_splits=splits)
        got = list(zip(tt.tolist(), par.tolist(), nr.tolist()))
        assert got == [tuple(w) for w in want], (splits, [L for L, a, w in zip(LENS, got, want) if a != tuple(w)])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_commit_appends_the_accepted_path_and_stops_at_the_width(device, dtype):
    from sglang_amd import kernels as K

    nd, width = 8, 16
    g = torch.Generator().manual_seed(5)
    table = torch.randint(0, 1000, (6, width), generator=g).to(torch.int32)
    rows, lens, acc = [4, 1, 5, 2], [3, 5, 14, 1], [0, 3, nd - 1, 3]                      # row 5: the append crosses the width
    cand = torch.randint(0, 1000, (4, nd), generator=g).to(dtype)
    index = torch.full((4, nd), -1, dtype=torch.int32)
    for b, n in enumerate(acc):
        index[b, :n + 1] = torch.tensor([0] + sorted(torch.randperm(nd - 1, generator=g)[:n].add(1).tolist()), dtype=torch.int32)
    bonus = torch.tensor([11, 22, 33, 44], dtype=torch.int32)
    want, want_lens = table.clone(), []
    for b, (r, L, n) in enumerate(zip(rows, lens, acc)):
        new = [int(cand[b, index[b, i]]) for i in range(1, n + 1)] + [int(bonus[b])]
        for i, t in enumerate(new):
            if L + i < width:
                want[r, L + i] = t
        want_lens.append(min(L + n + 1, width))
    table_d, lens_d = table.to(device), torch.tensor(lens, dtype=torch.int32, device=device)
    K.ngram_commit(table_d, torch.tensor(rows, device=device), lens_d, cand.to(device), index.to(device),
                   torch.tensor(acc, dtype=torch.int32, device=device), bonus.to(device))
    assert lens_d.tolist() == want_lens and torch.equal(table_d.cpu(), want)


@pytest.mark.parametrize("change,message", [
    (dict(nd=65), "nodes"), (dict(max_ngram=9), "sgl_amd_ngram_draft_max_ngram"), (dict(min_ngram=5), "min_ngram <="),
    (dict(num_splits=0), "num_splits"), (dict(stride=4098), "row stride"),
])
def test_argument_errors_are_reported_before_any_launch(change, message):
    from sglang_amd import native

    a = dict(stride=4096, batch=2, nd=8, max_ngram=4, min_ngram=1, branches=4, depth=7, window=0, num_splits=2)
    a.update(change)
    rc = native.lib().sgl_amd_ngram_draft_tree(None, a["stride"], None, None, a["batch"], a["nd"], a["max_ngram"], a["min_ngram"],
                                               a["branches"], a["depth"], a["window"], 0, None, None, None, a["num_splits"], None, None)
    assert rc == -1 and message in native.last_error(), native.last_error()
