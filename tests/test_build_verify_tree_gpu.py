"""kernels.build_verify_tree (speculative_sampling.hip): mask, mask_indptr and positions byte for byte against the construction of
Engine.verify_tree (a few lines of torch on the host), next_token / next_sibling against a host loop.  Request 0 carries the tree,
request 1 a pure chain and request 2 a star of the same size; the context lengths put the blocks at odd offsets of the flat mask."""
import pytest
import torch

from sglang_amd import kernels

pytestmark = pytest.mark.gpu
TREES = [[-1], [-1, 0, 0, 1, 1, 2, 5], [-1, 0, 0, 0, 0, 0, 1, 6, 7, 8, 9, 2, 2, 11, 3, 6]]
SEQ_LENS = [1, 70, 129]


@pytest.mark.parametrize("tree", TREES, ids=lambda t: f"nd{len(t)}")
def test_tables_match_the_host_construction(tree):
    nd = len(tree)
    parents = [tree, [j - 1 for j in range(nd)], [-1] + [0] * (nd - 1)]
    masks, positions, next_token, next_sibling = [], [], [], []
    for par, kv in zip(parents, SEQ_LENS):
        anc = torch.zeros((nd, nd), dtype=torch.bool)
        for j in range(nd):
            a = j
            while a >= 0:
                anc[j, a] = True
                a = par[a]
        masks.append(torch.cat([torch.ones((nd, kv), dtype=torch.bool), anc], dim=1).flatten())
        positions += [kv + int(anc[j].sum()) - 1 for j in range(nd)]
        next_token.append([min((i for i in range(nd) if par[i] == j), default=-1) for j in range(nd)])
        next_sibling.append([min((i for i in range(j + 1, nd) if j and par[i] == par[j]), default=-1) for j in range(nd)])
    indptr = [0]
    for m in masks:
        indptr.append(indptr[-1] + m.numel())
    got = kernels.build_verify_tree(torch.tensor(parents, dtype=torch.int32, device="cuda"),
                                    torch.tensor(SEQ_LENS, dtype=torch.int32, device="cuda"))
    mask, mask_indptr, pos, nt, ns = (t.cpu() for t in got)
    assert mask.dtype == torch.uint8 and torch.equal(mask, torch.cat(masks).view(torch.uint8))
    assert mask_indptr.dtype == torch.int64 and mask_indptr.tolist() == indptr
    assert pos.dtype == torch.int64 and pos.tolist() == positions
    assert nt.tolist() == next_token and ns.tolist() == next_sibling
