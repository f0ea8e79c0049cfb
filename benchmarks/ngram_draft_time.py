"""Time of the n-gram drafter of a speculative step, on the device and on the host, at B = 1 / 16 / 64 requests, histories of 1024 /
4096 / 16384 tokens (vocabulary 128256; the last four tokens are planted at six earlier places, so every draft has hits and, at the
default depth of nodes - 1, fills all of its nodes) and trees of 1 / 8 / 16 / 64 nodes:

  device  kernels.ngram_draft_tree (two launches) + kernels.ngram_commit (one launch) on the device-side token table, plus the copy
          that puts `lens` back for the next call: a graph of `--iters` such calls, device events.
  host    what a caller without the kernels does: `.cpu()` of the requests' rows and lengths, the drafting rule in Python, the upload
          of tree_tokens / parents; a host clock around it, ending in a device synchronise.

    python benchmarks/ngram_draft_time.py [--json profiles/ngram_draft_time.json]

The two are run alternately, `--reps` timed repetitions of each; median and spread (max - min) per call, and host / device.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sglang_amd import kernels as K  # noqa: E402
from benchmarks.tree_accept_time import graph_of  # noqa: E402

DEV = torch.device("cuda:0")
VOCAB, MAX_N, MIN_N, BRANCHES = 128256, 4, 1, 4


def draft_on_host(h, nd, max_n, min_n, branches, depth, window, pad_token):
    """The rule of sgl_amd_ngram_draft_tree on a host list (the reference of tests/test_ngram_draft_gpu.py)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    gen = torch.Generator().manual_seed(0)
    rows_out = []
    for L in (1024, 4096, 16384):
        width = L + 64                                      # room for the commits of a step
        for B in (1, 16, 64):
            hist = torch.randint(0, VOCAB, (B, width), generator=gen).to(torch.int32)
            for b in range(B):
                for at in torch.randint(8, L - 80, (6,), generator=gen).tolist():
                    hist[b, at:at + MAX_N] = hist[b, L - MAX_N:L]
            pool = torch.randperm(B, generator=gen).to(DEV)
            table = torch.empty((B, width), dtype=torch.int32, device=DEV)
            table[pool] = hist.to(DEV)
            lens0 = torch.full((B,), L, dtype=torch.int32, device=DEV)
            lens = lens0.clone()
            for nd in (1, 8, 16, 64):
                depth = max(1, nd - 1)
                n_acc = min(2, nd - 1)
                index = torch.full((B, nd), -1, dtype=torch.int32)
                index[:, :n_acc + 1] = torch.arange(n_acc + 1, dtype=torch.int32)
                index, acc = index.to(DEV), torch.full((B,), n_acc, dtype=torch.int32, device=DEV)
                bonus = torch.randint(0, VOCAB, (B,), generator=gen).to(torch.int32).to(DEV)

                def device_step():
                    lens.copy_(lens0)
                    tt, _, _ = K.ngram_draft_tree(table, pool, lens, nd, MAX_N, MIN_N, BRANCHES)
                    K.ngram_commit(table, pool, lens, tt, index, acc, bonus)

                def host_step():
                    rows, n = table[pool].cpu().tolist(), lens0.cpu().tolist()
                    out = [draft_on_host(r[:k], nd, MAX_N, MIN_N, BRANCHES, depth, 0, 0) for r, k in zip(rows, n)]
                    tt = torch.tensor([o[0] for o in out], dtype=torch.int64).to(DEV)
                    par = torch.tensor([o[1] for o in out], dtype=torch.int32).to(DEV)
                    torch.cuda.synchronize()
                    return tt, par, [o[2] for o in out]

                graph = graph_of(device_step, args.iters)
                lens.copy_(lens0)
                got = K.ngram_draft_tree(table, pool, lens, nd, MAX_N, MIN_N, BRANCHES)
                want = host_step()
                same = got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2]
                dev_us, host_us = [], []
                for _ in range(args.reps):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    graph.replay()
                    e.record()
                    torch.cuda.synchronize()
                    dev_us.append(s.elapsed_time(e) * 1e3 / args.iters)
                    t0 = time.perf_counter()
                    host_step()
                    host_us.append((time.perf_counter() - t0) * 1e6)
                row = dict(batch=B, history=L, nodes=nd, vocab=VOCAB, splits=K.choose_ngram_splits(B, width), same_result=same,
                           mean_num_real=sum(want[2]) / B,
                           device=dict(median_us=statistics.median(dev_us), spread_us=max(dev_us) - min(dev_us)),
                           host=dict(median_us=statistics.median(host_us), spread_us=max(host_us) - min(host_us)))
                row["host_over_device"] = row["host"]["median_us"] / row["device"]["median_us"]
                print(json.dumps(row), flush=True)
                rows_out.append(row)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text("[\n" + ",\n".join(json.dumps(r) for r in rows_out) + "\n]\n")   # a cell per line


if __name__ == "__main__":
    main()
