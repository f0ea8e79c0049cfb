"""Device time of the accept half of a speculative verify step at B = 64 requests x 8 tree nodes, V = 128256, bf16, T = 1:
kernels.tree_accept_from_logits (speculative_sampling.hip) beside softmax(logits.float() / T) alone on the same tensor -- the floor
of the route that materialises the [B * nd, V] probabilities before it can look at a single draft token -- and
kernels.build_verify_tree at a 1024-token context.

    python benchmarks/tree_accept_time.py [--json profiles/tree_accept_time.json]

Every route is captured as a graph of `--iters` calls and the graphs are replayed alternately, 5 timed repetitions each (device
events); median and spread (max - min) per call.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sglang_amd import kernels as K  # noqa: E402

DEV = torch.device("cuda:0")
PARENTS = [-1, 0, 0, 1, 1, 2, 2, 3]


def graph_of(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    B, nd, V = 64, len(PARENTS), 128256
    gen = torch.Generator(device=DEV).manual_seed(0)
    logits = (4 * torch.randn((B * nd, V), device=DEV, generator=gen)).to(torch.bfloat16)
    cand = torch.randint(0, V, (B, nd), device=DEV, generator=gen)
    # half of the requests carry the row's own arg-max down the path 0 -> 1 -> 3 -> 7: accepted and rejected drafts both occur
    for child in (1, 3, 7):
        rows = torch.arange(0, B, 2, device=DEV) * nd + PARENTS[child]
        cand[0::2, child] = logits[rows].float().argmax(-1)
    temps = torch.ones(B, dtype=torch.float32, device=DEV)
    uniform, ufinal = torch.rand((B, nd), device=DEV, generator=gen), torch.rand(B, device=DEV, generator=gen)
    parents = torch.tensor([PARENTS] * B, dtype=torch.int32, device=DEV)
    seq_lens = torch.full((B,), 1024, dtype=torch.int32, device=DEV)
    _, _, _, next_token, next_sibling = K.build_verify_tree(parents, seq_lens, 1024 * B)
    t_rows = temps.repeat_interleave(nd)[:, None]
    routes = {
        "tree_accept_from_logits": lambda: K.tree_accept_from_logits(logits, temps, cand, next_token, next_sibling, uniform, ufinal),
        "softmax_alone": lambda: torch.softmax(logits.float() / t_rows, dim=-1),
        "build_verify_tree": lambda: K.build_verify_tree(parents, seq_lens, 1024 * B),
    }
    accepted = routes["tree_accept_from_logits"]()[1]
    graphs = {k: graph_of(f, args.iters) for k, f in routes.items()}
    times = {k: [] for k in graphs}
    for _ in range(5):
        for key, g in graphs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            g.replay()
            e.record()
            torch.cuda.synchronize()
            times[key].append(s.elapsed_time(e) * 1e3 / args.iters)
    row = dict(batch=B, nodes=nd, vocab=V, dtype="bfloat16", temperature=1.0, mean_accept_len=float(accepted.float().mean()),
               ranges=[K.tree_accept_ranges(B * nd, V), K.tree_accept_ranges(B, V)])
    for key, ts in times.items():
        row[key] = dict(median_us=statistics.median(ts), spread_us=max(ts) - min(ts))
    print(json.dumps(row), flush=True)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(row, indent=1) + "\n")


if __name__ == "__main__":
    main()
