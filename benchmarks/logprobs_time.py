"""Device time of the sampler's return_logprob work at [64, 128256]: kernels.logprobs_from_logits behind the sampling call
against the full-matrix route it replaces (log_softmax / softmax + log over [B, V], a gather, topk).

    python benchmarks/logprobs_time.py --logprobs [--json profiles/logprobs_time.json]

Both routes are captured as graphs of `--iters` calls in one process and replayed alternately, 5 timed repetitions each
(device events); median and spread (max - min) per call.  The host side (.tolist(), the upload of listed ids) is in neither.
fp32 sampled: the full-matrix route overwrites its logits, so both graphs start every call with the same copy of them.
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


def routes(logits, greedy, n_top):
    """(new, old): one sampler call with return_logprob each, device work only."""
    B, V = logits.shape
    t = torch.tensor([(0.7, 1.0, 1.3)[b % 3] for b in range(B)], dtype=torch.float32, device=DEV)
    top_ks = torch.full((B,), 50, dtype=torch.int32, device=DEV)
    top_ps = torch.full((B,), 0.9, dtype=torch.float32, device=DEV)
    seeds = torch.arange(B, dtype=torch.int64, device=DEV)
    rows = torch.arange(B, device=DEV)
    fp32 = logits.dtype == torch.float32
    work = torch.empty_like(logits) if (fp32 and not greedy) else logits

    def outputs(logprobs, ids):
        chosen = logprobs[rows, ids.long()]
        return (chosen,) + (tuple(logprobs.topk(n_top, dim=-1)) if n_top else ())

    def new():
        if work is not logits:
            work.copy_(logits)
        if greedy:
            return K.logprobs_from_logits(work, None, K.argmax(work), n_top)
        ids = K.sample_from_logits(work, t, top_ks, top_ps, None, seeds, None)
        return K.logprobs_from_logits(work, t, ids, n_top)

    def old():
        if work is not logits:
            work.copy_(logits)
        if greedy:
            return outputs(torch.log_softmax(work.float(), dim=-1), K.argmax(work))
        probs = K.softmax_temperature_(work, t) if fp32 else K.softmax_temperature_from_bf16(work, t)
        return outputs(torch.log(probs), K.top_k_top_p_min_p_sample(probs, top_ks, top_ps, None, seeds, None))

    return new, old


def logprobs_sweep(args):
    B, V = 64, 128256
    out = []
    for dtype in (torch.bfloat16, torch.float32):
        logits = (4 * torch.randn((B, V), device=DEV)).to(dtype)
        for greedy in (True, False):
            for n_top in (0, 5, 20):
                graphs = dict(zip(("logprobs_from_logits", "full_matrix"), (graph_of(f, args.iters) for f in routes(logits, greedy, n_top))))
                times = {k: [] for k in graphs}
                for _ in range(5):
                    for key, g in graphs.items():
                        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s.record()
                        g.replay()
                        e.record()
                        torch.cuda.synchronize()
                        times[key].append(s.elapsed_time(e) * 1e3 / args.iters)
                row = dict(shape=[B, V], dtype=str(dtype).replace("torch.", ""), sampling="greedy" if greedy else "top_k50_top_p0.9", n_top=n_top)
                for key, ts in times.items():
                    row[key] = dict(median_us=statistics.median(ts), spread_us=max(ts) - min(ts))
                gap = row["full_matrix"]["median_us"] - row["logprobs_from_logits"]["median_us"]
                row["logprobs_from_logits_wins"] = gap > max(row["full_matrix"]["spread_us"], row["logprobs_from_logits"]["spread_us"])
                print(json.dumps(row), flush=True)
                out.append(row)
                del graphs
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(out, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logprobs", action="store_true", help="logprobs_from_logits vs the full-matrix route at [64, 128256]")
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not args.logprobs:
        ap.error("nothing to do: pass --logprobs")
    logprobs_sweep(args)


if __name__ == "__main__":
    main()
