"""Device time of one layer's TARGET_VERIFY attention: kernels.verify_attention (split-KV, at the splits
kernels.choose_verify_splits picks) against kernels.extend_attention with the same tree mask, on the same inputs, in one process.

    python benchmarks/verify_attention_time.py [--json profiles/verify_attention_time.json] [--quick]

Geometries: Llama-3-8B (Hq 32, Hkv 8, D 128) and a 70B / 8 rank (Hq 8, Hkv 1).  Shapes: B in {1, 16, 64} x draft tokens in {4, 8, 16} x
context in {1024, 4096, 16384}; cells whose rows (draft tokens x GQA group) exceed the kernel's 64 are listed as unsupported.
Both routes are captured as graphs of `--iters` calls and replayed alternately, 5 timed repetitions each (device events):
median and spread (max - min) per call.  COLD pools: call i of a graph reads pool copy i % n (up to 64 copies, together 1 GiB
where 64 suffice, and at least as many calls per graph as copies), as the layers of a model do -- one layer's rows of a small
batch would otherwise sit in the 256 MiB infinity cache; `n_pools` and `pool_mib` (one copy) are reported.  hbm_frac: the launch's unique K/V bytes (every request's rows once per kv head)
over the median time, against the 8 TB/s HBM peak -- the accounting of bench.py's attention_roofline.  Outputs of the two routes
are compared at every shape (max abs difference, bf16 results).
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
HBM_PEAK_GBPS = 8000.0
GEOMETRIES = {"llama3_8b": (32, 8, 128), "llama3_70b_tp8": (8, 1, 128)}


def graph_of(fn, iters, warmup=2):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(iters):
            fn(i)
    g.replay()
    torch.cuda.synchronize()
    return g


def make_inputs(B, nd, ctx, Hq, Hkv, D, iters):
    gen = torch.Generator(device=DEV).manual_seed(B * 131 + nd * 17 + ctx)
    seq = ctx + nd
    slots = B * seq
    pool_bytes = 2 * slots * Hkv * D * 2
    n_pools = max(1, min(64, -(-(1 << 30) // pool_bytes)))
    pools = [(torch.randn((slots, Hkv, D), device=DEV, generator=gen, dtype=torch.bfloat16),
              torch.randn((slots, Hkv, D), device=DEV, generator=gen, dtype=torch.bfloat16)) for _ in range(n_pools)]
    r2t = torch.randperm(slots, device=DEV, generator=gen).to(torch.int32).view(B, seq)
    qkv = torch.randn((B * nd, (Hq + 2 * Hkv) * D), device=DEV, generator=gen, dtype=torch.bfloat16)
    q = qkv[:, :Hq * D].view(B * nd, Hq, D)
    block = torch.zeros((nd, seq), dtype=torch.uint8, device=DEV)
    block[:, ctx:] = torch.tril(torch.ones((nd, nd), dtype=torch.uint8, device=DEV))
    args = dict(q=q, pools=pools, r2t=r2t, idx=torch.arange(B, dtype=torch.int64, device=DEV),
                seq=torch.full((B,), seq, dtype=torch.int32, device=DEV), pre=torch.full((B,), ctx, dtype=torch.int32, device=DEV),
                qo=torch.arange(0, (B + 1) * nd, nd, dtype=torch.int32, device=DEV), mask=block.flatten().repeat(B),
                mip=torch.arange(0, (B + 1) * nd * seq, nd * seq, dtype=torch.int64, device=DEV))
    return args, n_pools, pool_bytes


def sweep(args):
    out = []
    Bs, nds, ctxs = ((16,), (8,), (4096,)) if args.quick else ((1, 16, 64), (4, 8, 16), (1024, 4096, 16384))
    for name, (Hq, Hkv, D) in GEOMETRIES.items():
        for B in Bs:
            for nd in nds:
                for ctx in ctxs:
                    row = dict(geometry=name, heads=[Hq, Hkv, D], batch=B, draft_tokens=nd, context=ctx)
                    if not K.verify_attention_supported(nd, Hq // Hkv, D):
                        row["verify_attention"] = "unsupported: rows > %d" % K.verify_attention_max_rows()
                        print(json.dumps(row), flush=True)
                        out.append(row)
                        continue
                    a, n_pools, pool_bytes = make_inputs(B, nd, ctx, Hq, Hkv, D, args.iters)
                    splits = K.choose_verify_splits(B, Hkv, ctx + nd)
                    ws = K.verify_workspace(B * nd, Hq, D, splits, DEV) if splits > 1 else (None, None)
                    o_new, o_old = torch.empty_like(a["q"].contiguous()), torch.empty_like(a["q"].contiguous())

                    def new(i):
                        k, v = a["pools"][i % n_pools]
                        K.verify_attention(a["q"], o_new, k, v, a["r2t"], a["idx"], a["seq"], a["pre"], a["qo"], nd, D ** -0.5,
                                           custom_mask=a["mask"], mask_indptr=a["mip"], num_splits=splits, ws_acc=ws[0], ws_ml=ws[1])

                    def old(i):
                        k, v = a["pools"][i % n_pools]
                        K.extend_attention(a["q"], o_old, k, v, a["r2t"], a["idx"], a["seq"], a["pre"], a["qo"], nd, D ** -0.5, True,
                                           custom_mask=a["mask"], mask_indptr=a["mip"], skip_prefix_custom_mask=True)

                    new(0), old(0)
                    torch.cuda.synchronize()
                    row.update(splits=splits, n_pools=n_pools, pool_mib=pool_bytes / 2 ** 20,
                               max_abs_diff=float((o_new.float() - o_old.float()).abs().max()))
                    iters = max(args.iters, n_pools)
                    graphs = {"verify_attention": graph_of(new, iters), "extend_attention": graph_of(old, iters)}
                    times = {k: [] for k in graphs}
                    for _ in range(5):
                        for key, g in graphs.items():
                            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            s.record()
                            g.replay()
                            e.record()
                            torch.cuda.synchronize()
                            times[key].append(s.elapsed_time(e) * 1e3 / iters)
                    for key, ts in times.items():
                        med = statistics.median(ts)
                        row[key] = dict(median_us=med, spread_us=max(ts) - min(ts), hbm_frac=pool_bytes / (med * 1e-6) / 1e9 / HBM_PEAK_GBPS)
                    gap = row["extend_attention"]["median_us"] - row["verify_attention"]["median_us"]
                    row["verify_attention_wins"] = gap > max(row["extend_attention"]["spread_us"], row["verify_attention"]["spread_us"])
                    print(json.dumps(row), flush=True)
                    out.append(row)
                    del graphs, a, ws
                    torch.cuda.empty_cache()
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(out, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--quick", action="store_true", help="one shape per geometry (a rehearsal)")
    ap.add_argument("--json", default=None)
    sweep(ap.parse_args())


if __name__ == "__main__":
    main()
