"""Sweep of the weight-streaming decode GEMM's decomposition on one MI355X vs hipBLASLt (F.linear).

    python benchmarks/gemm_sweep.py [--json gpurun_out/gemm_sweep.json] [--quick]
"""
import argparse
import json
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sglang_amd import kernels as K  # noqa: E402

BF = torch.bfloat16
DEV = torch.device("cuda:0")


def timeit(fn, iters=24, warmup=3, reps=5):
    """Kernel time without host launch overhead: `iters` calls captured in one hipGraph, replayed."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / (iters * reps) * 1e-3


HBM_PEAK = 8.0e12            # MI355X_MICROARCH.md: HBM3E spec, bytes / s
MFMA_PEAK = 2.5e15           # bf16 dense, flop / s

# (model, projection, N = rows of w, K): Llama-3-8B, then one rank of eight of Llama-3-70B
DENSE_TILED_SHAPES = [("8b", "qkv", 6144, 4096), ("8b", "o", 4096, 4096), ("8b", "gate_up", 28672, 4096),
                      ("8b", "down", 4096, 14336), ("8b", "lm_head", 128256, 4096),
                      ("70b/8", "qkv", 1280, 8192), ("70b/8", "o", 8192, 1024), ("70b/8", "gate_up", 7168, 8192),
                      ("70b/8", "down", 8192, 3584)]


def graph_of(fn, iters=24, warmup=3):
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


def dense_tiled_sweep(args):
    """dense_tiled_gemm against the library path (F.linear, + the silu_and_mul kernel for the fused gate_up) at M = 256 and
    512: both captured as graphs of 24 calls in one process, replayed alternately, 5 timed repetitions each (device
    events); median, spread (max - min over the repetitions) and each path's share of the roofline bound
    max(bytes / HBM peak, flops / bf16 MFMA peak), bytes and flops counted from the shapes."""
    rows = []
    iters, reps = 24, 5
    for model, name, N, Kd in DENSE_TILED_SHAPES:
        copies = max(2, int(600e6 // (N * Kd * 2)) + 1)     # rotate so the weights come from HBM, not the infinity cache
        ws = [(torch.randn((N, Kd), device=DEV) * 0.02).to(BF) for _ in range(copies)]
        it = [0]

        def nxt():
            it[0] = (it[0] + 1) % copies
            return ws[it[0]]

        for M in (256, 512):
            x = torch.randn((M, Kd), device=DEV).to(BF)
            for fused in ((False, True) if name == "gate_up" else (False,)):
                n_out = N // 2 if fused else N
                out = torch.empty((M, n_out), dtype=BF, device=DEV)
                nbytes = (N * Kd + M * Kd + M * n_out) * 2
                flops = 2 * M * N * Kd
                t_hbm, t_mfma = nbytes / HBM_PEAK, flops / MFMA_PEAK
                if fused:
                    lib = graph_of(lambda: K.silu_and_mul(F.linear(x, nxt()), out=out), iters)
                    new = graph_of(lambda: K.dense_tiled_gemm(x, nxt(), epilogue="silu_and_mul", out=out), iters)
                else:
                    lib = graph_of(lambda: F.linear(x, nxt()), iters)
                    new = graph_of(lambda: K.dense_tiled_gemm(x, nxt(), out=out), iters)
                times = {"library": [], "dense_tiled": []}
                for _ in range(reps):
                    for key, g in (("library", lib), ("dense_tiled", new)):
                        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s.record()
                        g.replay()
                        e.record()
                        torch.cuda.synchronize()
                        times[key].append(s.elapsed_time(e) / iters * 1e-3)
                bn, sp = K.choose_dense_tiled_config(M, N, Kd, fused)
                row = dict(model=model, shape=name, fused_silu=fused, M=M, N=N, K=Kd, block_n=bn, splits=sp,
                           bound="hbm" if t_hbm >= t_mfma else "mfma", bound_us=max(t_hbm, t_mfma) * 1e6)
                for key, ts in times.items():
                    med = sorted(ts)[len(ts) // 2]
                    row[key] = dict(median_us=med * 1e6, spread_us=(max(ts) - min(ts)) * 1e6, share_of_bound=max(t_hbm, t_mfma) / med)
                row["dense_tiled_wins"] = (row["library"]["median_us"] - row["dense_tiled"]["median_us"]
                                           > max(row["library"]["spread_us"], row["dense_tiled"]["spread_us"]))
                rows.append(row)
                print(json.dumps(row), flush=True)
                del lib, new
        del ws
        torch.cuda.empty_cache()
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(rows, indent=1))


def fp8_sweep(args):
    """bf16 vs fp8 (e4m3, per-channel scale) weight-streaming GEMM in ONE run, each with its automatic decomposition: the decode
    projections of Llama-3-8B and the gate_up of Llama-3-70B at 16 / 64 / 128 rows.  Weights rotate over copies larger than the
    256 MiB infinity cache; a time is the median of five graph replays of 24 calls."""
    shapes = [("8b", "qkv", 6144, 4096, "none"), ("8b", "o", 4096, 4096, "none"), ("8b", "gate_up", 28672, 4096, "silu_and_mul"),
              ("8b", "down", 4096, 14336, "none"), ("70b", "gate_up", 57344, 8192, "silu_and_mul")]
    rows = []
    for model, name, N, Kd, ep in shapes:
        copies = max(2, int(600e6 // (N * Kd)) + 1)
        w16 = [(torch.randn((N, Kd), device=DEV) * 0.02).to(BF) for _ in range(max(2, copies // 2 + 1))]
        q = [K.quantize_fp8_weight(w16[i % len(w16)]) for i in range(copies)]
        for M in (16, 64, 128):
            x = torch.randn((M, Kd), device=DEV).to(BF)
            it = [0]

            def run16():
                it[0] += 1
                return K.wstream_gemm(x, w16[it[0] % len(w16)], epilogue=ep)

            def run8():
                it[0] += 1
                w8, sc = q[it[0] % copies]
                return K.wstream_gemm(x, w8, epilogue=ep, w_scale=sc)

            row = dict(model=model, shape=name, N=N, K=Kd, M=M, epilogue=ep)
            for key, fn in (("bf16", run16), ("fp8", run8)):
                ts = sorted(timeit(fn, reps=1) for _ in range(5))
                row[key + "_us"] = ts[2] * 1e6
                row[key + "_spread_us"] = (ts[-1] - ts[0]) * 1e6
            row["bf16_over_fp8"] = row["bf16_us"] / row["fp8_us"]
            row["fp8_fraction_of_8TBps"] = N * Kd / (row["fp8_us"] * 1e-6) / HBM_PEAK
            row["bf16_fraction_of_8TBps"] = N * Kd * 2 / (row["bf16_us"] * 1e-6) / HBM_PEAK
            row["fp8_decomposition"] = K.choose_wstream_decomposition(M, N, Kd, ep != "none", ep == "silu_and_mul", 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del w16, q
        torch.cuda.empty_cache()
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(rows, indent=1))


def fp8_tiled_sweep(args):
    """The fp8-weight MFMA tile GEMM (dense_tiled_gemm with w_scale, automatic tile / splits) at prefill-sized rows, per shape
    against (b) the path it replaces -- widen the weight to bf16, F.linear, scale in fp32, round (+ the silu_and_mul kernel for
    the fused gate_up) -- and (c) the bf16 path on bf16 weights (dense_tiled_gemm where dense_tiled_preferred(), the library GEMM
    elsewhere).  The three are captured as graphs in one process and replayed alternately, 5 timed repetitions each (device
    events): median, spread (max - min) and the new kernel's share of the bf16 MFMA roofline max(flops / peak, fp8 bytes / HBM
    peak).  Rows 96 and 128 are measured too (the policy leaves them on the weight stream)."""
    rows = []
    reps = 5
    for model, name, N, Kd in [s for s in DENSE_TILED_SHAPES if s[1] != "lm_head"]:      # lm_head stays bf16 in an fp8 engine
        copies = max(2, min(6, int(600e6 // (N * Kd)) + 1))   # rotate so the weights come from HBM, not the infinity cache
        w16 = [(torch.randn((N, Kd), device=DEV) * 0.02).to(BF) for _ in range(2)]
        q = [K.quantize_fp8_weight(w16[i % 2]) for i in range(copies)]
        it = [0]

        def nxt8():
            it[0] = (it[0] + 1) % copies
            return q[it[0]]

        def nxt16():
            it[0] = (it[0] + 1) % copies
            return w16[it[0] % 2]

        for M in (96, 128, 256, 512, 2048, 8192):
            x = torch.randn((M, Kd), device=DEV).to(BF)
            for fused in ((False, True) if name == "gate_up" else (False,)):
                n_out = N // 2 if fused else N
                out = torch.empty((M, n_out), dtype=BF, device=DEV)
                flops = 2 * M * N * Kd
                t_hbm, t_mfma = (N * Kd + (M * Kd + M * n_out) * 2) / HBM_PEAK, flops / MFMA_PEAK
                iters = max(2, min(24, int(20e-3 / (flops / 4e14 + 20e-6))))      # a graph of ~20 ms at most

                def new_fn():
                    w8, sc = nxt8()
                    K.dense_tiled_gemm(x, w8, epilogue="silu_and_mul" if fused else "none", out=out, w_scale=sc)

                def old_fn():
                    w8, sc = nxt8()
                    y = (F.linear(x, w8.to(BF)).float() * sc).to(BF)
                    if fused:
                        K.silu_and_mul(y, out=out)

                def bf16_fn():
                    w = nxt16()
                    if K.dense_tiled_preferred(M, N, Kd, fused):
                        K.dense_tiled_gemm(x, w, out=out)
                    elif fused:
                        K.silu_and_mul(F.linear(x, w), out=out)
                    else:
                        F.linear(x, w)

                graphs = {"fp8_tiled": graph_of(new_fn, iters, 2), "widen_library": graph_of(old_fn, iters, 2), "bf16": graph_of(bf16_fn, iters, 2)}
                times = {k: [] for k in graphs}
                for _ in range(reps):
                    for key, g in graphs.items():
                        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s.record()
                        g.replay()
                        e.record()
                        torch.cuda.synchronize()
                        times[key].append(s.elapsed_time(e) / iters * 1e-3)
                bn, sp = K.choose_dense_tiled_fp8_config(M, N, Kd, fused)
                row = dict(model=model, shape=name, fused_silu=fused, M=M, N=N, K=Kd, block_n=bn, splits=sp, calls_per_graph=iters,
                           bound="hbm" if t_hbm >= t_mfma else "mfma", bound_us=max(t_hbm, t_mfma) * 1e6)
                for key, ts in times.items():
                    med = sorted(ts)[len(ts) // 2]
                    row[key] = dict(median_us=med * 1e6, spread_us=(max(ts) - min(ts)) * 1e6)
                row["fp8_tiled"]["share_of_bound"] = row["bound_us"] / row["fp8_tiled"]["median_us"]
                row["widen_library_over_fp8_tiled"] = row["widen_library"]["median_us"] / row["fp8_tiled"]["median_us"]
                row["bf16_over_fp8_tiled"] = row["bf16"]["median_us"] / row["fp8_tiled"]["median_us"]
                row["fp8_tiled_slower_than_widen_library"] = (row["fp8_tiled"]["median_us"] - row["widen_library"]["median_us"]
                                                              > max(row["fp8_tiled"]["spread_us"], row["widen_library"]["spread_us"]))
                rows.append(row)
                print(json.dumps(row), flush=True)
                del graphs
        del w16, q
        torch.cuda.empty_cache()
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(rows, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--M", type=int, default=64)
    ap.add_argument("--blocked", action="store_true", help="chunk-major [K/128, M, 128] activations")
    ap.add_argument("--dense-tiled", action="store_true", help="dense_tiled_gemm vs the library path at M = 256 / 512")
    ap.add_argument("--weight-dtype", default="bf16", choices=("bf16", "fp8_e4m3"), help="fp8_e4m3: bf16 vs fp8 weight stream, one run; with --dense-tiled: the fp8-weight tile GEMM at 96..8192 rows")
    args = ap.parse_args()
    if args.dense_tiled and args.weight_dtype == "fp8_e4m3":
        return fp8_tiled_sweep(args)
    if args.dense_tiled:
        return dense_tiled_sweep(args)
    if args.weight_dtype == "fp8_e4m3":
        return fp8_sweep(args)
    shapes = [("gate_up", 28672, 4096), ("down", 4096, 14336), ("qkv", 6144, 4096), ("o", 4096, 4096),
              ("lm_head", 128256, 4096)]
    M = args.M
    rows = []
    # rotate over several weight copies so the stream comes from HBM, not the 256 MiB infinity cache
    for name, N, Kd in shapes:
        copies = max(2, int(600e6 // (N * Kd * 2)) + 1)
        ws = [(torch.randn((N, Kd), device=DEV) * 0.02).to(BF) for _ in range(copies)]
        x = torch.randn((M, Kd), device=DEV).to(BF)
        if args.blocked:
            x = x.view(M, Kd // 128, 128).permute(1, 0, 2).contiguous()
        wbytes = N * Kd * 2
        it = [0]

        def nxt():
            it[0] = (it[0] + 1) % copies
            return ws[it[0]]

        t = timeit(lambda: F.linear(K.unblock(x), nxt()))
        rows.append(dict(shape=name, N=N, K=Kd, M=M, impl="hipblaslt", us=t * 1e6, GBps=wbytes / t / 1e9))
        print(json.dumps(rows[-1]), flush=True)
        nch = Kd // 128
        cands = set()
        auto = K.choose_wstream_config(M, N, Kd)
        cands.add(auto)
        if not args.quick:
            for nw in (4, 5, 6, 7, 8):
                for s in (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16):
                    if s <= nch // 2:
                        cands.add((nw, s))
            for nw in (2, 3, 4):                      # two tiles per wave
                for s in (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16):
                    if s <= nch // 2 and N % 32 == 0:
                        cands.add((nw, s, 2))
        for cand in sorted(cands):
            nw, s = cand[:2]
            tpw = cand[2] if len(cand) > 2 else 1
            try:
                t = timeit(lambda: K.wstream_gemm(x, nxt(), waves_per_group=nw, splits=s, tiles_per_wave=tpw))
            except RuntimeError as e:
                print("skip", nw, s, e)
                continue
            rows.append(dict(shape=name, N=N, K=Kd, M=M, impl="wstream", nw=nw, splits=s, tpw=tpw, auto=(nw, s) == auto and tpw == 1,
                             us=t * 1e6, GBps=wbytes / t / 1e9))
            print(json.dumps(rows[-1]), flush=True)
        del ws
        torch.cuda.empty_cache()
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(rows, indent=1))
    # best per shape
    for name, _, _ in shapes:
        rs = [r for r in rows if r["shape"] == name]
        lib = [r for r in rs if r["impl"] == "hipblaslt"][0]
        best = min((r for r in rs if r["impl"] == "wstream"), key=lambda r: r["us"])
        print(f"{name:8s} hipblaslt {lib['us']:7.1f} us {lib['GBps']:6.0f} GB/s | best wstream nw={best['nw']} tpw={best['tpw']} s={best['splits']} "
              f"{best['us']:7.1f} us {best['GBps']:6.0f} GB/s")


if __name__ == "__main__":
    main()
