#!/usr/bin/env python
"""bench.py -- the RadixAttention serving hot path on MI355X.

    python bench.py --gpus 1 --steps 3 --warmup 1            # the plain run: set up, warm up, time the steps, one JSON line
    python bench.py --gpus 1 --steps 3 --warmup 1 --full     # + the side measurements listed below, after the timed region
    python bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR   # + DIR/<name>.npy: what the last timed step returned
    python bench.py --gpus 8 --model llama-3-70b           # spawns the 8 ranks itself (headline TP=8 config)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One "step" = one complete pass of the hot path over the synthetic shared-prefix
batch of BASELINE.json `configs[1]` (Llama-3-8B, bf16, 1024-in / 128-out):
  P-cold  prefill of the G group leaders (1024 new tokens each, empty radix tree)
  P-warm  prefill of the other B-G requests (896 tokens hit the radix cache, 128 new)
  D       127 decode steps at batch B (hipGraph replay), greedy, ignore_eos
followed by cache_finished_req for every request.  The cache is reset between
steps so every step does identical work.  value = output tokens / s over the K
timed steps (max over ranks); at N > 1 the model runs TP=N over RCCL with the
batch scaled to 64*N requests (weak scaling).  With --gpus N and no torchrun
environment the script spawns its N ranks itself; it FAILS (never degrades) when
it ends up with fewer ranks than asked, with eager decode where a hipGraph was
asked for, or with another model than requested.

A plain run does what `value` needs and nothing else: the line carries `value`, `ms_per_step` (milliseconds per timed step),
the phase times of the timed steps and the rooflines computed from them.  `--dump-outputs DIR` writes, after the timed steps,
the arrays the caller of the last timed step received (float64 / float32 .npy, rows in request order): `output_ids` [B, out]
(every request's greedy tokens), `cached_tokens` [B] (radix hits) and `last_decode_logits` [rows, vocab] with
`last_decode_logits_rows` (the logits of the step's last decode launch, as they stand in the decode graph's output buffer;
a fixed seeded sample of the rows where all of them would pass 48 MB).  Prompts and weights are seeded: the same arguments
give the same inputs in every run, so two builds compare output for output.

With `--full` the JSON line also carries (each in a run of its own after the timed region; the --no-* switches drop single legs)
  roofline            the WHOLE decode step (one hipGraph replay) vs 8 TB/s, SURVEY section 8(d)'s bytes per step, `traffic` =
                      HBM bytes of one step from the committed PMC passes (= step_roofline, kept under its old key too)
  dominant_kernel_roofline / kernel_table
                      the largest kernel of the step (weight-streaming gate_up GEMM) and the table of the layer's weight
                      streams (qkv + rope, o_proj + norm, gate_up + silu, down + norm, lm_head), each HIP-event timed over
                      the model's own layers in captured graphs
  attention_roofline  cascade / plain decode attention on the workload's slot pattern (+ PMC traffic)
  prefill_mfma        prefill FLOP/s vs the bf16 MFMA peak, the extend-attention kernel's own rate and the
                      PMC MFMA-busy fraction (`mfma_util`)
  parity              teacher-forced logits of THIS job against the oracle's plain torch ops on the GPU
                      (the reference's torch-native path): max / rms |dlogit|, fraction within 1e-3, arg-max
                      agreement, against the fp32-accumulating and the literal bf16 oracle (rank 0, N=1)
  cpu_baseline        the oracle = reference CPU torch-native path on the box's host cores, on a bounded sample
                      of the same phases: Qwen2.5-0.5B end to end and Llama-3-8B at B=4
  reference_scheduler the same job under the REFERENCE'S own Scheduler.run_event_loop() (overlap loop), ModelRunner, radix cache
                      and graph runner with this package as its plug-in (tests/golden/ref_model.py over the staged copy of the
                      reference's sources; a subprocess after the timed region): tokens/s, decode interval, graph replays,
                      radix hits, Triton launches (0), the pool / allocator classes.  Reported BESIDE `value`, never as it.
  + top-level copies  ttft_p50_ms, prefill_mfma_frac, decode_step_hbm_frac, ms_per_decode_step, reference_scheduler_tokens_per_s
"""
from __future__ import annotations

import argparse
import json
import os
import random
import socket
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

HBM_PEAK_GBPS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
MFMA_PEAK_TFLOPS = 2500.0     # bf16 dense
PMC_FILE = ROOT / "profiles" / "r06_pmc.json"
PMC_NAME = "profiles/" + PMC_FILE.name


def build_prompts(cfg, groups, per_group, prefix, unique, seed=1):
    """gen_prompt-style synthetic ids (benchmark/datasets/common.py:79-83): uniform in [0, vocab)."""
    rnd = random.Random(seed)
    prompts = []
    for _ in range(groups):
        sys_p = [rnd.randrange(cfg.vocab_size) for _ in range(prefix)]
        prompts.append([sys_p + [rnd.randrange(cfg.vocab_size) for _ in range(unique)] for _ in range(per_group)])
    return prompts


def load_pmc():
    """profiles/r04_pmc.json (benchmarks/summarize_pmc_phases.py over the rocprofv3 --pmc passes of
    benchmarks/pmc_workload.py): {"stamp": {"sources": {file: sha}}, "phases": {phase: {"kernels": {name: {"dispatches",
    counter: avg, ...}}}}}.  A record without a stamp is not quoted at all."""
    if not PMC_FILE.exists():
        return None
    try:
        pmc = json.loads(PMC_FILE.read_text())
    except Exception:
        return None
    return pmc if isinstance(pmc.get("stamp", {}).get("sources"), dict) else None


_SHARED_SOURCES = ("common.hpp", "kv_format.hpp")


def pmc_current(pmc, *sources):
    """The record's counters describe today's kernels of `sources` (csrc file names; none = every source): the sha256
    stamped at collection time still matches the files this process was built from.  A stale record yields no traffic /
    utilisation figure (null in the JSON line) rather than a number of some other revision's kernel."""
    if not pmc:
        return False
    import hashlib

    stamped = pmc["stamp"]["sources"]
    csrc = ROOT / "sglang_amd" / "csrc"
    names = (tuple(sources) + _SHARED_SOURCES) if sources else tuple(stamped) + tuple(f.name for f in csrc.iterdir() if f.is_file())
    for n in set(names):
        f = csrc / n
        if not f.is_file() or stamped.get(n) != hashlib.sha256(f.read_bytes()).hexdigest()[:16]:
            return False
    return True


def pmc_kernel(pmc, phase, substr, *sources):
    """Per-dispatch averages of the kernel of `phase` whose name contains `substr` (the most dispatched one when
    several match), or None -- also when the record predates the current `sources` of that kernel."""
    if not pmc or not pmc_current(pmc, *sources):
        return None
    hits = [rec for name, rec in pmc.get("phases", {}).get(phase, {}).get("kernels", {}).items() if substr in name]
    return max(hits, key=lambda r: r.get("dispatches", 0)) if hits else None


def hbm_bytes(rec):
    """MI355X_MICROARCH.md HBM section: on gfx950 FETCH_SIZE (KiB) reports half of a wide coalesced streaming
    read, so it is doubled; WRITE_SIZE (KiB) as is."""
    if not rec or "FETCH_SIZE" not in rec or "WRITE_SIZE" not in rec:
        return None
    return (2.0 * rec["FETCH_SIZE"] + rec["WRITE_SIZE"]) * 1024.0


def p_lin(cfg):
    """Matmul weights touched per token, excluding embedding / lm_head."""
    H, D = cfg.hidden_size, cfg.head_dim
    qkv = H * (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * D
    o = cfg.num_attention_heads * D * H
    if cfg.num_local_experts > 0:           # router + the experts a token visits
        mlp = H * cfg.num_local_experts + cfg.num_experts_per_tok * 3 * H * cfg.intermediate_size
    else:
        mlp = 3 * H * cfg.intermediate_size
    return cfg.num_hidden_layers * (qkv + o + mlp)


def decode_weight_bytes(cfg, batch):
    """Weight bytes a decode step touches once; MoE: the experts actually hit by batch*top_k picks
    (expected number of distinct experts under uniform routing)."""
    H, D = cfg.hidden_size, cfg.head_dim
    qkv = H * (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * D
    o = cfg.num_attention_heads * D * H
    if cfg.num_local_experts > 0:
        E, k = cfg.num_local_experts, cfg.num_experts_per_tok
        hit = E * (1.0 - (1.0 - k / E) ** batch)
        mlp = H * E + hit * 3 * H * cfg.intermediate_size
    else:
        mlp = 3 * H * cfg.intermediate_size
    return (cfg.num_hidden_layers * (qkv + o + mlp) + H * cfg.vocab_size) * 2


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--model", default="llama-3-8b",
                    help="llama-3-8b (configs[1], default), llama-3-70b (configs[2], the documented headline at "
                         "--gpus 8), mixtral-8x7b (configs[3], --gpus 2), qwen2.5-0.5b")
    ap.add_argument("--groups", type=int, default=4, help="prompt groups per GPU")
    ap.add_argument("--per-group", type=int, default=16)
    ap.add_argument("--prefix", type=int, default=896)
    ap.add_argument("--unique", type=int, default=128)
    ap.add_argument("--out", type=int, default=128)
    ap.add_argument("--page-size", type=int, default=1)
    ap.add_argument("--layers", type=int, default=0, help="override the layer count (NOT a valid bench line: the "
                                                           "config is marked reduced)")
    ap.add_argument("--kv-cache-dtype", default="auto", choices=("auto", "bfloat16", "fp8_e4m3"),
                    help="KV pool rows (server_args --kv-cache-dtype); fp8_e4m3 is NOT the baseline configuration: the "
                         "line's config says so and the bf16-KV parity leg is skipped")
    ap.add_argument("--rank-of", type=int, default=0, metavar="TP",
                    help="rank-shape run on ONE GPU: rank 0 of a TP-way job (that rank's weight shards, the weak-scaled batch "
                         "64 x TP, every collective launched as a world-of-1 loopback of the xGMI kernels: all launches of the "
                         "real job, no wire time).  The line is marked as such; it is NOT a multi-GPU measurement")
    ap.add_argument("--scaling", default="weak", choices=("weak", "strong"),
                    help="N > 1: weak = the batch grows with the TP degree (64 x N requests, the default and what `value` at N GPUs "
                         "means in SCALE files); strong = 64 requests at every N (the latency-bound regime)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--operator-surface", action="store_true",
                    help="decode through the unfused per-operator hooks only (the path the sglang.srt registration "
                         "hooks reach without patching model classes)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the side measurements: per-kernel / attention / sampler rooflines, parity "
                         "against the oracle, the CPU baseline, the job under the reference's Scheduler (the --no-* switches below "
                         "drop single legs of it); off by default: a plain run only times the steps")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one returned to DIR/<name>.npy (output_ids, cached_tokens, "
                         "last_decode_logits + last_decode_logits_rows)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-roofline", action="store_true")
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--no-reference-scheduler", action="store_true", help="skip the leg that runs the job under the reference's Scheduler")
    ap.add_argument("--cpu-budget-s", type=float, default=30.0)
    return ap.parse_args()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _spawned(local_rank, world, port, argv):
    os.environ.update({"RANK": str(local_rank), "LOCAL_RANK": str(local_rank), "WORLD_SIZE": str(world),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    sys.argv = argv
    worker(parse_args())


def main():
    args = parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no HIP device visible); there is no CPU fallback path")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # not under torchrun: start the N ranks ourselves, one process per GPU
        if torch.cuda.device_count() < args.gpus:
            raise SystemExit(f"--gpus {args.gpus} but only {torch.cuda.device_count()} HIP devices are visible")
        import torch.multiprocessing as mp

        mp.spawn(_spawned, args=(args.gpus, _free_port(), list(sys.argv)), nprocs=args.gpus, join=True)
        return
    worker(args)


def _trace(msg: str) -> None:
    """SGLANG_AMD_BENCH_TRACE=1: one stderr line per phase and rank (where a multi-rank launch stops, if it stops)."""
    if os.environ.get("SGLANG_AMD_BENCH_TRACE", "") not in ("", "0"):
        print(f"[bench rank {os.environ.get('RANK', '0')} +{time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


_T0 = time.perf_counter()


def worker(args):
    from sglang_amd.distributed import parallel_state as ps
    from sglang_amd.harness import models
    from sglang_amd.harness.engine import Engine, ModelRunner, Req
    from sglang_amd.harness.models import CONFIGS
    import torch.distributed as dist

    if args.operator_surface:
        models.OPERATOR_SURFACE_ONLY = True
    # SGLANG_AMD_BENCH_SHARE_GPU=1: the ranks of an N > 1 launch all use GPU 0 (gloo process groups, the xGMI kernels over hipIpc
    # between the processes) -- a DRY RUN of the driver's multi-GPU command on a one-GPU box (tests/test_engine_gpu.py): the launch
    # path, the rank checks and the JSON line are the real ones, the number is not a multi-GPU measurement and the line says so
    share_gpu = os.environ.get("SGLANG_AMD_BENCH_SHARE_GPU", "") not in ("", "0") and int(os.environ.get("WORLD_SIZE", "1")) > 1
    if share_gpu:
        # ranks that SHARE a GPU must leave each other CUs: a rank's all-reduce workgroups spin on flags that the peer's workgroups
        # write, and the peer's launches (its GEMMs first) need CUs to get there -- on a node every rank owns a GPU
        from sglang_amd import native

        native.call("sgl_amd_xgmi_debug_auto_blocks_cap", max(8, 128 // int(os.environ.get("WORLD_SIZE", "2"))))
        ps.init_distributed_environment(backend="gloo", device_index=0)
    else:
        ps.init_distributed_environment()
    world = ps.get_tensor_model_parallel_world_size()
    rank = int(os.environ.get("RANK", "0"))
    _trace(f"process groups up (world {world}), xGMI communicator {'on' if ps.get_xgmi_all_reduce() is not None else 'off'}")
    if args.rank_of:
        if world != 1 or args.gpus != 1:
            raise SystemExit("--rank-of runs on one GPU (--gpus 1)")
        ps.emulate_tensor_parallel_rank(0, args.rank_of, torch.device("cuda", torch.cuda.current_device()))
    tp = args.rank_of or world           # the TP degree the shapes belong to
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the job has {world} rank(s) (WORLD_SIZE="
                         f"{os.environ.get('WORLD_SIZE', 'unset')}): refusing to report a {world}-GPU number as {args.gpus}")
    dev = torch.device("cuda", torch.cuda.current_device())
    if args.model not in CONFIGS:
        raise SystemExit(f"unknown --model {args.model}; choices: {sorted(CONFIGS)}")
    cfg = CONFIGS[args.model]
    reduced = False
    if args.layers:
        import dataclasses

        cfg = dataclasses.replace(cfg, num_hidden_layers=args.layers)
        reduced = True

    G = args.groups * (tp if args.scaling == "weak" else 1)   # weak scaling: the batch grows with the TP degree
    P = args.per_group
    B = G * P
    in_len = args.prefix + args.unique
    ctx = in_len + args.out + 8
    prompts = build_prompts(cfg, G, P, args.prefix, args.unique)

    runner = ModelRunner(cfg, max_total_tokens=B * (in_len + args.out) + 4096, max_running_requests=B,
                         max_context_len=ctx, page_size=args.page_size, device=dev, use_graph=not args.no_graph,
                         graph_max_bs=B, strict_graph=True, kv_cache_dtype=args.kv_cache_dtype)
    _trace("model built, decode graphs captured")
    if not args.no_graph and runner.graph_runner is None:
        raise SystemExit("hipGraph decode was requested but no graph runner exists")
    if runner.model.config.name != cfg.name:
        raise SystemExit(f"built {runner.model.config.name}, asked for {cfg.name}")
    eng = Engine(runner)

    def sync():
        torch.cuda.synchronize()

    def barrier():
        if world > 1:
            dist.barrier()

    phase_times = []
    ttfts = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def job(record: bool, trace=None):
        # identical work every step: drop the previous step's tree / slots
        runner.tree_cache.reset()
        runner.token_to_kv_pool_allocator.clear()
        runner.req_to_token_pool.clear()
        eng.logits_device_trace = trace
        t0 = time.perf_counter()
        rid = 0
        leaders, rest = [], []
        for g in range(G):
            for p in range(P):
                q = Req(rid, prompts[g][p], args.out)
                q.t_arrive = t0
                (leaders if p == 0 else rest).append(q)
                rid += 1
        # the leaders' ids are handed over once the second pass is queued (the reference's overlap loop): the host
        # prepares the second pass under the first one's forward, and the phase boundary is a HIP event, not a sync
        e0.record()
        eng.prefill(leaders, defer_ids=bool(rest) and os.environ.get("SGLANG_AMD_BENCH_SYNC_PREFILL") != "1")
        e1.record()
        _trace("cold prefill queued")
        if rest:
            eng.prefill(rest)
        sync(); t2 = time.perf_counter()
        t1 = min(t2, t0 + e0.elapsed_time(e1) * 1e-3)
        _trace("warm prefill done")
        for _ in range(args.out - 1):
            eng.decode_step()
            eng.flush_decode_outputs(lag=1)   # per-step token hand-off, one step behind the launch (overlap scheduling)
        sync(); t3 = time.perf_counter()
        _trace("decode done")
        reqs = list(eng.running)
        hit = sum(q.cached_tokens for q in reqs)
        eng.finish(reqs)
        t4 = time.perf_counter()
        if record:
            phase_times.append((t1 - t0, t2 - t1, t3 - t2, t4 - t3))
            ttfts.extend(q.t_first_token - q.t_arrive for q in reqs)
        assert all(len(q.output_ids) == args.out for q in reqs)
        eng.logits_device_trace = None
        return hit, reqs

    for _ in range(args.warmup):
        job(False)
    sync(); barrier()
    t_start = time.perf_counter()
    hit_tokens, last_reqs = 0, []
    for _ in range(args.steps):
        hit_tokens, last_reqs = job(True)
    sync(); barrier()
    elapsed = time.perf_counter() - t_start
    if world > 1:
        t = torch.tensor([elapsed], device="cpu" if share_gpu else dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if args.dump_outputs and rank == 0 and last_reqs:
        dump_outputs(Path(args.dump_outputs), runner, last_reqs)

    out_tokens = B * args.out * args.steps
    value = out_tokens / elapsed
    cold = statistics.mean(p[0] for p in phase_times)
    warm = statistics.mean(p[1] for p in phase_times)
    dec = statistics.mean(p[2] for p in phase_times)
    t_decode_step = dec / max(1, args.out - 1)
    pmc = load_pmc()

    # ---- rooflines ------------------------------------------------
    L, Hq, Hkv, D = cfg.num_hidden_layers, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    kv_heads_rank = max(1, Hkv // tp)
    kv_fp8 = args.kv_cache_dtype == "fp8_e4m3"
    kv_row = 2 * L * kv_heads_rank * D * (1 if kv_fp8 else 2)   # bytes per cached token on one rank, all layers (131072 for 8B TP=1)
    plin = p_lin(cfg)
    w_act = decode_weight_bytes(cfg, B) / tp
    mean_len = in_len + args.out / 2
    kv_unique = (G * args.prefix + B * (mean_len - args.prefix)) * kv_row
    kv_nodedup = B * mean_len * kv_row
    kv_write = B * kv_row
    step_bytes = w_act + kv_unique + kv_write
    step_traffic = None
    if pmc_current(pmc) and pmc.get("model") == cfg.name and pmc.get("batch") == B and world == 1 and not kv_fp8:
        step_traffic = pmc.get("phases", {}).get("decode", {}).get("hbm_bytes_per_step")
    step_roofline = dict(bound="hbm", achieved=step_bytes / t_decode_step / 1e9, peak=HBM_PEAK_GBPS, unit="GB/s",
                         frac=step_bytes / t_decode_step / 1e9 / HBM_PEAK_GBPS, traffic=step_traffic,
                         traffic_source=PMC_NAME + ": sum over one eager decode step's dispatches of "
                                        "2 x FETCH_SIZE + WRITE_SIZE (separate rocprofv3 --pmc passes)",
                         bytes_per_step=step_bytes, kv_bytes_no_dedup=kv_nodedup, ms_per_decode_step=t_decode_step * 1e3)
    # The headline `roofline` is the WHOLE decode step -- one replay of the captured hipGraph is the path's launch unit --
    # not its best kernel: algorithmic bytes of SURVEY 8(d) per step / the measured step time.  The
    # kernels the step is made of follow in `kernel_table`, the largest of them in `dominant_kernel_roofline`.
    headline = dict(step_roofline)
    headline["kernel"] = ("one decode step = one hipGraph replay (per layer: qkv GEMM + rope/store combine, cascade attention + "
                          "merge, o_proj GEMM + add/norm combine, gate_up GEMM with silu epilogue, down GEMM + add/norm combine; "
                          "then lm_head + arg-max)")
    headline["us_per_launch"] = t_decode_step * 1e6
    headline["bytes_per_launch"] = step_bytes
    pair = 4 * L * Hq * D
    flops_cold = G * (2 * in_len * plin + pair * (in_len * (in_len + 1) / 2) + 2 * cfg.hidden_size * cfg.vocab_size)
    flops_warm = (B - G) * (2 * args.unique * plin + pair * (args.unique * args.prefix + args.unique * (args.unique + 1) / 2)
                            + 2 * cfg.hidden_size * cfg.vocab_size)
    prefill_tflops = (flops_cold + flops_warm) / tp / (cold + warm) / 1e12

    decode_mode = ("hipGraph" if runner.graph_runner is not None else "eager") + \
                  (", operator surface (unfused per-op hooks)" if args.operator_surface else ", fused TP=1 decode layer"
                   if tp == 1 else "")
    result = {
        "metric": "output tokens/s + p50 TTFT, Llama-3-8B TP=1 shared-prefix batch; 70B TP=8",
        "value": value, "unit": "tokens/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": args.scaling,
        "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "config": {"workload": f"{cfg.name} shared-prefix batch: {G} groups x {P} prompts, {args.prefix} shared + "
                               f"{args.unique} unique in, {args.out} out, greedy, page_size {args.page_size}"
                               + (" [fp8_e4m3 KV pool -- not the baseline configuration]" if kv_fp8 else "")
                               + (f" [REDUCED: {args.layers} layers -- not a valid bench line]" if reduced else ""),
                   "model": cfg.name, "global_batch": B, "seq_len": in_len,
                   "parallelism": (f"tp{world}" + (f" as {world} processes time-slicing ONE GPU (gloo groups, xGMI kernels over hipIpc): a dry run "
                                                      "of the launch path -- NOT a multi-GPU measurement" if share_gpu else "")) if not args.rank_of else
                   f"RANK SHAPES of tp{tp} on 1 GPU: rank 0's weight shards, the tp{tp} job's batch, collectives = world-of-1 "
                   f"loopback launches of the xGMI kernels (no wire time) -- not a multi-GPU measurement",
                   "decode": decode_mode},
        "ttft_p50_ms": statistics.median(ttfts) * 1e3,
        "phase_ms": {"prefill_cold": cold * 1e3, "prefill_warm": warm * 1e3, "decode": dec * 1e3},
        "decode_tokens_per_s": B / t_decode_step,
        "radix_hit_tokens": hit_tokens,
        "roofline": headline,
        "step_roofline": step_roofline,
        "prefill_mfma": {"achieved": prefill_tflops, "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": prefill_tflops / MFMA_PEAK_TFLOPS},
    }

    # ---- dominant hand-written kernels, measured live with HIP events on torch's stream ----
    if args.full and rank == 0 and not args.no_kernel_roofline and not args.rank_of:
        try:
            result["pmc_record"] = {"file": PMC_NAME, "present": pmc is not None, "all_sources_current": pmc_current(pmc),
                                    "git_revision": pmc["stamp"].get("git_revision") if pmc else None}
            kernel_rooflines(args, cfg, runner, result, B, G, P, in_len, ctx, t_decode_step, pmc, dev, world)
        except Exception as e:      # the measured line must survive a failure of these side measurements
            result.setdefault("dominant_kernel_roofline", {"error": f"{type(e).__name__}: {e}"})

    # ---- parity of this very job against the oracle's plain torch ops on the GPU ----------
    if args.full and rank == 0 and world == 1 and not args.no_parity and not kv_fp8 and not args.rank_of:
        try:
            from oracle.parity import teacher_forced_parity

            trace = []
            _, reqs = job(False, trace)
            order = [q.rid for q in reqs]
            inv = torch.tensor([order.index(i) for i in range(B)], device=dev)
            first = torch.cat(trace[:2]) if B > G else trace[0]
            steps_l = [first] + trace[(2 if B > G else 1):]
            steps_l = [s[inv] for s in steps_l]
            by_rid = sorted(reqs, key=lambda q: q.rid)
            flat = [p for grp in prompts for p in grp]
            t0 = time.perf_counter()
            rep = teacher_forced_parity(cfg, runner.model, flat, [q.output_ids for q in by_rid], steps_l, device=dev)
            rep["oracle"] = ("oracle/model.py on the GPU (plain torch SDPA / F.linear = the reference's torch_native "
                             "path), teacher-forced with this job's tokens, all prefill + decode positions")
            rep["seconds"] = time.perf_counter() - t0
            rep["north_star_tolerance"] = 1e-3
            result["parity"] = rep
            del trace, steps_l
            # per layer / per stage from the oracle's own inputs (tests/test_layer_parity_gpu.py asserts the same figures)
            if cfg.num_local_experts == 0:
                import dataclasses

                from oracle.layer_parity import _Patch, run_layer_parity, summarize

                patch = _Patch()
                try:
                    lcfg = dataclasses.replace(cfg, num_hidden_layers=min(3, cfg.num_hidden_layers), name=cfg.name + "-3layers")
                    lens = [33 + (7 * b) % 61 for b in range(64)]
                    rep["per_layer"] = summarize(*run_layer_parity(lcfg, dev, lens, patch, operator_surface=args.operator_surface))
                    rep["per_layer"]["workload"] = "the model's first three layers, B=64, prompts of 33..93 tokens: prefill + one decode step"
                finally:
                    patch.undo()
        except Exception as e:
            result["parity"] = {"error": f"{type(e).__name__}: {e}"}

    # ---- CPU baseline: the oracle (reference torch-native path) on host cores --------------
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and not args.rank_of:
        try:
            result["cpu_baseline"] = cpu_baseline(args, cfg, runner, prompts)
        except Exception as e:
            result["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}"}

    # ---- the same job under the REFERENCE'S scheduler with the plug-in (what a user of sglang gets) ------------------
    if (args.full and rank == 0 and world == 1 and not args.no_reference_scheduler and not args.rank_of and not kv_fp8 and not reduced
            and not args.operator_surface and args.page_size == 1 and cfg.name == "llama-3-8b"):
        try:
            result["reference_scheduler"] = reference_scheduler_leg(args)
        except Exception as e:
            result["reference_scheduler"] = {"error": f"{type(e).__name__}: {e}"}

    # top-level copies of the figures BASELINE.json's metric names beside tokens/s (the driver's record keeps top-level keys)
    result["ttft_p50_ms"] = statistics.median(ttfts) * 1e3
    result["prefill_mfma_frac"] = result["prefill_mfma"]["frac"]
    result["decode_step_hbm_frac"] = step_roofline["frac"]
    result["ms_per_decode_step"] = t_decode_step * 1e3
    rs = result.get("reference_scheduler") or {}
    result["reference_scheduler_tokens_per_s"] = rs.get("tokens_per_s")

    if rank == 0:
        print(json.dumps(result))
    if world > 1 or args.rank_of:
        ps.destroy()


DUMP_LOGITS_BYTES = 48 << 20   # of --dump-outputs' 64 MB: the float32 logits rows; the ids and hit counts are a few hundred KB


def dump_outputs(out_dir, runner, reqs):
    """--dump-outputs: the arrays the caller of the last timed step holds when it returns, read AFTER the timed region (nothing
    is recorded inside it).  `reqs` are that step's requests in the running batch's order = the row order of the decode graph's
    output buffer, which still holds the logits of the step's last decode launch; every array is written in request-id order."""
    import numpy as np

    out_dir.mkdir(parents=True, exist_ok=True)
    order = sorted(range(len(reqs)), key=lambda i: reqs[i].rid)
    np.save(out_dir / "output_ids.npy", np.asarray([reqs[i].output_ids for i in order], dtype=np.float64))
    np.save(out_dir / "cached_tokens.npy", np.asarray([reqs[i].cached_tokens for i in order], dtype=np.float64))
    gr = runner.graph_runner
    if gr is None:                  # --no-graph: an eager step keeps no logits behind
        return
    bs = next(b for b in gr.capture_bs if b >= len(reqs))
    logits = gr.outputs[bs][:len(reqs)]
    keep = max(1, DUMP_LOGITS_BYTES // (logits.shape[-1] * 4))
    rows = list(range(len(reqs))) if len(reqs) <= keep else sorted(random.Random(0).sample(range(len(reqs)), keep))
    picked = torch.tensor([order[r] for r in rows], device=logits.device)
    np.save(out_dir / "last_decode_logits.npy", logits[picked].float().cpu().numpy())
    np.save(out_dir / "last_decode_logits_rows.npy", np.asarray(rows, dtype=np.float64))


def reference_scheduler_leg(args):
    """BASELINE's job shape under the reference's OWN `Scheduler.run_event_loop()` (the server's default overlap loop), `ModelRunner`,
    `ScheduleBatch`, radix cache, allocator / pool classes from the platform factories and graph runner -- with this package loaded
    by the reference's plug-in loader: what a user of sglang who installs the plug-in runs.  The reference's
    sources are not on the GPU box: `__graft_entry__.build()` stages a copy under oracle/_ref (git-ignored, test infrastructure)
    in the build container, and tests/golden/ref_model.py imports it with the absent third-party packages stubbed; without a
    staged copy the leg reports that and nothing else.  Runs in its own process after the timed region; `value` above stays the
    harness measurement -- this figure is reported beside it, with the kernels the reference's loop adds (its eager slot
    bookkeeping, sampling glue, output streaming) inside its clock."""
    import subprocess
    import tempfile

    script = ROOT / "tests" / "golden" / "ref_model.py"
    staged = ROOT / "oracle" / "_ref" / "sglang_model" / "sglang"
    ref = os.environ.get("SGLANG_REFERENCE_ROOT")
    if not (staged.exists() or (ref and os.access(os.path.join(ref, "python", "sglang"), os.R_OK))):
        return {"skipped": "no staged reference sources (oracle/_ref/sglang_model): run __graft_entry__.build() with SGLANG_REFERENCE_ROOT "
                           "naming a checkout of the reference"}
    job = f"{args.groups},{args.per_group},{args.prefix},{args.unique},{args.out}"
    out = Path(tempfile.mkdtemp(prefix="ref_sched_")) / "job.json"
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, str(script), "--run", "scheduler", "--dims", "llama3_8b", "--job", job, "--overlap", "--json", str(out)],
                       cwd=ROOT, env=dict(os.environ, SGLANG_USE_AITER="0"), capture_output=True, text=True, timeout=420)
    if p.returncode != 0 or not out.exists():
        return {"error": (p.stderr or p.stdout)[-800:]}
    rep = json.loads(out.read_text())
    t = rep["timed"]
    return {"tokens_per_s": t["output_tokens_per_s"], "seconds_per_job": t["seconds"], "decode_step_ms_p50": t.get("decode_step_ms_p50"),
            "event_loop": rep["event_loop"], "scheduler": rep["scheduler"], "graph_runner": rep["graph_runner"],
            "graph_replays": rep["graph_replays_in_the_timed_job"], "eager_decode_forwards": rep["eager_fused_decode_forwards_in_the_timed_job"],
            "batches_run": t["batches_run"], "radix_hit_tokens_per_request": t["cached_tokens_of_others"],
            "finished_requests": t["finished_requests"], "triton_launches": rep.get("triton_launches_in_the_timed_job"),
            "kv_pool_class": rep.get("kv_pool_class"), "allocator_class": rep.get("allocator_class"),
            "attention_backend": rep["attention_backend"], "sampler_class": rep["sampler_class"], "plugin_counts": rep.get("plugin_counts"),
            "job": f"{args.groups} x {args.per_group} requests, {args.prefix} shared + {args.unique} own tokens in, {args.out} out, greedy; leaders "
                   "first, the others once the leaders decode (their prompts are in the radix tree); Llama-3-8B architecture, dummy weights",
            "wall_s_incl_start_up": time.perf_counter() - t0,
            "note": "the reference's Scheduler (staged copy of its sources, zmq socket read scripted) with this package as its plug-in; "
                    "not `value` (the harness job above), reported beside it"}


def kernel_rooflines(args, cfg, runner, result, B, G, P, in_len, ctx, t_decode_step, pmc, dev, world):
    from sglang_amd import kernels as K

    D = cfg.head_dim

    def graph_time(fn, launches, reps=10, warm=10):
        """Average duration of one launch: `fn` (which enqueues `launches` kernels) captured into a
        hipGraph, replayed `reps` times between two HIP events on the current stream.  `warm` untimed replays run
        first, back to back with the timed ones: the first replays after host-side work measure 8-10 % slower
        (benchmarks/archive/r02_exp19_model_weights.py: 45.5 us, then 41.8 us for the same launches)."""
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        for _ in range(warm):
            g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (reps * launches) * 1e-3

    # (1) the kernel with the largest share of the step: the weight-streaming GEMM of gate_up_proj
    # (fused silu_and_mul epilogue).  One launch per layer over the model's OWN weights, so every
    # launch streams a different 235 MB from HBM (nothing is left in the 256 MiB infinity cache).
    mlps = [layer.mlp for layer in runner.model.layers if hasattr(layer.mlp, "gate_up_proj")]
    Mg = min(B, 64)               # the weight-streaming design point (larger per-rank batches: DESIGN.md)
    if mlps and K.wstream_preferred(Mg, *mlps[0].gate_up_proj.weight.shape):
        wN, wK = mlps[0].gate_up_proj.weight.shape
        # the call the timed decode step makes: the fused TP=1 layer hands activations between its GEMMs chunk-major
        # ([K/128, M, 128], LlamaMLP.forward_fused_norm); the operator-surface path passes plain [M, K] rows
        blocked = world == 1 and not args.operator_surface and cfg.hidden_size % 128 == 0 and wN % 256 == 0
        if blocked:
            xg = K.blocked_activation(Mg, cfg.hidden_size, dev)
            xg.copy_(torch.randn(xg.shape, device=dev).to(torch.bfloat16))
        else:
            xg = torch.randn((Mg, cfg.hidden_size), device=dev).to(torch.bfloat16)
        t_g = graph_time(lambda: [K.wstream_gemm(xg, m.gate_up_proj.weight.data, epilogue="silu_and_mul", out_blocked=blocked)
                                  for m in mlps], len(mlps))
        alg = wN * wK * 2 + Mg * wK * 2 + Mg * (wN // 2) * 2      # weights once + activations in + out
        nw_s = K.choose_wstream_config(Mg, wN, wK, True, True)
        rec = pmc_kernel(pmc, "decode", "wstream_gemm_kernel<4, 4, 2", "wstream_gemm.hip") if (Mg, wN, wK) == (64, 28672, 4096) else None
        result["dominant_kernel_roofline"] = {"bound": "hbm", "achieved": alg / t_g / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                              "frac": alg / t_g / 1e9 / HBM_PEAK_GBPS, "traffic": hbm_bytes(rec),
                              "traffic_source": PMC_NAME + ": 2 x FETCH_SIZE (gfx950 counts 64 B per 128 B "
                                                "request) + WRITE_SIZE, KiB per dispatch",
                              "kernel": "wstream_gemm_kernel<4,4,2> (gate_up_proj + silu_and_mul)",
                              "us_per_launch": t_g * 1e6, "bytes_per_launch": alg,
                              "shape": {"M": Mg, "N": wN, "K": wK, "waves_per_group": nw_s[0], "k_splits": nw_s[1],
                                        "activations": "chunk-major [K/128, M, 128]" if blocked else "row-major [M, K]"},
                              "rocprof_note": "the --stats row of this instance averages the layers' gate_up launches with the "
                                              "step's one lm_head launch (same template instance, 4.4 x the bytes)",
                              "share_of_decode_step": len(mlps) * t_g / t_decode_step}
        # the other weight streams of the layer, each over the model's own 32 (80) matrices: what the step's time is made of
        rows = [dict(kernel="gate_up_proj + silu_and_mul (wstream_gemm_kernel)", us=t_g * 1e6, bytes=alg, launches_per_layer=1)]
        try:
            layers = list(runner.model.layers)
            attn0 = layers[0].self_attn
            Hq_, Hkv_, D_ = attn0.num_heads, attn0.num_kv_heads, attn0.head_dim
            H_ = cfg.hidden_size
            pool = runner.token_to_kv_pool
            pos_g = torch.full((Mg,), in_len, dtype=torch.int64, device=dev)
            loc_g = torch.arange(1, Mg + 1, dtype=torch.int64, device=dev)
            res_g = torch.randn((Mg, H_), device=dev).to(torch.bfloat16)
            xn = K.blocked_activation(Mg, H_, dev) if blocked else torch.randn((Mg, H_), device=dev).to(torch.bfloat16)
            a_in = torch.randn((Mg, Hq_ * D_), device=dev).to(torch.bfloat16)
            act_in = K.wstream_gemm(xg, mlps[0].gate_up_proj.weight.data, epilogue="silu_and_mul", out_blocked=blocked)
            if world == 1 and not args.operator_surface and attn0.qkv_proj.bias is None:
                t_q = graph_time(lambda: [K.wstream_qkv_rope(xn, l.self_attn.qkv_proj.weight.data, None, pos_g, l.self_attn.rotary_emb.cos_sin_cache,
                                                             Hq_, Hkv_, D_, pool.get_key_buffer(i), pool.get_value_buffer(i), loc_g)
                                          for i, l in enumerate(layers)], len(layers))
                nq = (Hq_ + 2 * Hkv_) * D_
                rows.append(dict(kernel="qkv_proj + rope + KV-row store (wstream GEMM + combine)", us=t_q * 1e6,
                                 bytes=nq * H_ * 2 + Mg * H_ * 2 + Mg * nq * 2, launches_per_layer=2))
                t_o = graph_time(lambda: [K.wstream_gemm(a_in, l.self_attn.o_proj.weight.data, epilogue="add_rmsnorm", residual=res_g,
                                                         norm_weight=l.post_attention_layernorm.weight.data, eps=1e-5, out_blocked=True)
                                          for l in layers], len(layers))
                rows.append(dict(kernel="o_proj + residual add + RMSNorm (wstream GEMM + combine)", us=t_o * 1e6,
                                 bytes=H_ * Hq_ * D_ * 2 + Mg * Hq_ * D_ * 2 + 3 * Mg * H_ * 2, launches_per_layer=2))
                t_d = graph_time(lambda: [K.wstream_gemm(act_in, l.mlp.down_proj.weight.data, epilogue="add_rmsnorm", residual=res_g,
                                                         norm_weight=l.input_layernorm.weight.data, eps=1e-5, out_blocked=True)
                                          for l in layers], len(layers))
                rows.append(dict(kernel="down_proj + residual add + next RMSNorm (wstream GEMM + combine)", us=t_d * 1e6,
                                 bytes=H_ * (wN // 2) * 2 + Mg * (wN // 2) * 2 + 3 * Mg * H_ * 2, launches_per_layer=2))
            head = runner.model.lm_head.data
            if K.wstream_preferred(Mg, *head.shape):
                hn = torch.randn((Mg, H_), device=dev).to(torch.bfloat16)
                t_h = graph_time(lambda: K.wstream_gemm(hn, head), 1, reps=20)
                rows.append(dict(kernel="lm_head (wstream_gemm_kernel)", us=t_h * 1e6, bytes=head.numel() * 2 + Mg * H_ * 2 + Mg * head.shape[0] * 2,
                                 launches_per_step=1))
        except Exception as e:      # side measurements: the table may be short, the line survives
            rows.append(dict(kernel="(table incomplete)", error=f"{type(e).__name__}: {e}"))
        for r in rows:
            if "us" in r:
                r["achieved"] = r["bytes"] / r["us"] / 1e3
                r["frac"] = r["achieved"] / HBM_PEAK_GBPS
                n_l = len(mlps) if "launches_per_layer" in r else 1
                r["share_of_decode_step"] = n_l * r["us"] * 1e-6 / t_decode_step
        result["kernel_table"] = {"unit": "GB/s of algorithmic bytes (weights once + activations in / out), HIP-event timed over the "
                                          "model's own weights in captured graphs", "peak": HBM_PEAK_GBPS, "rows": rows}

    # (1b) mixture-of-experts models: the dominant kernels are the two grouped expert GEMMs of fused_experts at the
    # decode batch (align -> up + silu -> down x router weight -> sum): bytes = the experts hit x their three matrices
    moes = [layer.mlp.experts for layer in runner.model.layers if hasattr(layer.mlp, "experts")]
    if moes:
        Mg = min(B, 64)
        xg = torch.randn((Mg, cfg.hidden_size), device=dev).to(torch.bfloat16)
        tw, ti = K.topk_softmax(torch.randn((Mg, cfg.num_local_experts), device=dev), cfg.num_experts_per_tok, True)
        hit = int(torch.unique(ti).numel())
        t_m = graph_time(lambda: [K.fused_experts(xg, m.w13_weight.data, m.w2_weight.data, tw, ti) for m in moes], len(moes))
        E_, N2, Kd = moes[0].w13_weight.shape
        alg = hit * (N2 * Kd + Kd * (N2 // 2)) * 2 + Mg * Kd * 2 * 2
        result["dominant_kernel_roofline"] = {"bound": "hbm", "achieved": alg / t_m / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                              "frac": alg / t_m / 1e9 / HBM_PEAK_GBPS, "traffic": None,
                              "kernel": "fused_experts at the decode batch: moe_align + wstream grouped up-GEMM (silu_and_mul "
                                        "epilogue) + grouped down-GEMM (x router weight) + moe_sum_reduce",
                              "us_per_launch": t_m * 1e6, "bytes_per_launch": alg,
                              "shape": {"M": Mg, "experts": E_, "experts_hit": hit, "top_k": cfg.num_experts_per_tok,
                                        "N": N2 // 2, "K": Kd},
                              "share_of_decode_step": len(moes) * t_m / t_decode_step}
        # and at a prefill batch: the row-tiled MFMA form
        Mp = 4096
        xp = torch.randn((Mp, cfg.hidden_size), device=dev).to(torch.bfloat16)
        twp, tip = K.topk_softmax(torch.randn((Mp, cfg.num_local_experts), device=dev), cfg.num_experts_per_tok, True)
        t_p = graph_time(lambda: K.fused_experts(xp, moes[0].w13_weight.data, moes[0].w2_weight.data, twp, tip), 1, reps=3)
        fl = Mp * cfg.num_experts_per_tok * 3 * (N2 // 2) * Kd * 2
        plan = K.moe_tile_plan(Mp * cfg.num_experts_per_tok, cfg.num_local_experts, N2 // 2, Kd)
        result["moe_prefill_mfma"] = {"kernel": ("moe_gemm256_kernel (256 x 256 x 64 tiles)" if plan[1] == 256 else
                                                 "moe_tiled_gemm_kernel (128 x 128 tiles)") + " x 2 + moe_align + moe_sum_reduce",
                                      "tile_plan(align, up rows, down rows)": list(plan), "M": Mp,
                                      "ms": t_p * 1e3, "achieved": fl / t_p / 1e12, "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                                      "frac": fl / t_p / 1e12 / MFMA_PEAK_TFLOPS}

    # (2) decode attention over the workload's own slot pattern (shared prefix rows + private rows)
    from sglang_amd.layers.attention.hip_backend import choose_num_splits

    Hq_r, Hkv_r = runner.num_attention_heads_per_rank, runner.num_kv_heads_per_rank
    len_k = in_len + args.out // 2
    r2t = runner.req_to_token_pool.req_to_token
    perm = (torch.randperm(runner.token_to_kv_pool.size - 1, device=dev) + 1).to(torch.int32)
    off = 0
    for b in range(B):
        r2t[b + 1, :len_k] = perm[off: off + len_k]
        off += len_k
        leader = (b // P) * P
        r2t[b + 1, :args.prefix] = r2t[leader + 1, :args.prefix]
    pool_idx = torch.arange(1, B + 1, device=dev)
    seq = torch.full((B,), len_k, dtype=torch.int32, device=dev)
    q = torch.randn((B, Hq_r, D), device=dev).to(torch.bfloat16)
    o = torch.empty_like(q)
    kc, vc = runner.token_to_kv_pool.get_key_buffer(0), runner.token_to_kv_pool.get_value_buffer(0)
    kc.normal_(); vc.normal_()
    row_bytes = 2 * Hkv_r * D * 2
    NREP = 8
    att = {}
    if D in (64, 128) and B >= 2:
        cws = K.CascadeWorkspace(B, Hq_r, D, ctx, dev)
        K.cascade_plan(cws, r2t, pool_idx, seq, Hq_r, Hkv_r)
        # (NREP calls per captured graph, like the layer loop of a step: one call per replay adds the replay's own ~5 us
        # to a 20 us launch pair)
        t_c = graph_time(lambda: [K.cascade_decode_attention(cws, q, kc, vc, o, r2t, pool_idx, seq, D ** -0.5) for _ in range(NREP)],
                         NREP, reps=10)
        # ... and the same launches over EIGHT layers' pools in turn: every row then comes from HBM, as inside the step (one layer's
        # 65 MB stay in the 256 MiB memory-side cache from replay to replay: the figure above is a cache-warm one)
        nl = min(NREP, len(runner.model.layers))
        pools = [(runner.token_to_kv_pool.get_key_buffer(i), runner.token_to_kv_pool.get_value_buffer(i)) for i in range(nl)]
        t_cc = graph_time(lambda: [K.cascade_decode_attention(cws, q, kc_, vc_, o, r2t, pool_idx, seq, D ** -0.5) for kc_, vc_ in pools],
                          nl, reps=10) if nl >= 4 else None
        uniq = (G * args.prefix + B * (len_k - args.prefix)) * row_bytes
        tr = None
        casc_src = ("cascade_attention.hip", "cascade_plan.hpp")
        rc, rm = pmc_kernel(pmc, "decode", "cascade_chunk_kernel", *casc_src), pmc_kernel(pmc, "decode", "cascade_merge2_kernel", *casc_src)
        if hbm_bytes(rc) is not None and hbm_bytes(rm) is not None:
            tr = hbm_bytes(rc) + hbm_bytes(rm)
        att["cascade"] = {"kernel": "cascade_chunk_kernel + cascade_merge2_kernel", "us_per_layer": t_c * 1e6,
                          "bytes_unique": uniq, "achieved": uniq / t_c / 1e9, "frac": uniq / t_c / 1e9 / HBM_PEAK_GBPS,
                          "traffic": tr,
                          "us_per_layer_cold_pools": t_cc * 1e6 if t_cc else None,
                          "frac_cold_pools": uniq / t_cc / 1e9 / HBM_PEAK_GBPS if t_cc else None}
    splits = choose_num_splits(B, Hkv_r, Hq_r // Hkv_r, len_k)
    ws = K.decode_workspace(B, Hq_r, D, splits, dev) if splits > 1 else (None, None)
    t_k = graph_time(lambda: [K.decode_attention(q, kc, vc, o, r2t, pool_idx, seq, D ** -0.5, splits, ws[0], ws[1]) for _ in range(NREP)],
                     NREP, reps=10)
    alg = B * len_k * row_bytes     # len * (2*H_kv*D*2 B) per request and layer, no dedup
    att["plain"] = {"kernel": "decode_stage1_kernel", "us_per_layer": t_k * 1e6, "bytes_no_dedup": alg,
                    "achieved": alg / t_k / 1e9, "frac": alg / t_k / 1e9 / HBM_PEAK_GBPS}
    result["attention_roofline"] = {"bound": "hbm", "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                    "shape": {"B": B, "Hq": Hq_r, "Hkv": Hkv_r, "D": D, "kv_len": len_k,
                                              "shared_prefix": args.prefix, "groups": G}, **att}

    # (3) the hand-written prefill kernel: extend attention of the cold pass (G x in_len causal) and of the warm
    # pass ((B-G) x unique over a prefix), MFMA bound
    ext = {}
    for name, nreq, pre, e in (("cold", G, 0, in_len), ("warm", B - G, args.prefix, args.unique)):
        if nreq <= 0:
            continue
        T = nreq * e
        qx = torch.randn((T, Hq_r, D), device=dev).to(torch.bfloat16)
        ox = torch.empty_like(qx)
        seq_x = torch.full((nreq,), pre + e, dtype=torch.int32, device=dev)
        pre_x = torch.full((nreq,), pre, dtype=torch.int32, device=dev)
        qo = (torch.arange(nreq + 1, device=dev) * e).to(torch.int32)
        pool_x = torch.arange(1, nreq + 1, device=dev)
        t_x = graph_time(lambda: [K.extend_attention(qx, ox, kc, vc, r2t, pool_x, seq_x, pre_x, qo, e, D ** -0.5, True) for _ in range(NREP)],
                         NREP, reps=5)
        fl = nreq * 4 * Hq_r * D * (e * pre + e * (e + 1) / 2)
        ext[name] = {"us": t_x * 1e6, "tflops": fl / t_x / 1e12, "frac": fl / t_x / 1e12 / MFMA_PEAK_TFLOPS,
                     "shape": {"requests": nreq, "extend": e, "prefix": pre}}
    rec = pmc_kernel(pmc, "prefill_cold", "extend_attention", "extend_attention.hip")
    if rec and rec.get("GRBM_GUI_ACTIVE") and rec.get("SQ_VALU_MFMA_BUSY_CYCLES") is not None:
        # busy SIMD-cycles / (active cycles per XCD x 1024 SIMDs); GRBM_GUI_ACTIVE is summed over the 8 XCDs on gfx950
        ext["mfma_util_pmc"] = rec["SQ_VALU_MFMA_BUSY_CYCLES"] * 8 / (rec["GRBM_GUI_ACTIVE"] * 1024)
        ext["pmc"] = {k: rec[k] for k in rec if k != "dispatches"}
    result["prefill_mfma"]["extend_attention_kernel"] = ext
    whole = pmc.get("phases", {}).get("prefill_cold", {}) if pmc_current(pmc) else {}
    if whole.get("mfma_util") is not None:
        result["prefill_mfma"]["mfma_util"] = whole["mfma_util"]
        result["prefill_mfma"]["mfma_util_source"] = (PMC_NAME + ": sum of SQ_VALU_MFMA_BUSY_CYCLES over the "
                                                      "cold prefill's dispatches / (sum of GRBM_GUI_ACTIVE / 8 XCDs x 1024 SIMDs)")

    # (4) the sampler at the decode batch: temperature 1, top_k 50, top_p 0.9, seeded, [B, vocab]
    # logits in the model dtype -- Sampler.forward end to end (widen, softmax_temperature, radix-select top-k / top-p,
    # seeded gumbel arg-max) and the greedy arg-max beside it
    from sglang_amd.layers.sampler import LogitsProcessorOutput, Sampler, SamplingBatchInfo

    V = cfg.vocab_size
    Bs = min(B, 64)
    lg = (torch.randn((Bs, V), device=dev) * 2.0).to(torch.bfloat16)
    info = SamplingBatchInfo(torch.ones((Bs, 1), device=dev), torch.full((Bs,), 0.9, device=dev),
                             torch.full((Bs,), 50, dtype=torch.int32, device=dev), torch.zeros(Bs, device=dev), False,
                             need_top_p_sampling=True, need_top_k_sampling=True,
                             sampling_seed=torch.arange(Bs, device=dev, dtype=torch.int64) + 1234)
    pos_s = torch.full((Bs,), in_len, dtype=torch.int64, device=dev)
    smp = Sampler()
    t_s = graph_time(lambda: smp(LogitsProcessorOutput(next_token_logits=lg), info, positions=pos_s), 1, reps=20)
    t_a = graph_time(lambda: K.argmax(lg), 1, reps=20)
    alg_s = Bs * V * 4
    result["sampler"] = {"bound": "hbm", "kernel": "Sampler.forward on bf16 logits: sample_logit_candidates_kernel (softmax partials + every column "
                                                    "range's largest logits, from registers) + sample_finish_fast_kernel (probabilities of the candidates only, "
                                                    "pruned list ranked in LDS, the three rules, fp64 gumbel arg-max with the reference's murmur hash; rows the "
                                                    "candidates cannot decide are redone from their full probability row there)",
                         "config": {"temperature": 1.0, "top_k": 50, "top_p": 0.9, "seeded": True, "batch": Bs, "vocab": V},
                         "us_per_call": t_s * 1e6, "algorithmic_bytes": alg_s, "achieved": alg_s / t_s / 1e9, "peak": HBM_PEAK_GBPS,
                         "unit": "GB/s", "frac": alg_s / t_s / 1e9 / HBM_PEAK_GBPS,
                         "note": "algorithmic bytes stay SURVEY 8(d)'s B x V x 4 B (the fp32 probabilities read once) so that rounds compare; "
                                 "since round 6 the path reads the B x V x 2 B bf16 logits once and never writes the probabilities -- "
                                 "what bounds it is the vector ALU (one fp32 division and one expf per logit for the softmax sum), not memory",
                         "greedy_argmax_us": t_a * 1e6, "share_of_decode_step_if_sampling": t_s / t_decode_step}


def cpu_baseline(args, cfg, runner, prompts):
    """the oracle (reference CPU torch-native path) timed on the host cores with the identical phases
    (cold prefill of the group leader, radix-style warm prefill of the others, greedy decode), wall clock via
    perf_counter after one warm-up forward, bounded to about --cpu-budget-s:
      (a) Qwen2.5-0.5B end to end (BASELINE configs[0]) at the WORKLOAD'S OWN prompt shape -- one group of 4 prompts,
          896 shared + 128 unique tokens in, 16 out;
      (b) the benchmarked model at B = 4 with its GPU weights copied to the host, the prompt shape sized from two probe
          forwards so that the leg fits the budget, with tokens and FLOPs stated so that the figure can be scaled."""
    from oracle.model import OracleLM, weights_from_product_model
    from sglang_amd.harness.models import CONFIGS, CausalLM

    cores = torch.get_num_threads()
    legs = {}

    def flops_of(cfg_x, pre, uni, n_req, n_out):
        pl = p_lin(cfg_x)
        pair = 4 * cfg_x.num_hidden_layers * cfg_x.num_attention_heads * cfg_x.head_dim
        n_in = pre + uni
        head = 2 * cfg_x.hidden_size * cfg_x.vocab_size
        cold = 2 * n_in * pl + pair * n_in * (n_in + 1) / 2 + head
        warm = (n_req - 1) * (2 * uni * pl + pair * (uni * pre + uni * (uni + 1) / 2) + head)
        dec = sum(n_req * (2 * pl + pair * (n_in + s) + head) for s in range(1, n_out))
        return cold + warm + dec

    def run(cfg_x, w, pre, uni, n_req, n_out, label):
        rnd = random.Random(1)
        sys_p = [rnd.randrange(cfg_x.vocab_size) for _ in range(pre)]
        ps_ = [sys_p + [rnd.randrange(cfg_x.vocab_size) for _ in range(uni)] for _ in range(n_req)]
        slots = n_req * (pre + uni + n_out) + 64
        OracleLM(cfg_x, w, num_slots=64, max_ctx=16, max_reqs=1).generate([ps_[0][:2]], 1)      # warm-up
        t0 = time.perf_counter()
        OracleLM(cfg_x, w, num_slots=slots, max_ctx=pre + uni + n_out + 8, max_reqs=n_req).generate(
            ps_, n_out, share_prefix_groups=[list(range(n_req))], shared_len=pre)
        dt = time.perf_counter() - t0
        fl = flops_of(cfg_x, pre, uni, n_req, n_out)
        return {"tokens_per_s": n_req * n_out / dt, "wall_s": dt, "tokens_in": n_req * (pre + uni),
                "tokens_in_computed": pre + uni + (n_req - 1) * uni, "tokens_out": n_req * n_out, "flops": fl,
                "gflops_per_s": fl / dt / 1e9,
                "sample": f"{label}: 1 group x {n_req} prompts, {pre} shared + {uni} unique in, {n_out} out, greedy, "
                          f"bf16, cold + radix-style warm prefill + {n_out - 1} decode steps"}

    budget = args.cpu_budget_s
    t_begin = time.perf_counter()
    # (b) -- first, with the whole budget to itself -- the benchmarked model, B = 4: a 2-token forward costs one pass over
    # the weights (t_w), a 64-token forward adds 62 tokens of compute -> per-token cost c; then
    # cold + warm + decode = 11 u c + (n_out + 1) t_w  for prompts of 7 u + u.  Never below 224 + 32 tokens in and 8 decode
    # steps (the earlier 28 + 4 / 2-out sample was a toy), even where that exceeds the budget a little.
    w = weights_from_product_model(runner.model)

    def probe(n):
        t0 = time.perf_counter()
        OracleLM(cfg, w, num_slots=n + 8, max_ctx=n + 8, max_reqs=1).generate([list(range(1, n + 1))], 1)
        return time.perf_counter() - t0

    t_w = probe(2)
    t_64 = probe(64)
    c_tok = max((t_64 - t_w) / 62.0, 1e-4)
    left = max(budget - (time.perf_counter() - t_begin), 4 * t_w)
    n_out = 16 if left > 24 * t_w else max(9, int(left / t_w / 2))
    u = int(max(0.0, left - (n_out + 1) * t_w) / (11.0 * c_tok))
    u = max(32, min(args.unique, u // 4 * 4))
    pre = u * (args.prefix // max(args.unique, 1)) if args.unique else 7 * u
    legs[cfg.name] = run(cfg, w, pre, u, 4, n_out, f"{cfg.name} (GPU weights copied to the host)")
    legs[cfg.name]["probe"] = {"weights_pass_s": t_w, "per_prompt_token_s": c_tok}
    main_leg = legs[cfg.name]
    del w
    # (a) Qwen2.5-0.5B end to end (BASELINE configs[0]) at the workload's OWN prompt shape, 8 tokens out
    qcfg = CONFIGS["qwen2.5-0.5b"]
    if cfg.name != qcfg.name:
        qm = CausalLM(qcfg, torch.device("cpu"), "cpu")
        legs[qcfg.name] = run(qcfg, weights_from_product_model(qm), args.prefix, args.unique, 4, 8, "qwen2.5-0.5b end to end")
        del qm
    # the same job on the GPU side, for scale: FLOPs of the measured workload per second of the timed run
    return {"value": main_leg["tokens_per_s"], "unit": "tokens/s", "cores": cores, "kind": "port",
            "sample": main_leg["sample"] + f"; {main_leg['wall_s']:.1f} s wall", "host_cpu_count": os.cpu_count(),
            "tokens_in": main_leg["tokens_in"], "tokens_out": main_leg["tokens_out"], "flops": main_leg["flops"],
            "workload_flops_ratio": flops_of(cfg, args.prefix, args.unique, args.per_group, args.out) * args.groups / main_leg["flops"],
            "legs": legs, "budget_s": budget, "wall_s_all_legs": time.perf_counter() - t_begin,
            "note": "reported baseline, not the optimisation target.  The leg of the benchmarked model (`value`) keeps B = 4 and the "
                    "7 : 1 shared : unique ratio, with prompts of at least 224 + 32 tokens and at least 8 decode steps, sized from two "
                    "probe forwards to --cpu-budget-s; the Qwen2.5-0.5B leg runs the workload's own prompt shape (896 + 128 in, B = 4, "
                    "8 out) on top of that budget -- tokens_in / tokens_out / flops are stated, workload_flops_ratio = FLOPs of the "
                    "whole benchmarked job / FLOPs of this sample"}


if __name__ == "__main__":
    main()
