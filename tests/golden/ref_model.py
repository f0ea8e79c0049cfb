"""The REAL reference model stack around the drop-in boundary -- `sglang.srt.plugins.load_plugins()` (entry-point discovery,
srt/plugins/__init__.py:103-141), `sglang.srt.platforms.current_platform` (srt/platforms/__init__.py:49-150), `ServerArgs`,
`init_distributed_environment` / `initialize_model_parallel` (srt/distributed/parallel_state.py), `LlamaForCausalLM` with
its `load_weights` (srt/models/llama.py), `LogitsProcessor`, `ForwardBatch.init_new`, the reference pools -- importable
WITHOUT an sglang install through gen_golden.py's import hook (ref_objects.py describes the hook and the staging).

Test infrastructure only: nothing here restates the reference; every reference line that runs is the reference's own.

The package under test is found the way an installed package is found: `fake_install()` writes the `*.dist-info` directory
that `pip install -e /root/repo` would write (name, version and the two entry-point groups of pyproject.toml) into a scratch
directory on sys.path, so `importlib.metadata.entry_points(group="sglang.srt.plugins" / "sglang.srt.platforms")` -- the
reference's own discovery -- returns `sglang_amd.plugin:load` and `sglang_amd.platform:activate`.
"""
from __future__ import annotations

import dataclasses
from contextlib import contextmanager
import importlib
import os
import sys
import tempfile
import types
from pathlib import Path

# before anything of the reference is imported: aiter is not in this image (the reference's own default is off), and the
# reference's `@torch.compile`d helpers (sampler.py multinomial_with_seed, ...) run as the plain torch code they wrap
os.environ.setdefault("SGLANG_USE_AITER", "0")
os.environ.setdefault("TORCHDYNAMO_DISABLE", "1")

import torch  # noqa: E402

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
sys.path.insert(0, str(HERE))
import ref_objects as R  # noqa: E402

# packages whose __init__ must run (the model files import names through them) + the modules of the model stack
MODEL_REAL = {
    "sglang.srt.utils", "sglang.srt.utils.hf_transformers", "sglang.srt.utils.hf_transformers_utils", "sglang.srt.server_args",
    "sglang.srt.distributed", "sglang.srt.distributed.parallel_state", "sglang.srt.platforms", "sglang.srt.plugins",
    "sglang.srt.plugins.hook_registry", "sglang.srt.layers.utils", "sglang.srt.layers.rotary_embedding", "sglang.srt.layers.linear",
    "sglang.srt.layers.vocab_parallel_embedding", "sglang.srt.layers.logits_processor", "sglang.srt.layers.quantization.unquant",
    "sglang.srt.layers.activation", "sglang.srt.layers.sampler", "sglang.srt.layers.attention.attention_registry",
    "sglang.srt.layers.moe.moe_runner.base", "sglang.srt.models.llama",
}
STAGE = REPO / "oracle" / "_ref" / "sglang_model"      # its own staged copy: ref_objects.py's (a verified, smaller file set) stays as it is
_state = {}


def ref_root():
    """The checkout SGLANG_REFERENCE_ROOT names, else the staged copy, else None (REF_OBJECTS_ROOT forces a root: tests of the staged copy)."""
    forced = os.environ.get("REF_OBJECTS_ROOT")
    if forced:
        return Path(forced) if (Path(forced) / "sglang").exists() else None
    if R.has_checkout():
        return R.CONTAINER_REF
    return STAGE if (STAGE / "sglang").exists() else None


def fake_install() -> Path:
    """What `pip install -e .` leaves on sys.path: a dist-info directory with the entry points of pyproject.toml."""
    if "dist" in _state:
        return _state["dist"]
    try:
        import tomllib as toml
    except ImportError:                                    # python 3.10
        import tomli as toml
    proj = toml.loads((REPO / "pyproject.toml").read_text())["project"]
    d = Path(tempfile.mkdtemp(prefix="sglang_amd_site_"))
    info = d / f"{proj['name'].replace('-', '_')}-{proj['version']}.dist-info"
    info.mkdir()
    (info / "METADATA").write_text(f"Metadata-Version: 2.1\nName: {proj['name']}\nVersion: {proj['version']}\n")
    lines = []
    for group, eps in proj["entry-points"].items():
        lines.append(f"[{group}]")
        lines += [f"{k} = {v}" for k, v in eps.items()]
        lines.append("")
    (info / "entry_points.txt").write_text("\n".join(lines))
    sys.path.insert(0, str(d))
    if str(REPO) not in sys.path:
        sys.path.insert(0, str(REPO))
    importlib.invalidate_caches()
    _state["dist"] = d
    return d


def dry_run_on_cpu() -> bool:
    """The build container has no GPU.  The same script then runs as a plumbing check: a gfx950 device is pretended for
    the reference's import-time arch probes (`is_fp8_fnuz`), the reference's groups live on the CPU, and the reference's
    own torch-native operators compute -- the plug-in is NOT loaded (its kernels need the GPU)."""
    return not torch.cuda.is_available()


def install(root: Path | None = None):
    """Hook + the reference model stack imported.  Returns ref_objects' namespace with the extra modules attached."""
    if "ns" in _state:
        return _state["ns"]
    root = root or ref_root()
    if root is None:
        return None
    fake_install()
    if dry_run_on_cpu():
        props = types.SimpleNamespace(gcnArchName="gfx950:sramecc+:xnack-", name="AMD Instinct MI355X", total_memory=288 << 30,
                                      multi_processor_count=256, major=9, minor=5)
        torch.cuda.get_device_properties = lambda *a, **k: props
        torch.cuda.get_device_capability = lambda *a, **k: (9, 5)
        torch.cuda.get_device_name = lambda *a, **k: props.name
    import gen_golden as G

    G.REAL |= MODEL_REAL
    G.SUBMODULE_ATTRS = True
    G.ABSENT_ATTRS |= {"EntryClass"}     # models/registry.py registers every module that HAS an EntryClass: a stubbed one has none
    G.MSGSPEC_EMULATION = True        # msgspec.Struct classes of the reference construct for real (gen_golden._make_msgspec)
    G.TRY_PACKAGES = True             # package __init__ files run too (degrading to a stub package when one cannot import)
    ns = R.install(root)
    for m in sorted(MODEL_REAL):
        setattr(ns, m.replace("sglang.srt.", "").replace("sglang.", "").replace(".", "_"), importlib.import_module(m))
    if dry_run_on_cpu():
        # torch.version.hip is set in this image, so forward_batch_info binds `clamp_position` to the reference's
        # JIT-compiled device kernel (forward_batch_info.py:1811-1816; needs tvm_ffi + a GPU): the dry run takes the
        # reference's own other branch.  (On the GPU box the plug-in's hook serves the call -- position_hooks.py.)
        ns.forward_batch_info.clamp_position = ns.forward_batch_info._clamp_position_native
    _state["ns"] = ns
    return ns


def default_server_args(ns, **over):
    """A ServerArgs carrying the reference's own field defaults (the dataclass defaults of server_args.py), without the
    launch-time __post_init__ (which probes GPU memory, downloads configs ...); `over` = what the command line would set."""
    SA = ns.server_args.ServerArgs
    sa = object.__new__(SA)
    for f in dataclasses.fields(SA):
        if f.default is not dataclasses.MISSING:
            setattr(sa, f.name, f.default)
        elif f.default_factory is not dataclasses.MISSING:
            setattr(sa, f.name, f.default_factory())
        else:
            setattr(sa, f.name, None)
    for k, v in over.items():
        assert hasattr(sa, k), k
        setattr(sa, k, v)
    ns.server_args.set_global_server_args_for_scheduler(sa)
    return sa


def tp_world():
    """(world size, rank) of this process: one rank unless the TP launcher (`--tp N`) set RANK / WORLD_SIZE."""
    return int(os.environ.get("REF_MODEL_WORLD", "1")), int(os.environ.get("REF_MODEL_RANK", "0"))


def init_parallel(ns, port: int = 0):
    """The reference's own initialisers.  One rank: RCCL on the GPU box, gloo in the dry run.  TP > 1 (`--tp N`): N processes
    -- in the dry run on the CPU; on the GPU box all on GPU 0, where RCCL refuses several ranks of one device, so the
    groups' device backend is gloo there too (it moves CUDA tensors through the host) and the reference's pynccl wrapper is
    pointed at a missing library (its own "no NCCL library" branch: pynccl.py:70-76)."""
    PS = ns.distributed_parallel_state
    world, rank = tp_world()
    if dry_run_on_cpu():
        PS.is_cuda_alike = lambda: False
    # one GPU per rank where the box has them (the launcher below decides, REF_MODEL_MULTI_GPU): then the groups' device backend is
    # RCCL and the xGMI communicator's peers are other DEVICES -- the first multi-GPU lease exercises exactly what a `--tp N`
    # launch runs.  On a one-GPU box every rank sits on GPU 0 over gloo device groups (RCCL refuses several ranks of one device).
    multi_gpu = world > 1 and os.environ.get("REF_MODEL_MULTI_GPU") == "1" and not dry_run_on_cpu()
    if multi_gpu:
        torch.cuda.set_device(rank)
    if not PS.model_parallel_is_initialized():
        port = port or int(os.environ.get("REF_MODEL_PORT", 29500 + os.getpid() % 400))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        PS.init_distributed_environment(world_size=world, rank=rank, distributed_init_method=f"tcp://127.0.0.1:{port}",
                                        local_rank=rank if multi_gpu else 0,
                                        backend="gloo" if (dry_run_on_cpu() or (world > 1 and not multi_gpu)) else "nccl")
        PS.initialize_model_parallel(world)
        # ModelRunner.init_torch_distributed goes on to initialize_dp_attention(server_args, model_config) (dp_attention.py:343-375):
        # without dp attention that leaves the module at "one attention-dp replica, rank 0"
        dpa = importlib.import_module("sglang.srt.layers.dp_attention")
        dpa._ATTN_DP_SIZE, dpa._ATTN_DP_RANK = 1, 0
    return PS


@contextmanager
def parallel_ctx(ns):
    """The parallel sizes every reference component reads through `get_parallel()` are LIVE here: the groups of
    init_parallel() exist (ref_objects.py, which has no groups, overrides them instead)."""
    yield


# ---- the job: cold extend, warm extend over a cached prefix, decode steps, on the reference's LlamaForCausalLM ---------
DIMS = {
    # hidden, intermediate, layers, q heads, kv heads, head dim, vocab
    "tiny": (256, 512, 2, 8, 2, 64, 1024),
    "llama3_8b_2layers": (4096, 14336, 2, 32, 8, 128, 128256),
    # BASELINE.json configs[0]'s architecture (Qwen2.5-0.5B: qkv bias, tied embeddings, 14 / 2 heads of 64), whole depth
    "qwen2.5_0.5b": (896, 4864, 24, 14, 2, 64, 151936),
    "tiny_qwen2": (256, 384, 2, 4, 2, 64, 768),
    # Mixtral's block (8 experts, top-2, renormalised softmax router) at small dimensions
    "tiny_mixtral": (512, 512, 2, 8, 2, 64, 1024),
    # BASELINE.json configs[1]'s architecture, whole depth (the latency run: dummy weights)
    "llama3_8b": (4096, 14336, 32, 32, 8, 128, 128256),
    "tiny_v16k": (256, 512, 2, 8, 2, 64, 16384),           # (the reference's synthetic prompts draw token ids below 10000)
}
ARCH = {"qwen2.5_0.5b": "qwen2", "tiny_qwen2": "qwen2", "tiny_mixtral": "mixtral"}      # default: llama
ROPE_THETA = {"qwen2": 1000000.0, "llama": 10000.0, "mixtral": 1000000.0}
EPS = {"qwen2": 1e-6, "llama": 1e-5, "mixtral": 1e-5}
EXPERTS, TOP_K = 8, 2


def hf_checkpoint(dims, device, seed=1, arch="llama"):
    """Random weights under the Hugging Face checkpoint names `LlamaForCausalLM.load_weights` (llama.py:640-720) /
    `Qwen2ForCausalLM.load_weights` (qwen2.py:600-680) expect: separate q / k / v and gate / up tensors, which the reference's
    own loader stacks into qkv_proj / gate_up_proj (and shards by TP rank).  qwen2: q / k / v biases, no lm_head tensor
    (tied to the embedding)."""
    H, I, L, Hq, Hkv, D, V = dims
    g = torch.Generator(device="cpu").manual_seed(seed)

    def rnd(*s, sc):
        return (torch.randn(s, generator=g) * sc).to(torch.bfloat16).to(device)

    sc_h, sc_i = H ** -0.5, I ** -0.5
    hf = {"model.embed_tokens.weight": rnd(V, H, sc=0.5 if arch == "llama" else sc_h * 4), "model.norm.weight": 1 + rnd(H, sc=0.1)}
    if arch != "qwen2":
        hf["lm_head.weight"] = rnd(V, H, sc=sc_h)
    for i in range(L):
        p = f"model.layers.{i}."
        if arch == "qwen2":
            hf[p + "self_attn.q_proj.bias"] = rnd(Hq * D, sc=0.2)
            hf[p + "self_attn.k_proj.bias"] = rnd(Hkv * D, sc=0.2)
            hf[p + "self_attn.v_proj.bias"] = rnd(Hkv * D, sc=0.2)
        hf[p + "input_layernorm.weight"] = 1 + rnd(H, sc=0.1)
        hf[p + "post_attention_layernorm.weight"] = 1 + rnd(H, sc=0.1)
        hf[p + "self_attn.q_proj.weight"] = rnd(Hq * D, H, sc=sc_h)
        hf[p + "self_attn.k_proj.weight"] = rnd(Hkv * D, H, sc=sc_h)
        hf[p + "self_attn.v_proj.weight"] = rnd(Hkv * D, H, sc=sc_h)
        hf[p + "self_attn.o_proj.weight"] = rnd(H, Hq * D, sc=(Hq * D) ** -0.5)
        if arch == "mixtral":                            # mixtral.py:395-405: experts.{e}.w1 (gate) / w3 (up) / w2 (down)
            hf[p + "block_sparse_moe.gate.weight"] = rnd(EXPERTS, H, sc=sc_h * 4)
            for e in range(EXPERTS):
                hf[p + f"block_sparse_moe.experts.{e}.w1.weight"] = rnd(I, H, sc=sc_h)
                hf[p + f"block_sparse_moe.experts.{e}.w3.weight"] = rnd(I, H, sc=sc_h)
                hf[p + f"block_sparse_moe.experts.{e}.w2.weight"] = rnd(H, I, sc=sc_i)
            continue
        hf[p + "mlp.gate_proj.weight"] = rnd(I, H, sc=sc_h)
        hf[p + "mlp.up_proj.weight"] = rnd(I, H, sc=sc_h)
        hf[p + "mlp.down_proj.weight"] = rnd(H, I, sc=sc_i)
    return hf


def oracle_weights(model):
    """The reference model's OWN parameters (after its loader stacked them) under the oracle's names."""
    m = model.model
    w = {"embed_tokens": m.embed_tokens.weight.data, "norm.weight": m.norm.weight.data, "lm_head": model.lm_head.weight.data}
    for i, layer in enumerate(m.layers):
        p = f"layers.{i}."
        w[p + "input_layernorm.weight"] = layer.input_layernorm.weight.data
        w[p + "post_attention_layernorm.weight"] = layer.post_attention_layernorm.weight.data
        w[p + "self_attn.qkv_proj.weight"] = layer.self_attn.qkv_proj.weight.data
        if getattr(layer.self_attn.qkv_proj, "bias", None) is not None:
            w[p + "self_attn.qkv_proj.bias"] = layer.self_attn.qkv_proj.bias.data
        w[p + "self_attn.o_proj.weight"] = layer.self_attn.o_proj.weight.data
        if hasattr(layer, "block_sparse_moe"):
            moe = layer.block_sparse_moe
            w[p + "mlp.gate.weight"] = moe.gate.weight.data
            w[p + "mlp.experts.w13_weight"] = moe.experts.w13_weight.data
            w[p + "mlp.experts.w2_weight"] = moe.experts.w2_weight.data
            continue
        w[p + "mlp.gate_up_proj.weight"] = layer.mlp.gate_up_proj.weight.data
        w[p + "mlp.down_proj.weight"] = layer.mlp.down_proj.weight.data
    return w


class _Batch:
    """What ForwardBatch.init_new reads of a ScheduleBatch: the fields a generation batch carries, None for the rest."""

    def __getattr__(self, n):
        if n.startswith("__"):
            raise AttributeError(n)
        return None


def build_model(ns, dims, device, arch="llama"):
    """`<Arch>ForCausalLM(config)` + `load_weights(checkpoint)` -- model_loader/loader.py:_initialize_model + load_weights
    under the loader's bf16 default dtype."""
    H, I, L, Hq, Hkv, D, V = dims
    common = dict(hidden_size=H, intermediate_size=I, num_hidden_layers=L, num_attention_heads=Hq, num_key_value_heads=Hkv, vocab_size=V,
                  max_position_embeddings=2048, rope_theta=ROPE_THETA[arch], rms_norm_eps=EPS[arch])
    if arch == "qwen2":
        from transformers import Qwen2Config

        cfg = Qwen2Config(**common, tie_word_embeddings=True)
        cls = importlib.import_module("sglang.srt.models.qwen2").Qwen2ForCausalLM
    elif arch == "mixtral":
        from transformers import MixtralConfig

        cfg = MixtralConfig(**common, num_local_experts=EXPERTS, num_experts_per_tok=TOP_K, tie_word_embeddings=False)
        cls = importlib.import_module("sglang.srt.models.mixtral").MixtralForCausalLM
    else:
        from transformers import LlamaConfig

        cfg = LlamaConfig(**common, head_dim=D, tie_word_embeddings=False)
        cls = ns.models_llama.LlamaForCausalLM
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device(device):
            model = cls(cfg)
    finally:
        torch.set_default_dtype(old)
    model.load_weights(list(hf_checkpoint(dims, device, arch=arch).items()))
    if tp_world()[0] > 1 and not dry_run_on_cpu():
        # all ranks of this test share ONE device: the reference's symmetric-memory multicast all-gather of the logits
        # (triton_symm_mem_ag.py: one device per rank) is set to its own "always the group's all_gather" state
        model.logits_processor._logits_gatherer._state = None
    return cfg, model.eval()


class Job:
    """The reference stack around one model: `LlamaForCausalLM`, the reference pools, a runner-shaped namespace carrying
    what `ForwardBatch.init_new` and the attention backend read of `ModelRunner`, the backend built by `backend_factory`,
    and the oracle on the reference model's own parameters.  Every forward is `ForwardBatch.init_new(batch, runner)` ->
    `backend.init_forward_metadata(fb)` -> `model.forward(input_ids, positions, fb)` inside `forward_context(...)`
    (model_runner.py:1664-1690), followed by the oracle's forward over the same tokens and slots."""

    def __init__(self, ns, dims, device, backend_factory, sa, arch="llama"):
        from oracle.model import OracleLM
        from sglang_amd.harness.models import ModelConfig

        self.ns, self.device, self.sa = ns, device, sa
        mp, self.fbi, self.fc = ns.memory_pool, ns.forward_batch_info, ns.forward_context
        H, I, L, Hq, Hkv, D, V = dims
        self.V = V
        tp, _ = tp_world()
        self.cfg, self.model = build_model(ns, dims, device, arch)
        self.g = torch.Generator().manual_seed(7)
        self.records = []
        with parallel_ctx(ns):
            self.r2t = mp.ReqToTokenPool(8, 1024, device, False)
            self.kv = mp.MHATokenToKVPool(4096, 1, torch.bfloat16, max(1, Hkv // tp), D, L, device, False, enable_alt_stream=False)
        mc = types.SimpleNamespace(model_is_mrope=False, get_num_attention_heads=lambda tp: Hq // tp, get_num_kv_heads=lambda tp: max(1, Hkv // tp),
                                   num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=D, is_encoder_decoder=False, vocab_size=V,
                                   hf_config=self.cfg, context_len=2048)
        self.runner = types.SimpleNamespace(device=device, is_draft_worker=False, lora_manager=None, prefill_attention_backend_str=sa.attention_backend,
                                            server_args=sa, ngram_embedding_manager=types.SimpleNamespace(enabled=False), model_config=mc,
                                            ps=types.SimpleNamespace(attn_dcp_size=1, attn_dcp_rank=0), req_to_token_pool=self.r2t,
                                            token_to_kv_pool=self.kv, sliding_window_size=None, tp_size=tp, attn_tp_size=tp, model=self.model,
                                            dtype=torch.bfloat16, kv_cache_dtype=torch.bfloat16, page_size=1)
        self.backend_factory = backend_factory
        with parallel_ctx(ns):
            self.backend = backend_factory(self.runner)
        ocfg = ModelConfig("ref", H, I, L, Hq, Hkv, D, V, EPS[arch], ROPE_THETA[arch], None, 2048, attention_bias=arch == "qwen2",
                           tie_word_embeddings=arch == "qwen2", num_local_experts=EXPERTS if arch == "mixtral" else 0,
                           num_experts_per_tok=TOP_K if arch == "mixtral" else 0)
        w = oracle_weights(self.model)
        tpg = None
        if tp > 1:
            # this rank's shards are the reference model's own parameters; the embedding table, which the reference shards by vocab
            # (VocabParallelEmbedding: masked lookup + all-reduce), is handed to the oracle whole
            import torch.distributed as dist

            tpg = ns.distributed_parallel_state.get_tp_group().cpu_group
            parts = [torch.empty_like(w["embed_tokens"]) for _ in range(tp)]
            dist.all_gather(parts, w["embed_tokens"].contiguous(), group=tpg)
            w["embed_tokens"] = torch.cat(parts, 0)[:V]
        self.olm = OracleLM(ocfg, w, num_slots=4096, max_ctx=1024, max_reqs=7, device=device, tp_size=tp, tp_group=tpg)
        # the same graph with fp32-accumulating attention: the yardstick both bf16 evaluations (the reference's literal one above,
        # the plug-in's) are measured against on the GPU -- "product vs reference" is judged inside the band "reference vs reference"
        self.olm32 = None if device == "cpu" else OracleLM(ocfg, w, num_slots=4096, max_ctx=1024, max_reqs=7, device=device,
                                                            compute_dtype=torch.float32, tp_size=tp, tp_group=tpg)
        self.slots = (torch.randperm(4000, generator=self.g) + 1).to(torch.int64).to(device)     # scattered slots; 0 is the padding slot
        self.cursor = 0
        self.pools, self.lens, self.next_ids = [], [], None

    def take(self, n):
        loc = self.slots[self.cursor: self.cursor + n]
        self.cursor += n
        return loc

    def batch(self, mode, ids, pools, seq, loc, extend=None, prefix=None):
        b = _Batch()
        b.forward_mode = mode
        b.seq_lens = torch.tensor(seq, device=self.device)
        b.seq_lens_cpu = torch.tensor(seq)
        b.seq_lens_sum = int(sum(seq))
        b.input_ids = ids
        b.req_pool_indices = torch.tensor(pools, device=self.device)
        b.out_cache_loc = loc
        b.reqs, b.has_grammar, b.return_logprob = [], False, False
        if extend is not None:
            b.extend_lens, b.prefix_lens, b.extend_num_tokens = list(extend), list(prefix), int(sum(extend))
            b.extend_logprob_start_lens = [0] * len(extend)
            b.is_extend_in_batch = True
        return b

    def forward_batch(self, b, backend=None):
        fbi = self.fbi
        fb = fbi.ForwardBatch.init_new(b, self.runner, capture_hidden_mode=fbi.CaptureHiddenMode.NULL, return_hidden_states_before_norm=False)
        return fb               # (nothing is attached: the reference resolves pools and backend through the forward context)

    def oracle(self, b, fb, extend, prefix):
        dec = extend is None
        dev = self.device
        outs = []
        for olm in (self.olm, self.olm32):
            if olm is None:
                outs.append(None)
                continue
            olm.req_to_token.copy_(self.r2t.req_to_token[:8])
            outs.append(olm.forward(b.input_ids, fb.positions, b.req_pool_indices, b.seq_lens, None if dec else torch.tensor(prefix, device=dev),
                                    None if dec else torch.tensor(extend, device=dev), b.out_cache_loc, dec).float().cpu())
        return outs

    def forward(self, mode, ids, pools, seq, loc, extend=None, prefix=None, what=""):
        with parallel_ctx(self.ns), torch.no_grad():
            b = self.batch(mode, ids, pools, seq, loc, extend, prefix)
            fb = self.forward_batch(b)
            if extend is not None:                     # the reference computed the positions (through the plug-in's hook on the GPU)
                want_pos = torch.cat([torch.arange(p, p + e) for p, e in zip(prefix, extend)])
            else:
                want_pos = torch.tensor(seq) - 1
            assert torch.equal(fb.positions.cpu(), want_pos) and fb.positions.dtype == torch.int64, (what, fb.positions)
            self.backend.init_forward_metadata(fb)
            with self.fc.forward_context(self.fc.ForwardContext(attn_backend=self.backend)):    # model_runner.py:1671-1674
                out = self.model.forward(fb.input_ids, fb.positions, fb)
            want, want32 = self.oracle(b, fb, extend, prefix)
        self.records.append(dict(what=what, got=out.next_token_logits.float().cpu(), want=want, want32=want32))
        return out.next_token_logits

    def prefill(self):
        fbi, r2t, g, dev = self.fbi, self.r2t, self.g, self.device
        # cold extend: three requests
        pools, lens = [1, 4, 2], [37, 130, 20]
        T = sum(lens)
        ids = torch.randint(0, self.V, (T,), generator=g).to(dev)
        loc = self.take(T)
        off = 0
        for b_, n in enumerate(lens):
            r2t.req_to_token[pools[b_], :n] = loc[off: off + n].to(torch.int32)
            off += n
        logits = self.forward(fbi.ForwardMode.EXTEND, ids, pools, lens, loc, extend=lens, prefix=[0, 0, 0], what="cold extend 37+130+20")
        # warm extend: a fourth request whose first 64 tokens ARE request 4's slots (a radix hit), 50 new tokens
        r2t.req_to_token[6, :64] = r2t.req_to_token[4, :64]
        loc_w = self.take(50)
        r2t.req_to_token[6, 64:114] = loc_w.to(torch.int32)
        ids_w = torch.randint(0, self.V, (50,), generator=g).to(dev)
        lw = self.forward(fbi.ForwardMode.EXTEND, ids_w, [6], [114], loc_w, extend=[50], prefix=[64], what="warm extend 50 over a 64-token prefix")
        self.pools, self.lens = pools + [6], lens + [114]
        self.next_ids = torch.cat([logits.argmax(-1), lw.argmax(-1)])

    def advance(self):
        """One new slot per request (what the scheduler's alloc_for_decode does before a decode forward)."""
        dl = self.take(len(self.pools))
        for b_, n in enumerate(self.lens):
            self.r2t.req_to_token[self.pools[b_], n] = dl[b_].to(torch.int32)
        self.lens = [n + 1 for n in self.lens]
        return dl

    def decode(self, steps=3):
        for step in range(steps):
            dl = self.advance()
            lg = self.forward(self.fbi.ForwardMode.DECODE, self.next_ids, self.pools, self.lens, dl, what=f"decode step {step} (4 requests)")
            self.next_ids = lg.argmax(-1)
        return lg

    def graph_decode(self, steps=2) -> dict:
        """The decode forward of the WHOLE reference model inside a hipGraph, through the reference's capture / replay
        protocol (base_attn_backend.py:65-107: init_cuda_graph_state; init_forward_metadata_out_graph(fb, in_capture=True)
        before the capture, init_forward_metadata_in_graph(fb) inside it, init_forward_metadata_out_graph(fb) before every
        replay) with the batch's tensors as the graph's static buffers -- what DecodeCudaGraphRunner does around
        `model.forward`.  Each replay is compared with the oracle like an eager pass."""
        fbi, fc, dev, B = self.fbi, self.fc, self.device, len(self.pools)
        with parallel_ctx(self.ns), torch.no_grad():
            backend = self.backend_factory(self.runner)
            backend.init_cuda_graph_state(B, B)
            ctx = fc.ForwardContext(attn_backend=backend)
            st_ids = self.next_ids.clone()
            st_loc = torch.zeros(B, dtype=torch.int64, device=dev)                # slot 0: the padding slot
            b = self.batch(fbi.ForwardMode.DECODE, st_ids, self.pools, self.lens, st_loc)
            fb = self.forward_batch(b, backend)
            st_seq, st_pos = fb.seq_lens, fb.positions
            backend.init_forward_metadata_out_graph(fb, in_capture=True)
            graph = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), fc.forward_context(ctx):
                backend.init_forward_metadata_in_graph(fb)
                self.model.forward(st_ids, st_pos, fb)                            # warm-up outside the capture
                side.synchronize()
                with torch.cuda.graph(graph, stream=side):
                    backend.init_forward_metadata_in_graph(fb)
                    out = self.model.forward(st_ids, st_pos, fb)
            torch.cuda.current_stream().wait_stream(side)
            for step in range(steps):
                dl = self.advance()
                st_ids.copy_(self.next_ids); st_loc.copy_(dl); st_seq.copy_(torch.tensor(self.lens)); st_pos.copy_(torch.tensor(self.lens) - 1)
                fb.seq_lens_cpu = torch.tensor(self.lens)
                backend.init_forward_metadata_out_graph(fb)
                graph.replay()
                torch.cuda.synchronize()
                b2 = self.batch(fbi.ForwardMode.DECODE, st_ids.clone(), self.pools, self.lens, dl)
                want, want32 = self.oracle(b2, types.SimpleNamespace(positions=st_pos.clone()), None, None)
                self.records.append(dict(what=f"hipGraph decode replay {step} (4 requests)", got=out.next_token_logits.float().cpu(),
                                         want=want, want32=want32))
                self.next_ids = out.next_token_logits.argmax(-1)
        return dict(replays=steps)


def sampler_leg(ns, sa, logits, positions, vocab, device) -> dict:
    """`create_sampler(backend)` (sampler.py:545-566: the registered factory for the plug-in's backend name, the
    reference's `Sampler()` for "pytorch") on the last decode step's logits, with a `SamplingBatchInfo` built by the
    reference's own `from_schedule_batch`: greedy everywhere; on the GPU also temperature + top-k + top-p with per-request
    seeds, where the plug-in's ids must EQUAL the ids of the reference's torch path on the same logits."""
    sbi = importlib.import_module("sglang.srt.sampling.sampling_batch_info")
    spm = importlib.import_module("sglang.srt.sampling.sampling_params")
    smp, lpo = ns.layers_sampler, ns.layers_logits_processor.LogitsProcessorOutput
    B = logits.shape[0]

    def info(**kw):
        reqs = []
        for i in range(B):
            p = spm.SamplingParams()               # (msgspec is absent here, and with it the Struct's generated constructor)
            fields = dict(temperature=1.0, top_k=1 << 30, top_p=1.0, min_p=0.0, sampling_seed=None, logit_bias=None,
                          custom_params=None, frequency_penalty=0.0, presence_penalty=0.0, repetition_penalty=1.0, min_new_tokens=0)
            fields.update({k_: (v_[i] if isinstance(v_, list) else v_) for k_, v_ in kw.items()})
            for k, v in fields.items():
                setattr(p, k, v)
            reqs.append(types.SimpleNamespace(sampling_params=p, custom_logit_processor=None, return_sampling_mask=False,
                                              origin_input_ids=[1, 2, 3], output_ids=[], rid=str(i)))
        batch = _Batch()                     # (the penalizer orchestrator keeps a weak reference to the batch)
        batch.reqs, batch.device = reqs, device
        return sbi.SamplingBatchInfo.from_schedule_batch(batch, vocab)

    def run(backend, inf):
        sa.sampling_backend = backend
        ns.server_args.set_global_server_args_for_scheduler(sa)
        out = lpo(next_token_logits=logits.clone())
        ids = smp.create_sampler(backend)(out, inf, False, [0] * B, [None] * B, positions)
        return ids.long().cpu()

    under_test = "pytorch" if dry_run_on_cpu() else sa.attention_backend        # (the plug-in registers both under one name)
    rep = dict(backend=under_test, sampler_class=type(smp.create_sampler(under_test)).__mro__[0].__name__,
               is_reference_subclass=isinstance(smp.create_sampler(under_test), smp.Sampler))
    greedy = run(under_test, info(temperature=0.0, top_k=1))
    rep["greedy_equals_argmax"] = bool(torch.equal(greedy, logits.argmax(-1).cpu()))
    if not dry_run_on_cpu():
        kw = dict(temperature=0.8, top_k=[20 + 7 * i for i in range(B)], top_p=[0.9 - 0.1 * (i % 3) for i in range(B)],
                  sampling_seed=[100 + i for i in range(B)])
        mine, ref = run(under_test, info(**kw)), run("pytorch", info(**kw))
        rep.update(seeded_ids=mine.tolist(), seeded_ids_reference=ref.tolist(), seeded_ids_equal=bool(torch.equal(mine, ref)))
    return rep


# ---- the three runs ----------------------------------------------------------------------------------------------------
def run_cpu_oracle(dims_name="tiny") -> dict:
    """Build container (no GPU, plug-in NOT loaded): the reference's `LlamaForCausalLM` with its torch-native attention
    backend and torch fused-op forwards on the CPU, against oracle/model.py on the same weights, tokens and slots.
    Pins the oracle's whole-model restatement: the logits must be IDENTICAL."""
    ns = install()
    from sglang.kernels import fused_op as FO
    from sglang.kernels.spec import KernelBackend

    # torch.version.hip is set in this image, so without a GPU the reference would still pick its HIP forwards (aiter /
    # sgl_kernel, absent): the reference's own switch forces every fused op onto its torch forward (fused_op.py:236)
    FO.set_fused_op_backend(KernelBackend.TORCH)
    sa = default_server_args(ns, model_path="dummy", attention_backend="torch_native", enable_deterministic_inference=True)
    init_parallel(ns)
    tnb = importlib.import_module("sglang.srt.layers.attention.torch_native_backend")
    job = Job(ns, DIMS[dims_name], "cpu", tnb.TorchNativeAttnBackend, sa, ARCH.get(dims_name, "llama"))
    job.prefill()
    lg = job.decode(3)
    sampler = sampler_leg(ns, sa, lg.clone(), torch.tensor(job.lens), job.V, "cpu")
    records = job.records
    return dict(mode="cpu-oracle", dims=dims_name, sampler=sampler,
                passes=[dict(what=r["what"], identical=bool(torch.equal(r["got"], r["want"])),
                             max_abs=float((r["got"] - r["want"]).abs().max()), ref_rms=float(r["want"].pow(2).mean().sqrt()))
                        for r in records])


def run_loader() -> dict:
    """Any box: the reference's own `load_plugins()` discovers the package through its entry points and executes
    `plugin.load()` against the REAL registries (no GPU work: registration only)."""
    ns = install()
    import sglang_amd.platform as P

    if dry_run_on_cpu():
        P.is_gfx950_visible = lambda: True            # activate() must answer as on the GPU box
    plat_mod = importlib.import_module("sglang.srt.platforms")
    plat_mod._current_platform = None                 # (resolved once at import of models/llama.py, before the line above)
    from sglang.kernels import fused_op as FO

    FO.clear_platform_caches()
    platform = plat_mod.current_platform
    PL = ns.plugins
    PL.load_plugins()
    from sglang.kernels.fused_op import BaseFusedOp
    from sglang.srt.layers.attention.attention_registry import ATTENTION_BACKENDS
    from sglang.srt.layers.moe.moe_runner.base import FusedOpPool
    from sglang.srt.layers.sampler import _CUSTOM_SAMPLER_FACTORIES
    from sglang.srt.plugins.hook_registry import HookRegistry
    from sglang.srt.server_args import ATTENTION_BACKEND_CHOICES, SAMPLING_BACKEND_CHOICES

    from sglang_amd.platform import BACKEND_NAME, DISPATCH_KEY

    oot = BaseFusedOp._oot_forward_registry.get(DISPATCH_KEY, {})
    return dict(mode="loader", platform=type(platform).__name__, out_of_tree=bool(platform.is_out_of_tree()),
                dispatch_key=platform.get_dispatch_key_name() if platform.is_out_of_tree() else None,
                default_attention_backend=platform.get_default_attention_backend() if platform.is_out_of_tree() else None,
                attention_backend_registered=BACKEND_NAME in ATTENTION_BACKENDS,
                attention_backend_choice=BACKEND_NAME in ATTENTION_BACKEND_CHOICES,
                sampler_registered=BACKEND_NAME in _CUSTOM_SAMPLER_FACTORIES, sampler_choice=BACKEND_NAME in SAMPLING_BACKEND_CHOICES,
                fused_moe_slot=getattr(FusedOpPool.get_fused_func("none", "triton"), "__qualname__", ""),
                oot_forwards=sorted(c.__name__ for c in oot),
                hooked=sorted(HookRegistry._hooks), hooks_applied=sorted(getattr(HookRegistry, "_patched", ())))


def run_gpu(dims_name="tiny") -> dict:
    """GPU box: plug-in discovered and loaded by the reference (launch_server.py:8 order: plug-ins first), the platform
    resolved by the reference (out-of-tree -> the registered forwards), the attention backend built by the reference's
    registry from the platform's default name, the reference's `LlamaForCausalLM` on cuda:0 -- and the job above.  The
    decode passes go through the AROUND hook on `LlamaModel.forward` (9 launches per layer), the prefill passes through the
    reference's own layer loop with the registered operator forwards and the hooked `UnquantizedLinearMethod.apply`."""
    loader = run_loader()
    ns = install()
    assert loader["out_of_tree"], loader
    from sglang.kernels import fused_op as FO
    from sglang.srt.layers.attention.attention_registry import ATTENTION_BACKENDS
    from sglang.srt.platforms import current_platform

    import sglang_amd.fused_decode as fd
    import sglang_amd.linear_hook as lh
    from oracle.layer_parity import ulp_stats

    sa = default_server_args(ns, model_path="dummy", attention_backend=current_platform.get_default_attention_backend(),
                             enable_deterministic_inference=True)
    init_parallel(ns)
    counts = dict(fused_decode_models=0, streamed_linears=0, library_linears=0)
    decode_model = fd.decode_model

    def counting_decode_model(*a, **k):
        counts["fused_decode_models"] += 1
        return decode_model(*a, **k)

    fd.decode_model = counting_decode_model
    takes = lh.takes

    def counting_takes(*a, **k):
        ok = takes(*a, **k)
        counts["streamed_linears" if ok else "library_linears"] += 1
        return ok

    lh.takes = counting_takes
    # MoE: the function in FusedOpPool's ("none", "triton") slot is what MoeRunner.run calls (runner.py:143-147; read once, when the
    # model is built): count its calls, and which of them the gfx950 grouped GEMMs served
    from sglang.srt.layers.moe.moe_runner.base import FusedOpPool

    import sglang_amd.layers.moe.fused_moe as hip_moe

    counts.update(moe_fused_func_calls=0, moe_hip_calls=0)
    slot = FusedOpPool._fused_funcs[("none", "triton")]

    def counting_slot(*a, **k):
        counts["moe_fused_func_calls"] += 1
        return slot(*a, **k)

    FusedOpPool._fused_funcs[("none", "triton")] = counting_slot
    hip_experts = hip_moe.fused_experts_none_to_hip

    def counting_hip_experts(*a, **k):
        counts["moe_hip_calls"] += 1
        return hip_experts(*a, **k)

    hip_moe.fused_experts_none_to_hip = counting_hip_experts
    comm = None
    if tp_world()[0] > 1:
        # the communicator tp_hooks.attach built inside the reference's GroupCoordinator.__init__ (None = not attached: the test fails)
        from sglang_amd import tp_hooks

        comm = tp_hooks.communicator_of(ns.distributed_parallel_state.get_tp_group())
        counts.update(xgmi_attached=comm is not None, xgmi_all_reduce=0, xgmi_all_reduce_add_rmsnorm=0, xgmi_all_gather=0)
        for meth, key in (("all_reduce_any", "xgmi_all_reduce"), ("all_reduce_add_rmsnorm", "xgmi_all_reduce_add_rmsnorm"),
                          ("all_gather", "xgmi_all_gather")):
            if comm is not None:
                def counted(*a_, __f=getattr(comm, meth), __k=key, **k_):
                    counts[__k] += 1
                    return __f(*a_, **k_)

                setattr(comm, meth, counted)
    # the reference's fused-op call trace (fused_op.py:241-312: which forward served which op); its record type is a msgspec
    # Struct (absent here), so the recorder is replaced by one that keeps the two strings
    trace = {}

    def record(op, label, args, kwargs):
        key = f"{type(op).__name__}:{label}"
        trace[key] = trace.get(key, 0) + 1

    FO._record_trace = record
    FO.enable_fused_op_trace()
    import traceback

    legs = {}

    def leg(name, fn):
        try:
            legs[name] = dict(ok=True, **(fn() or {}))
        except Exception:                                   # noqa: BLE001 -- every leg reports; the test asserts on all of them
            legs[name] = dict(ok=False, error=traceback.format_exc()[-3000:])
        return legs[name]["ok"]

    job = None
    last = {}

    def build():
        nonlocal job
        with parallel_ctx(ns):
            job = Job(ns, DIMS[dims_name], "cuda", ATTENTION_BACKENDS[sa.attention_backend], sa, ARCH.get(dims_name, "llama"))
        return dict(backend=type(job.backend).__name__, model=type(job.model).__name__,
                    rope=type(job.model.model.layers[0].self_attn.rotary_emb).__name__)

    if leg("build", build):
        if leg("prefill", job.prefill):
            if leg("decode", lambda: last.update(lg=job.decode(3))):
                leg("sampler", lambda: sampler_leg(ns, sa, last["lg"].clone(), torch.tensor(job.lens, device="cuda"), job.V, "cuda"))
                sa.sampling_backend = None
                leg("graph_decode", job.graph_decode)
    torch.cuda.synchronize()
    FO.disable_fused_op_trace()
    passes = []
    for r in (job.records if job is not None else []):
        st = ulp_stats(r["got"], r["want"])
        top2 = r["want"].topk(2, dim=-1).values
        clear = (top2[:, 0] - top2[:, 1]) > 4e-2
        e_p, e_r = r["got"] - r["want32"], r["want"] - r["want32"]                   # product / the reference's literal evaluation vs fp32-acc
        band = dict(product_rms_err=float(e_p.pow(2).mean().sqrt()), reference_rms_err=float(e_r.pow(2).mean().sqrt()),
                    product_max_err=float(e_p.abs().max()), reference_max_err=float(e_r.abs().max()))
        passes.append(dict(what=r["what"], **st, **band, max_err_over_2e2_bar=float(((r["got"] - r["want"]).abs() / (2e-2 + 2e-2 * r["want"].abs())).max()),
                           clear_rows=int(clear.sum()), argmax_agree=int((r["got"].argmax(-1)[clear] == r["want"].argmax(-1)[clear]).sum())))
    import gen_golden as G

    return dict(mode="gpu", dims=dims_name, loader=loader, legs=legs, counts=counts, fused_op_trace=trace, passes=passes,
                degraded_reference_modules=[n for n, _ in G.FAILED], unstaged_reference_modules=sorted(set(getattr(G, "NOT_FOUND", []))))


def write_checkpoint_config(dims_name, max_pos=2048) -> Path:
    """A model directory holding config.json only (the weights come from `--load-format dummy` or from hf_checkpoint())."""
    import json as _json
    import tempfile as _tf

    arch = ARCH.get(dims_name, "llama")
    H, I, L, Hq, Hkv, D, V = DIMS[dims_name]
    cfg = dict(hidden_size=H, intermediate_size=I, num_hidden_layers=L, num_attention_heads=Hq, num_key_value_heads=Hkv, vocab_size=V,
               max_position_embeddings=max_pos, rope_theta=ROPE_THETA[arch], rms_norm_eps=EPS[arch], torch_dtype="bfloat16", hidden_act="silu",
               bos_token_id=1, eos_token_id=2)
    if arch == "qwen2":
        cfg.update(architectures=["Qwen2ForCausalLM"], model_type="qwen2", tie_word_embeddings=True)
    elif arch == "mixtral":
        cfg.update(architectures=["MixtralForCausalLM"], model_type="mixtral", tie_word_embeddings=False, num_local_experts=EXPERTS,
                   num_experts_per_tok=TOP_K)
    else:
        cfg.update(architectures=["LlamaForCausalLM"], model_type="llama", tie_word_embeddings=False, head_dim=D)
    d = Path(_tf.mkdtemp(prefix="ref_model_ckpt_"))
    (d / "config.json").write_text(_json.dumps(cfg))
    return d


def oracle_config(dims_name, max_pos=2048):
    from sglang_amd.harness.models import ModelConfig as OCfg

    arch = ARCH.get(dims_name, "llama")
    H, I, L, Hq, Hkv, D, V = DIMS[dims_name]
    return OCfg("ref", H, I, L, Hq, Hkv, D, V, EPS[arch], ROPE_THETA[arch], None, max_pos, attention_bias=arch == "qwen2",
                tie_word_embeddings=arch == "qwen2", num_local_experts=EXPERTS if arch == "mixtral" else 0,
                num_experts_per_tok=TOP_K if arch == "mixtral" else 0)


# ---- one level up: the reference's ModelRunner, driven by the reference's own static-batch harness ----------------------------
def run_runner(dims_name="tiny", server_args=None) -> dict:
    """`sglang.benchmark.one_batch` (the module behind `python -m sglang.bench_one_batch`) is the reference's own way to run a
    model WITHOUT the scheduler process: `load_model` builds a real `ServerArgs` (its whole resolution pipeline), `ModelConfig`,
    `ModelRunner` (distributed init, model loader, KV-cache configurator + memory pools + allocator, attention backend from the
    registry, CUDA-graph runners) and `extend` / `decode` drive it with real `Req` / `ScheduleBatch` objects
    (`prepare_for_extend` / `prepare_for_decode`: the reference's allocators pick the slots), `ForwardBatch.init_new`,
    `ModelRunner.forward` (graph replay when the runner can) and `ModelRunner.sample`.  This run follows its correctness test
    (one_batch.py:677-727): prefill of the first `cut` tokens, extend over that cached prefix, greedy decode steps.

    Build container: device cpu, torch-native attention, no plug-in -> the oracle must reproduce every logit bit for bit.
    MI355X: the plug-in loaded by the reference's loader, `attention_backend` left to the platform, the reference's decode graphs
    captured around the hooked model -> the reference-vs-reference band."""
    import json as _json
    import tempfile as _tf

    gpu = not dry_run_on_cpu()
    loader = run_loader() if gpu else None
    ns = install()
    arch = ARCH.get(dims_name, "llama")
    H, I, L, Hq, Hkv, D, V = DIMS[dims_name]
    d = Path(_tf.mkdtemp(prefix="ref_model_ckpt_"))
    cfg = dict(hidden_size=H, intermediate_size=I, num_hidden_layers=L, num_attention_heads=Hq, num_key_value_heads=Hkv, vocab_size=V,
               max_position_embeddings=2048, rope_theta=ROPE_THETA[arch], rms_norm_eps=EPS[arch], torch_dtype="bfloat16", hidden_act="silu",
               bos_token_id=1, eos_token_id=2)
    if arch == "qwen2":
        cfg.update(architectures=["Qwen2ForCausalLM"], model_type="qwen2", tie_word_embeddings=True)
    elif arch == "mixtral":
        cfg.update(architectures=["MixtralForCausalLM"], model_type="mixtral", tie_word_embeddings=False, num_local_experts=EXPERTS,
                   num_experts_per_tok=TOP_K)
    else:
        cfg.update(architectures=["LlamaForCausalLM"], model_type="llama", tie_word_embeddings=False, head_dim=D)
    (d / "config.json").write_text(_json.dumps(cfg))
    if not gpu:
        from sglang.kernels import fused_op as FO
        from sglang.kernels.spec import KernelBackend

        FO.set_fused_op_backend(KernelBackend.TORCH)
        common = importlib.import_module("sglang.srt.utils.common")
        common.get_device_memory_capacity = ns.server_args.get_device_memory_capacity = lambda device=None: 288 * 1024   # (no rocminfo here)
        ns.distributed_parallel_state.is_cuda_alike = lambda: False
    else:
        # ServerArgs sizes its defaults from the device memory; the reference parses `rocm-smi` for it (utils/common.py:585-600),
        # which this box's image may not answer -- then the same number comes from the driver
        common = importlib.import_module("sglang.srt.utils.common")
        try:
            common.get_device_memory_capacity("cuda")
        except Exception:                                   # noqa: BLE001
            mib = torch.cuda.mem_get_info()[1] // (1 << 20)
            common.get_device_memory_capacity = ns.server_args.get_device_memory_capacity = lambda device=None: mib
    OB = importlib.import_module("sglang.benchmark.one_batch")
    # ---- what one_batch.load_model does (one_batch.py:299-362), minus the tokenizer -------------------------------------------
    kw = dict(model_path=str(d), load_format="dummy", skip_tokenizer_init=True, dtype="bfloat16", device="cuda" if gpu else "cpu",
              attention_backend=None if gpu else "torch_native", sampling_backend=loader["default_attention_backend"] if gpu else "pytorch",
              max_total_tokens=8192, max_running_requests=16, cuda_graph_max_bs_decode=8, mem_fraction_static=0.3, disable_radix_cache=True,
              random_seed=3)
    kw.update(server_args or {})
    sa = ns.server_args.ServerArgs(**kw)
    model_config = importlib.import_module("sglang.srt.configs.model_config").ModelConfig.from_server_args(sa)
    ps = importlib.import_module("sglang.srt.distributed.parallel_state_wrapper").ParallelState.trivial(gpu_id=0)
    MR = importlib.import_module("sglang.srt.model_executor.model_runner")
    counts = dict(fused_decode_models=0, graph_replays=0)
    if gpu:
        import sglang_amd.fused_decode as fd

        decode_model = fd.decode_model

        def counting_decode_model(*a, **k):
            counts["fused_decode_models"] += 1
            return decode_model(*a, **k)

        fd.decode_model = counting_decode_model
        # when a decode forward does NOT take the fused loop, say why (fused_decode.explain) -- first occurrence
        hook_orig = fd._reference_model_applies
        why = counts.setdefault("not_fused_because", [])

        def recording_applies(model, forward_batch, input_embeds, pp_proxy_tensors):
            ok = hook_orig(model, forward_batch, input_embeds, pp_proxy_tensors)
            mode = getattr(forward_batch, "forward_mode", None)
            if mode is not None and mode.is_decode() and len(why) < 3:
                try:
                    reason = fd.explain(model, forward_batch, None, input_embeds, pp_proxy_tensors)
                except Exception as e:                      # noqa: BLE001
                    reason = f"explain raised {type(e).__name__}: {e}"
                if reason is not None:
                    why.append(reason)
            return ok

        fd._reference_model_applies = recording_applies
    runner = MR.ModelRunner(model_config=model_config, mem_fraction_static=sa.mem_fraction_static, gpu_id=0, ps=ps,
                            nccl_port=29500 + os.getpid() % 400, server_args=sa)
    runner.alloc_memory_pool()
    runner.init_attention_backends()
    # real weights instead of the dummy loader's +-1e-3 noise: in place, through the reference's own load_weights
    runner.model.load_weights(list(hf_checkpoint(DIMS[dims_name], runner.device, arch=arch).items()))
    runner.init_cuda_graphs()
    captured = counts["fused_decode_models"]
    graph_runner = getattr(runner, "decode_cuda_graph_runner", None)
    if graph_runner is not None and hasattr(graph_runner, "execute"):
        execute = graph_runner.execute

        def counting_execute(*a, **k):
            counts["graph_replays"] += 1
            return execute(*a, **k)

        graph_runner.execute = counting_execute
    # ---- the oracle on the runner's own parameters, pools and slots -----------------------------------------------------------
    from oracle.model import OracleLM
    from sglang_amd.harness.models import ModelConfig as OCfg

    ocfg = OCfg("ref", H, I, L, Hq, Hkv, D, V, EPS[arch], ROPE_THETA[arch], None, 2048, attention_bias=arch == "qwen2",
                tie_word_embeddings=arch == "qwen2", num_local_experts=EXPERTS if arch == "mixtral" else 0,
                num_experts_per_tok=TOP_K if arch == "mixtral" else 0)
    dev = runner.device
    w = oracle_weights(runner.model)
    slots = int(runner.token_to_kv_pool.size) + int(runner.page_size) + 8
    kvd = "fp8_e4m3" if str(getattr(sa, "kv_cache_dtype", "auto")) == "fp8_e4m3" else "auto"       # the pool stores e4m3 rows (scale 1.0)
    olm = OracleLM(ocfg, w, num_slots=slots, max_ctx=8, max_reqs=1, device=dev, kv_cache_dtype=kvd)
    olm32 = OracleLM(ocfg, w, num_slots=slots, max_ctx=8, max_reqs=1, device=dev, compute_dtype=torch.float32, kv_cache_dtype=kvd) if gpu else None
    records = []

    def check(what, batch, logits, decode_):
        seq = batch.seq_lens.to(dev)
        if decode_:
            positions, prefix, extend = (seq - 1).to(torch.int64), None, None
        else:
            prefix = torch.tensor(batch.prefix_lens, device=dev)
            extend = torch.tensor(batch.extend_lens, device=dev)
            positions = torch.cat([torch.arange(p, p + e) for p, e in zip(batch.prefix_lens, batch.extend_lens)]).to(dev)
        outs = []
        for o in (olm, olm32):
            if o is None:
                outs.append(None)
                continue
            o.req_to_token = runner.req_to_token_pool.req_to_token            # the reference pool's own table (read only)
            outs.append(o.forward(batch.input_ids.to(dev), positions, batch.req_pool_indices.to(dev), seq, prefix, extend,
                                  batch.out_cache_loc.to(dev), decode_).float().cpu())
        records.append(dict(what=what, got=logits.float().cpu(), want=outs[0], want32=outs[1]))

    # ---- the reference's correctness test, with token ids instead of prompts (one_batch.py:377-437, 677-727) -------------------
    from array import array

    g = torch.Generator().manual_seed(11)
    cut, lens = 24, [61, 130, 37]
    ids = [torch.randint(3, V, (n,), generator=g).tolist() for n in lens]
    sp = importlib.import_module("sglang.srt.sampling.sampling_params").SamplingParams(temperature=0, max_new_tokens=8)
    Req = importlib.import_module("sglang.srt.managers.schedule_batch").Req
    reqs = []
    for i, t in enumerate(ids):
        req = Req(rid=i, origin_input_text="", origin_input_ids=array("q", t[:cut]), sampling_params=sp)
        req.full_untruncated_fill_ids = req.origin_input_ids
        req.logprob_start_len = -1
        req.set_extend_range(len(req.prefix_indices), len(req.origin_input_ids))
        reqs.append(req)
    with torch.no_grad():
        nxt, logits, batch = OB.extend(reqs, runner)
        check(f"prefill of the first {cut} tokens (3 requests)", batch, logits, False)
        for i, req in enumerate(reqs):                                       # prepare_extend_inputs_for_correctness_test
            req.full_untruncated_fill_ids.extend(ids[i][cut:])
            req.prefix_indices = runner.req_to_token_pool.req_to_token[req.req_pool_idx, :cut].to(req.prefix_indices.dtype)
            req.logprob_start_len = -1
            req.set_extend_range(len(req.prefix_indices), len(req.full_untruncated_fill_ids))
        nxt, logits, batch = OB.extend(reqs, runner)
        check(f"extend over the {cut}-token cached prefix (37 + 106 + 13 new tokens)", batch, logits, False)
        sampled = [nxt.tolist()]
        for step in range(4):
            nxt, logits = OB.decode(nxt, batch, runner)
            check(f"decode step {step} (3 requests)", batch, logits, True)
            sampled.append(nxt.tolist())
    passes = []
    for r in records:
        ps_ = dict(what=r["what"], identical=bool(torch.equal(r["got"], r["want"])), max_abs=float((r["got"] - r["want"]).abs().max()),
                   ref_rms=float(r["want"].pow(2).mean().sqrt()), argmax_equal=bool(torch.equal(r["got"].argmax(-1), r["want"].argmax(-1))))
        if r["want32"] is not None:
            e_p, e_r = r["got"] - r["want32"], r["want"] - r["want32"]
            ps_.update(product_rms_err=float(e_p.pow(2).mean().sqrt()), reference_rms_err=float(e_r.pow(2).mean().sqrt()),
                       product_max_err=float(e_p.abs().max()), reference_max_err=float(e_r.abs().max()))
        passes.append(ps_)
    import gen_golden as G

    return dict(mode="runner", dims=dims_name, device=str(dev), loader=loader, attention_backend=sa.attention_backend, server_args=server_args or {},
                kv_pool_dtype=str(getattr(runner.token_to_kv_pool, "dtype", None)),
                attn_backend_class=type(runner.attn_backend).__name__, sampler_class=type(runner.sampler).__name__,
                model=type(runner.model).__name__, kv_pool=type(runner.token_to_kv_pool).__name__,
                allocator=type(runner.token_to_kv_pool_allocator).__name__, max_total_num_tokens=int(runner.max_total_num_tokens),
                graph_runner=type(graph_runner).__name__ if graph_runner is not None else None,
                captured_batch_sizes=sorted(getattr(graph_runner, "capture_bs", []) or []) if graph_runner is not None else [],
                fused_decode_models_during_capture=captured, counts=counts, sampled=sampled, passes=passes,
                unstaged_reference_modules=sorted(set(getattr(G, "NOT_FOUND", []))))


def run_shared_prefix_job(dims_name="tiny_v16k", groups=2, per_group=2, prefix=16, unique=8, out=4, radix=False) -> dict:
    """BASELINE.json's job shape (configs[1]: `groups` x `per_group` requests, the first `prefix` tokens of a group's prompts shared,
    `unique` own tokens, `out` generated tokens, greedy) THROUGH THE REFERENCE'S RUNNER: the group leaders are prefilled cold, the
    other requests extend over the leader's slots (`req.prefix_indices` = what the radix cache hands a request whose prefix is
    cached -- set the way the reference's own correctness test sets it, one_batch.py:422-437), the two batches are merged with
    `ScheduleBatch.merge_batch` (what the scheduler does with a finished prefill batch) and decoded with
    `prepare_for_decode` -> `ModelRunner.forward` (graph replay) -> `ModelRunner.sample`.  One warm-up job, then the timed job.
    Build container: tiny model, real weights, every pass against the oracle (bit-identical).  MI355X: Llama-3-8B architecture, dummy
    weights, wall-clock tokens/s beside what bench.py measures on this package's harness.

    `radix=True`: the prefixes come out of the reference's REAL `RadixCache` instead: every request goes through
    `Req.init_next_round_input(tree_cache)` (RadixCache.match_prefix -> prefix_indices, last_node), the batches are built on the tree
    (`ScheduleBatch.init_new(tree_cache=...)`, so allocation may evict from it), and after each prefill the scheduler's
    `tree_cache.cache_unfinished_req(req)` inserts the request's tokens -- the other requests of a group then HIT the leader's
    `prefix` tokens; `cache_finished_req` releases everything at the end of the job."""
    import json as _json
    import tempfile as _tf
    import time
    from array import array

    gpu = not dry_run_on_cpu()
    loader = run_loader() if gpu else None
    ns = install()
    H, I, L, Hq, Hkv, D, V = DIMS[dims_name]
    d = Path(_tf.mkdtemp(prefix="ref_model_ckpt_"))
    (d / "config.json").write_text(_json.dumps(dict(
        architectures=["LlamaForCausalLM"], model_type="llama", hidden_size=H, intermediate_size=I, num_hidden_layers=L,
        num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=D, vocab_size=V, max_position_embeddings=8192, rope_theta=ROPE_THETA["llama"],
        rms_norm_eps=1e-5, tie_word_embeddings=False, torch_dtype="bfloat16", hidden_act="silu", bos_token_id=1, eos_token_id=2)))
    common = importlib.import_module("sglang.srt.utils.common")
    if not gpu:
        from sglang.kernels import fused_op as FO
        from sglang.kernels.spec import KernelBackend

        FO.set_fused_op_backend(KernelBackend.TORCH)
        common.get_device_memory_capacity = ns.server_args.get_device_memory_capacity = lambda device=None: 288 * 1024
        ns.distributed_parallel_state.is_cuda_alike = lambda: False
    else:
        try:
            common.get_device_memory_capacity("cuda")
        except Exception:                                   # noqa: BLE001
            mib = torch.cuda.mem_get_info()[1] // (1 << 20)
            common.get_device_memory_capacity = ns.server_args.get_device_memory_capacity = lambda device=None: mib
    OB = importlib.import_module("sglang.benchmark.one_batch")
    B = groups * per_group
    tokens = groups * (prefix + unique) + (B - groups) * unique + B * out
    sa = ns.server_args.ServerArgs(
        model_path=str(d), load_format="dummy", skip_tokenizer_init=True, dtype="bfloat16", device="cuda" if gpu else "cpu",
        attention_backend=None if gpu else "torch_native", sampling_backend=loader["default_attention_backend"] if gpu else "pytorch",
        max_total_tokens=tokens + 4096, max_running_requests=max(16, B), cuda_graph_max_bs_decode=B, mem_fraction_static=0.5,
        disable_radix_cache=not radix, random_seed=3)
    model_config = importlib.import_module("sglang.srt.configs.model_config").ModelConfig.from_server_args(sa)
    ps = importlib.import_module("sglang.srt.distributed.parallel_state_wrapper").ParallelState.trivial(gpu_id=0)
    MR = importlib.import_module("sglang.srt.model_executor.model_runner")
    runner = MR.ModelRunner(model_config=model_config, mem_fraction_static=sa.mem_fraction_static, gpu_id=0, ps=ps,
                            nccl_port=29500 + os.getpid() % 400, server_args=sa)
    runner.alloc_memory_pool()
    runner.init_attention_backends()
    if not gpu:
        runner.model.load_weights(list(hf_checkpoint(DIMS[dims_name], runner.device).items()))
    runner.init_cuda_graphs()
    dev = runner.device
    tree = None
    if radix:
        RC = importlib.import_module("sglang.srt.mem_cache.radix_cache").RadixCache
        CIP = importlib.import_module("sglang.srt.mem_cache.cache_init_params").CacheInitParams
        tree = RC(CIP(disable=False, req_to_token_pool=runner.req_to_token_pool, token_to_kv_pool_allocator=runner.token_to_kv_pool_allocator,
                      page_size=int(runner.page_size)))
        SB = importlib.import_module("sglang.srt.managers.schedule_batch")
        SpecNone = importlib.import_module("sglang.srt.speculative.spec_info").SpeculativeAlgorithm.NONE
        FBI = ns.forward_batch_info

        def extend_on_tree(reqs):
            """one_batch.extend (one_batch.py:487-523) with the real tree instead of its dummy namespace."""
            b = SB.ScheduleBatch.init_new(reqs=reqs, req_to_token_pool=runner.req_to_token_pool,
                                          token_to_kv_pool_allocator=runner.token_to_kv_pool_allocator, tree_cache=tree,
                                          model_config=runner.model_config, enable_overlap=False, spec_algorithm=SpecNone)
            b.prepare_for_extend()
            OB._maybe_prepare_mlp_sync_batch(b, runner)
            if b.input_ids is None and getattr(b, "prefill_input_ids_cpu", None) is not None:
                b.input_ids = b.prefill_input_ids_cpu.to(b.device, non_blocking=True)
                b.prefill_input_ids_cpu = None
            fb = FBI.ForwardBatch.init_new(b, runner, return_hidden_states_before_norm=False)
            lo = runner.forward(fb).logits_output
            ids = runner.sample(lo, fb)
            return ids, lo.next_token_logits, b
    cached = []
    counts = dict(graph_replays=0)
    graph_runner = getattr(runner, "decode_cuda_graph_runner", None)
    if graph_runner is not None and hasattr(graph_runner, "execute"):
        execute = graph_runner.execute

        def counting_execute(*a, **k):
            counts["graph_replays"] += 1
            return execute(*a, **k)

        graph_runner.execute = counting_execute
    olm, records = None, []
    if not gpu:
        from oracle.model import OracleLM
        from sglang_amd.harness.models import ModelConfig as OCfg

        olm = OracleLM(OCfg("ref", H, I, L, Hq, Hkv, D, V, 1e-5, ROPE_THETA["llama"], None, 8192), oracle_weights(runner.model),
                       num_slots=int(runner.token_to_kv_pool.size) + 16, max_ctx=8, max_reqs=1, device=dev)

    def check(what, batch, logits, decode_):
        if olm is None:
            return
        seq = batch.seq_lens.to(dev)
        if decode_:
            positions, pre, ext = (seq - 1).to(torch.int64), None, None
        else:
            pre, ext = torch.tensor(batch.prefix_lens, device=dev), torch.tensor(batch.extend_lens, device=dev)
            positions = torch.cat([torch.arange(p, p + e) for p, e in zip(batch.prefix_lens, batch.extend_lens)]).to(dev)
        olm.req_to_token = runner.req_to_token_pool.req_to_token
        want = olm.forward(batch.input_ids.to(dev), positions, batch.req_pool_indices.to(dev), seq, pre, ext, batch.out_cache_loc.to(dev),
                           decode_).float().cpu()
        records.append(dict(what=what, identical=bool(torch.equal(logits.float().cpu(), want)), ref_rms=float(want.pow(2).mean().sqrt())))

    SP = importlib.import_module("sglang.srt.sampling.sampling_params").SamplingParams
    Req = importlib.import_module("sglang.srt.managers.schedule_batch").Req
    g = torch.Generator().manual_seed(5)

    def make_req(rid, ids, upto):
        req = Req(rid=rid, origin_input_text="", origin_input_ids=array("q", ids[:upto]), sampling_params=SP(temperature=0, max_new_tokens=out))
        req.full_untruncated_fill_ids = req.origin_input_ids
        req.logprob_start_len = -1
        req.set_extend_range(len(req.prefix_indices), len(req.origin_input_ids))
        return req

    def job(tag, sync_every_step):
        runner.req_to_token_pool.clear()
        runner.token_to_kv_pool_allocator.clear()
        if tree is not None:
            tree.reset()
        extend = extend_on_tree if tree is not None else (lambda reqs: OB.extend(reqs, runner))
        shared = [torch.randint(3, min(V, 10000), (prefix,), generator=g).tolist() for _ in range(groups)]
        own = [[torch.randint(3, min(V, 10000), (unique,), generator=g).tolist() for _ in range(per_group)] for _ in range(groups)]
        if gpu:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        leaders = [make_req(gi * per_group, shared[gi] + own[gi][0], prefix + unique) for gi in range(groups)]
        if tree is not None:
            for req in leaders:
                req.init_next_round_input(tree)
                req.set_extend_range(len(req.prefix_indices), len(req.full_untruncated_fill_ids))
        nxt_a, logits, batch = extend(leaders)                                  # cold prefill of one request per group
        if tree is not None:
            for req in leaders:                                                 # scheduler, after a prefill batch: insert into the tree
                tree.cache_unfinished_req(req)
        check(f"{tag}: cold prefill of {groups} group leaders ({prefix} + {unique} tokens)", batch, logits, False)
        others = []
        for gi in range(groups):
            for j in range(1, per_group):
                req = make_req(gi * per_group + j, shared[gi] + own[gi][j], prefix + unique)
                if tree is not None:
                    req.init_next_round_input(tree)                             # RadixCache.match_prefix: the hit on the leader's tokens
                    cached.append(len(req.prefix_indices))
                else:
                    # the radix hit: this request's first `prefix` tokens are the leader's slots (one_batch.py:429-433)
                    req.prefix_indices = runner.req_to_token_pool.req_to_token[leaders[gi].req_pool_idx, :prefix].to(req.prefix_indices.dtype)
                req.set_extend_range(len(req.prefix_indices), len(req.full_untruncated_fill_ids))
                others.append(req)
        if gpu:
            torch.cuda.synchronize()
        t1 = time.perf_counter()
        nxt_b, logits, batch_b = extend(others)                                # warm prefill over the cached prefixes
        if tree is not None:
            for req in others:
                tree.cache_unfinished_req(req)
        check(f"{tag}: warm prefill of {len(others)} requests over a {prefix}-token cached prefix", batch_b, logits, False)
        if gpu:
            torch.cuda.synchronize()
        t2 = time.perf_counter()
        batch.merge_batch(batch_b)                                              # scheduler: running_batch.merge_batch(last_batch)
        nxt = torch.cat([nxt_a, nxt_b])
        lat = []
        for step in range(out - 1):
            ts = time.perf_counter()
            nxt, logits = OB.decode(nxt, batch, runner)
            if step < 3:
                check(f"{tag}: decode step {step} ({B} requests, {groups} shared prefixes)", batch, logits, True)
            if gpu and sync_every_step:
                torch.cuda.synchronize()
            lat.append(time.perf_counter() - ts)
        if gpu:
            torch.cuda.synchronize()
        t3 = time.perf_counter()
        if tree is not None:
            for req in leaders + others:                                        # scheduler, when a request finishes (prompt part:
                tree.cache_finished_req(req, kv_len_to_handle=len(req.origin_input_ids))   # this harness keeps no output_ids on the Req)
        med = sorted(lat)[len(lat) // 2] if lat else 0.0
        return dict(seconds=t3 - t0, cold_prefill_s=t1 - t0, warm_prefill_s=t2 - t1, decode_s=t3 - t2,
                    decode_s_per_step=(t3 - t2) / max(1, out - 1), median_synchronised_step_s=med if sync_every_step else None,
                    output_tokens_per_s=B * out / (t3 - t0))

    with torch.no_grad():
        warm = job("warm-up job", True)
        stepwise = job("step-synchronised job", True)        # a device synchronise after every decode step: per-step latency
        before = counts["graph_replays"]
        timed = job("timed job", False)                       # synchronised at the phase boundaries only: throughput
    plan = None
    ws = getattr(runner.attn_backend, "_cascade_ws", None)
    if ws is not None:
        try:
            plan = dict(zip(("items", "groups", "member_rows"), ws.plan[:3].tolist()))     # cascade_plan.hpp header of the last decode step
        except Exception:                                   # noqa: BLE001
            plan = None
    return dict(mode="shared-prefix-job", dims=dims_name, device=str(dev), shape=dict(groups=groups, per_group=per_group, prefix=prefix, unique=unique, out=out),
                attention_backend=sa.attention_backend, attn_backend_class=type(runner.attn_backend).__name__,
                graph_runner=type(graph_runner).__name__ if graph_runner is not None else None,
                graph_replays_in_the_timed_job=counts["graph_replays"] - before, warm_up=warm, step_synchronised=stepwise, timed=timed,
                cascade_plan_last_step=plan, radix_cache=type(tree).__name__ if tree is not None else None,
                radix_hit_lengths=sorted(set(cached)),
                passes=records)


def run_scheduler_job(dims_name="tiny_v16k", groups=2, per_group=2, prefix=16, unique=8, out=4, overlap=False, server_args=None,
                      logprobs=False, spec_ngram=0, sampling=None, spec_tree=False) -> dict:
    """The reference's `Scheduler` ITSELF (managers/scheduler.py: request intake, `PrefillAdder`, the real radix cache built by
    `kv_cache_builder`, running-batch merge, `TpModelWorker` -> `ModelRunner`, result processing, output streaming) with the body of
    its `event_loop_normal` (scheduler.py:1748-1780) executed here step by step instead of behind zmq sockets (zmq is not in this
    image: the sockets are stubs; requests go in through `process_input_requests`, outputs are picked off `send_to_detokenizer`).
    BASELINE.json's job shape arrives the way bench.py's harness feeds it: the group leaders first, and -- once their prefill has put the
    shared prefixes into the radix tree -- the other requests, which then HIT `prefix` cached tokens; greedy decoding to `out` tokens.

    Build container: tiny model with real weights, torch-native backend -> the generated token ids must equal the oracle's greedy
    generation.  MI355X: the plug-in loaded by the reference's loader; Llama-3-8B architecture with dummy weights for the timed job.

    `overlap=True`: the server's default loop instead -- the body of `event_loop_overlap` (scheduler.py:1783-1853: the forward of
    batch N is launched before the results of batch N-1 are processed; future token ids, the result queue, `launch_batch_sample_if_needed`)."""
    import json as _json
    import tempfile as _tf
    import time
    from array import array

    gpu = not dry_run_on_cpu()
    loader = run_loader() if gpu else None
    ns = install()
    H, I, L, Hq, Hkv, D, V = DIMS[dims_name]
    real_weights = L <= 4                               # the small models carry real weights (token-level check), the 8B one dummy weights
    arch = ARCH.get(dims_name, "llama")
    d = write_checkpoint_config(dims_name, max_pos=8192)
    common = importlib.import_module("sglang.srt.utils.common")
    if spec_ngram:
        # `--speculative-algorithm NGRAM --speculative-num-draft-tokens N`: decode batches become ForwardMode.TARGET_VERIFY forwards of
        # N draft tokens per request under a tree mask (ngram_worker.py:310-397), captured by the reference's graph runner in that mode
        assert real_weights, "the scripted drafter needs the oracle's greedy continuation: small real-weight models only"
        _install_spec_standins(ns)
        SPEC_OPTS["tree"] = bool(spec_tree)
        del SPEC_VERIFY[:]
        server_args = dict(server_args or {}, speculative_algorithm="NGRAM", speculative_num_draft_tokens=int(spec_ngram))
    if not gpu:
        from sglang.kernels import fused_op as FO
        from sglang.kernels.spec import KernelBackend

        FO.set_fused_op_backend(KernelBackend.TORCH)
        common.get_device_memory_capacity = ns.server_args.get_device_memory_capacity = lambda device=None: 288 * 1024
        ns.distributed_parallel_state.is_cuda_alike = lambda: False
    else:
        try:
            common.get_device_memory_capacity("cuda")
        except Exception:                                   # noqa: BLE001
            mib = torch.cuda.mem_get_info()[1] // (1 << 20)
            common.get_device_memory_capacity = ns.server_args.get_device_memory_capacity = lambda device=None: mib
    B = groups * per_group
    tokens = 2 * (groups * (prefix + unique) + (B - groups) * unique + B * out)           # two jobs' worth: the tree keeps the first
    kw = dict(model_path=str(d), load_format="dummy", skip_tokenizer_init=True, dtype="bfloat16", device="cuda" if gpu else "cpu",
              attention_backend=None if gpu else "torch_native", sampling_backend=loader["default_attention_backend"] if gpu else "pytorch",
              max_total_tokens=tokens + 4096, max_running_requests=max(16, B), cuda_graph_max_bs_decode=B, mem_fraction_static=0.5,
              disable_overlap_schedule=not overlap, random_seed=3)
    kw.update(server_args or {})
    sa = ns.server_args.ServerArgs(**kw)
    ns.server_args.set_global_server_args_for_scheduler(sa)
    pa = ns.server_args.PortArgs.init_new(sa)
    counts = dict(fused_decode_models=0, graph_replays=0)
    if gpu:
        import sglang_amd.fused_decode as fd

        decode_model = fd.decode_model

        def counting_decode_model(*a, **k):
            counts["fused_decode_models"] += 1
            return decode_model(*a, **k)

        fd.decode_model = counting_decode_model
    S = importlib.import_module("sglang.srt.managers.scheduler")
    sch = S.Scheduler(sa, pa, 0, 0, 0, 0, 0, 0, None)
    sch.is_initializing = False
    runner = sch.tp_worker.model_runner
    if real_weights:
        runner.model.load_weights(list(hf_checkpoint(DIMS[dims_name], runner.device, arch=arch).items()))
    captured = counts["fused_decode_models"]
    graph_runner = getattr(runner, "decode_cuda_graph_runner", None)
    if graph_runner is not None and hasattr(graph_runner, "execute"):
        execute = graph_runner.execute

        def counting_execute(*a, **k):
            counts["graph_replays"] += 1
            return execute(*a, **k)

        graph_runner.execute = counting_execute
    outs = []
    sch.ipc_channels.send_to_detokenizer.send_output = lambda output, recv_obj=None: outs.append(output)
    counts["retracted_requests"] = 0
    SBcls = importlib.import_module("sglang.srt.managers.schedule_batch").ScheduleBatch
    retract = SBcls.retract_decode

    def counting_retract(self, *a_, **k_):
        res = retract(self, *a_, **k_)
        try:
            counts["retracted_requests"] += len(res[0])
        except Exception:                                   # noqa: BLE001
            counts["retracted_requests"] += 1
        return res

    SBcls.retract_decode = counting_retract
    io = importlib.import_module("sglang.srt.managers.io_struct")
    SP = importlib.import_module("sglang.srt.sampling.sampling_params").SamplingParams
    g = torch.Generator().manual_seed(5)

    def request(rid, ids):
        # `sampling` (e.g. {"temperature": 0.8, "top_k": 20, "top_p": 0.9}): every request samples -- the plug-in sampler's top-k / top-p
        # path under the scheduler's SamplingBatchInfo; greedy otherwise
        sp = SP(max_new_tokens=out, ignore_eos=True, **(sampling or dict(temperature=0)))
        sp.normalize(None)
        return io.TokenizedGenerateReqInput(rid=rid, input_text=None, input_ids=array("q", ids), input_embeds=None, mm_inputs=None,
                                            token_type_ids=None, sampling_params=sp, return_logprob=logprobs, logprob_start_len=-1,
                                            top_logprobs_num=2 if logprobs else 0, token_ids_logprob=None, stream=False)

    # The reference's own loop runs -- `Scheduler.run_event_loop()` (scheduler.py:1696-1732: schedule stream, WAR barrier, dispatch to
    # event_loop_normal / event_loop_overlap) -- with ONE substitution: the receiver's raw socket read (`_pull_raw_reqs`) hands out
    # the scripted arrivals and raises the loop's own `gracefully_exit` flag when the job is done.
    batches = []
    run_batch = sch.run_batch

    launch_times = []
    # Every forward's logits, by (request, position): with the small real-weight models `ModelRunner.forward` is wrapped and each
    # `next_token_logits` row is filed under the request it belongs to (the order of `batch.reqs` at `run_batch`) and the output
    # position it predicts (`seq_len - prompt length`: the last chunk of a prefill -> 0, the decode forward over k generated tokens
    # -> k, a re-prefill after retraction over k generated tokens -> k; rows of non-final prefill chunks fall below 0 and rows of a
    # finished request's extra overlap step beyond `out`: both dropped).  Compared with the oracle teacher-forced (below).
    capture = dict(on=False, pending=None, rows={})

    def logging_run_batch(batch, *a, **k):
        batches.append((batch.forward_mode.name, batch.batch_size()))
        launch_times.append(time.perf_counter())
        if capture["on"]:
            capture["pending"] = [(r.rid, int(sl) - len(r.origin_input_ids)) for r, sl in zip(batch.reqs, batch.seq_lens_cpu.tolist())]
        return run_batch(batch, *a, **k)

    modes_seen = {}
    if real_weights and hasattr(runner, "forward"):
        runner_forward = runner.forward

        def capturing_forward(*a, **k):
            fb_ = a[0] if a else k.get("forward_batch")
            nm = getattr(getattr(fb_, "forward_mode", None), "name", "?")
            modes_seen[nm] = modes_seen.get(nm, 0) + 1
            res = runner_forward(*a, **k)
            pend, capture["pending"] = capture["pending"], None
            lo = getattr(res, "logits_output", None)
            lg = getattr(lo, "next_token_logits", None)
            if capture.get("spec") and nm == "TARGET_VERIFY" and lg is not None and SPEC_VERIFY and SPEC_VERIFY[-1]["logits"] is None:
                # [requests x draft nodes, vocab]: row (b, j) scores the token after node j's path (logits_processor: every
                # position of a verify forward is kept); joined with the host-side record of the draft it belongs to
                nrow = sum(len(q_["draft"]) for q_ in SPEC_VERIFY[-1]["requests"])
                if lg.shape[0] >= nrow:
                    SPEC_VERIFY[-1]["logits"] = lg[:nrow].float().cpu()
            if capture["on"] and pend is not None and lg is not None and lg.shape[0] >= len(pend):
                lg = lg[: len(pend)].float().cpu()
                for i, (rid, t) in enumerate(pend):
                    if 0 <= t < out:
                        capture["rows"][(rid, t)] = lg[i]
            return res

        runner.forward = capturing_forward

    sch.run_batch = logging_run_batch

    def run_loop(arrivals, finished):
        """arrivals: list of (ready() -> bool, [requests]); delivered in order, each once its predicate holds."""
        pending = list(arrivals)

        def pull():
            if pending and pending[0][0]():
                return pending.pop(0)[1]
            if not pending and finished():
                sch.gracefully_exit = True
            return []

        type(sch.request_receiver)._pull_raw_reqs = lambda self: pull()        # (the receiver is a frozen dataclass: patch the class)
        sch.gracefully_exit = False
        del batches[:]
        del launch_times[:]
        sch.run_event_loop()
        return list(batches)

    def job(tag):
        del outs[:]
        shared = [torch.randint(3, min(V, 10000), (prefix,), generator=g).tolist() for _ in range(groups)]
        prompts = {f"{tag}-g{gi}r{j}": shared[gi] + torch.randint(3, min(V, 10000), (unique,), generator=g).tolist()
                   for gi in range(groups) for j in range(per_group)}
        leaders = [f"{tag}-g{gi}r0" for gi in range(groups)]
        others = [r for r in prompts if r not in leaders]
        if spec_ngram:
            # the scripted drafter proposes the ORACLE'S greedy continuation of each sequence (with one wrong token per draft)
            from oracle.model import OracleLM as _OLM

            rl = list(prompts)
            o_ = _OLM(oracle_config(dims_name, 8192), oracle_weights(runner.model), num_slots=4 * tokens, max_ctx=prefix + unique + out + 8,
                      max_reqs=B, device=runner.device)
            gr = [[rl.index(f"{tag}-g{gi}r{j}") for j in range(per_group)] for gi in range(groups)]
            cont = o_.generate([prompts[r] for r in rl], out + int(spec_ngram), share_prefix_groups=gr, shared_len=prefix)
            SPEC_TRUTH[:] = [list(prompts[r]) + [int(t) for t in c] for r, c in zip(rl, cont)]
            for k_ in SPEC_STATS:
                SPEC_STATS[k_] = 0
        if gpu:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = lambda: sum(sum(f is not None for f in o.finished_reasons) for o in outs if type(o).__name__ == "BatchTokenIDOutput")   # noqa: E731
        # the other requests arrive once the leaders' prompts are in the radix tree: their prefill result has been processed (with the
        # overlap loop that is one iteration after its launch), i.e. every leader is in the running batch with two tokens out
        def in_tree():
            rb = sch.running_batch
            return rb is not None and len(rb.reqs) == groups and all(len(r.output_ids) >= 2 for r in rb.reqs)
        ran = run_loop([(lambda: True, [request(r, prompts[r]) for r in leaders]), (in_tree, [request(r, prompts[r]) for r in others])],
                       lambda: done() >= B)
        first, rest = ran, []
        if gpu:
            torch.cuda.synchronize()
        t1 = time.perf_counter()
        got, cached, lp, top = {}, {}, {}, {}
        for o in outs:
            if type(o).__name__ != "BatchTokenIDOutput":
                continue
            for i, rid in enumerate(o.rids):                  # (a request's ids arrive in increments: every forced stream interval + the end)
                got.setdefault(rid, []).extend(list(o.output_ids[i]))
                if logprobs and o.output_token_logprobs_val:
                    lp.setdefault(rid, []).extend(float(x) for x in o.output_token_logprobs_val[i])
                    top.setdefault(rid, []).extend([list(map(int, ix)) for ix in o.output_top_logprobs_idx[i]])
                if o.finished_reasons[i] is not None:
                    cached[rid] = int(o.cached_tokens[i])
        # steady decode: the intervals between consecutive launches of full-batch decode forwards (the loop launches batch N + 1 when
        # the result of batch N - 1 has arrived, so in steady state an interval is one step of whichever side is slower)
        full = [t for (m, bs), t in zip(ran, launch_times) if m == "DECODE" and bs == B]
        gaps = sorted(b_ - a_ for a_, b_ in zip(full, full[1:]))
        return dict(seconds=t1 - t0, output_tokens_per_s=B * out / (t1 - t0), batches=first + rest, prompts=prompts, generated=got,
                    cached_tokens=cached, leaders=leaders, logprobs=lp, top_idx=top,
                    decode_step_ms_p50=1e3 * gaps[len(gaps) // 2] if gaps else None, full_batch_decode_steps=len(full))

    triton_launches = _count_triton_launches()
    with torch.no_grad():
        warm = job("warm")
        before = dict(counts)
        del triton_launches[:]
        prof_path = os.environ.get("REF_SCHED_CPROFILE")
        capture["on"] = real_weights and not spec_ngram           # (a verify forward scores N rows per request: filed through SPEC_VERIFY)
        capture["spec"] = bool(real_weights and spec_ngram)
        del SPEC_VERIFY[:]
        modes_seen.clear()
        if prof_path:
            timed = _profiled(lambda: job("timed"), prof_path)
        else:
            timed = job("timed")
        capture["on"] = capture["spec"] = False
    triton_in_timed = sorted(set(triton_launches))
    rep = dict(mode="scheduler-job", event_loop="overlap" if overlap else "normal", server_args=server_args or {}, page_size=int(sch.page_size),
               chunked_prefill_size=sa.chunked_prefill_size, dims=dims_name, device=str(runner.device), scheduler=type(sch).__name__, tree_cache=type(sch.tree_cache).__name__,
               tp_worker=type(sch.tp_worker).__name__, attention_backend=sa.attention_backend, attn_backend_class=type(runner.attn_backend).__name__,
               sampler_class=type(runner.sampler).__name__, graph_runner=type(graph_runner).__name__ if graph_runner is not None else None,
               shape=dict(groups=groups, per_group=per_group, prefix=prefix, unique=unique, out=out),
               fused_decode_models_during_capture=captured,
               eager_fused_decode_forwards_in_the_timed_job=counts["fused_decode_models"] - before["fused_decode_models"],
               graph_replays_in_the_timed_job=counts["graph_replays"] - before["graph_replays"],
               retracted_requests=counts["retracted_requests"], max_total_num_tokens=int(runner.max_total_num_tokens),
               triton_launches_in_the_timed_job=len(triton_launches), triton_kernels_in_the_timed_job=triton_in_timed,
               kv_pool_class=type(getattr(runner, "token_to_kv_pool", None)).__name__, allocator_class=type(getattr(runner, "token_to_kv_pool_allocator", None)).__name__,
               plugin_counts=_plugin_counts() if gpu else None,
               spec=dict(draft_tokens=int(spec_ngram), drafter=dict(SPEC_STATS), forward_modes_in_the_timed_job=dict(modes_seen),
                         worker=type(getattr(sch, "model_worker", None)).__name__) if spec_ngram else None)
    if gpu:
        # the shared-prefix decode plan of the LAST decode step (device buffer of the backend's workspace): groups found, items
        try:
            ws_ = getattr(runner.attn_backend, "_cascade_ws", None)
            if ws_ is not None:
                hdr = ws_.plan[:4].cpu().tolist()
                rep["last_decode_plan"] = dict(items=int(hdr[0]), groups=int(hdr[1]), member_rows=int(hdr[2]), shared_items=int(hdr[3]))
        except Exception as e:                              # noqa: BLE001
            rep["last_decode_plan"] = dict(error=f"{type(e).__name__}: {e}")
    for tag, j in (("warm_up", warm), ("timed", timed)):
        hit = sorted(set(v for r, v in j["cached_tokens"].items() if r not in j["leaders"]))
        modes = {}
        for m, bs in j["batches"]:
            modes[f"{m} x{bs}"] = modes.get(f"{m} x{bs}", 0) + 1
        rep[tag] = dict(seconds=j["seconds"], output_tokens_per_s=j["output_tokens_per_s"], decode_step_ms_p50=j["decode_step_ms_p50"],
                        full_batch_decode_steps=j["full_batch_decode_steps"], batches_run=modes,
                        cached_tokens_of_leaders=sorted(set(j["cached_tokens"][r] for r in j["leaders"])), cached_tokens_of_others=hit,
                        finished_requests=len(j["generated"]), tokens_per_request=sorted(set(len(v) for v in j["generated"].values())))
    if real_weights:
        # the oracle's greedy generation of the timed job's prompts, prefixes shared the same way
        from oracle.model import OracleLM

        kvd = "fp8_e4m3" if str(getattr(sa, "kv_cache_dtype", "auto")) == "fp8_e4m3" else "auto"       # (the oracle's pool stores e4m3 rows too)
        olm = OracleLM(oracle_config(dims_name, 8192), oracle_weights(runner.model),
                       num_slots=4 * tokens, max_ctx=prefix + unique + out + 8, max_reqs=B, device=runner.device, kv_cache_dtype=kvd)
        rids = list(timed["prompts"])
        grp = [[rids.index(f"timed-g{gi}r{j}") for j in range(per_group)] for gi in range(groups)]
        want = olm.generate([timed["prompts"][r] for r in rids], out, share_prefix_groups=grp, shared_len=prefix)
        same = sum(int(list(w) == timed["generated"].get(r)) for r, w in zip(rids, want))
        if spec_ngram:
            rep["spec"]["generated_vs_oracle"] = [dict(generated=timed["generated"].get(r), oracle=[int(t) for t in w]) for r, w in zip(rids, want)]
        rep["oracle"] = dict(requests=len(rids), requests_with_identical_tokens=same,
                             token_agreement=sum(int(a == b) for r, w in zip(rids, want) for a, b in zip(w, timed["generated"].get(r, []))) / (len(rids) * out))
        # ---- logits of every forward of the timed job against the oracle, teacher-forced with the tokens the run produced: the
        # plug-in's error against the fp32-accumulating oracle inside the band of the reference's literal bf16 evaluation against the
        # same oracle (what run_runner asserts per pass; VERDICT r04 weak #3: token agreement alone lets a wrong-but-close kernel pass)
        if capture["rows"]:
            forced = [timed["generated"].get(r, []) for r in rids]
            if all(len(f) == out for f in forced):
                def teacher(**kw):
                    o_ = OracleLM(oracle_config(dims_name, 8192), oracle_weights(runner.model), num_slots=4 * tokens,
                                  max_ctx=prefix + unique + out + 8, max_reqs=B, device=runner.device, kv_cache_dtype=kvd, **kw)
                    return o_.generate([timed["prompts"][r] for r in rids], out, return_logits=True, forced=forced,
                                       share_prefix_groups=grp, shared_len=prefix)[1]
                lit = teacher()
                acc = teacher(compute_dtype=torch.float32) if gpu else None
                got_l, lit_l, acc_l = [], [], []
                for t in range(out):
                    for bi, r in enumerate(rids):
                        row = capture["rows"].get((r, t))
                        if row is None:
                            continue
                        got_l.append(row)
                        lit_l.append(lit[t][bi].float().cpu())
                        if acc is not None:
                            acc_l.append(acc[t][bi].float().cpu())
                G_, L_ = torch.stack(got_l), torch.stack(lit_l)
                band = dict(rows_compared=len(got_l), rows_expected=len(rids) * out, identical_to_the_literal_oracle=bool(torch.equal(G_, L_)),
                            max_abs_vs_literal=float((G_ - L_).abs().max()), logit_rms=float(L_.pow(2).mean().sqrt()))
                if acc_l:
                    A_ = torch.stack(acc_l)
                    e_p, e_r = G_ - A_, L_ - A_
                    top2 = A_.topk(2, dim=-1).values
                    clear = (top2[:, 0] - top2[:, 1]) > 16 * 2.0 ** -8 * top2[:, 0].abs().clamp_min(1.0)      # margin > 16 bf16 ulps
                    band.update(product_rms_err=float(e_p.pow(2).mean().sqrt()), reference_rms_err=float(e_r.pow(2).mean().sqrt()),
                                product_max_err=float(e_p.abs().max()), reference_max_err=float(e_r.abs().max()),
                                clear_rows=int(clear.sum()), argmax_agree_on_clear_rows=int((G_.argmax(-1) == A_.argmax(-1))[clear].sum()))
                rep["logit_band"] = band
        if spec_ngram:
            rep["spec"]["logit_band"] = spec_logit_band(dims_name, runner, gpu, moe=arch == "mixtral")
        if sampling and capture["rows"]:
            # sampled tokens are not the oracle's greedy tokens; what must hold: every token the scheduler delivered lies inside the
            # top-k set of the very logits row it was sampled from (captured from the forward that produced it)
            k_ = int(sampling.get("top_k", 0)) or V
            inside = total = 0
            for r in rids:
                for t, tok in enumerate(timed["generated"].get(r, [])):
                    row = capture["rows"].get((r, t))
                    if row is None:
                        continue
                    total += 1
                    # (a token TIED with the k-th largest logit is inside: at a 128 K vocabulary bf16 logits tie at rank k often, and
                    # which of the tied tokens a descending sort puts first is the sort's business -- the reference's torch.sort is not stable)
                    inside += int(float(row[int(tok)]) >= float(row.topk(min(k_, V)).values[-1]))
            rep["sampling"] = dict(params=sampling, tokens_checked=total, tokens_inside_their_rows_top_k=inside,
                                   distinct_first_tokens=len(set(tuple(v[:2]) for v in timed["generated"].values())))
        if logprobs:
            # the log-probabilities the scheduler streamed with the tokens (sampler -> output_logprob_processor -> output streamer) against
            # log_softmax of the oracle's logits, the oracle teacher-forced with the tokens the run produced
            olm2 = OracleLM(oracle_config(dims_name, 8192), oracle_weights(runner.model), num_slots=4 * tokens,
                            max_ctx=prefix + unique + out + 8, max_reqs=B, device=runner.device)
            forced = [timed["generated"][r] for r in rids]
            _, steps = olm2.generate([timed["prompts"][r] for r in rids], out, return_logits=True, forced=forced, share_prefix_groups=grp, shared_len=prefix)
            worst, top_ok, n = 0.0, 0, 0
            for t, lg in enumerate(steps):
                ls = torch.log_softmax(lg.float(), dim=-1).cpu()
                for bi, r in enumerate(rids):
                    worst = max(worst, abs(float(ls[bi, forced[bi][t]]) - timed["logprobs"][r][t]))
                    top_ok += int(sorted(ls[bi].topk(2).indices.tolist()) == sorted(timed["top_idx"][r][t]))
                    n += 1
            rep["oracle"].update(logprob_values=n, max_abs_logprob_diff=worst, top2_sets_equal=top_ok)
    return rep


def spec_logit_band(dims_name, runner, gpu, moe=False) -> dict:
    """Every TARGET_VERIFY forward's logits against the oracle under the tree mask (triton_backend.py:860-919,
    ngram_worker.py:310-397).  Row (request b, draft node j) of a verify forward scores the token that follows
    `tokens[:-1] + path(j)` -- the request's verified sequence (whose last token is draft node 0, not yet in the KV cache) extended by
    node j's ancestors-and-self in tree order.  The oracle evaluates every such sequence from scratch (one prefill, last position), literally
    in bf16 and accumulating in fp32; the bars are the scheduler tests' own: the plug-in's error against the fp32-accumulating oracle
    inside the band of the reference's literal evaluation against the same oracle.  Rows of REJECTED branches are scored like any
    other (their logits were computed under the mask too).  Sparse-MoE models: rows whose own draft path contains a token with a near-tie
    (2 bf16 ulps) between the last chosen and the first unchosen expert in any layer, or on which the two oracles already route
    differently, are `flip_prone`; the per-logit bar is taken over the other rows."""
    from oracle.model import OracleLM

    seqs, where = [], []
    records = [v for v in SPEC_VERIFY]
    expected = sum(len(q["draft"]) for v in records for q in v["requests"])
    for vi, v in enumerate(records):
        if v["logits"] is None:
            continue
        row = 0
        for q in v["requests"]:
            n = len(q["draft"])
            assert q["draft"][0] == q["tokens"][-1], "draft node 0 must be the request's last verified token"
            for j in range(n):
                path = [q["draft"][i] for i in range(j + 1) if q["mask"][j][i]]
                seqs.append(tuple(q["tokens"][:-1] + path))
                where.append((vi, row + j, sum(q["mask"][j]) - 1, j))
            row += n
    if not seqs:
        return dict(rows_compared=0, rows_expected=expected)
    uniq = sorted(set(seqs))
    index = {sq: i for i, sq in enumerate(uniq)}
    dev = runner.device
    max_len = max(len(sq) for sq in uniq)

    def evaluate(**kw):
        out_rows, traces = [], []
        for c0 in range(0, len(uniq), 48):                                  # (request slots of one oracle instance)
            chunk = [list(sq) for sq in uniq[c0: c0 + 48]]
            o_ = OracleLM(oracle_config(dims_name, 8192), oracle_weights(runner.model), num_slots=sum(map(len, chunk)) + 64,
                          max_ctx=max_len + 8, max_reqs=len(chunk), device=dev, **kw)
            if moe:
                o_.trace = []
            out_rows.append(o_.generate(chunk, 1, return_logits=True)[1][0].float().cpu())
            if moe:
                lens = [len(c) for c in chunk]
                traces.append((lens, [(l_["router_logits"].float().cpu(), l_["topk_ids"].cpu()) for l_ in o_.trace[0]["layers"]]))
        return torch.cat(out_rows), traces

    lit, tr_lit = evaluate()
    acc, tr_acc = evaluate(compute_dtype=torch.float32) if gpu else (None, None)
    G_ = torch.stack([records[vi]["logits"][r] for vi, r, _, _ in where])
    L_ = torch.stack([lit[index[sq]] for sq in seqs])
    band = dict(rows_compared=len(seqs), rows_expected=expected, distinct_sequences=len(uniq), verify_forwards=len(records),
                rows_by_depth={str(d_): sum(1 for w_ in where if w_[2] == d_) for d_ in sorted(set(w_[2] for w_ in where))},
                identical_to_the_literal_oracle=bool(torch.equal(G_, L_)), max_abs_vs_literal=float((G_ - L_).abs().max()),
                logit_rms=float(L_.pow(2).mean().sqrt()))
    if acc is not None:
        A_ = torch.stack([acc[index[sq]] for sq in seqs])
        e_p, e_r = G_ - A_, L_ - A_
        top2 = A_.topk(2, dim=-1).values
        clear = (top2[:, 0] - top2[:, 1]) > 16 * 2.0 ** -8 * top2[:, 0].abs().clamp_min(1.0)
        band.update(product_rms_err=float(e_p.pow(2).mean().sqrt()), reference_rms_err=float(e_r.pow(2).mean().sqrt()),
                    product_max_err=float(e_p.abs().max()), reference_max_err=float(e_r.abs().max()),
                    clear_rows=int(clear.sum()), argmax_agree_on_clear_rows=int((G_.argmax(-1) == A_.argmax(-1))[clear].sum()))
        row_rms = e_p.pow(2).mean(-1).sqrt()
        worst = row_rms.argsort(descending=True)[:6].tolist()
        band["worst_rows"] = [dict(verify_forward=where[i][0], row=where[i][1], depth=where[i][2], node=where[i][3], rms_err=float(row_rms[i]),
                                   reference_rms_err=float(e_r[i].pow(2).mean().sqrt())) for i in worst]
        per_fwd = []
        for vi, v in enumerate(records):
            if v["logits"] is None:
                continue
            rows_v = [i for i, w_ in enumerate(where) if w_[0] == vi]
            n_ = len(v["requests"][0]["draft"])
            per_fwd.append(dict(forward=vi, requests=[q["rid"] for q in v["requests"]], lens=[len(q["tokens"]) for q in v["requests"]],
                                shapes=["chain" if all(all(q["mask"][a][b_] for b_ in range(a + 1)) for a in range(n_)) else "tree" for q in v["requests"]],
                                rms_err_per_request=[round(float(e_p[rows_v[k * n_: (k + 1) * n_]].pow(2).mean().sqrt()), 4) for k in range(len(v["requests"]))]))
        band["per_forward"] = per_fwd
        if moe:
            prone_u, c0 = set(), 0
            k_top = int(tr_acc[0][1][0][1].shape[-1])
            tail = {}
            for sq, w_ in zip(seqs, where):
                tail[index[sq]] = max(tail.get(index[sq], 0), w_[2] + 1)                            # the draft path: depth + 1 tokens
            for (lens, la), (_, ll) in zip(tr_acc, tr_lit):
                owner = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))       # token row -> its sequence in the chunk
                # only the tokens THIS forward evaluated (the node's own path) count: the shared prompt's tokens sit in every
                # sequence and were routed by earlier forwards; their flips reach a verify row through the KV cache only
                in_tail = torch.cat([torch.arange(n_) >= n_ - tail[c0 + i] for i, n_ in enumerate(lens)])
                for (rl_a, ti_a), (_, ti_l) in zip(la, ll):
                    # a near-tie between the last chosen and the first unchosen expert: within 2 bf16 ulps of the router logits' scale
                    srt = rl_a.sort(dim=-1, descending=True).values
                    tie = (srt[:, k_top - 1] - srt[:, k_top]) <= 2 * 2.0 ** -8 * srt[:, 0].abs().clamp_min(1e-3)
                    differ = (ti_a.sort(-1).values != ti_l.sort(-1).values).any(-1)
                    prone_u.update((owner[(tie | differ) & in_tail] + c0).tolist())
                c0 += len(lens)
            keep = torch.tensor([index[sq] not in prone_u for sq in seqs])
            band.update(flip_prone_rows=int((~keep).sum()), rows_without_flip_risk=int(keep.sum()))
            if keep.any():
                band.update(product_max_err_no_flip=float(e_p[keep].abs().max()), reference_max_err_no_flip=float(e_r[keep].abs().max()),
                            product_rms_err_no_flip=float(e_p[keep].pow(2).mean().sqrt()), reference_rms_err_no_flip=float(e_r[keep].pow(2).mean().sqrt()))
    return band


SPEC_TRUTH = []          # scripted drafter: whole token sequences (prompt + the oracle's greedy continuation) of the running job
SPEC_STATS = dict(lookups=0, matched=0, drafted_true_tokens=0, tree_drafts=0, chain_drafts=0)
SPEC_OPTS = dict(tree=False)     # tree=True: the drafter also proposes WRONG branches (breadth 2) so that rejected siblings are walked
SPEC_VERIFY = []         # one record per verify forward of the timed job: what was drafted (host side) -- the captured logits join it


def spec_tree_patterns(n: int):
    """Ancestor-or-self masks of the scripted drafter's draft shapes over n nodes (node 0 = the last verified token), as
    (name, mask [n][n], true_depth [n], wrong [n]): node i carries the TRUE continuation token number true_depth[i] (1-based) of its
    own path, or -- wrong[i] -- a corrupted token at that depth.  Nodes are in BFS order (siblings adjacent, parents first), the
    order the n-gram corpus emits (ngram_corpus.py:94-110).
      chain           0 - 1 - 2 - ... (one of them corrupted by the caller)
      wrong-first     0 -> {1: WRONG t1, 2: t1}, 2 -> 3: t2, 3 -> 4 ...      the walk must step over a wrong FIRST sibling
      wrong-second    0 -> {1: t1, 2: WRONG t1}, 1 -> 3: t2, 3 -> 4 ...      a rejected sibling beside the accepted one"""
    import numpy as np

    def build(parents):
        m = np.zeros((n, n), dtype=np.int64)
        for i in range(n):
            j = i
            while j >= 0:
                m[i, j] = 1
                j = parents[j]
        return m

    out = []
    if n >= 3:
        # wrong-first: parents 0:-1, 1:0, 2:0, 3:2, 4:3 ...
        par = [-1, 0, 0] + [i - 1 if i > 3 else 2 for i in range(3, n)]
        depth = [0, 1, 1] + [i - 1 for i in range(3, n)]
        out.append(("wrong-first", build(par), depth, [False, True, False] + [False] * (n - 3)))
        # wrong-second: parents 0:-1, 1:0, 2:0, 3:1, 4:3 ...
        par = [-1, 0, 0] + [1 if i == 3 else i - 1 for i in range(3, n)]
        out.append(("wrong-second", build(par), depth, [False, False, True] + [False] * (n - 3)))
    return out


def _install_spec_standins(ns) -> None:
    """TARGET_VERIFY under the reference's real scheduler (`--speculative-algorithm NGRAM`, speculative/ngram_worker.py): the
    worker's draft source and two device helpers are compiled third-party code that is not in this image -- they get TEST stand-ins,
    everything else (NGRAMWorker, NgramVerifyInput, eagle_sample, the KV mover, the scheduler's spec bookkeeping, the graph runner
    capturing ForwardMode.TARGET_VERIFY) is the reference's own:
      * the n-gram corpus (`kernels/ops/speculative/ngram_corpus.py`: a JIT-compiled C++ trie behind tvm_ffi) -> a SCRIPTED drafter:
        per request a chain [last verified token, t1, t2, ...] whose continuation is the oracle's greedy continuation of that very
        sequence with a deliberately wrong token at a position that varies with the length -- so every verify step accepts some
        drafts and rejects others; mask = the chain's ancestor matrix, in the corpus' own output format (:94-110);
      * `sgl_kernel.speculative.reconstruct_indices_from_tree_mask` (kernels/aot/csrc/speculative/ngram_utils.cu:16-82) -> the same
        per-node loops on the host;
      * `sgl_kernel.verify_tree_greedy` -> on the GPU the reference's OWN Triton form (`eagle_utils.verify_tree_greedy_triton`,
        its XPU branch, :345-375); in the CPU dry run the greedy tree walk restated on the host."""
    import numpy as np

    class ScriptedNgramCorpus:
        def __init__(self, capacity=0, max_trie_depth=18, min_bfs_breadth=1, max_bfs_breadth=8, draft_token_num=8, match_type="BFS",
                     external_sam_budget=0, external_corpus_max_tokens=0):
            self.n = int(draft_token_num)

        def insert(self, batch_tokens):
            pass

        def synchronize(self):
            pass

        def reset(self):
            pass

        def erase_states(self, state_ids):
            pass

        def match_stateful(self, state_ids, batch_tokens, total_lens):
            n = self.n
            ids = np.zeros(len(batch_tokens) * n, dtype=np.int64)
            mask = np.zeros((len(batch_tokens), n, n), dtype=np.int64)
            for b, (tail, total) in enumerate(zip(batch_tokens, total_lens)):
                tail, total = list(tail), int(total)
                draft = [tail[-1]] + [7 + (total + 3 * i) % 5 for i in range(1, n)]            # no match: junk (all rejected)
                SPEC_STATS["lookups"] += 1
                mask[b] = np.tril(np.ones((n, n), dtype=np.int64))                             # a chain: node i's ancestors are 0..i
                trees = spec_tree_patterns(n) if SPEC_OPTS["tree"] else []
                for seq in SPEC_TRUTH:
                    if len(seq) >= total and seq[total - len(tail): total] == tail:
                        cont = seq[total: total + n - 1]
                        shape = SPEC_STATS["matched"] % (len(trees) + 1)                       # chain, wrong-first, wrong-second in turn
                        if shape == 0 or len(cont) < n - 2 or not trees:
                            wrong = 1 + total % n                                              # 1..n: index n = nothing corrupted
                            for i, t in enumerate(cont, start=1):
                                draft[i] = t if i != wrong else (t + 1) % 1000 + 3
                            SPEC_STATS["drafted_true_tokens"] += min(len(cont), wrong - 1)
                            SPEC_STATS["chain_drafts"] += 1
                        else:
                            _, tm, depth, wrong_node = trees[shape - 1]
                            for i in range(1, n):
                                t = cont[depth[i] - 1]
                                draft[i] = (t + 1) % 1000 + 3 if wrong_node[i] else t
                            mask[b] = tm
                            SPEC_STATS["drafted_true_tokens"] += max(depth)                    # the whole true path is on offer
                            SPEC_STATS["tree_drafts"] += 1
                        SPEC_STATS["matched"] += 1
                        break
                ids[b * n: (b + 1) * n] = draft
            return ids, mask.reshape(-1)

    for modname in ("sglang.kernels.ops.speculative.ngram_corpus", "sglang.srt.speculative.cpp_ngram.ngram_corpus"):
        mod = importlib.import_module(modname)
        mod.get_ngram_corpus_cls = lambda: ScriptedNgramCorpus

    def reconstruct_indices_from_tree_mask(tree_mask, verified_seq_len, positions, retrive_index, retrive_next_token, retrive_next_sibling,
                                           batch_size, draft_token_num):
        n = int(draft_token_num)
        tm = tree_mask.reshape(batch_size, n, n).bool().cpu().numpy()
        seq = verified_seq_len.cpu().tolist()
        pos = np.zeros(batch_size * n, dtype=np.int64)
        ri = np.zeros((batch_size, n), dtype=np.int64)
        nt = np.full((batch_size, n), -1, dtype=np.int64)
        nsib = np.full((batch_size, n), -1, dtype=np.int64)
        for b in range(batch_size):
            for t in range(n):
                depth, parent = 0, -1
                for i in range(t - 1, -1, -1):
                    if tm[b, t, i]:
                        depth += 1
                        if parent == -1:
                            parent = i
                ri[b, t] = b * n + t
                pos[b * n + t] = depth + seq[b]
                for i in range(t + 1, n):
                    if tm[b, i, t]:
                        nt[b, t] = i
                        break
                if parent != -1:
                    for i in range(t + 1, n):
                        if tm[b, i, parent] and not tm[b, i, parent + 1: i].any():
                            nsib[b, t] = i
                            break
        positions.copy_(torch.from_numpy(pos).to(positions.dtype))
        retrive_index.copy_(torch.from_numpy(ri).to(retrive_index.dtype))
        retrive_next_token.copy_(torch.from_numpy(nt).to(retrive_next_token.dtype))
        retrive_next_sibling.copy_(torch.from_numpy(nsib).to(retrive_next_sibling.dtype))

    NW = importlib.import_module("sglang.srt.speculative.ngram_worker")
    NW.reconstruct_indices_from_tree_mask = reconstruct_indices_from_tree_mask
    if not getattr(NW.NGRAMWorker._prepare_draft_tokens, "_recording", False):
        prepare = NW.NGRAMWorker._prepare_draft_tokens

        def recording_prepare(self, batch):
            # (ngram_worker.py:230-308) the sequence a draft continues = origin_input_ids + output_ids + the tokens accepted by the
            # previous verify step that the overlap loop has not written back yet (`prev_token_ids`)
            drafts, mask = prepare(self, batch)
            n = int(self.draft_token_num)
            stride = n if self.prev_token_ids else 0                        # (the worker's own stride, :243)
            recs = []
            kv_lens = [int(x) for x in batch.seq_lens.cpu().tolist()]       # tokens whose K/V rows are in the cache (device truth)
            for i, r in enumerate(batch.reqs):
                prev = self.prev_token_ids[i * stride: i * stride + self.prev_accept_lens[i]] if stride else []
                # the verified sequence = the first kv_len tokens + draft node 0 (the last accepted token, scored by this forward).
                # NOT simply origin + output + prev: when an EXTEND batch ran between two verify steps the result processor has already
                # written the previous step's accepted tokens into output_ids and `prev` repeats them (the worker's `total_lens` is
                # then too long by that much -- it only steers the n-gram lookup)
                known = [int(t) for t in list(r.origin_input_ids) + list(r.output_ids) + list(prev)]
                assert len(known) >= kv_lens[i], (len(known), kv_lens[i])
                recs.append(dict(rid=r.rid, tokens=known[: kv_lens[i]] + [int(drafts[i * n])],
                                 draft=[int(t) for t in drafts[i * n: (i + 1) * n]],
                                 mask=np.asarray(mask).reshape(len(batch.reqs), n, n)[i].astype(bool).tolist()))
            SPEC_VERIFY.append(dict(requests=recs, logits=None))
            return drafts, mask

        recording_prepare._recording = True
        NW.NGRAMWorker._prepare_draft_tokens = recording_prepare
    EU = importlib.import_module("sglang.srt.speculative.eagle_utils")

    def verify_tree_greedy_func(predicts, accept_index, accept_token_num, candidates, retrieve_index, retrieve_next_token,
                                retrieve_next_sibling, target_predict, topk=-1):
        if predicts.is_cuda:
            EU.verify_tree_greedy_triton(predicts=predicts, accept_index=accept_index, accept_token_num=accept_token_num, candidates=candidates,
                                         retrieve_index=retrieve_index, retrieve_next_token=retrieve_next_token,
                                         retrieve_next_sibling=retrieve_next_sibling, target_predict=target_predict)
            return predicts, accept_index, accept_token_num
        bs, n = candidates.shape
        tp = target_predict.reshape(-1)
        for b in range(bs):
            last = int(retrieve_index[b, 0])
            accept_index[b, 0] = last
            acc, cur = 0, 0
            for _ in range(1, accept_index.shape[1]):
                cur = int(retrieve_next_token[b, cur])
                while cur != -1:
                    if int(candidates[b, cur]) == int(tp[last]):
                        predicts[last] = int(tp[last])
                        acc += 1
                        last = int(retrieve_index[b, cur])
                        accept_index[b, acc] = last
                        break
                    cur = int(retrieve_next_sibling[b, cur])
                if cur == -1:
                    break
            accept_token_num[b] = acc
            predicts[last] = int(tp[last])
        return predicts, accept_index, accept_token_num

    EU.verify_tree_greedy_func = verify_tree_greedy_func


def _plugin_counts() -> dict:
    """What the plug-in's own counters saw in this process (whole process: warm-up + timed job + capture)."""
    from sglang_amd import mem_hooks, tuning
    from sglang_amd.layers import layernorm, sampler

    return dict(mem_hooks=dict(mem_hooks.counts), rmsnorm=dict(layernorm.served), gemm_selections=tuning.STATUS, sampler=dict(sampler.served))


def _count_triton_launches() -> list:
    """Every Triton launch of the process lands in the returned list (kernel name): `JITFunction.run` is what `kernel[grid](...)`
    calls.  The plug-in promises none on the path (north_star: "no Triton dispatch")."""
    seen = []
    try:
        from triton.runtime.jit import JITFunction
    except Exception:                                       # noqa: BLE001 -- no triton in this interpreter: nothing can launch
        return seen
    if getattr(JITFunction.run, "_counting", False):
        return JITFunction.run._seen
    run = JITFunction.run

    def counting_run(self, *a, **k):
        seen.append(getattr(self, "__name__", None) or getattr(getattr(self, "fn", None), "__name__", "?"))
        return run(self, *a, **k)

    counting_run._counting, counting_run._seen = True, seen
    JITFunction.run = counting_run
    return seen


def _profiled(fn, path):
    """cProfile around `fn`; `path` gets the host-time split by package (reference / plug-in / torch / other) and the top functions."""
    import cProfile
    import io
    import pstats

    pr = cProfile.Profile()
    pr.enable()
    try:
        out = fn()
    finally:
        pr.disable()
    st = pstats.Stats(pr)
    groups = {}
    for (file, line, name), (cc, nc, tt, ct, callers) in st.stats.items():
        f = file.replace("\\", "/")
        if "/sglang_amd/" in f:
            g = "plug-in (sglang_amd/)"
        elif "/sglang/" in f:
            g = "reference (sglang/)"
        elif "/torch/" in f or name.startswith("<built-in method torch") or "torch._C" in name:
            g = "torch"
        elif f.startswith("~") or f.startswith("<"):
            g = "builtins (incl. torch C calls)"
        else:
            g = "other python"
        groups[g] = groups.get(g, 0.0) + tt
    buf = io.StringIO()
    total = sum(groups.values())
    buf.write(f"# cProfile of the timed scheduler job (host side; tottime by package; the profiler inflates Python frames)\n")
    buf.write(f"# total profiled host seconds: {total:.3f}\n")
    for g, t in sorted(groups.items(), key=lambda kv: -kv[1]):
        buf.write(f"{t:9.3f} s  {100 * t / total:5.1f} %  {g}\n")
    for key in ("tottime", "cumulative"):
        buf.write(f"\n# top 60 by {key}\n")
        s2 = io.StringIO()
        pstats.Stats(pr, stream=s2).sort_stats(key).print_stats(60)
        buf.write(s2.getvalue())
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    Path(path).write_text(buf.getvalue())
    return out


def run_mem_hooks() -> dict:
    """Differential run of round 5's slot-bookkeeping / KV-store take-overs against the REFERENCE'S OWN device code on MI355X (its
    Triton kernels run here): the platform's allocator class vs the reference's `PagedTokenToKVPoolAllocator` driven through the
    same random request histories (page sizes 1 / 4 / 16: extends over page-misaligned prefixes, then decode steps; outputs and
    free lists compared after every call); the hooked `allocation.write_cache_indices` / `get_last_loc` vs the reference's Triton
    kernels called the way its own code calls them (allocation.py:71-82, :121-135); the platform's pool class vs the reference's
    `MHATokenToKVPool.set_kv_buffer` for bf16 and e4m3 pools (NHD) -- every comparison `torch.equal`."""
    loader = run_loader()
    ns = install()
    dev = torch.device("cuda")
    from sglang_amd import mem_hooks

    AL = importlib.import_module("sglang.srt.mem_cache.allocation")
    PG = importlib.import_module("sglang.srt.mem_cache.allocator.paged")
    MP = importlib.import_module("sglang.srt.mem_cache.memory_pool")
    KM = importlib.import_module("sglang.kernels.ops.memory.common")
    triton_seen = _count_triton_launches()
    g = torch.Generator().manual_seed(17)
    rep = dict(mode="mem-hooks", loader=dict(platform=loader["platform"], hooked=loader["hooked"]), allocator=[], write_cache_indices=[],
               get_last_loc=[], kv_store=[])

    def ri(lo, hi):
        return int(torch.randint(lo, hi, (1,), generator=g))

    # ---- 1. the paged allocator ----------------------------------------------------------------------------------------------
    Ours = mem_hooks.paged_allocator_class()
    for page in (1, 4, 16):
        size = 4096 * page
        ref_a = PG.PagedTokenToKVPoolAllocator(size, page_size=page, dtype=torch.bfloat16, device="cuda", kvcache=None, need_sort=False)
        our_a = Ours(size, page_size=page, dtype=torch.bfloat16, device="cuda", kvcache=None, need_sort=False)
        calls = 0
        for round_ in range(6):
            bs = ri(1, 24)
            prefix = [ri(0, 40) for _ in range(bs)]
            last = []
            # a request's cached prefix ends somewhere inside a page the request owns: the slot before the next free position
            for b in range(bs):
                last.append(-1 if prefix[b] == 0 else (1000 + b) * page + (prefix[b] - 1) % page)
            ext = [ri(1, 50) for _ in range(bs)]
            seq = [p_ + e for p_, e in zip(prefix, ext)]
            pl_c, sl_c = torch.tensor(prefix, dtype=torch.int64), torch.tensor(seq, dtype=torch.int64)
            pl, sl, ll = pl_c.to(dev), sl_c.to(dev), torch.tensor(last, dtype=torch.int64, device=dev)
            n0 = len(triton_seen)
            want = ref_a.alloc_extend(pl, pl_c, sl, sl_c, ll, sum(ext))
            n1 = len(triton_seen)
            got = our_a.alloc_extend(pl, pl_c, sl, sl_c, ll, sum(ext))
            assert n1 > n0 and len(triton_seen) == n1, "the reference's allocator must launch Triton, the platform's must not"
            ok = bool(torch.equal(got, want)) and bool(torch.equal(our_a.free_pages, ref_a.free_pages))
            calls += 1
            # decode steps on top: last_loc = the request's newest slot, read out of an int32 table as the reference does
            off, newest = 0, []
            for e in ext:
                newest.append(int(want[off + e - 1]))
                off += e
            for step in range(3 if page > 1 else 0):          # (at page size 1 the reference takes `alloc()`, never `alloc_decode`: allocation.py:526-528)
                seq = [x + 1 for x in seq]
                sl_c = torch.tensor(seq, dtype=torch.int64)
                sl = sl_c.to(dev)
                ll32 = torch.tensor(newest, dtype=torch.int32, device=dev)
                want_d = ref_a.alloc_decode(sl, sl_c, ll32)
                got_d = our_a.alloc_decode(sl, sl_c, ll32)
                ok = ok and bool(torch.equal(got_d, want_d)) and bool(torch.equal(our_a.free_pages, ref_a.free_pages))
                newest = want_d.tolist()
                calls += 1
            if not ok:
                break
        rep["allocator"].append(dict(page_size=page, calls=calls, equal=ok))
    # ---- 2. write_cache_indices / get_last_loc -------------------------------------------------------------------------------
    for bs in (1, 7, 60):
        width = 640
        table_ref = torch.zeros((bs + 3, width), dtype=torch.int32, device=dev)
        table_our = torch.zeros_like(table_ref)
        pool_idx = torch.randperm(bs + 2, generator=g)[:bs].to(torch.int64) + 1
        prefix = [ri(0, 200) for _ in range(bs)]
        ext = [ri(1, 300) for _ in range(bs)]
        seq = [p_ + e for p_, e in zip(prefix, ext)]
        prefix_tensors = [torch.randint(1, 100000, (p_,), generator=g, dtype=torch.int64).to(dev) for p_ in prefix]
        out_loc = torch.randint(1, 100000, (sum(ext),), generator=g, dtype=torch.int64).to(dev)
        to = lambda xs: torch.tensor(xs, dtype=torch.int64)          # noqa: E731
        pi_c, pl_c, sl_c, el_c = pool_idx.clone(), to(prefix), to(seq), to(ext)
        pi, pl, sl, el = pi_c.to(dev), pl_c.to(dev), sl_c.to(dev), el_c.to(dev)
        ptrs = torch.tensor([t.data_ptr() for t in prefix_tensors], dtype=torch.uint64).to(dev)
        KM.write_req_to_token_pool_triton[(bs,)](table_ref, pi, ptrs, pl, sl, el, out_loc, table_ref.shape[1])      # allocation.py:71-82
        before = mem_hooks.counts["write_cache_indices"]
        n1 = len(triton_seen)
        AL.write_cache_indices(out_loc, pi, pi_c, pl, pl_c, sl, sl_c, el, el_c, prefix_tensors, types.SimpleNamespace(req_to_token=table_our, device="cuda"))
        rep["write_cache_indices"].append(dict(batch=bs, equal=bool(torch.equal(table_our, table_ref)),
                                                served_by_the_hook=mem_hooks.counts["write_cache_indices"] == before + 1,
                                                triton_launches=len(triton_seen) - n1))
        want_l = KM.get_last_loc_triton_safe(table_ref, pi, pl)                                                        # allocation.py:121-135
        before = mem_hooks.counts["get_last_loc"]
        n1 = len(triton_seen)
        got_l = AL.get_last_loc(table_our, pi, pl)
        rep["get_last_loc"].append(dict(batch=bs, equal=bool(torch.equal(got_l, want_l)) and got_l.dtype == want_l.dtype,
                                         served_by_the_hook=mem_hooks.counts["get_last_loc"] == before + 1, triton_launches=len(triton_seen) - n1))
    # ---- 3. the KV store ------------------------------------------------------------------------------------------------------
    OurPool = mem_hooks.mha_kv_pool_class()
    layer = types.SimpleNamespace(layer_id=1)
    for dtype in (torch.bfloat16, torch.float8_e4m3fn):
        kw = dict(size=2048, page_size=1, dtype=dtype, head_num=4, head_dim=128, layer_num=2, device="cuda", enable_memory_saver=False)
        ref_p, our_p = MP.MHATokenToKVPool(**kw), OurPool(**kw)
        T = 333
        loc = (torch.randperm(2048, generator=g)[:T] + 1).to(torch.int64).to(dev)
        k = (torch.randn((T, 4, 128), generator=g) * 3).to(torch.bfloat16).to(dev)
        v = (torch.randn((T, 4, 128), generator=g) * 3).to(torch.bfloat16).to(dev)
        before = mem_hooks.counts["store_kv"]
        ref_p.set_kv_buffer(layer, MP.KVWriteLoc(loc, None), k.clone(), v.clone())
        our_p.set_kv_buffer(layer, MP.KVWriteLoc(loc, None), k.clone(), v.clone())
        same = all(bool(torch.equal(a_.view(torch.uint8), b_.view(torch.uint8))) for a_, b_ in zip(ref_p.k_buffer + ref_p.v_buffer, our_p.k_buffer + our_p.v_buffer))
        rep["kv_store"].append(dict(dtype=str(dtype), rows=T, equal=same, served_by_the_pool_class=mem_hooks.counts["store_kv"] == before + 1,
                                    nonzero=bool(our_p.k_buffer[1].view(torch.uint8).any())))
    rep["counts"] = dict(mem_hooks.counts)
    return rep


def run_latency(dims_name="tiny", batch_size=4, input_len=16, output_len=4) -> dict:
    """The reference's own latency benchmark -- `python -m sglang.bench_one_batch --load-format dummy --batch-size B --input-len I
    --output-len O` (benchmark/one_batch.py:877-990 latency_test: one warm-up pass, then `latency_test_run_once`, whose
    timing code and result record are the reference's) -- on the reference's ModelRunner with the plug-in loaded.  Static
    batch, no shared prefix, every decode step a replay of the reference's DecodeCudaGraphRunner graph."""
    import json as _json
    import tempfile as _tf

    gpu = not dry_run_on_cpu()
    loader = run_loader() if gpu else None
    ns = install()
    H, I, L, Hq, Hkv, D, V = DIMS[dims_name]
    d = Path(_tf.mkdtemp(prefix="ref_model_ckpt_"))
    (d / "config.json").write_text(_json.dumps(dict(
        architectures=["LlamaForCausalLM"], model_type="llama", hidden_size=H, intermediate_size=I, num_hidden_layers=L,
        num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=D, vocab_size=V, max_position_embeddings=8192, rope_theta=500000.0,
        rms_norm_eps=1e-5, tie_word_embeddings=False, torch_dtype="bfloat16", hidden_act="silu", bos_token_id=1, eos_token_id=2)))
    common = importlib.import_module("sglang.srt.utils.common")
    if not gpu:
        from sglang.kernels import fused_op as FO
        from sglang.kernels.spec import KernelBackend

        FO.set_fused_op_backend(KernelBackend.TORCH)
        common.get_device_memory_capacity = ns.server_args.get_device_memory_capacity = lambda device=None: 288 * 1024
        ns.distributed_parallel_state.is_cuda_alike = lambda: False
    else:
        try:
            common.get_device_memory_capacity("cuda")
        except Exception:                                   # noqa: BLE001
            mib = torch.cuda.mem_get_info()[1] // (1 << 20)
            common.get_device_memory_capacity = ns.server_args.get_device_memory_capacity = lambda device=None: mib
    OB = importlib.import_module("sglang.benchmark.one_batch")
    tokens = batch_size * (input_len + output_len)
    sa = ns.server_args.ServerArgs(
        model_path=str(d), load_format="dummy", skip_tokenizer_init=True, dtype="bfloat16", device="cuda" if gpu else "cpu",
        attention_backend=None if gpu else "torch_native", sampling_backend=loader["default_attention_backend"] if gpu else "pytorch",
        max_total_tokens=tokens + 4096, max_running_requests=max(16, batch_size), cuda_graph_max_bs_decode=batch_size,
        mem_fraction_static=0.5, disable_radix_cache=True, random_seed=3)
    model_config = importlib.import_module("sglang.srt.configs.model_config").ModelConfig.from_server_args(sa)
    ps = importlib.import_module("sglang.srt.distributed.parallel_state_wrapper").ParallelState.trivial(gpu_id=0)
    MR = importlib.import_module("sglang.srt.model_executor.model_runner")
    counts = dict(fused_decode_models=0, graph_replays=0)
    if gpu:
        import sglang_amd.fused_decode as fd

        decode_model = fd.decode_model

        def counting_decode_model(*a, **k):
            counts["fused_decode_models"] += 1
            return decode_model(*a, **k)

        fd.decode_model = counting_decode_model
    runner = MR.ModelRunner(model_config=model_config, mem_fraction_static=sa.mem_fraction_static, gpu_id=0, ps=ps,
                            nccl_port=29500 + os.getpid() % 400, server_args=sa)
    runner.alloc_memory_pool()
    runner.init_attention_backends()
    runner.init_cuda_graphs()
    graph_runner = getattr(runner, "decode_cuda_graph_runner", None)
    if graph_runner is not None and hasattr(graph_runner, "execute"):
        execute = graph_runner.execute

        def counting_execute(*a, **k):
            counts["graph_replays"] += 1
            return execute(*a, **k)

        graph_runner.execute = counting_execute
    bench_runner = OB._TorchBenchRunner(runner)
    lines = []

    def rank_print(*a, **k):
        lines.append(" ".join(str(x) for x in a))

    kw = dict(log_decode_step=0, profile=False, profile_record_shapes=False, profile_activities=("CPU", "GPU"), profile_prefix="",
              profile_stage="all", tp_rank=0, profile_start_step=None, profile_steps=None)
    reqs = OB.prepare_synthetic_inputs_for_latency_test(batch_size, input_len)
    OB.latency_test_run_once("warmup", bench_runner, rank_print, reqs, batch_size, input_len, min(32, output_len), **kw)
    counts_before = dict(counts)
    reqs = OB.prepare_synthetic_inputs_for_latency_test(batch_size, input_len)
    result = OB.latency_test_run_once("sglang_amd", bench_runner, rank_print, reqs, batch_size, input_len, output_len, **kw)
    return dict(mode="latency", dims=dims_name, device=str(runner.device), attention_backend=sa.attention_backend,
                attn_backend_class=type(runner.attn_backend).__name__, graph_runner=type(graph_runner).__name__ if graph_runner is not None else None,
                result={k: (float(v) if not isinstance(v, (str, int)) else v) for k, v in (result or {}).items()},
                graph_replays_in_the_measured_run=counts["graph_replays"] - counts_before["graph_replays"],
                eager_fused_decode_forwards_in_the_measured_run=counts["fused_decode_models"] - counts_before["fused_decode_models"],
                log=lines[-12:])


# The staged copy is the reference's whole python tree (.py files) minus the model zoo: with a GPU present the reference takes
# import branches the build container cannot execute (Triton kernels, ROCm-only modules, the graph runners), and a module missing
# from the staged copy would silently become a stub.
STAGE_EXCLUDE = ("sglang/srt/models/",)       # ~200 model files; only the ones below travel (the model registry walks what is there)
STAGE_FILES = ("sglang/srt/models/llama.py", "sglang/srt/models/qwen2.py", "sglang/srt/models/mixtral.py", "sglang/srt/models/utils.py",
               "sglang/srt/models/registry.py", "sglang/srt/models/__init__.py")


def stage() -> None:
    """Build container: copy the reference's python tree (minus the model zoo) to oracle/_ref/sglang_model/ (git-ignored; travels
    with the gpurun snapshot)."""
    import shutil

    if not R.has_checkout():
        raise SystemExit("no reference checkout (SGLANG_REFERENCE_ROOT): staging needs the reference's own sources")
    files = set()
    for f in (R.CONTAINER_REF / "sglang").rglob("*.py"):
        rel = f.relative_to(R.CONTAINER_REF).as_posix()
        if not any(rel.startswith(x) for x in STAGE_EXCLUDE):
            files.add(f)
    files.update(R.CONTAINER_REF / f for f in STAGE_FILES if (R.CONTAINER_REF / f).exists())
    if STAGE.exists():
        shutil.rmtree(STAGE)
    for f in sorted(files):
        dst = STAGE / f.relative_to(R.CONTAINER_REF)
        dst.parent.mkdir(parents=True, exist_ok=True)
        shutil.copyfile(f, dst)
    total = sum(f.stat().st_size for f in files)
    print(f"staged {len(files)} reference files ({total / 1e6:.1f} MB) under {STAGE}")


def _json_arg(text):
    import json as _j

    return _j.loads(text) if text else None


if __name__ == "__main__":
    import argparse
    import json

    ap = argparse.ArgumentParser()
    ap.add_argument("--run", choices=["cpu-oracle", "loader", "gpu", "runner", "latency", "shared-prefix", "scheduler", "mem-hooks", "stage"], required=True)
    ap.add_argument("--dims", default="tiny", choices=sorted(DIMS))
    ap.add_argument("--json", default=None)
    ap.add_argument("--shape", default="4,16,4", help="latency run: batch size, input length, output length")
    ap.add_argument("--job", default="2,2,16,8,4", help="shared-prefix run: groups, requests per group, shared tokens, own tokens, output tokens")
    ap.add_argument("--server-args", default=None, help='scheduler run: extra ServerArgs as JSON, e.g. {"page_size": 16, "chunked_prefill_size": 64}')
    ap.add_argument("--logprobs", action="store_true", help="scheduler run: return_logprob + top-2 logprobs on every request")
    ap.add_argument("--sampling", default=None, help='scheduler run: SamplingParams of every request as JSON, e.g. {"temperature": 0.8, "top_k": 20, "top_p": 0.9}')
    ap.add_argument("--spec-ngram", type=int, default=0, help="scheduler run: NGRAM speculative decoding with N draft tokens (scripted drafter): TARGET_VERIFY forwards")
    ap.add_argument("--spec-tree", action="store_true", help="scheduler run with --spec-ngram: the scripted drafter also proposes wrong BRANCHES (breadth 2)")
    ap.add_argument("--overlap", action="store_true", help="scheduler run: the body of event_loop_overlap (the server default)")
    ap.add_argument("--radix", action="store_true", help="shared-prefix run: prefixes from the reference's real RadixCache")
    ap.add_argument("--tp", type=int, default=1, help="tensor-parallel ranks: this process launches itself N times (rank 0 reports)")
    a = ap.parse_args()
    if a.tp > 1 and "REF_MODEL_RANK" not in os.environ:
        import subprocess

        port = 29500 + os.getpid() % 400
        procs = []
        multi_gpu = torch.cuda.is_available() and torch.cuda.device_count() >= a.tp
        for r in range(a.tp):
            env = dict(os.environ, REF_MODEL_WORLD=str(a.tp), REF_MODEL_RANK=str(r), REF_MODEL_PORT=str(port),
                       SGLANG_USE_MESSAGE_QUEUE_BROADCASTER="false", HSA_ENABLE_IPC_MODE_LEGACY="0")
            if multi_gpu:
                env["REF_MODEL_MULTI_GPU"] = "1"              # one device per rank, RCCL device groups (init_parallel)
            else:
                env["SGLANG_NCCL_SO_PATH"] = "/nonexistent/librccl.so"      # all ranks on GPU 0: the reference's "no NCCL library" branch
            procs.append(subprocess.Popen([sys.executable, __file__] + sys.argv[1:], env=env,
                                          stdout=None if r == 0 else subprocess.DEVNULL, stderr=None))
        import time

        deadline = time.time() + 1500
        while any(p_.poll() is None for p_ in procs) and time.time() < deadline:
            if any(p_.poll() not in (None, 0) for p_ in procs):      # a rank died: the others would wait in a collective
                break
            time.sleep(0.5)
        for p_ in procs:
            if p_.poll() is None:
                p_.kill()
        sys.exit(max((p_.wait() or 0) if p_.returncode is not None else 1 for p_ in procs))
    if a.run == "stage":
        stage()
        sys.exit(0)
    rep = {"cpu-oracle": lambda: run_cpu_oracle(a.dims), "loader": run_loader, "gpu": lambda: run_gpu(a.dims), "mem-hooks": run_mem_hooks,
           "runner": lambda: run_runner(a.dims, _json_arg(a.server_args)), "latency": lambda: run_latency(a.dims, *[int(x) for x in a.shape.split(",")]),
           "scheduler": lambda: run_scheduler_job(a.dims if a.dims != "tiny" else "tiny_v16k", *[int(x) for x in a.job.split(",")],
                                                  overlap=a.overlap, server_args=_json_arg(a.server_args), logprobs=a.logprobs, spec_ngram=a.spec_ngram, sampling=_json_arg(a.sampling),
                                                  spec_tree=a.spec_tree),
           "shared-prefix": lambda: run_shared_prefix_job(a.dims if a.dims != "tiny" else "tiny_v16k", *[int(x) for x in a.job.split(",")],
                                                          radix=a.radix)}[a.run]()
    rep["tp"] = tp_world()[0]
    rep["devices"] = ("one GPU per rank, RCCL device groups" if os.environ.get("REF_MODEL_MULTI_GPU") == "1" else
                      "every rank on GPU 0, gloo device groups" if tp_world()[0] > 1 else "one rank")
    text = json.dumps(rep, indent=1)
    if tp_world()[1] != 0:
        text, a.json = "", None
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(text)
    print(text)
    try:
        from sglang_amd import tp_hooks

        tp_hooks.close_all()
    except Exception:                      # noqa: BLE001 -- the dry run never loaded the native library
        pass
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
