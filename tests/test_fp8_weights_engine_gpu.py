"""End-to-end GPU parity of the engine over weight-only fp8 (e4m3 + per-channel scale) projections, hipGraph decode, against the
CPU oracle model run on the DEQUANTISED weights: same bar as the bf16 dense models of test_engine_gpu.py."""
import random

import pytest
import torch

import oracle.model as om

pytestmark = pytest.mark.gpu


def _shared_prefix_prompts(cfg, groups=2, per_group=3, shared=70, unique=9, seed=1):
    rnd = random.Random(seed)
    prompts = []
    for _ in range(groups):
        sys_p = [rnd.randrange(cfg.vocab_size) for _ in range(shared)]
        prompts += [sys_p + [rnd.randrange(cfg.vocab_size) for _ in range(unique)] for _ in range(per_group)]
    return prompts


def _dequantised_weights(model):
    """weights_from_product_model, with every quantised projection as fp32 w8 * scale (exact: 4 x 24 significand bits fit)."""
    w = om.weights_from_product_model(model)
    for i, layer in enumerate(model.layers):
        for key, lin in ((f"layers.{i}.self_attn.qkv_proj", layer.self_attn.qkv_proj), (f"layers.{i}.self_attn.o_proj", layer.self_attn.o_proj),
                         (f"layers.{i}.mlp.gate_up_proj", layer.mlp.gate_up_proj), (f"layers.{i}.mlp.down_proj", layer.mlp.down_proj)):
            w[key + ".weight"] = lin.weight.data.cpu().float() * lin.weight_scale.data.cpu()[:, None]
    return w


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-qwen"])
def test_fp8_weight_generation_matches_oracle_on_dequantised_weights(device, name, monkeypatch):
    from sglang_amd.harness.engine import Engine, ModelRunner, Req
    from sglang_amd.harness.models import CONFIGS

    cfg = CONFIGS[name]
    runner = ModelRunner(cfg, max_total_tokens=4096, max_running_requests=16, max_context_len=512, device=device, init_device="cpu",
                         use_graph=True, weight_dtype="fp8_e4m3")
    eng = Engine(runner)
    for layer in runner.model.layers:
        for lin in (layer.self_attn.qkv_proj, layer.self_attn.o_proj, layer.mlp.gate_up_proj, layer.mlp.down_proj):
            assert lin.weight.dtype == torch.float8_e4m3fn and lin.weight_scale.shape == (lin.weight.shape[0],)
    assert runner.model.lm_head.dtype == torch.bfloat16
    prompts, new_tokens = _shared_prefix_prompts(cfg), 6
    eng.logits_trace = []
    eng.prefill([Req(i, prompts[i], new_tokens) for i in (0, 3)])
    eng.prefill([Req(i, prompts[i], new_tokens) for i in (1, 2, 4, 5)])
    for _ in range(new_tokens - 1):
        eng.decode_step()
    # the decode steps took the fused fp8 layer inside a captured graph
    x = torch.zeros((6, cfg.hidden_size), dtype=torch.bfloat16, device=device)
    assert all(layer.fusable(x, 1) for layer in runner.model.layers)
    assert runner.graph_runner is not None and len(runner.graph_runner.graphs) > 0
    reqs = list(eng.running)
    eng.finish(reqs)
    order = [0, 3, 1, 2, 4, 5]
    outs = [None] * 6
    for q in reqs:
        outs[q.rid] = q.output_ids
    tr = eng.logits_trace
    inv = [order.index(i) for i in range(6)]
    trace = [s[inv] for s in [torch.cat([tr[0], tr[1]])] + tr[2:]]

    # the oracle multiplies in the activations' dtype: run its linears in fp32 so that the fp32 dequantised weights are not re-rounded
    lin = torch.nn.functional.linear
    with monkeypatch.context() as mp:
        mp.setattr(om.F, "linear", lambda x, w, b=None: lin(x.float(), w.float(), None if b is None else b.float()).to(x.dtype))
        oracle = om.OracleLM(cfg, _dequantised_weights(runner.model), compute_dtype=torch.float32, max_reqs=63, num_slots=4096)
        _, ref_logits = oracle.generate(prompts, new_tokens, return_logits=True, forced=outs)
    worst = agree = total = 0
    for step, (got, ref) in enumerate(zip(trace, ref_logits)):
        worst = max(worst, float((got.float() - ref.float()).abs().max()))
        print(f"step {step}: max |logit error| {float((got.float() - ref.float()).abs().max()):.4g}")
        torch.testing.assert_close(got, ref, atol=2e-2, rtol=2e-2, msg=f"logits step {step}")      # (= no outlier rows)
        top2 = ref.topk(2, dim=-1).values
        clear = (top2[:, 0] - top2[:, 1]) > 4e-2
        total += int(clear.sum())
        agree += int((got.argmax(-1)[clear] == ref.argmax(-1)[clear]).sum())
    print(f"{name}: max |logit error| over {new_tokens} steps {worst:.4g}")
    assert agree == total, f"argmax differs on {total - agree}/{total} clear-margin rows"


def test_auto_weight_dtype_stays_bf16(device):
    from sglang_amd.harness.models import CONFIGS, CausalLM, Linear

    model = CausalLM(CONFIGS["tiny-llama"], device, "cpu")
    lins = [m for m in model.modules() if isinstance(m, Linear)]
    assert len(lins) == 8 and all(l.weight.dtype == torch.bfloat16 and l.weight_scale is None for l in lins)
