"""Prefill over weight-only fp8 (e4m3) projections runs on the fp8-weight MFMA tile GEMM: end-to-end logits against the CPU
oracle on the dequantised weights (the bar of test_fp8_weights_engine_gpu.py), and the routing of Linear / MLP."""
import random

import pytest
import torch

import oracle.model as om
from test_fp8_weights_engine_gpu import _dequantised_weights

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _no_fallback(self, x):
    raise AssertionError("Linear._forward_fp8_rows reached")


def test_fp8_prefill_of_600_rows_matches_oracle_on_dequantised_weights(device, monkeypatch):
    from sglang_amd.harness.engine import Engine, ModelRunner, Req
    from sglang_amd.harness.models import CONFIGS, Linear

    cfg = CONFIGS["tiny-llama"]
    runner = ModelRunner(cfg, max_total_tokens=4096, max_running_requests=16, max_context_len=512, device=device, init_device="cpu",
                         use_graph=False, weight_dtype="fp8_e4m3")
    eng = Engine(runner)
    rnd = random.Random(7)
    prompts = [[rnd.randrange(cfg.vocab_size) for _ in range(200)] for _ in range(3)]      # 600 rows: a third row block
    eng.logits_trace = []
    with monkeypatch.context() as mp:
        mp.setattr(Linear, "_forward_fp8_rows", _no_fallback)
        eng.prefill([Req(i, prompts[i], 2) for i in range(3)])
    got = eng.logits_trace[0]
    eng.finish(list(eng.running))
    lin = torch.nn.functional.linear
    with monkeypatch.context() as mp:
        mp.setattr(om.F, "linear", lambda x, w, b=None: lin(x.float(), w.float(), None if b is None else b.float()).to(x.dtype))
        oracle = om.OracleLM(cfg, _dequantised_weights(runner.model), compute_dtype=torch.float32, max_reqs=63, num_slots=4096)
        _, ref_logits = oracle.generate(prompts, 1, return_logits=True)
    print(f"max |logit error| {float((got.float() - ref_logits[0].float()).abs().max()):.4g}")
    torch.testing.assert_close(got, ref_logits[0], atol=2e-2, rtol=2e-2)


def test_fp8_linear_and_mlp_route_300_rows_to_the_tile_kernel(device, monkeypatch):
    from sglang_amd import kernels
    from sglang_amd.harness.models import CONFIGS, Linear, LlamaMLP

    monkeypatch.setattr(Linear, "_forward_fp8_rows", _no_fallback)
    cfg = CONFIGS["tiny-llama"]
    mlp = LlamaMLP(cfg, "layers.0.mlp", "cpu", device, 0, 1, weight_dtype="fp8_e4m3")
    x = (torch.randn((300, cfg.hidden_size), generator=torch.Generator().manual_seed(3)) * 0.5).to(BF).to(device)
    gu, down = mlp.gate_up_proj, mlp.down_proj
    assert torch.equal(gu(x), kernels.dense_tiled_gemm(x, gu.weight.data, w_scale=gu.weight_scale.data))
    act = kernels.dense_tiled_gemm(x, gu.weight.data, epilogue="silu_and_mul", w_scale=gu.weight_scale.data)
    assert act.shape == (300, cfg.intermediate_size)
    assert torch.equal(mlp(x), kernels.dense_tiled_gemm(act, down.weight.data, w_scale=down.weight_scale.data))
