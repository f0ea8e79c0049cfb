"""A TARGET_VERIFY forward_extend through HipAttnBackend reaches the split-KV verify kernel when routing is on, and layers
the kernel does not serve (sliding window) keep the extend kernel -- read off the backend's `served` counters."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
BF, TOL = torch.bfloat16, 4e-3
Hq, Hkv, D, B, ND = 8, 2, 128, 3, 4


def test_target_verify_routes_to_the_verify_kernel(device):
    from sglang_amd.layers.attention.hip_backend import HipAttnBackend
    from sglang_amd.layers.radix_attention import RadixAttention
    from sglang_amd.mem_cache.memory_pool import MHATokenToKVPool, ReqToTokenPool
    from sglang_amd.model_executor.forward_batch_info import ForwardBatch, ForwardMode, VerifyInput

    g = torch.Generator().manual_seed(7)
    r2t, kv = ReqToTokenPool(8, 512, device), MHATokenToKVPool(2048, 1, BF, Hkv, D, 1, device)
    runner = types.SimpleNamespace(device=device, req_to_token_pool=r2t, token_to_kv_pool=kv, num_attention_heads_per_rank=Hq,
                                   num_kv_heads_per_rank=Hkv, head_dim=D, enable_verify_attention=True, enable_cascade_attention=False)
    backend = HipAttnBackend(runner)
    pools, prefix = [4, 1, 6], [37, 130, 300]
    seq = [p + ND for p in prefix]
    slots = (torch.randperm(2000, generator=g) + 1)
    cur = 0
    for b in range(B):
        r2t.req_to_token[pools[b], :seq[b]] = slots[cur:cur + seq[b]].int().to(device)
        cur += seq[b]
    kv.k_buffer[0].copy_(torch.randn(kv.k_buffer[0].shape, generator=g).to(BF))
    kv.v_buffer[0].copy_(torch.randn(kv.v_buffer[0].shape, generator=g).to(BF))
    loc = torch.cat([r2t.req_to_token[pools[b], prefix[b]:seq[b]] for b in range(B)]).long()
    blocks, trees = [], []
    for b in range(B):
        tree = torch.tril(torch.ones((ND, ND), dtype=torch.bool))
        tree[3, 1:3] = False                                   # token 3 hangs off token 0: a tree, not a chain
        m = torch.zeros((ND, seq[b]), dtype=torch.bool)        # zeros under the prefix: never consulted
        m[:, prefix[b]:] = tree
        blocks.append(m.flatten()); trees.append(tree)
    spec = VerifyInput(custom_mask=torch.cat(blocks).to(device), draft_token_num=ND)
    fb = ForwardBatch(forward_mode=ForwardMode.TARGET_VERIFY, batch_size=B, input_ids=torch.zeros(B * ND, dtype=torch.int64, device=device),
                      req_pool_indices=torch.tensor(pools, device=device), seq_lens=torch.tensor(prefix, dtype=torch.int32, device=device),
                      out_cache_loc=loc, seq_lens_cpu=torch.tensor(prefix), req_to_token_pool=r2t, token_to_kv_pool=kv,
                      attn_backend=backend, spec_info=spec)
    backend.init_forward_metadata_out_graph(fb)
    backend.init_forward_metadata_in_graph(fb)
    assert backend.forward_metadata.verify_splits > 1
    qkv = torch.randn((B * ND, (Hq + 2 * Hkv) * D), generator=g).to(BF).to(device)
    q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)

    want = torch.zeros((B * ND, Hq, D), dtype=torch.float64)
    for b in range(B):
        rows = r2t.req_to_token[pools[b], :seq[b]].long()
        kk, vv = (x[rows].double().cpu().repeat_interleave(Hq // Hkv, 1) for x in (kv.k_buffer[0], kv.v_buffer[0]))
        kk[prefix[b]:], vv[prefix[b]:] = (x[b * ND:(b + 1) * ND].reshape(ND, Hkv, D).double().cpu().repeat_interleave(Hq // Hkv, 1) for x in (k, v))
        vis = torch.ones((ND, seq[b]), dtype=torch.bool)
        vis[:, prefix[b]:] = trees[b]
        s = torch.einsum("ehd,shd->hes", q[b * ND:(b + 1) * ND].reshape(ND, Hq, D).double().cpu(), kk) * D ** -0.5
        want[b * ND:(b + 1) * ND] = torch.einsum("hes,shd->ehd", torch.softmax(s.masked_fill(~vis, float("-inf")), -1), vv)

    for window, kernel in ((-1, "verify_attention"), (4096, "extend_attention")):       # a window wider than every context: same result
        layer = RadixAttention(Hq, D, D ** -0.5, Hkv, 0, sliding_window_size=window)
        before = dict(backend.served)
        out = layer(q, k, v, fb).view(B * ND, Hq, D)
        assert backend.served[kernel] == before[kernel] + 1 and sum(backend.served.values()) == sum(before.values()) + 1
        err = (out.double().cpu() - want).abs()
        print(f"{kernel}: max abs err {float(err.max()):.3e}")
        assert bool((err <= TOL + TOL * want.abs()).all()), (kernel, float(err.max()))
