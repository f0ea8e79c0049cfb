"""Engine.ngram_speculative_step on the radix-shared three-request tiny-llama batch of test_speculative_step_gpu.py, with prompts
from a 6-token alphabet, greedy, two consecutive steps: the drafted tree equals the drafting rule applied to the host's
origin_input_ids + output_ids as they were before the step (for the second step: ngram_commit kept the device table current), the
appended tokens equal the greedy accept rule applied in float64 to the returned logits, and the allocator lost exactly the committed
slots.  Synthetic weights sample tokens outside the alphabet, which never occurred before: the first step's last sampled token is
replaced by the prompt's own first token before anything on the device has seen it, so that its draft has hits.  Then a plain decode
step and finish: every slot is back; and generate_speculative (continuations of two tokens: trees that branch) ends every request at
its limit with every slot back."""
import pytest
import torch
from test_ngram_draft_gpu import ngram_draft_reference

pytestmark = pytest.mark.gpu
ND = 8


def test_ngram_speculative_steps_draft_from_the_device_history(device):
    from sglang_amd.harness.engine import Engine, ModelRunner, Req
    from sglang_amd.harness.models import CONFIGS

    cfg = CONFIGS["tiny-llama"]
    runner = ModelRunner(cfg, max_total_tokens=4096, max_running_requests=8, max_context_len=192, device=device, use_graph=False)
    eng = Engine(runner)
    alloc = runner.token_to_kv_pool_allocator
    pool_size = alloc.available_size()
    g = torch.Generator().manual_seed(21)
    shared = torch.randint(0, 6, (70,), generator=g).tolist()
    prompts = [shared + torch.randint(0, 6, (n,), generator=g).tolist() for n in (5, 9, 1)]
    reqs = [Req(i, p, 16) for i, p in enumerate(prompts)]
    eng.prefill(reqs[:1]); eng.prefill(reqs[1:])
    for q in reqs:
        q.output_ids[-1] = q.origin_input_ids[0]

    for step in range(2):
        hist = [q.origin_input_ids + q.output_ids for q in reqs]
        free_before = alloc.available_size()
        new, logits, (tree, parents, num_real) = eng.ngram_speculative_step(ND, return_logits=True)
        tree, parents, num_real = tree.tolist(), parents.tolist(), num_real.tolist()
        want = []
        for b, h in enumerate(hist):
            assert (tree[b], parents[b], num_real[b]) == ngram_draft_reference(h, ND, 4, 1, 4, ND - 1, 0, 0), (step, b)
            top = logits[b].double().argmax(-1).tolist()    # verify_tree_greedy, literally, on the returned logits
            cur, path = 0, []
            while True:
                nxt = next((c for c in range(ND) if parents[b][c] == cur and tree[b][c] == top[cur]), -1)
                if nxt < 0:
                    break
                cur = nxt
                path.append(tree[b][cur])
            want.append(path + [top[cur]])
        assert new == want and [q.output_ids[-len(n):] for q, n in zip(reqs, new)] == want
        assert free_before - alloc.available_size() == sum(len(n) for n in new)

    eng.decode_step(); eng.flush_decode_outputs()
    eng.finish(list(eng.running))
    assert alloc.available_size() + runner.tree_cache.evictable_size() == pool_size

    again = [Req(10 + i, p[:40 + i], 7) for i, p in enumerate(prompts)]
    eng.generate_speculative(again, 6, depth=2)
    assert [len(q.output_ids) for q in again] == [7, 7, 7] and not eng.running
    assert alloc.available_size() + runner.tree_cache.evictable_size() == pool_size
