"""Engine.speculative_step on the radix-shared three-request batch of the TARGET_VERIFY test, greedy: the tree carries the model's
own continuation on the path 0 -> 1 -> 3, so drafts are accepted; the appended tokens equal the accept rule applied in float64 to
the returned logits, the allocator lost exactly the committed slots, and the next decode step sees the right KV rows."""
import pytest
import torch

pytestmark = pytest.mark.gpu
PARENTS = [-1, 0, 0, 1, 1, 2, 5]


def test_speculative_step_commits_the_accepted_path(device):
    from oracle.model import OracleLM, weights_from_product_model
    from sglang_amd.harness.engine import Engine, ModelRunner, Req
    from sglang_amd.harness.models import CONFIGS

    cfg, nd = CONFIGS["tiny-llama"], len(PARENTS)
    runner = ModelRunner(cfg, max_total_tokens=4096, max_running_requests=8, max_context_len=192, device=device, use_graph=False)
    eng = Engine(runner)
    alloc = runner.token_to_kv_pool_allocator
    pool_size = alloc.available_size()
    g = torch.Generator().manual_seed(21)
    shared = torch.randint(0, cfg.vocab_size, (70,), generator=g).tolist()
    prompts = [shared + torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist() for n in (5, 9, 1)]
    reqs = [Req(i, p, 16) for i, p in enumerate(prompts)]
    eng.prefill(reqs[:1]); eng.prefill(reqs[1:])
    eng.decode_step(); eng.decode_step(); eng.flush_decode_outputs()
    trees = [[q.output_ids[-1]] + torch.randint(0, cfg.vocab_size, (nd - 1,), generator=g).tolist() for q in reqs]
    for node, child in ((0, 1), (1, 3)):                    # the model's own next token at node 0, then behind it at node 1
        scores = eng.verify_tree(trees, PARENTS)
        for b in range(len(reqs)):
            trees[b][child] = int(scores[b, node].double().argmax())

    free_before = alloc.available_size()
    new, logits = eng.speculative_step(trees, PARENTS, return_logits=True)
    want = []
    for b in range(len(reqs)):                              # verify_tree_greedy, literally, on the returned logits
        top = logits[b].double().argmax(-1).tolist()
        cur, path = 0, []
        while True:
            nxt = next((c for c in range(nd) if PARENTS[c] == cur and trees[b][c] == top[cur]), -1)
            if nxt < 0:
                break
            cur = nxt
            path.append(trees[b][cur])
        want.append(path + [top[cur]])
    assert new == want and [q.output_ids[-len(n):] for q, n in zip(reqs, new)] == want
    assert max(len(n) for n in new) >= 2, new                # at least one request accepted a draft
    assert free_before - alloc.available_size() == sum(len(n) for n in new)

    eng.logits_by_req = {}
    seqs = [q.origin_input_ids + q.output_ids for q in reqs]
    eng.decode_step(); eng.flush_decode_outputs()
    oracle = OracleLM(cfg, weights_from_product_model(runner.model, device), num_slots=8192, max_ctx=192, max_reqs=1, device=device,
                      compute_dtype=torch.float32)
    for q, seq in zip(reqs, seqs):
        oracle.next_slot = 1
        ref = oracle.generate([seq], 1, return_logits=True)[1][0][0]
        worst = float((eng.logits_by_req[q.rid][-1].to(ref.device) - ref).abs().max())
        assert worst < 3e-2, (q.rid, worst)
    eng.finish(list(eng.running))
    assert alloc.available_size() + runner.tree_cache.evictable_size() == pool_size
