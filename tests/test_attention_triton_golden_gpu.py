"""The HIP attention kernels against outputs of the REFERENCE'S OWN Triton kernels (extend_attention_fwd,
decode_attention_fwd; kernels/ops/attention/extend_attention.py:753, decode_attention.py:1163), recorded on an MI355X
by tests/golden/gen_triton_golden.py: logit soft cap, sliding window, the TARGET_VERIFY custom mask
(triton_backend.py:860-919) with and without the prefix part masked, and their combinations -- the features the
torch-native SDPA goldens cannot express.  Bar: one bf16 ulp of the output (the reference kernels round P to bf16
before PV; ours keep P in bf16 for the MFMA too)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _cases(golden_dir):
    cases = {}          # stored in parts (tests/golden/gen_triton_golden.py save_parts): {case: {some of its keys}} per file
    for f in sorted(golden_dir.glob("attention_triton.*.pt")):
        for name, part in torch.load(f).items():
            cases.setdefault(name, {}).update(part)
    assert sorted(cases) == ["_meta", "gqa4_d128", "mha_d64"] and all(len(cases[k]) == 27 for k in ("gqa4_d128", "mha_d64")), sorted(cases)
    return {k: v for k, v in cases.items() if not k.startswith("_")}


def _close(got, ref, what, max_abs=2.0 ** -7, rms=1e-3):
    e = (got.float().cpu() - ref.float()).abs()
    assert float(e.max()) <= max_abs * max(1.0, float(ref.float().abs().max())), (what, float(e.max()))
    assert float(e.pow(2).mean().sqrt()) <= rms, (what, float(e.pow(2).mean().sqrt()))


def _extend(device, c, q, scaling, **opt):
    from sglang_amd import kernels as K

    ext = c["extend_seq_lens"].to(torch.int32)
    qo = torch.zeros(len(ext) + 1, dtype=torch.int32)
    qo[1:] = torch.cumsum(ext, 0)
    out = torch.empty_like(q, device=device)
    if opt.get("custom_mask") is not None:
        opt["custom_mask"] = opt["custom_mask"].to(device)
        opt["mask_indptr"] = opt["mask_indptr"].to(torch.int64).to(device)
    K.extend_attention(q.to(device), out, c["k_cache"].to(device), c["v_cache"].to(device), c["req_to_token"].to(device),
                       c["req_pool_indices"].to(torch.int64).to(device), c["seq_lens"].to(torch.int32).to(device),
                       c["extend_prefix_lens"].to(torch.int32).to(device), qo.to(device), int(ext.max()), scaling, True, **opt)
    return out


@pytest.mark.parametrize("shape", ["auto", "82", "42", "41"])
def test_extend_cap_window_vs_reference_triton(device, golden_dir, extend_shape, shape):
    extend_shape(shape)
    for name, d in _cases(golden_dir).items():
        cap, win = d["logit_cap"], d["sliding_window"]
        for tag, opt in dict(causal={}, cap=dict(logit_cap=cap), window=dict(sliding_window=win),
                             cap_window=dict(logit_cap=cap, sliding_window=win)).items():
            _close(_extend(device, d, d["q"], d["scaling"], **opt), d["out_extend_" + tag], f"{name} {tag} shape={shape}")


def test_verify_mask_vs_reference_triton(device, golden_dir):
    for name, d in _cases(golden_dir).items():
        v = d["verify"]
        for tag in ("verify", "verify_prefix_masked"):
            for cap in (0.0, d["logit_cap"]):
                o = _extend(device, v, v["q"], d["scaling"], custom_mask=d[tag + "_mask"], mask_indptr=d[tag + "_mask_indptr"], logit_cap=cap)
                _close(o, d["out_" + tag + ("_cap" if cap else "")], f"{name} {tag} cap={cap}")


def test_verify_mask_prefix_part_is_not_consulted_with_skip_prefix(device, golden_dir):
    """The reference's TARGET_VERIFY call leaves skip_prefix_custom_mask at its default (extend_attention.py:774): the
    prefix columns of the mask are never read.  Zero them: with the flag the result is still the golden's."""
    for name, d in _cases(golden_dir).items():
        v = d["verify"]
        mask, mip = d["verify_mask"].clone(), d["verify_mask_indptr"]
        for b in range(len(v["seq_lens"])):
            pre, ext, kv = int(v["extend_prefix_lens"][b]), int(v["extend_seq_lens"][b]), int(v["seq_lens"][b])
            blk = mask[int(mip[b]): int(mip[b]) + ext * kv].view(ext, kv)
            blk[:, :pre] = False
        o = _extend(device, v, v["q"], d["scaling"], custom_mask=mask, mask_indptr=mip, skip_prefix_custom_mask=True)
        _close(o, d["out_verify"], f"{name} verify, prefix part zeroed + skip_prefix")


@pytest.mark.parametrize("splits", [1, 3])
def test_decode_cap_vs_reference_triton(device, golden_dir, splits):
    from sglang_amd import kernels as K

    for name, d in _cases(golden_dir).items():
        q = d["q_decode"]
        B, Hq, D = q.shape
        # the reference's MHA decode kernel sums bf16 products (decode_attention.py:362): its outputs sit up to 6e-2 from
        # an fp32 evaluation of the same inputs (tests/test_oracle_golden.py), so that case only bounds gross errors
        loose = Hq == d["k_cache"].shape[1]
        bars = dict(max_abs=0.08, rms=1e-2) if loose else {}
        for cap in (0.0, d["logit_cap"]):
            out = torch.empty_like(q, device=device)
            ws = K.decode_workspace(B, Hq, D, splits, device) if splits > 1 else (None, None)
            K.decode_attention(q.to(device), d["k_cache"].to(device), d["v_cache"].to(device), out, d["req_to_token"].to(device),
                               d["req_pool_indices"].to(torch.int64).to(device), d["seq_lens"].to(torch.int32).to(device),
                               d["scaling"], splits, ws[0], ws[1], logit_cap=cap)
            _close(out, d["out_decode_cap" if cap else "out_decode"], f"{name} decode cap={cap} splits={splits}", **bars)
