"""The logprob entry points are exported and refuse bad arguments on the host, before any launch (no GPU needed)."""
import ctypes

from sglang_amd import native


def test_logprob_symbols_and_cap():
    lib = native.lib()
    for name in ("sgl_amd_logprobs_from_logits", "sgl_amd_logprobs_workspace_bytes", "sgl_amd_logprobs_max_top"):
        assert name in native.declared_symbols() and hasattr(lib, name)
    assert lib.sgl_amd_logprobs_max_top() >= 20
    assert lib.sgl_amd_logprobs_workspace_bytes(64, 32, 20) >= 64 * 32 * (8 + 20 * 8)


def test_argument_errors_are_reported_not_thrown():
    lib = native.lib()
    cap = lib.sgl_amd_logprobs_max_top()
    buf = ctypes.create_string_buffer(64)        # stands for every pointer: nothing is dereferenced before the checks pass
    p = ctypes.addressof(buf)

    def call(n_top, chosen=p, top_val=p, top_idx=p, req_val=p, req_total=0):
        return lib.sgl_amd_logprobs_from_logits(p, 1, 8, None, p, 0, 1, 8, n_top, p, p, req_total, chosen, top_val, top_idx, req_val, 1, p, None)

    assert call(cap + 1) == -1 and b"n_top" in lib.sgl_amd_last_error()
    assert call(1, top_val=None) == -1 and b"top_val" in lib.sgl_amd_last_error()
    assert call(1, top_idx=None) == -1 and b"top_idx" in lib.sgl_amd_last_error()
    assert call(0, chosen=None) == -1 and b"chosen_logprob" in lib.sgl_amd_last_error()
    assert call(0, req_val=None, req_total=3) == -1 and b"req_val" in lib.sgl_amd_last_error()
