"""Host side of the split-KV verify attention: the row cap, argument rejections before any launch, the split policy."""
import pytest

from sglang_amd import kernels, native


def _call(max_extend_len=4, Hq=8, Hkv=2, D=128, splits=1):
    row = (Hq + 2 * Hkv) * D
    return native.lib().sgl_amd_verify_attention(None, None, None, None, None, 64, None, None, None, None, 2, 2 * max_extend_len,
                                                 max_extend_len, Hq, Hkv, D, row, Hq * D, Hkv * D, Hkv * D, 0.1, None, None, splits,
                                                 None, None, None)


def test_row_cap():
    assert kernels.verify_attention_max_rows() == 64


@pytest.mark.parametrize("kw,word", [(dict(max_extend_len=17), "exceeds 64 rows"), (dict(D=96), "head_dim=96"), (dict(splits=2), "ws_acc"),
                                     (dict(splits=0), "num_splits"), (dict(Hq=7), "multiple")])
def test_bad_arguments_are_rejected_without_a_device(kw, word):
    assert _call(**kw) == -1
    assert word in native.last_error()


def test_split_policy_keeps_a_tile_per_split_and_the_cap():
    for batch in (1, 3, 16, 64, 300):
        for hkv in (1, 8):
            for max_len in (1, 63, 64, 65, 127, 128, 1000, 4096, 131072):
                s = kernels.choose_verify_splits(batch, hkv, max_len)
                assert 1 <= s <= kernels.VERIFY_MAX_SPLITS
                assert max_len < 64 or s * 64 <= max_len, (batch, hkv, max_len, s)
    assert kernels.choose_verify_splits(1, 1, 131072) == kernels.VERIFY_MAX_SPLITS
    assert kernels.verify_attention_supported(8, 4, 128, {}) and not kernels.verify_attention_supported(8, 4, 128, dict(kv_fp8=True))
    assert not kernels.verify_attention_supported(8, 4, 128, dict(sliding_window=64)) and not kernels.verify_attention_supported(17, 4, 128)
