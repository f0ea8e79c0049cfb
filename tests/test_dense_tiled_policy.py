"""Host policy of the dense MFMA tile GEMM (kernels.dense_tiled_supported / choose_dense_tiled_config): no GPU needed."""
import pytest

from sglang_amd import kernels

# (N, K): Llama-3-8B qkv / o / gate_up / down / lm_head, then the 70B rank-of-8 projections
SHAPES = [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336), (128256, 4096),
          (1280, 8192), (8192, 1024), (7168, 8192), (8192, 3584)]


def test_dense_tiled_supported_is_the_shape_contract():
    assert [kernels.dense_tiled_supported(M, 4096, 4096) for M in (128, 129, 512, 513)] == [False, True, True, False]
    assert not kernels.dense_tiled_supported(256, 4096 + 8, 4096)
    assert not kernels.dense_tiled_supported(256, 4096, 4096 + 64)
    assert not kernels.dense_tiled_supported(256, 4096, 0)


@pytest.mark.parametrize("M", [129, 256, 257, 512])
@pytest.mark.parametrize("N,K", SHAPES)
def test_choose_dense_tiled_config_bounds(M, N, K):
    bn, s = kernels.choose_dense_tiled_config(M, N, K, False)
    assert bn in (64, 128) and 1 <= s <= K // 128
    assert s == 1 or s * M * N * 4 <= N * K * 2
    assert kernels.choose_dense_tiled_config(M, N, K, True)[1] == 1
