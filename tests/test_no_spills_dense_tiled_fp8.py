"""Build-time guard for dense_tiled_fp8_gemm.hip: the kernels keep the accumulators (and, with block scales, the chunk
accumulators), the raw and widened weight fragments and two k-steps of activation fragments in registers at two waves per SIMD;
a spill would sit between the matrix instructions (and its reload would wait for every LDS-DMA in flight).  Cross-compiles for
gfx950; no GPU needed."""
from pathlib import Path

import pytest
from test_no_spills import HIPCC, _resource_usage

LDS = {"ILi256ELb0E": 3 * 48 * 1024, "ILi128ELb0E": 4 * 40 * 1024, "ILi128ELb1E": 4 * 40 * 1024}      # stages x (W + X tile)


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_dense_tiled_fp8_kernels_do_not_spill(tmp_path):
    usage = _resource_usage("dense_tiled_fp8_gemm.hip", tmp_path)
    main = {k: v for k, v in usage.items() if "dense_tiled_fp8_gemm_kernel" in k}
    assert len(main) == 3, sorted(usage)          # wide, narrow, narrow with block scales
    for name, u in main.items():
        assert u["vgpr_spill_count"] == 0 and u["sgpr_spill_count"] == 0, (name, u)
        assert u["vgpr_count"] <= 256, (name, u)                    # eight waves per workgroup: two per SIMD
        assert u["group_segment_fixed_size"] == next(v for k, v in LDS.items() if k in name), (name, u)
