"""Build-time guard for wstream_fp8_gemm.hip: the main kernels keep the accumulators (and, with block scales, the chunk
accumulators), a slot's raw weight pieces, two stages of activation fragments and the widened weights in registers; a spill would
sit between the matrix instructions of the stream.  Cross-compiles for gfx950; no GPU needed."""
from pathlib import Path

import pytest
from test_no_spills import HIPCC, _resource_usage


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_wstream_fp8_main_kernels_do_not_spill(tmp_path):
    usage = _resource_usage("wstream_fp8_gemm.hip", tmp_path)
    main = {k: v for k, v in usage.items() if "wstream_fp8_gemm_kernel" in k}
    assert len(main) == 96, sorted(usage)       # row tiles {1, 2, 3, 4, 6, 8} x (waves 4..8 | 2..4 two-tile) x {channel, block} scales
    for name, u in main.items():
        assert u["vgpr_spill_count"] == 0 and u["sgpr_spill_count"] == 0, (name, u)
        assert u["vgpr_count"] <= 256, (name, u)                    # eight waves per workgroup: two per SIMD
        assert u["group_segment_fixed_size"] <= 160 * 1024, (name, u)
