"""Build-time guard for speculative_sampling.hip: the range kernels hold a burst of 32 columns per thread in registers; a spill
would sit inside the one pass over the logits.  Cross-compiles for gfx950; no GPU needed."""
from pathlib import Path

import pytest
from test_no_spills import HIPCC, _resource_usage


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_tree_accept_and_tree_table_kernels_do_not_spill(tmp_path):
    usage = _resource_usage("speculative_sampling.hip", tmp_path)
    assert len(usage) == 9, sorted(usage)                       # ranges / walk / final / pick x {bf16, fp32} + the tree tables
    for name, u in usage.items():
        assert u["vgpr_spill_count"] == 0 and u["sgpr_spill_count"] == 0 and u["vgpr_count"] <= 128, (name, u)
