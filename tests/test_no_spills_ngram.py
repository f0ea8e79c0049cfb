"""Build-time guard for ngram_draft.hip: the scan kernel keeps the suffix, a tile's scores and its share of the hit list in registers;
a spill would sit inside the per-tile loop.  Cross-compiles for gfx950; no GPU needed."""
from pathlib import Path

import pytest
from test_no_spills import HIPCC, _resource_usage


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_ngram_draft_kernels_do_not_spill(tmp_path):
    usage = _resource_usage("ngram_draft.hip", tmp_path)
    assert len(usage) == 3, sorted(usage)                       # scan / tree / commit
    for name, u in usage.items():
        assert u["vgpr_spill_count"] == 0 and u["sgpr_spill_count"] == 0 and u["vgpr_count"] <= 64, (name, u)
