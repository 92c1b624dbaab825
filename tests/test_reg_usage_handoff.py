"""Register budget of the team kernel's hand-off form (k_sqp_rti_team_ho, csrc/sqp_rti_team_ho.hip; tools/reg_usage.py,
the compiler's resource remarks for the product flags). It holds the team tick and the one-wave segmented tick in one
kernel and runs one wave per SIMD (__launch_bounds__(256, 1)), so each instantiation has the SIMD's 512 arch +
accumulation VGPRs per lane, and none may spill to scratch: a spill in either tick's stage loop would cost more than
the hand-off gains."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.skipif(not shutil.which("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_handoff_kernels_fit_one_wave_per_simd_without_scratch():
    import reg_usage
    use = {k: v for k, v in reg_usage.usage("sqp_rti_team_ho.hip").items() if "k_sqp_rti_team_ho" in k}
    assert len(use) == 4, sorted(use)  # diff and tric, solve and run mode
    assert sum("Diff2" in k for k in use) == 2 and sum("Tric3" in k for k in use) == 2, sorted(use)
    for k, (v, a, s) in use.items():
        assert v + a <= 512 and s == 0, (k, v, a, s)
