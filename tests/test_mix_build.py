"""The kernels of csrc/mix.hip keep everything in registers: no scratch, no spilled registers (needs hipcc, no GPU)."""
import os

import pytest

from tests.helpers import HIPCC, _resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_no_kernel_of_the_unit_uses_scratch_or_spills():
    res = _resources("mix")
    kernels = {n: r for n, r in res.items() if "mix_" in n}
    assert len(kernels) == 3 and {k for n in kernels for k in ("counts", "masks", "gather") if f"mix_{k}_kernel" in n} == \
        {"counts", "masks", "gather"}, sorted(res)
    for name, r in res.items():
        print(name, r)
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
