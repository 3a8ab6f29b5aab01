"""Compile-time audit of the hot kernels (no GPU): the wave-specialised 3x3 kernels and the nine-tap weight gradient of the default
arithmetic must not spill.  Round 4 found the forward wave-specialised kernels reloading 5-12 spilled registers behind
`s_waitcnt vmcnt(0)` in EVERY tile's epilogue -- invisible in every functional test, worth ~10 % of the kernel -- so the
resource remarks of the compiler are asserted here (about a minute of hipcc)."""
import os
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests.helpers import HIPCC, _resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_hot_kernels_do_not_spill():
    with ThreadPoolExecutor(2) as ex:
        ws, wg = ex.map(_resources, ["conv_ws", "conv_wgrad_sp"])
    hot = {n: r for n, r in ws.items() if "igemm_patch_ws" in n and ("ILi4E" in n or "ILi1E" in n)}      # fp16x2 and bf16 instances
    hot.update({n: r for n, r in wg.items() if "wgrad9_sp_group_kernel" in n and ("ILi4E" in n or "ILi1E" in n)})
    assert len(hot) >= 24, sorted(hot)
    bad = {n: r for n, r in hot.items() if r.get("scratch", 1) or r.get("spill", 1)}
    assert not bad, bad
    # the persistent 512-thread kernels run two waves per SIMD: 256 registers is the limit, not a target
    assert all(r["vgprs"] <= 256 for r in hot.values())
