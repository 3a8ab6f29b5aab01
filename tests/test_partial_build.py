"""What the compiler made of the partial-label coverage kernels (csrc/augment.hip), from its resource remarks: the instance
for up to 16 channels carries 32 accumulators and must keep them in registers.  Needs hipcc, no GPU."""
import re

from tests.helpers import _resources


def _cover_instances():
    """{(NC, partial): resources} of the aug_targets_cover<NC, PARTIAL> instances"""
    out = {}
    for name, r in _resources("augment").items():
        m = re.search(r"aug_targets_coverILi(\d+)ELb([01])EE", name)
        if m:
            out[(int(m.group(1)), m.group(2) == "1")] = r
    return out


def test_partial_coverage_instances_stay_in_registers():
    res = _cover_instances()
    print(res)
    assert sorted(res) == [(16, False), (16, True), (32, True), (64, False)], sorted(res)
    narrow = res[(16, True)]
    assert narrow["scratch"] == 0 and narrow["spill"] == 0, narrow
    # the wide instance walks the footprint once per 32 channels so that it, too, needs no scratch
    wide = res[(32, True)]
    assert wide["scratch"] == 0 and wide["spill"] == 0, wide
    # the fully labelled instances did not pay for the second set
    assert res[(16, False)]["scratch"] == 0 and res[(64, False)]["scratch"] == 0
    assert res[(16, False)]["vgprs"] < narrow["vgprs"]
