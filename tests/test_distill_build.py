"""What the compiler made of the tree distillation kernels (csrc/distill.hip), from its resource remarks: the CT ladder 4 / 8 / 16
with the gate compiled in and out gives six instances of each kernel, and the segmented scans keep every one of them in
registers.  Needs hipcc, no GPU."""
import re

from tests.helpers import _resources


def test_all_twelve_instances_exist_and_stay_in_registers():
    res = {}
    for name, r in _resources("distill").items():
        m = re.search(r"(tree_kl_kernel|tree_kl_bwd_kernel)ILi(\d+)ELb([01])EE", name)
        if m:
            res[(m.group(1), int(m.group(2)), m.group(3) == "1")] = r
    print(res)
    want = sorted((k, ct, gate) for k in ("tree_kl_kernel", "tree_kl_bwd_kernel") for ct in (4, 8, 16) for gate in (False, True))
    assert sorted(res) == want, sorted(res)
    for key, r in res.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (key, r)
