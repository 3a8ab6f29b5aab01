"""What the compiler made of the consensus kernels (csrc/consensus.hip), from its resource remarks: one instance per member
count, none with scratch or spilled vector registers, none above 256 vector registers.  Needs hipcc, no GPU."""
import re

from tests.helpers import _resources


def test_consensus_kernels_stay_in_registers():
    res = {n: r for n, r in _resources("consensus").items() if "consensus_labels_kernel" in n}
    print(res)
    members = sorted(int(re.search(r"consensus_labels_kernelILi(\d+)E", n).group(1)) for n in res)
    assert members == [1, 2, 3, 4, 5, 6, 7, 8], sorted(res)
    for name, r in res.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        assert r["vgprs"] <= 256, (name, r)                     # 256 lanes per block: at least two waves per SIMD
