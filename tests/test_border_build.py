"""What the compiler made of the border weight kernels (csrc/border_weight.hip) and of the per-pixel-weight instances of the loss
kernels (csrc/loss.hip), from its resource remarks.  Needs hipcc, no GPU."""
import re

from tests.helpers import _resources


def test_border_weight_kernels_stay_in_registers():
    res = {n: r for n, r in _resources("border_weight").items() if "bw_" in n}
    print(res)
    assert sorted(re.search(r"bw_\w+?_kernel", n).group(0) for n in res) == ["bw_labels_kernel", "bw_search_kernel"], sorted(res)
    for name, r in res.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)


def _loss_instances():
    """{(kernel, CT, focal, ohem, pw): resources} of loss_partials_kernel / loss_bwd_kernel <CT, FOCAL, OHEM, PW>"""
    out = {}
    for name, r in _resources("loss").items():
        m = re.search(r"(loss_partials_kernel|loss_bwd_kernel)ILi(\d+)ELb([01])ELb([01])ELb([01])EE", name)
        if m:
            out[(m.group(1), int(m.group(2)), m.group(3) == "1", m.group(4) == "1", m.group(5) == "1")] = r
    return out


def test_pw_instances_need_no_more_scratch_than_their_twins():
    res = _loss_instances()
    print(res)
    pw = sorted(k for k in res if k[4])
    # every CT, focal and not, of both kernels -- and none with OHEM
    assert pw == sorted((kern, ct, focal, False, True) for kern in ("loss_partials_kernel", "loss_bwd_kernel") for ct in (4, 8, 16)
                        for focal in (False, True)), pw
    for kern, ct, focal, _, _ in pw:
        twin, mine = res[(kern, ct, focal, False, False)], res[(kern, ct, focal, False, True)]
        assert mine["scratch"] <= twin["scratch"], (kern, ct, focal, mine, twin)
