"""The tree distillation reference (tests/distill_ref.py) pinned without the kernels: the chain rule of KL over a tree with leaves
at different depths, the reference gradient against autograd, a bound that admits the same formulas in fp32 and refuses three
mistakes, and gated cases that a keep-all or drop-all kernel cannot pass.  No GPU."""
import numpy as np
import pytest
import torch

from tests import distill_ref as R


def _tree_levels(rng, B, hw):
    """three levels, leaves at depths 0, 1 and 2: level 0 = {a, b, c} (softmax root; c is a leaf), level 1 = a -> {a0, a1},
    b -> {b0, b1, b2} (a1, b0, b2 leaves), level 2 = a0 -> {x, y}, b1 -> {s, t, v}"""
    shapes = [(3, [0], [3]), (5, [0, 1], [2, 3]), (5, [0, 3], [2, 3])]
    return [(torch.from_numpy(1.3 * rng.randn(B, C, hw)), gp, gs) for C, gp, gs in shapes]


@pytest.mark.parametrize("T", [1.0, 2.0, 0.5])
def test_level_terms_add_up_to_the_leaf_kl(T):
    rng = np.random.RandomState(5)
    B, hw = 2, 37
    teacher, student = _tree_levels(rng, B, hw), _tree_levels(rng, B, hw)
    beta = 1.0 / T
    want, tprobs = R.leaf_kl(teacher, student, beta)
    assert len(R.leaf_distributions(teacher, beta)[0][0]) == 1 + 3 + 5
    total = 0.0
    for L, ((u, gp, gs), (z, _, _)) in enumerate(zip(teacher, student)):
        r = R.tree_kl_ref(z, u, None if L == 0 else tprobs[L - 1], None, gp, gs, beta, 0.0)
        total = total + r["out"][:, 0].sum()
    assert abs(float(total) - float(want)) <= 1e-12 * abs(float(want)), (float(total), float(want))
    assert float(want) > 1.0          # (not a comparison of two zeros)


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_gradient_is_autograd_of_the_reference_value(name):
    c = R.make_case(name)
    z = c["z"].double().requires_grad_(True)
    r = R.tree_kl_ref(z, c["u"], c["wprev"], c["pw"], c["gp"], c["gs"], c["beta"], c["thresh"], c["g"], c["scale"])
    (r["value"].sum() * (c["g"] * c["scale"])).backward()
    # autograd differentiates the value w.r.t. z = logits; d/dz of kl(beta z) carries the factor beta
    dz = r["dz"].detach()
    err = (z.grad - dz).abs().max()
    assert float(err) <= 1e-12 * max(1.0, float(dz.abs().max())), float(err)
    assert float(dz.abs().max()) > 0 or sum(c["gs"]) == len(c["gs"])


def _fp32(name, variant=None, dtype=torch.float32):
    c = R.make_case(name)
    r = R.tree_kl_ref(c["z"], c["u"], c["wprev"], c["pw"], c["gp"], c["gs"], c["beta"], c["thresh"], c["g"], c["scale"], dtype=dtype,
                      variant=variant)
    return r["out"], r["dz"], c["dz0"] + r["dz"].float()


@pytest.mark.parametrize("name", list(R.CASES))
def test_the_same_formulas_in_fp32_stay_inside_the_bound(name):
    out, dz, acc = _fp32(name)
    assert R.check_against(name, out, dz, acc) == []
    _, r = R.reference(name)
    assert bool(torch.isfinite(r["out"]).all()) and bool(torch.isfinite(r["value_bound"]).all())
    # not vacuous: the bound is small against the value wherever the value is not tiny itself
    big = r["out"][:, 0].abs() > 1e-3
    assert bool((r["value_bound"][big] <= 1e-3 * r["out"][:, 0].abs()[big]).all())


@pytest.mark.parametrize("variant", ["swapped", "no_beta_in_grad", "gate_at_T"])
def test_each_wrong_variant_leaves_the_bound_on_some_case(variant):
    caught = [name for name in R.CASES if R.check_against(name, *_fp32(name, variant, torch.float64)[:2])]
    assert caught, variant
    if variant == "no_beta_in_grad":
        assert all(R.CASES[n][6] != 1.0 for n in caught)
    if variant == "gate_at_T":
        assert all(R.CASES[n][6] != 1.0 and R.CASES[n][7] > 0 for n in caught)


@pytest.mark.parametrize("name", R.GATED)
def test_gated_cases_keep_between_a_fifth_and_four_fifths(name):
    c, r = R.reference(name)
    frac = float(r["keep"].double().mean())
    assert 0.2 <= frac <= 0.8, frac
    # and no conf sits on the threshold: the fp32 comparison of the kernel cannot depend on an ulp
    for gi, sl in enumerate(R.group_slices(c["gs"])):
        omega = torch.ones(c["B"], c["hw"], dtype=torch.float64) if c["wprev"] is None else c["wprev"].double()[:, c["gp"][gi]]
        assert float((R.gate_conf(c["u"].double()[:, sl], omega) - c["thresh"]).abs().min()) >= R.GATE_MARGIN


def test_the_case_list_covers_what_it_must():
    Cs = {sum(v[2]) for v in R.CASES.values()}
    assert {1, 3, 4, 5, 8, 9, 16} <= Cs
    tables = [v[2] for v in R.CASES.values()]
    assert [1, 2, 3] in tables and [16] in tables and [1] * 16 in tables and [2, 1, 5] in tables
    assert any(v[2] == [2, 1, 5] and v[3] == [2, 0, 2] for v in R.CASES.values())      # repeated and out-of-order parents
    assert {v[1][0] * v[1][1] for v in R.CASES.values()} == {1, 259, 1023, 4100}
    assert {v[0] for v in R.CASES.values()} == {1, 3}
    assert {v[6] for v in R.CASES.values()} == {0.5, 1.0, 2.0} and {v[7] for v in R.CASES.values()} == {0.0, 0.6}
    assert {v[8] for v in R.CASES.values()} == {0, 1} and {v[5] for v in R.CASES.values()} == {"none", "rand", "zeros"}
    assert {v[9] for v in R.CASES.values()} == {None, "teacher", "student", "both"}
