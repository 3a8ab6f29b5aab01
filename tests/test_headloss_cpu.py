"""tests/headloss_ref.py pinned on the CPU, so that tests/test_headloss_gpu.py cannot be wrong together with its reference:

  * the references reproduce the values the reference project itself produced (tests/golden) and the oracle's restatements;
  * at the exact inputs of the GPU test, the float32 torch-CPU evaluation of every reference stays within a QUARTER of the bar
    the GPU test applies to that quantity -- the inputs leave fp32 arithmetic room, the bars are not met by luck.  Where an
    input missed this, the input was changed, never the bar (noted at the case);
  * the share of near-tie pixels the consistency backward comparison has to leave out stays under its cap.

Run with -s to see the measured fp32 distances per group."""
import pytest
import torch

from oracle import losses as OL
from tests import headloss_ref as R
from tests.helpers import CASES, load_golden, load_tree

HEADROOM = 0.25
# Two quantities cannot keep a quarter of their bar in ANY fp32 evaluation, torch's own included, whatever the input; their
# GPU bars stay as they are, the room they really have is asserted here instead:
#  * AdamW's p with weight decay: p is rounded twice per step (p *= 1 - lr*wd, p -= update), ten half-ulp roundings of p
#    itself in five steps; error and normaliser (max |p|) scale together, and over 8.4 M elements the worst random walk
#    reaches 2.5e-7 to 2.9e-7 for normal, uniform, clipped and rescaled p alike.  Without weight decay (five roundings) and
#    for m and v the quarter holds.
#  * the logits-resize backward at 155 output pixels: the source coordinate scale * index is an fp32 number up to 38 (half
#    an ulp = 2e-6), which moves that much weight between neighbouring input pixels: 2.5e-6 to 3e-6 of max |din|.
HEADROOM_EXCEPTIONS = {("adamw", "p"): 1.0 / 3.0, ("logits_up", "din"): 1.0 / 3.0}


def _groups(tree_file):
    from hrseg_amd.utils.hierarchy import build_hierarchy_indices, child_groups
    levels, parent_of, children_of = build_hierarchy_indices(load_tree(tree_file))
    trees = [([levels[L].index(p) for p, _ in groups], [len(ch) for _, ch in groups])
             for L, groups in enumerate(child_groups(levels, children_of))]
    return levels, parent_of, trees


# ------------------------------------------------------------------------------------------------ the references are right
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c[1]])
def test_compose_and_consistency_reproduce_the_model_goldens(name):
    g = load_golden(name)
    levels, parent_of, trees = _groups(CASES[name][2])
    probs = [R.sigmoid(torch.from_numpy(g["logits0"]).double())]
    for L, tree in enumerate(trees, start=1):
        probs.append(R.compose(torch.from_numpy(g[f"logits{L}"]).double(), probs[-1], *tree))
    for L, p in enumerate(probs):
        assert R.rel(p, torch.from_numpy(g[f"probs{L}"])) < 2e-6, L
    gold = [torch.from_numpy(g[f"probs{L}"]).double() for L in range(len(levels))]
    total, count = 0.0, 0
    for L, tree in enumerate(trees, start=1):
        n = gold[L].shape[0] * gold[L].shape[2] * gold[L].shape[3]
        total += float(R.consistency_sums(gold[L], gold[L - 1], *tree).sum()) / n
        count += len(tree[0])
    assert abs(total / count - float(g["cons_probs"])) < 1e-6
    assert abs(total / count - float(OL.hierarchical_consistency_loss(gold, levels, parent_of))) < 1e-12


def test_ce_dice_reproduces_the_loss_golden():
    g = load_golden("loss_cases")
    w = [float(v) for v in g["w"]]
    z = torch.from_numpy(g["z"]).double().requires_grad_(True)
    ce, dice, nvalid = R.ce_dice(z, torch.from_numpy(g["t"]).double(), w)
    assert abs(float(ce) - float(g["ce"])) < 1e-6 and abs(float(dice) - float(g["dice"])) < 1e-6 and nvalid == 2
    (ce + dice).backward()
    assert R.rel(z.grad, torch.from_numpy(g["dz"])) < 1e-5
    ce2, dice2, nvalid2 = R.ce_dice(torch.from_numpy(g["z_all"]).double(), torch.from_numpy(g["t_all"]).double(), w)
    assert abs(float(ce2) - float(g["ce_all"])) < 1e-6 and dice2 is None and nvalid2 == 0


def test_consistency_sums_equal_the_oracle_on_every_tree():
    """single-level trees in the oracle's terms: parents may come in any order there (it looks children up by name)"""
    for tree in R.TREES:
        parents, sizes = tree
        x = R.cons_inputs(tree, (5, 7))
        prev_names = [f"p{i}" for i in range(x["prev"].shape[1])]
        cur_names, parent_of = [], {}
        for gi, (par, n) in enumerate(zip(parents, sizes)):
            for j in range(n):
                cur_names.append(f"c{gi}_{j}")
                parent_of[cur_names[-1]] = prev_names[par]
        want = OL.hierarchical_consistency_loss([x["prev"].double(), x["cur"].double()], [prev_names, cur_names], parent_of, "sum")
        got = R.consistency_sums(x["cur"].double(), x["prev"].double(), *tree).sum() / len(parents)
        assert abs(float(got) - float(want)) < 1e-10 * max(1.0, abs(float(want)))


def test_adamw_step_is_torch_adamw():
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(257, generator=g, dtype=torch.float64)
    grads = [torch.randn(257, generator=g, dtype=torch.float64) for _ in range(5)]
    lrs = [1e-3, 1e-3, 5e-4, 5e-4, 2e-3]
    for wd in (0.0, 0.01):
        pr = torch.nn.Parameter(p0.clone())
        opt = torch.optim.AdamW([pr], lr=lrs[0], betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        for k in range(5):
            opt.param_groups[0]["lr"] = lrs[k]
            pr.grad = 0.25 * grads[k]
            opt.step()
            R.adamw_step(p, grads[k], m, v, k + 1, lrs[k], 0.9, 0.999, 1e-8, wd, gscale=0.25)
            st = opt.state[pr]
            assert R.rel(p, pr.data) < 1e-14 and R.rel(m, st["exp_avg"]) < 1e-14 and R.rel(v, st["exp_avg_sq"]) < 1e-14


# ------------------------------------------------------------------------------------------------ fp32 headroom of the bars
def _headroom(group, cases, run, bars, absolute=()):
    worst = {}
    for case in cases:
        ref, f32 = run(*case, torch.float64), run(*case, torch.float32)
        for name, bar in bars.items():
            if name not in ref:
                continue
            d = R.absdiff(f32[name], ref[name]) if name in absolute else R.rel(f32[name], ref[name])
            assert d <= HEADROOM_EXCEPTIONS.get((group.split()[0], name), HEADROOM) * bar, (group, [c for c in case if not isinstance(c, dict)], name, d, bar)
            worst[name] = max(worst.get(name, 0.0), d)
    print(f"\nfp32-CPU distance from fp64, {group}: " + ", ".join(f"{k} {v:.2e} (bar {bars[k]:.0e})" for k, v in worst.items()))


def test_headroom_head():
    _headroom("head", [(c,) for c in R.HEAD_CASES], R.head_run, R.HEAD_BARS)


def test_headroom_logits_up():
    _headroom("logits_up", [(s, a, C) for s in R.UP_SIZES for a in (True, False) for C in R.UP_C], R.up_run, R.UP_BARS)


def test_headroom_sigmoid_compose():
    _headroom("sigmoid", [(s,) for s in R.SIGMOID_SCALES], R.sigmoid_run, R.SIGMOID_BARS)
    _headroom("compose", [(t, s, hw) for t in R.TREES for s in R.COMPOSE_SCALES for hw in R.COMPOSE_HW], R.compose_run,
              R.COMPOSE_BARS)
    _headroom("compose chain", [(s, hw) for s in R.COMPOSE_SCALES for hw in R.COMPOSE_HW], R.chain_run, R.CHAIN_BARS)


@pytest.mark.parametrize("C", R.LOSS_C)
def test_headroom_loss(C):
    cases = [(C, hw, B, pat) for hw in R.LOSS_HW for B in R.LOSS_B for pat in R.LOSS_PATTERNS]
    _headroom(f"loss C={C}", cases, R.loss_run, R.LOSS_BARS, absolute=("ce", "dice"))
    for case in cases:
        assert R.loss_run(*case, torch.float32)["nvalid"] == R.loss_run(*case, torch.float64)["nvalid"]


def test_headroom_consistency_and_tie_share():
    for maker in (R.cons_inputs, R.cons_onehot_inputs):
        cases = [(maker(t, hw), t) for t in R.TREES for hw in R.CONS_HW]
        _headroom("consistency " + maker.__name__, cases, R.cons_run, R.CONS_BARS, absolute=("mean",))
    worst = 0.0
    for tree in R.TREES:
        for hw in R.CONS_HW:
            r = R.cons_run(R.cons_inputs(tree, hw), tree, torch.float64)
            share = float(r["tie"].any(dim=1).float().mean())             # pixels with a near tie in any group
            assert share <= R.CONS_MAX_TIE_SHARE, (tree, hw, share)
            assert float((r["diffs"] > 0).float().mean()) > 0.1 and float((r["diffs"] < 0).float().mean()) > 0.1   # both signs
            worst = max(worst, share)
            # away from the ties the fp32 evaluation has the sign of the fp64 one: the exact comparison is legitimate
            r32 = R.cons_run(R.cons_inputs(tree, hw), tree, torch.float32)
            keep = ~r["tie"]
            assert torch.equal(torch.sign(r32["diffs"])[keep].double(), torch.sign(r["diffs"])[keep])
            # the one-hot inputs are exact in any float format: ties are exact zeros, everything else is +-1
            d = R.cons_run(R.cons_onehot_inputs(tree, hw), tree, torch.float64)["diffs"]
            assert set(d.unique().tolist()) <= {-1.0, 0.0, 1.0} and float((d == 0).float().mean()) > 0.3
    print(f"\nconsistency: worst near-tie pixel share {worst:.2e} (cap {R.CONS_MAX_TIE_SHARE:.0e})")
    assert R.e2e_ties() == 0            # the end-to-end inputs have no near tie at all: every gradient entry is compared
    for reduction in ("mean", "sum"):
        a, b = R.e2e_run(reduction, torch.float64), R.e2e_run(reduction, torch.float32)
        assert abs(float(a["loss"]) - float(b["loss"])) <= HEADROOM * R.BAR_LOSS * max(1.0, abs(float(a["loss"])))
        for ga, gb in zip(a["grads"], b["grads"]):
            assert R.rel(gb, ga) <= HEADROOM * R.BAR_POINT


@pytest.mark.parametrize("n", R.ADAMW_N)
def test_headroom_adamw(n):
    x = R.adamw_inputs(n)
    _headroom(f"adamw n={n}", [(x, wd) for wd in R.ADAMW_WDS], R.adamw_run, R.ADAMW_BARS)


def test_headroom_gap_film():
    _headroom("gap", [(hw,) for hw in R.GAP_HW], R.gap_run, R.GAP_BARS)
    _headroom("film_linear", [(c,) for c in R.FILM_CASES], R.film_run, R.FILM_BARS)
