"""Mixing augmentation on the host (Data/mix.py, the refusals of csrc/mix.hip) and the torch-CPU restatement tests/mix_ref.py:
the k_of_n table, candidate sets by level, the draws, the packed table, properties of the restatement on the inputs the GPU
tests use, and that those inputs are not trivial (no GPU)."""
import ctypes

import pytest
import torch

from tests import mix_ref as MR


# ------------------------------------------------------------------------------------------------ k_of_n
def test_k_of_n_against_hand_written_values():
    from hrseg_amd.Data.mix import k_of_n_table
    want = {0.5: {0: 0, 1: 1, 2: 1, 3: 2, 64: 32}, 1.0: {0: 0, 1: 1, 2: 2, 3: 3, 64: 64}, 0.01: {0: 0, 1: 1, 2: 1, 3: 1, 64: 1}}
    for share, rows in want.items():
        t = k_of_n_table(share)
        assert len(t) == 65 and all(type(v) is int for v in t)
        for n, k in rows.items():
            assert t[n] == k, (share, n, t[n])
        assert t == MR.k_of_n(share)
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="share"):
            k_of_n_table(bad)


# ------------------------------------------------------------------------------------------------ candidates
def _cands(key, model_type, **kw):
    from hrseg_amd.Data.dataset import build_target_luts
    from hrseg_amd.Data.mix import candidates
    tree, cmap = MR.tree_of(key)
    names, parent, _, _ = build_target_luts(tree, cmap, model_type)
    flags = candidates(names, parent, model_type, **kw)
    assert len(flags) == len(names) and set(flags) <= {0, 1}
    got = [n for n, f in zip(names, flags) if f]
    ref_names = MR.PR.emitted(tree, model_type)[0]
    assert got == [ref_names[c] for c in sorted(MR.candidates(tree, model_type, kw.get("level", 0), kw.get("nodes")))]
    return got


def test_candidate_sets_by_level():
    assert _cands("tl", 1, level=0) == ["background", "upper", "lower", "tooth"]
    assert _cands("tl", 1, level=1) == ["pulp", "dentin", "enamel", "composite"]
    assert _cands("ext", 1, level=2) == ["upper", "lower", "composite", "healthy"]
    assert _cands("ext", 1, level=3) == ["pulp", "dentin", "enamel"]
    assert _cands("tl", 0, level=0) == ["background", "upper", "lower", "pulp", "dentin", "enamel", "composite"]
    assert _cands("tl", 1, nodes=["tooth"]) == ["tooth"]
    assert _cands("ext", 1, nodes=["enamel", "alveolar"]) == ["alveolar", "enamel"]
    assert len(_cands("wide", 1, level=0)) == 8 and len(_cands("wide", 1, level=1)) == 56


def test_candidate_refusals_name_what_is_wrong():
    with pytest.raises(ValueError, match="molar"):
        _cands("tl", 1, nodes=["tooth", "molar"])
    with pytest.raises(ValueError, match="level 2"):
        _cands("tl", 1, level=2)
    with pytest.raises(ValueError, match="level -1"):
        _cands("tl", 1, level=-1)
    with pytest.raises(ValueError, match="level 1"):
        _cands("tl", 0, level=1)
    with pytest.raises(ValueError, match="tooth"):
        _cands("tl", 0, nodes=["tooth"])                # no channel of a flat model


# ------------------------------------------------------------------------------------------------ sample
def _sample(seed, B=6, C=8, **kw):
    from hrseg_amd.Data.mix import sample_params
    return sample_params(B, C, torch.Generator().manual_seed(seed), **kw)


def test_the_same_seed_gives_the_same_draws():
    a, b, c = _sample(3, max_shift=9), _sample(3, max_shift=9), _sample(4, max_shift=9)
    assert a.keys() == b.keys() == {"apply", "donor", "prio", "dx", "dy", "boxed", "box"}
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert any(not torch.equal(a[k], c[k]) for k in a)
    assert a["prio"].shape == (6, 8) and all(sorted(r.tolist()) == list(range(8)) for r in a["prio"])
    assert int(a["dx"].abs().max()) <= 9 and int(a["dy"].abs().max()) <= 9 and bool((a["dx"] != 0).any())
    assert bool(a["apply"].all()) and not bool(a["boxed"].any())
    z = _sample(3)
    assert not bool(z["dx"].any()) and not bool(z["dy"].any())


def test_a_donor_never_equals_the_sample_and_the_lists_are_honoured():
    for seed in range(20):
        p = _sample(seed)
        assert all(int(d) != i for i, d in enumerate(p["donor"]))
        q = _sample(seed, donors=[0, 1], recipients=[1, 4, 5])
        for i in range(6):
            assert bool(q["apply"][i]) == (i in (1, 4, 5))
            if bool(q["apply"][i]):
                assert int(q["donor"][i]) in (0, 1) and int(q["donor"][i]) != i
    assert {int(_sample(s, donors=[0, 1], recipients=[4])["donor"][4]) for s in range(20)} == {0, 1}
    assert 0 < sum(int(_sample(s, p=0.5)["apply"].sum()) for s in range(20)) < 120
    assert not bool(_sample(0, p=0.0)["apply"].any())


def test_an_empty_donor_set_switches_the_sample_off():
    p = _sample(5, donors=[2])
    assert [bool(v) for v in p["apply"]] == [True, True, False, True, True, True]
    assert [int(v) for v in p["donor"]] == [2, 2, 2, 2, 2, 2]
    assert not bool(_sample(5, B=1)["apply"][0]), "a batch of one has nobody to take from"
    assert not bool(_sample(5, donors=[])["apply"].any())
    with pytest.raises(ValueError, match="donors"):
        _sample(5, donors=[6])
    with pytest.raises(ValueError, match="recipients"):
        _sample(5, recipients=[-1])


def test_cutmix_boxes_follow_rand_bbox():
    from hrseg_amd.Data.mix import rand_bbox
    assert rand_bbox(62, 0.75, 31, 31) == (16, 16, 46, 46)           # cut = int(62 * 0.5) = 31, half 15
    assert rand_bbox(62, 0.75, 0, 61) == (46, 0, 62, 15)             # clipped to the frame
    assert rand_bbox(62, 1.0, 10, 10) == (10, 10, 10, 10)            # lam 1: nothing
    assert rand_bbox(62, 0.0, 31, 31) == (0, 0, 62, 62)
    p = _sample(7, mode="cutmix", S=62)
    assert bool(p["boxed"].all())
    for r0, c0, r1, c1 in p["box"].tolist():
        assert 0 <= r0 <= r1 <= 62 and 0 <= c0 <= c1 <= 62
    with pytest.raises(ValueError, match="image size"):
        _sample(7, mode="cutmix")
    with pytest.raises(ValueError, match="mode"):
        _sample(7, mode="mixup")


# ------------------------------------------------------------------------------------------------ pack_params
def test_pack_params_round_trip():
    from hrseg_amd.Data import mix as M
    p = MR.CASES["G"]["params"]
    table, prio = M.pack_params(p, 62, 8)
    assert table.dtype == prio.dtype == torch.int32 and table.shape == (4, 16) and prio.shape == (4, 8)
    assert table[:, M.P_FLAGS].tolist() == [M.APPLY | M.BOX] * 4 and table[:, M.P_DONOR].tolist() == [1, 2, 3, 0]
    assert table[:, M.P_DX].tolist() == [0, 0, 0, -5] and table[:, M.P_DY].tolist() == [0, 0, 0, 9]
    assert table[:, M.P_BOX:M.P_BOX + 4].tolist() == MR.G_BOXES and not bool(table[:, 8:].any())
    assert torch.equal(prio.long(), p["prio"])
    q = MR.CASES["A"]["params"]
    table, _ = M.pack_params(q, 62, 8)
    assert table[:, M.P_FLAGS].tolist() == [1, 1, 1, 0, 1] and table[:, M.P_DY].tolist() == [0, 0, 2, -61, 0]
    assert not bool(table[:, M.P_BOX:].any())
    big = dict(q, dx=torch.tensor([2**31 - 1, -2**31, 0, 0, 0]))
    assert M.pack_params(big, 62, 8)[0][:, M.P_DX].tolist() == [2**31 - 1, -2**31, 0, 0, 0]


def test_pack_params_refusals():
    from hrseg_amd.Data.mix import pack_params
    good = MR.CASES["G"]["params"]

    def refused(match, S=62, **over):
        with pytest.raises(ValueError, match=match):
            pack_params(dict(good, **over), S, 8)
    refused("donor 4", donor=torch.tensor([1, 2, 4, 0]))
    refused("donor -1", donor=torch.tensor([-1, 2, 3, 0]))
    bad = good["prio"].clone()
    bad[2, 0] = bad[2, 1]
    refused("sample 2: prio", prio=bad)
    refused("prio must be", prio=good["prio"][:, :7])
    refused("dx 2147483648", dx=torch.tensor([0, 2**31, 0, 0]))
    refused("box", S=61)
    refused("box", box=torch.tensor([[5, 0, 4, 62]] * 4))
    refused("box", box=torch.tensor([[0, -1, 4, 62]] * 4))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", sorted(MR.CASES))
def test_properties_of_the_reference(name):
    case = MR.resolved(name)
    x, y, p, ref = case["x"], case["y"], case["params"], case["ref"]
    B, C, S, _ = y.shape
    assert torch.equal(ref["counts"].long(), torch.stack([torch.stack([(y[b, c] == 1).sum() for c in range(C)]) for b in range(B)]))
    full, got = torch.cat([x, y], 1).view(torch.int32), torch.cat([ref["x2"], ref["y2"]], 1).view(torch.int32)
    for b in range(B):
        d, dx, dy = int(p["donor"][b]), int(p["dx"][b]), int(p["dy"][b])
        if not bool(p["apply"][b]):
            assert torch.equal(got[b], full[b]) and not bool(ref["mask"][b].any()) and ref["chosen"][b] == []
            continue
        # every output column is the donor's (moved) or the recipient's, by the mask; walked pixel by pixel
        for r in range(S):
            for c in range(S):
                if int(ref["mask"][b, r, c]):
                    assert 0 <= r - dy < S and 0 <= c - dx < S
                    assert torch.equal(got[b, :, r, c], full[d, :, r - dy, c - dx])
                else:
                    assert torch.equal(got[b, :, r, c], full[b, :, r, c])
        if not bool(p["boxed"][b]):
            present = [c for c in case["cand"] if int(ref["counts"][d, c]) >= case["min_pixels"]]
            assert len(ref["chosen"][b]) == case["k_of_n"][len(present)] and set(ref["chosen"][b]) <= set(present)


def test_the_named_inputs_are_not_trivial():
    A = MR.resolved("A")
    p, ref = A["params"], A["ref"]
    applied = [b for b in range(5) if bool(p["apply"][b])]
    assert applied == [0, 1, 2, 4]
    for b in applied:
        if abs(int(p["dx"][b])) < 62 and abs(int(p["dy"][b])) < 62:
            assert bool((ref["mask"][b] == 0).any()) and bool((ref["mask"][b] == 1).any()), b
    assert not bool(ref["mask"][4].any()) and ref["chosen"][4], "a shift by the whole frame pastes nothing, whatever is chosen"
    assert any(len(cs) >= 2 for cs in ref["chosen"])
    # the special values sit on both sides of the masks
    xi = A["x"].view(torch.int32)
    special = torch.zeros_like(xi, dtype=torch.bool)
    for v in MR.SPECIALS:
        special |= xi == v
    inside = special & (ref["mask"][:, None] == 1)
    assert bool(inside.any()) and bool((special & (ref["mask"][:, None] == 0)).any())
    assert int(torch.isnan(A["x"]).sum()) >= 10 and int(torch.isinf(A["x"]).sum()) >= 10
    # one applied sample has a donor without the candidate
    T = MR.resolved("A_tooth")
    empty = [b for b in applied if T["ref"]["chosen"][b] == []]
    assert empty == [1] and not bool(T["ref"]["mask"][1].any())
    assert all(T["ref"]["chosen"][b] == [3] for b in (0, 2, 4)) and bool(T["ref"]["mask"][0].any())
    # the row that comes in from below
    A3 = MR.resolved("A_all")["ref"]["mask"][3]
    assert bool(A3[0].any()) and not bool(A3[0].all()) and not bool(A3[1:].any())
    # selection over many channels
    assert max(len(cs) for cs in MR.resolved("C_kids_all")["ref"]["chosen"]) > 32
    assert 0 < max(len(cs) for cs in MR.resolved("C_all_40")["ref"]["chosen"]) < 8
    assert max(len(cs) for cs in MR.resolved("C_half")["ref"]["chosen"]) == 4
    # boxes: the whole frame is the donor, the empty box nothing, one pixel, and a box cut by the shift
    G = MR.resolved("G")
    gm = G["ref"]["mask"]
    assert bool(gm[0].all()) and torch.equal(G["ref"]["x2"][0].view(torch.int32), G["x"][1].view(torch.int32))
    assert not bool(gm[1].any()) and int(gm[2].sum()) == 1 and int(gm[2, 61, 61]) == 1
    assert int(gm[3].sum()) == (50 - 10) * (40 - 5) and 0 < int(gm[3].sum())
    # partial labels: an ignored pixel is never taken, an internal pixel comes with -1 below it
    H = MR.resolved("H")
    hy2, hm = H["ref"]["y2"], H["ref"]["mask"]
    took_internal = False
    for b in applied:
        d, dx, dy = int(p["donor"][b]), int(p["dx"][b]), int(p["dy"][b])
        lab = torch.from_numpy(H["labels"][d])
        for r, c in hm[b].nonzero().tolist():
            v = int(lab[r - dy, c - dx])
            assert v != 254
            if v == 9:
                took_internal = True
                assert hy2[b, :, r, c].tolist() == [0, 0, 0, 1, -1, -1, -1, -1]
    assert took_internal and bool((torch.from_numpy(H["labels"]) == 254).any())


# ------------------------------------------------------------------------------------------------ C refusals
def test_c_refusals_come_before_any_launch():
    """placeholder pointers, never dereferenced (cand is read on the host: real memory)"""
    from hrseg_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.hrseg_last_error_string.restype = ctypes.c_char_p
    for name in ("hrseg_mix_counts", "hrseg_mix_masks", "hrseg_mix_gather"):
        getattr(lib, name).argtypes = _lib.PROTOTYPES[name]
    P, Q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    cand = _lib.int_array([1] * 64)

    def refused(rc, name, text):
        msg = lib.hrseg_last_error_string().decode()
        assert rc == -1 and msg.startswith(f"{name}: ") and text in msg, (rc, msg)

    def counts(y=P, out=P, B=2, C=8, hw=100):
        return lib.hrseg_mix_counts(y, out, B, C, hw, None)

    def masks(y=P, counts=P, params=P, prio=P, kn=P, cand=cand, min_pixels=1, mask=P, chosen=P, B=2, C=8, S=10):
        return lib.hrseg_mix_masks(y, counts, params, prio, kn, cand, min_pixels, mask, chosen, B, C, S, None)

    def gather(src=P, mask=P, params=P, out=Q, B=2, K=3, S=10):
        return lib.hrseg_mix_gather(src, mask, params, out, B, K, S, None)

    for bad in (dict(y=None), dict(out=None)):
        refused(counts(**bad), "hrseg_mix_counts", "null pointer")
    refused(counts(B=0), "hrseg_mix_counts", "B=0")
    refused(counts(C=0), "hrseg_mix_counts", "C=0 not in 1..64")
    refused(counts(C=65), "hrseg_mix_counts", "C=65 not in 1..64")
    refused(counts(hw=0), "hrseg_mix_counts", "hw=0")
    refused(counts(hw=1 << 31), "hrseg_mix_counts", "hw=2147483648")

    for bad in ("y", "params", "prio", "kn", "mask", "chosen"):
        refused(masks(**{bad: None}), "hrseg_mix_masks", "null pointer")
    refused(masks(cand=None), "hrseg_mix_masks", "null pointer")
    refused(masks(B=0), "hrseg_mix_masks", "B=0")
    refused(masks(C=0), "hrseg_mix_masks", "C=0 not in 1..64")
    refused(masks(C=65), "hrseg_mix_masks", "C=65 not in 1..64")
    refused(masks(S=0), "hrseg_mix_masks", "S=0")
    refused(masks(min_pixels=0), "hrseg_mix_masks", "min_pixels=0")
    refused(masks(B=8, C=64, S=2048), "hrseg_mix_masks", "2^31 or more")
    refused(masks(B=1, C=1, S=46341), "hrseg_mix_masks", "2^31 or more")

    for bad in ("src", "mask", "params", "out"):
        refused(gather(**{bad: None}), "hrseg_mix_gather", "null pointer")
    refused(gather(B=0), "hrseg_mix_gather", "B=0")
    refused(gather(K=0), "hrseg_mix_gather", "K=0")
    refused(gather(S=0), "hrseg_mix_gather", "S=0")
    refused(gather(B=2, K=256, S=2048), "hrseg_mix_gather", "2^31 or more")
    refused(gather(B=2**30, K=2**30, S=2**30), "hrseg_mix_gather", "2^31 or more")
    refused(gather(out=P), "hrseg_mix_gather", "must not alias")
