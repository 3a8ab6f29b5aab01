"""The two entry points of the tree distillation refuse bad arguments by return code and under their own name before anything is
launched (placeholder pointers, never dereferenced; only the group table is real memory), and their launch-counter family exists
and reads 0 in a fresh process.  No GPU."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

P = ctypes.c_void_p(4096)
NAMES = ("hrseg_tree_kl", "hrseg_tree_kl_bwd")


def _caller(name):
    from hrseg_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.hrseg_last_error_string.restype = ctypes.c_char_p
    fn = getattr(lib, name)
    fn.argtypes = _lib.PROTOTYPES[name]

    def call(z=P, u=P, wprev=P, pw=P, inv_temp=1.0, thresh=0.5, out=P, g=P, dz=P, B=2, C=4, Cprev=3, hw=100, ngroups=2,
             parents=(0, 2), sizes=(1, 3)):
        gp = None if parents is None else _lib.int_array(list(parents))
        gs = None if sizes is None else _lib.int_array(list(sizes))
        if name == "hrseg_tree_kl":
            rc = fn(z, u, wprev, pw, inv_temp, thresh, out, B, C, Cprev, hw, ngroups, gp, gs, None)
        else:
            rc = fn(z, u, wprev, pw, inv_temp, thresh, g, 1.0, dz, 0, B, C, Cprev, hw, ngroups, gp, gs, None)
        who, _, text = lib.hrseg_last_error_string().decode().partition(": ")
        assert rc == -1 and who == name, (name, rc, who, text)
        return text
    return call


@pytest.mark.parametrize("name", NAMES)
def test_tree_kl_refusals(name):
    call = _caller(name)
    for null in ("z", "u") + (("out",) if name == "hrseg_tree_kl" else ("g", "dz")):
        assert "null pointer" in call(**{null: None}), null
    for bad in (dict(B=0), dict(B=-1), dict(C=0), dict(C=17), dict(hw=0), dict(hw=-5)):
        assert "bad arguments" in call(**bad), bad
    # the group table: the three messages of the composition's entry points
    for bad in (dict(ngroups=0), dict(ngroups=17), dict(sizes=None), dict(parents=None)):
        assert "bad group table" in call(**bad), bad
    assert "group 1 out of range" in call(parents=(0, 3))           # a parent outside Cprev
    assert "group 0 out of range" in call(parents=(-1, 2))
    assert "group 1 out of range" in call(sizes=(4, 0))
    assert "group sizes sum to 3, level has 4 channels" in call(sizes=(1, 2))
    for Cprev in (0, -1, 17):
        assert f"wprev is set and Cprev={Cprev} is outside 1..16" in call(Cprev=Cprev), Cprev
    for inv_temp in (0.0, -1.0, float("inf"), float("nan")):
        assert "inv_temp must be finite and > 0" in call(inv_temp=inv_temp), inv_temp
    for thresh in (-0.25, 1.5, float("nan"), float("inf")):
        assert "thresh must be in [0, 1]" in call(thresh=thresh), thresh


@pytest.mark.parametrize("name", NAMES)
def test_without_parents_neither_cprev_nor_the_parent_column_is_read(name):
    """wprev = NULL: a Cprev of 0 and parents that no level has are not what the call is refused for (it goes on to the next
    check, which here is the temperature)"""
    call = _caller(name)
    assert "inv_temp must be finite and > 0" in call(wprev=None, Cprev=0, parents=(99, -7), inv_temp=0.0)
    assert "inv_temp must be finite and > 0" in call(wprev=None, Cprev=0, parents=None, inv_temp=0.0)


def test_both_are_bound_with_the_house_tail():
    from hrseg_amd import _lib
    for name in NAMES:
        assert _lib.PROTOTYPES[name][-8:] == [ctypes.c_int] * 3 + [ctypes.c_long, ctypes.c_int] + [ctypes.c_void_p] * 3, name


_CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.hrseg_launch_count.argtypes = [ctypes.c_char_p, ctypes.c_int]
lib.hrseg_launch_count.restype = ctypes.c_long
print(json.dumps({"tree_kl": lib.hrseg_launch_count(b"tree_kl", 0), "total": lib.hrseg_launch_count(None, 0)}))
"""


def test_the_family_reads_zero_in_a_fresh_process():
    from hrseg_amd import _lib
    r = subprocess.run([sys.executable, "-c", _CHILD, _lib.LIB_PATH], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["tree_kl"] == 0 and out["total"] == 0
    # (an unknown name reads 0 as well: that the family is a row of csrc/runtime.h is what the source says)
    from tests.helpers import CSRC
    with open(os.path.join(CSRC, "runtime.h")) as f:
        assert 'X(TREE_KL, "tree_kl", 0)' in f.read()
