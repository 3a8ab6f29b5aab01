"""The three entry points of the border weights refuse bad arguments by return code and under their own name before anything is
launched (placeholder pointers, never dereferenced), and their launch-counter family exists and reads 0 in a fresh process.
No GPU."""
import ctypes
import json
import subprocess
import sys

P = ctypes.c_void_p(4096)


def _lib_and_protos():
    from hrseg_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.hrseg_last_error_string.restype = ctypes.c_char_p
    for name in ("hrseg_border_weights", "hrseg_loss_partials_pw", "hrseg_loss_bwd_pw"):
        getattr(lib, name).argtypes = _lib.PROTOTYPES[name]
    return lib


def _refused(lib, name, rc):
    who, _, text = lib.hrseg_last_error_string().decode().partition(": ")
    assert rc == -1 and who == name, (name, rc, who, text)
    return text


def test_border_weights_refusals():
    lib = _lib_and_protos()

    def call(t=P, B=2, C=4, H=8, W=9, radius=5, lut=P, labels=P, v=P, d2=P):
        return _refused(lib, "hrseg_border_weights", lib.hrseg_border_weights(t, B, C, H, W, radius, lut, labels, v, d2, None))
    for null in ("t", "lut", "labels", "v"):
        assert "null pointer" in call(**{null: None}), null
    for bad in (dict(B=0), dict(B=-1), dict(C=0), dict(C=17), dict(H=0), dict(W=0), dict(W=-3)):
        assert "bad arguments" in call(**bad), bad
    assert "2^31 pixels or more" in call(H=65536, W=32768)
    assert "2^31 pixels or more" in call(H=1 << 30, W=2)
    for radius in (0, -1, 33):
        assert f"radius {radius} outside 1..32" in call(radius=radius)


def test_border_tile_is_a_constant_of_the_library():
    from hrseg_amd import _lib
    w, h = _lib.border_tile()
    assert w == 64 and h >= 1 and (w, h) == _lib.border_tile()


def test_loss_pw_refusals():
    lib = _lib_and_protos()

    def partials(z=P, t=P, pw=P, partial=P, B=2, C=4, hw=100, gamma=0.0):
        return _refused(lib, "hrseg_loss_partials_pw", lib.hrseg_loss_partials_pw(z, t, pw, partial, B, C, hw, gamma, None))

    def bwd(z=P, t=P, pw=P, coef=P, g=P, dz=P, B=2, C=4, hw=100, gamma=0.0):
        return _refused(lib, "hrseg_loss_bwd_pw", lib.hrseg_loss_bwd_pw(z, t, pw, coef, g, dz, 0, B, C, hw, gamma, None))
    for fn, pointers in ((partials, ("z", "t", "partial")), (bwd, ("z", "t", "coef", "g", "dz"))):
        for null in pointers:
            assert "bad arguments" in fn(**{null: None}), (fn.__name__, null)
        for bad in (dict(B=0), dict(C=0), dict(C=17), dict(hw=0)):
            assert "bad arguments" in fn(**bad), (fn.__name__, bad)
        for gamma in (-1.0, float("nan"), float("inf")):
            assert "gamma must be finite and >= 0" in fn(gamma=gamma), (fn.__name__, gamma)
        assert "null pointer (pw)" in fn(pw=None), fn.__name__


_CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.hrseg_launch_count.argtypes = [ctypes.c_char_p, ctypes.c_int]
lib.hrseg_launch_count.restype = ctypes.c_long
print(json.dumps({"border_weights": lib.hrseg_launch_count(b"border_weights", 0), "total": lib.hrseg_launch_count(None, 0)}))
"""


def test_the_family_reads_zero_in_a_fresh_process():
    from hrseg_amd import _lib
    r = subprocess.run([sys.executable, "-c", _CHILD, _lib.LIB_PATH], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["border_weights"] == 0 and out["total"] == 0
    # (an unknown name reads 0 as well: that the family is a row of csrc/runtime.h is what the source says)
    from tests.helpers import CSRC
    import os
    with open(os.path.join(CSRC, "runtime.h")) as f:
        assert 'X(BORDER_WEIGHTS, "border_weights", 0)' in f.read()
