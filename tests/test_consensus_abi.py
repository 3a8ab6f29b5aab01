"""hrseg_consensus_labels refuses bad arguments by return code and under its own name before anything is launched
(placeholder pointers, never dereferenced; only the member array, the host descriptor table and the struct are real memory),
and its launch-counter family exists and reads 0 in a fresh process.  No GPU."""
import ctypes
import json
import os
import re
import subprocess
import sys

P = ctypes.c_void_p(4096)
NAME = "hrseg_consensus_labels"


def _lib_and_protos():
    from hrseg_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.hrseg_last_error_string.restype = ctypes.c_char_p
    getattr(lib, NAME).argtypes = _lib.PROTOTYPES[NAME]
    return lib


def _struct(nlevels=2, C=(4, 4), quorum=2, none_val=2, out_val=None):
    from hrseg_amd import _lib
    s = _lib.Consensus()
    s.nlevels = nlevels
    out_val = out_val or [[0, 212, 255, 1], [127, 170, 85, 42]]
    for L, n in enumerate(C):
        s.C[L] = n
        for c in range(min(max(n, 0), 16)):
            s.out_val[L][c] = out_val[L][c] if L < len(out_val) and c < len(out_val[L]) else 100 + 16 * L + c
    s.none_val, s.quorum = none_val, quorum
    return s


def _call(lib, M=3, B=2, rows=None, members="ok", desc=P, desc_host="ok", path_lut=P, cons="ok", labels=P, support=P, counts=P, **kw):
    rows = rows if rows is not None else [(0, 4, 5, 1), (20, 3, 7, 1)] * max(M, 1)
    table = (ctypes.c_long * (4 * len(rows)))(*[v for row in rows for v in row])
    if members == "ok":
        members = (ctypes.c_void_p * max(M, 1))(*([4096] * max(M, 1)))
    struct = _struct(**kw)
    rc = getattr(lib, NAME)(M, members, desc, ctypes.cast(table, ctypes.c_void_p) if desc_host == "ok" else desc_host, path_lut,
                            ctypes.byref(struct) if cons == "ok" else cons, labels, support, counts, B, 0, None)
    who, _, text = lib.hrseg_last_error_string().decode().partition(": ")
    assert rc == -1 and who == NAME, (rc, who, text)
    return text


def test_refusals():
    from hrseg_amd import _lib
    lib = _lib_and_protos()
    launched = _lib.launch_count("consensus_labels")
    for null in ("members", "desc", "desc_host", "path_lut", "cons", "labels", "counts"):
        assert "null pointer (members, desc, desc_host, path_lut, cons, labels, counts)" in _call(lib, **{null: None}), null
    holes = (ctypes.c_void_p * 3)(4096, None, 4096)
    assert _call(lib, members=holes) == "null pointer (member 1)"
    for B in (0, -1, 65536):
        assert _call(lib, B=B) == f"B={B} not in 1..65535"
    for M in (0, -2, 9):
        assert _call(lib, M=M) == f"M={M} not in 1..8"
    for M, q in ((3, 1), (3, 4), (2, 1), (4, 2), (8, 4), (8, 9), (1, 0), (3, -1)):
        assert _call(lib, M=M, quorum=q) == f"quorum {q} of {M} members: need 2 * quorum > M and quorum <= M"
    for nlevels in (0, 9):
        assert _call(lib, nlevels=nlevels) == f"nlevels={nlevels} not in 1..8"
    assert _call(lib, C=(4, 0)) == "C[1]=0 not in 1..16"
    assert _call(lib, C=(17, 4)) == "C[0]=17 not in 1..16"
    assert _call(lib, nlevels=5, C=(13,) * 5) == "65 channels over all levels, at most 64"
    assert _call(lib, none_val=256) == "none_val=256 not in 0..255"
    assert _call(lib, none_val=-1) == "none_val=-1 not in 0..255"
    assert _call(lib, out_val=[[0, 212, 255, 1], [127, 300, 85, 42]]) == "(level 1, channel 1) has the output value 300, not in 0..255"
    assert _call(lib, out_val=[[0, 212, 255, 1], [127, -1, 85, 42]]) == "(level 1, channel 1) has the output value -1, not in 0..255"
    assert _call(lib, out_val=[[0, 212, 255, 1], [127, 170, 212, 42]]) == "(level 0, channel 1) and (level 1, channel 2) share the byte 212"
    assert _call(lib, none_val=85) == "(level 1, channel 2) and none_val share the byte 85"
    # the host descriptor table: a bad row, 2^31 pixels or more, members that disagree
    good = [(0, 4, 5, 1), (20, 3, 7, 1)]
    for row in ((-1, 4, 5, 1), (0, 0, 5, 1), (0, 4, 0, 1), (0, 4, 5, 3)):
        off, H, W, ch = row
        assert _call(lib, rows=good + [good[0], row] + good) == \
            f"member 1, image 1: bad descriptor (offset {off}, {H} x {W}, {ch} channels)"
    assert _call(lib, M=1, B=1, quorum=1, rows=[(0, 65536, 32768, 1)]) == "member 0, image 0: 65536 x 32768 has 2^31 pixels or more"
    assert _call(lib, rows=good + good + [good[0], (20, 7, 3, 1)]) == "member 2, image 1: 7 x 3, member 0 has 3 x 7"
    assert _call(lib, counts=ctypes.c_void_p(4100)) == "counts and path_lut must be 8-byte aligned"
    assert _call(lib, path_lut=ctypes.c_void_p(4100)) == "counts and path_lut must be 8-byte aligned"
    for off in (1, 2, 3):
        assert _call(lib, labels=ctypes.c_void_p(4096 + off)) == "labels must be 4-byte aligned"
    assert _lib.launch_count("consensus_labels") == launched, "a refusal launches nothing"


def test_prototype_and_struct_follow_the_header():
    """the struct of _lib.py has the fields of hrseg_consensus_t in the header's order and sizes, and the step macros are the
    wrapper's constants"""
    from hrseg_amd import _lib, ops
    from tests.helpers import ROOT
    with open(os.path.join(ROOT, "include", "hrseg.h")) as f:
        src = f.read()
    body = re.search(r"typedef struct \{([^}]*)\} hrseg_consensus_t;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.match(r"int\s+(\w+)((?:\[\w+\])*)", d.strip()).groups() for d in body.split(";") if d.strip()]
    dims = {"HRSEG_SCORE_MAX_LEVELS": 8, "HRSEG_SCORE_MAX_CHANNELS": 16}
    want = [(n, int(np_prod([dims[x] for x in re.findall(r"\[(\w+)\]", d)]))) for n, d in fields]
    got = [(n, ctypes.sizeof(t) // 4) for n, t in _lib.Consensus._fields_]
    assert got == want == [("nlevels", 1), ("C", 8), ("out_val", 128), ("none_val", 1), ("quorum", 1)]
    macros = dict(re.findall(r"#define (HRSEG_CONSENSUS_\w+) (\d+)", src))
    assert int(macros["HRSEG_CONSENSUS_MAX_MEMBERS"]) == ops.CONSENSUS_MAX_MEMBERS == 8
    assert int(macros["HRSEG_CONSENSUS_LANE_STEP"]) == ops.CONSENSUS_LANE_STEP
    assert int(macros["HRSEG_CONSENSUS_BLOCK_STEP"]) == ops.CONSENSUS_BLOCK_STEP


def np_prod(xs):
    out = 1
    for x in xs:
        out *= x
    return out


_CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.hrseg_launch_count.argtypes = [ctypes.c_char_p, ctypes.c_int]
lib.hrseg_launch_count.restype = ctypes.c_long
print(json.dumps({"consensus_labels": lib.hrseg_launch_count(b"consensus_labels", 0), "total": lib.hrseg_launch_count(None, 0)}))
"""


def test_the_family_reads_zero_in_a_fresh_process():
    from hrseg_amd import _lib
    r = subprocess.run([sys.executable, "-c", _CHILD, _lib.LIB_PATH], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["consensus_labels"] == 0 and out["total"] == 0
    # (an unknown name reads 0 as well: that the family is a row of csrc/runtime.h is what the source says)
    from tests.helpers import CSRC
    with open(os.path.join(CSRC, "runtime.h")) as f:
        assert 'X(CONSENSUS_LABELS, "consensus_labels", 0)' in f.read()
