"""The C-ABI library loads, exports every symbol include/hrseg.h declares, and the ctypes
prototypes in _lib.py agree with the header argument by argument (no compute calls: CPU only)."""
import ctypes
import os
import re

from tests.helpers import ROOT

HEADER = os.path.join(ROOT, "include", "hrseg.h")


def parse_header():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(int|long|size_t|const char\*)\s+(hrseg_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = [a.strip() for a in m.group(3).replace("\n", " ").split(",")]
        decls[m.group(2)] = [] if args == ["void"] else args
    return decls


def ctype_of(arg):
    if "*" in arg or "hrseg_stream_t" in arg:
        return ctypes.c_void_p
    base = arg.rsplit(" ", 1)[0].strip()
    return {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "size_t": ctypes.c_size_t}[base]


def test_header_symbols_exported_and_prototypes_match():
    from hrseg_amd import _lib
    decls = parse_header()
    assert len(decls) >= 35
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, args in decls.items():
        assert hasattr(lib, name), f"{name} declared in hrseg.h but not exported"
        if name in ("hrseg_last_error_string", "hrseg_abi_version", "hrseg_tune", "hrseg_conv_wgrad_workspace_bytes",
                    "hrseg_launch_count", "hrseg_conv_x_split_ok"):
            continue
        protos = _lib.RAW_PROTOTYPES if name in _lib.RAW_PROTOTYPES else _lib.PROTOTYPES
        assert name in protos, f"{name} has no ctypes prototype"
        want = [ctype_of(a) for a in args]
        got = list(protos[name])
        got = [ctypes.c_void_p if (isinstance(t, type) and issubclass(t, ctypes._Pointer)) else t for t in got]
        assert got == want, f"{name}: ctypes {got} != header {want}"
    for name in list(_lib.PROTOTYPES) + list(_lib.RAW_PROTOTYPES):
        assert name in decls, f"{name} bound in _lib.py but missing from hrseg.h"
    assert _lib.abi_version() == _lib.ABI_VERSION == 17
    assert not any(n.startswith("hrseg_debug_") for n in decls), "experimental switches do not belong in the public header"


def test_invalid_arguments_are_reported_without_a_gpu():
    from hrseg_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.hrseg_last_error_string.restype = ctypes.c_char_p
    shape = _lib.ConvShape(B=1, Hi=8, Wi=8, Cin=16, ldx=16, Ho=7, Wo=8, Cout=16, ldy=16, ksize=3, stride=1)
    one = (ctypes.c_void_p * 1)(None)
    lib.hrseg_conv_fwd_group.argtypes = _lib.PROTOTYPES["hrseg_conv_fwd_group"]
    rc = lib.hrseg_conv_fwd_group(1, one, one, None, one, (_lib.ConvShape * 1)(shape), None)
    assert rc == -1
    assert b"does not match" in lib.hrseg_last_error_string()
    lib.hrseg_set_scratch.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    assert lib.hrseg_set_scratch(None, 0) == 0                      # detach: always fine
    assert lib.hrseg_set_scratch(ctypes.c_void_p(4096), 1024) == -1 and b"at least 1 MiB" in lib.hrseg_last_error_string()
    assert lib.hrseg_set_scratch(ctypes.c_void_p(4097), 1 << 20) == -1 and b"aligned" in lib.hrseg_last_error_string()
    # hrseg_head_bwd moves 16 bytes per channel quad: row strides below the row length or off the 4-float grid are refused
    # before anything is launched (placeholder pointers, never dereferenced)
    lib.hrseg_head_bwd.argtypes = _lib.PROTOTYPES["hrseg_head_bwd"]
    P = ctypes.c_void_p(4096)

    def head_bwd(ldf=64, lddz=5, df=P, lddf=64):
        return lib.hrseg_head_bwd(P, ldf, None, P, P, lddz, df, lddf, 0, P, P, None, 2, 143, 64, 5, None)
    for bad in (dict(ldf=60), dict(ldf=66), dict(lddz=4), dict(lddf=60), dict(lddf=67)):
        assert head_bwd(**bad) == -1 and b"hrseg_head_bwd: bad row strides" in lib.hrseg_last_error_string(), bad
    assert lib.hrseg_head_bwd(P, 64, None, P, P, 5, P, 64, 0, P, P, None, 2, 143, 62, 5, None) == -1
    assert b"hrseg_head_bwd: bad arguments" in lib.hrseg_last_error_string()
    # hrseg_bn_fwd_group_phases asks of a problem what the phases that run touch, and refuses before anything is launched
    lib.hrseg_bn_fwd_group_phases.argtypes = _lib.PROTOTYPES["hrseg_bn_fwd_group_phases"]

    def bn_fwd(training, phases, **missing):
        prob = dict(y=4096, ldy=64, npix=35, C=64, running_mean=4096, running_var=4096, z=4096, ldz=64, coef=4096, partial=4096,
                    nchunks=2)
        prob.update(missing)
        return lib.hrseg_bn_fwd_group_phases(1, (_lib.BnFwd * 1)(_lib.BnFwd(**prob)), training, phases, None)
    assert bn_fwd(0, 4, z=None) == -1 and b"hrseg_bn_fwd_group: bad tensor arguments" in lib.hrseg_last_error_string()
    assert bn_fwd(1, 1, partial=None) == -1 and b"hrseg_bn_fwd_group: training needs partial" in lib.hrseg_last_error_string()
    assert bn_fwd(1, 0) == -1 and b"hrseg_bn_fwd_group_phases: phases is a mask" in lib.hrseg_last_error_string()
    lib.hrseg_tune.argtypes = [ctypes.c_char_p, ctypes.c_int]
    assert lib.hrseg_tune(b"igemm_wtm", 0) == 0
    assert lib.hrseg_tune(b"no_such_knob", 1) == -1 and b"unknown key" in lib.hrseg_last_error_string()


def test_conv_group_of_one_refusals():
    """A group of one through the three grouped convolution entry points: every refusal a single problem can earn, by return
    code and by the text behind the `name:` prefix, before anything is launched (placeholder pointers, never dereferenced)"""
    from hrseg_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.hrseg_last_error_string.restype = ctypes.c_char_p
    for name in ("hrseg_conv_fwd_group", "hrseg_conv_dgrad_group", "hrseg_conv_wgrad_group"):
        getattr(lib, name).argtypes = _lib.PROTOTYPES[name]
    P, NULL = (ctypes.c_void_p * 1)(4096), (ctypes.c_void_p * 1)(None)

    def refused(which, null=False, **over):
        dims = dict(B=1, Hi=8, Wi=8, Cin=16, ldx=16, Ho=8, Wo=8, Cout=16, ldy=16, ksize=3, stride=1)
        dims.update(over)
        shapes = (_lib.ConvShape * 1)(_lib.ConvShape(**dims))
        first = NULL if null else P         # (x resp. dy: the array is there, the problem's pointer is not)
        if which == "fwd":
            rc = lib.hrseg_conv_fwd_group(1, first, P, None, P, shapes, None)
        elif which == "dgrad":
            rc = lib.hrseg_conv_dgrad_group(1, first, P, P, _lib.int_array([0]), shapes, None)
        else:
            rc = lib.hrseg_conv_wgrad_group(1, first, P, P, shapes, None)
        name, _, text = lib.hrseg_last_error_string().decode().partition(": ")
        assert name == f"hrseg_conv_{which}_group", "a refusal names the entry point that was called"
        return rc, text

    mismatch = "output 7x8 does not match input 8x8 k3 s1 (expect 8x8)"
    for which in ("fwd", "dgrad", "wgrad"):
        assert refused(which, Ho=7) == (-1, mismatch), which
        assert refused(which, null=True) == (-1, "null pointer"), which
        assert refused(which, null=True, Ho=7) == (-1, mismatch), f"{which}: the shape is checked ahead of the pointers"
        assert refused(which, ldx=18) == (-1, "ld must be a multiple of 4"), which
    assert refused("fwd", Cout=24, ldy=24) == (-1, "Cout 24 not a multiple of 16")
    assert refused("fwd", Cin=24, ldx=24) == (-1, "Cin 24 not a multiple of 16")
    for which in ("dgrad", "wgrad"):
        assert refused(which, Cin=24, ldx=24) == (-1, "channels (24,16) must be multiples of 16"), which
    x_split = "x_split is set but this problem does not run the wave-specialised / nine-tap kernels (ask hrseg_conv_x_split_ok first)"
    assert refused("wgrad", x_split=1) == (-3, x_split)
    assert refused("wgrad", x_split=1, Ho=7) == (-3, x_split), "the weight gradient refuses x_split ahead of the shape"


GROUP_TABLE_ENTRY_POINTS = ["hrseg_compose_fwd", "hrseg_compose_bwd", "hrseg_consistency", "hrseg_consistency_bwd", "hrseg_group_kl",
                            "hrseg_group_kl_bwd"]


def test_group_table_refusals_name_their_entry_point():
    """The six entry points that take a class-tree group table refuse bad sizes first ("bad arguments"), then a bad table, each
    under its own name, before anything is launched (placeholder pointers, never dereferenced)"""
    from hrseg_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.hrseg_last_error_string.restype = ctypes.c_char_p
    P = ctypes.c_void_p(4096)
    for name in GROUP_TABLE_ENTRY_POINTS:
        proto = _lib.PROTOTYPES[name]
        # every one ends (B, C, Cprev, hw, ngroups, group_parent, group_size, stream); in front: its own pointers and scalars
        assert proto[-8:] == [ctypes.c_int] * 3 + [ctypes.c_long, ctypes.c_int] + [ctypes.c_void_p] * 3, name
        fn = getattr(lib, name)
        fn.argtypes = proto
        own = [P if t is ctypes.c_void_p else 1 for t in proto[:-8]]

        def refused(C=4, ngroups=2, parents=(0, 1), sizes=(2, 2)):
            rc = fn(*own, 1, C, 2, 16, ngroups, _lib.int_array(parents), _lib.int_array(sizes), None)
            return rc, lib.hrseg_last_error_string().decode()
        for bad in (dict(ngroups=0), dict(C=17)):
            rc, msg = refused(**bad)
            assert rc == -1 and f"{name}: bad arguments" in msg, (name, bad, msg)
        for bad, want in ((dict(ngroups=17), "bad group table"),
                          (dict(parents=(2, 0)), "group 0 out of range"),
                          (dict(sizes=(2, 1)), "group sizes sum to 3, level has 4 channels")):
            rc, msg = refused(**bad)
            assert rc == -1 and f"{name}: {want}" in msg, (name, bad, msg)


def test_host_descriptor_refusals_name_their_entry_point():
    """The seven entry points that read a host descriptor table refuse a bad row, an image of 2^31 pixels or more and (the
    three that take a [2][B][4] pair) unequal sizes with the full message behind their own name, before anything is launched
    (placeholder pointers, never dereferenced; only the host table, C and the thresholds are real memory)"""
    from hrseg_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.hrseg_last_error_string.restype = ctypes.c_char_p
    P, one, zeros = ctypes.c_void_p(4096), _lib.int_array([2]), _lib.int_array([0, 0, 0, 0])
    protos = dict(_lib.PROTOTYPES)
    protos.update(_lib.RAW_PROTOTYPES)
    # name -> (call(table), halves of the table, the word in front of "image" per half)
    entry = {
        "hrseg_label_components": (lambda t: (P, P, t, 1, P, 8, P, P, None), 1, ("",)),
        "hrseg_filter_components": (lambda t: (P, P, t, 1, P, P, P, P, P, P, P, None), 1, ("",)),
        "hrseg_boundary_workspace_bytes": (lambda t: (t, 1, 1, one), 1, ("",)),
        "hrseg_score_boundaries": (lambda t: (P, P, P, P, t, P, 1, one, 0, 50, P, P, 1, None), 2, ("", "")),
        "hrseg_instances_workspace_bytes": (lambda t: (t, 1), 2, (None, "ground-truth ")),     # reads the second half only
        "hrseg_mask_void_labels": (lambda t: (P, P, P, P, t, P, -1, P, 1, None), 2, ("predicted ", "ground-truth ")),
        "hrseg_score_instances": (lambda t: (P, P, P, P, P, P, P, P, t, P, P, zeros, P, P, P, P, P, 1, 0, None), 2,
                                  ("predicted ", "ground-truth ")),
    }
    assert len(entry) == 7
    good = (0, 4, 5, 1)

    def call(name, rows):
        fn = getattr(lib, name)
        fn.argtypes = protos[name]
        sizes = name.endswith("_workspace_bytes")
        fn.restype = ctypes.c_size_t if sizes else ctypes.c_int
        table = (ctypes.c_long * (4 * len(rows)))(*[v for row in rows for v in row])
        rc = fn(*entry[name][0](ctypes.cast(table, ctypes.c_void_p)))
        return (rc, 0 if sizes else -1), lib.hrseg_last_error_string().decode()

    for name, (_, halves, words) in entry.items():
        for half, what in enumerate(words):
            if what is None:
                continue

            def refused(row):
                rows = [good] * halves
                rows[half] = row
                (rc, want), msg = call(name, rows)
                assert rc == want, (name, row, rc)
                return msg
            for row in ((-1, 4, 5, 1), (0, 0, 5, 1), (0, 4, 0, 1), (0, 4, 5, 3)):
                off, H, W, ch = row
                assert refused(row) == f"{name}: {what}image 0: bad descriptor (offset {off}, {H} x {W}, {ch} channels)", (name, row)
            assert refused((0, 65536, 32768, 1)) == f"{name}: {what}image 0: 65536 x 32768 has 2^31 pixels or more", name
    for name in ("hrseg_score_boundaries", "hrseg_mask_void_labels", "hrseg_score_instances"):
        (rc, want), msg = call(name, [(0, 4, 5, 1), (0, 4, 6, 1)])
        assert rc == want and msg == f"{name}: image 0: predicted map 4 x 5, ground truth 4 x 6", (name, msg)
    # only the boundary scorer has a side limit below 2^31 pixels
    for name in ("hrseg_boundary_workspace_bytes", "hrseg_score_boundaries"):
        (rc, want), msg = call(name, [(0, 40000, 4, 1)] * entry[name][1])
        assert rc == want and msg == f"{name}: image 0: 40000 x 4, a side above 32768", (name, msg)
    (rc, _), _ = call("hrseg_instances_workspace_bytes", [(0, 40000, 4, 1)] * 2)
    assert rc == 160000 * 8 + 160000 * 4, "40000 x 4 is an image like any other to the instance scorer"


KNOBS = ["igemm_wtm", "igemm_kc", "igemm_db", "igemm_ksplit", "group_wtm", "wgrad_pix", "wgrad_db", "wgrad_blocks",
         "wgrad_group_mult", "wgrad_group_min", "wgrad_group_max", "sp_wtm", "sp_wtn", "sp_ksplit", "sp_patch", "sp_persist",
         "sp_ws", "sp_ws_waste", "small_cin3", "sp_ws_bf16", "sp_ws_n48", "sp_img", "wgrad9", "ws_epi_early", "exp_nosplit_x",
         "x_split", "ws_epi_cost", "ws_epi_acc_cost", "wgrad9_blocks", "wgrad9_blocks1", "wgrad9_blocks2", "wgrad9_blocks3",
         "wgrad9_blocks4", "sp_wide", "sp_ws_canvas", "wgrad_group_sp", "wgrad_sp_t5", "wgrad_sp_wide", "sp_wide_min_blocks",
         "sp_patch_min_tiles", "auto_min_pixels", "sp_ws_min_tiles", "deterministic"]
FAMILIES = ["ws", "ws_group", "patch_sp", "sp_im2col", "sp_pgroup", "sp_group", "f32", "f32_group", "wgrad_sp", "wgrad_f32",
            "wgrad_f32_group", "wgrad9", "small_cin", "sp_wide", "ws_canvas", "wgrad_sp_group", "wgrad_sp_t5", "wgrad_sp_wide",
            "augment_image", "augment_targets", "decode_labels"]

_REGISTRY_CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.hrseg_last_error_string.restype = ctypes.c_char_p
lib.hrseg_tune.argtypes = [ctypes.c_char_p, ctypes.c_int]
lib.hrseg_launch_count.argtypes = [ctypes.c_char_p, ctypes.c_int]
lib.hrseg_launch_count.restype = ctypes.c_long
spec = json.load(sys.stdin)
out = {"knobs": {k: lib.hrseg_tune(k.encode(), 0) for k in spec["knobs"]},
       "unknown": [lib.hrseg_tune(b"no_such_knob", 0), lib.hrseg_last_error_string().decode()],
       "families": {f: lib.hrseg_launch_count(f.encode(), 0) for f in spec["families"]},
       "total": lib.hrseg_launch_count(None, 0)}
print(json.dumps(out))
"""


def test_every_knob_and_family_is_registered():
    """hrseg_tune knows each of the 43 keys and hrseg_launch_count each of the 21 families (csrc/runtime.h), by their literal
    names; in a child process, so that the knob writes (0 switches several kernels off) cannot leak into other tests"""
    import json
    import subprocess
    import sys
    from hrseg_amd import _lib
    assert len(set(KNOBS)) == 43 and len(set(FAMILIES)) == 21
    r = subprocess.run([sys.executable, "-c", _REGISTRY_CHILD, _lib.LIB_PATH], input=json.dumps({"knobs": KNOBS, "families": FAMILIES}),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["knobs"] == {k: 0 for k in KNOBS}
    assert out["unknown"][0] == -1 and "unknown key" in out["unknown"][1]
    assert out["families"] == {f: 0 for f in FAMILIES}, "a process that launched nothing has only zero counters"
    assert out["total"] == 0
