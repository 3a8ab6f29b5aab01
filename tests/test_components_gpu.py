"""Device post-processing (csrc/components.hip, Data/postprocess.py, predictEval) against the numpy reference
tests/components_ref.py.  Roots, areas, label bytes and statistics are integers: every comparison is torch.equal."""
import argparse

import numpy as np
import pytest
import torch

from tests import components_ref as R
from tests.decode_harness import _source
from tests.decode_harness import _tree
from tests.helpers import build_model

pytestmark = pytest.mark.gpu

SENTINEL = -7
IDENT = np.arange(256, dtype=np.uint8)
PAIRS = IDENT.copy()                   # values 2k and 2k + 1 form one group (values 0..253), 254 and 255 are group 255
PAIRS[:254] = (np.arange(254) // 2).astype(np.uint8)
PAIRS[254:] = 255


def _tile():
    from hrseg_amd import ops
    return ops.components_tile()


def _shapes():
    TW, TH = _tile()
    return [(H, W) for H in (1, TH - 1, TH, TH + 1, 2 * TH + 1) for W in (1, 3, TW - 1, TW, TW + 1, 2 * TW + 3)]


def _pack(maps, start, gap):
    """maps -> (packed uint8 host buffer, [B,4] host descriptors, mask of the bytes inside a span).  `start` bytes lie in
    front of the first map, `gap` bytes between two maps and behind the last.  The bytes outside hold valid classes of the
    groups next to them: in front of a map its first pixel's value, behind it its last pixel's (a gap is split between its
    two maps): a read outside a span, or a connection across a seam, changes roots and areas."""
    n = start + sum(m.size + gap for m in maps)
    buf = np.zeros(n, dtype=np.uint8)
    inside = np.zeros(n, dtype=bool)
    rows, off = [], start
    for k, m in enumerate(maps):
        flat = m.reshape(-1)
        front = off - (start if k == 0 else gap - gap // 2)
        buf[front:off] = flat[0]
        buf[off:off + m.size] = flat
        inside[off:off + m.size] = True
        behind = gap if k == len(maps) - 1 else gap // 2
        buf[off + m.size:off + m.size + behind] = flat[-1]
        rows.append([off, m.shape[0], m.shape[1], 1])
        off += m.size + gap
    return buf, torch.tensor(rows, dtype=torch.int64), inside


_LABEL_CACHE = {}


def _ref_label(m, group, conn):
    key = (m.shape, m.tobytes(), group.tobytes(), conn)
    if key not in _LABEL_CACHE:
        _LABEL_CACHE[key] = R.label(m, group, conn)
    return _LABEL_CACHE[key]


def _label(maps, group, conn, start=0, gap=0):
    """run ops.label_components on the packed maps -> (roots, area) on the host, after checking both against the
    reference inside the spans and for the untouched sentinel outside"""
    from hrseg_amd import ops
    buf, host, inside = _pack(maps, start, gap)
    want_r = np.full(buf.size, SENTINEL, dtype=np.int32)
    want_a = np.full(buf.size, SENTINEL, dtype=np.int32)
    for (off, H, W, _), m in zip(host.tolist(), maps):
        r, a = _ref_label(m, group, conn)
        want_r[off:off + H * W], want_a[off:off + H * W] = r.reshape(-1), a.reshape(-1)
    roots = torch.full((buf.size,), SENTINEL, dtype=torch.int32, device="cuda")
    area = torch.full((buf.size,), SENTINEL, dtype=torch.int32, device="cuda")
    got = ops.label_components(torch.from_numpy(buf).cuda(), host.cuda(), host, torch.from_numpy(group).cuda(), conn, out=(roots, area))
    assert got[0] is roots and got[1] is area
    gr, ga = roots.cpu(), area.cpu()
    bad = (gr != torch.from_numpy(want_r)).nonzero().flatten().tolist()[:6]
    assert torch.equal(gr, torch.from_numpy(want_r)), [(i, int(gr[i]), int(want_r[i])) for i in bad]
    bad = (ga != torch.from_numpy(want_a)).nonzero().flatten().tolist()[:6]
    assert torch.equal(ga, torch.from_numpy(want_a)), [(i, int(ga[i]), int(want_a[i])) for i in bad]
    return gr, ga


def _rules_tensor(rules):
    t = np.tile(np.array([0, 0, -1], dtype=np.int32), (256, 1))
    for g, r in rules.items():
        t[g] = r
    return torch.from_numpy(t).cuda()


def _filter(maps, group, rules, conn, start=0, gap=0, stats=None, times=1):
    """label + filter on the packed maps against the reference: out inside the spans, the sentinel byte outside, stats
    (added to `stats` when given) -> (out, stats) device tensors"""
    from hrseg_amd import ops
    buf, host, inside = _pack(maps, start, gap)
    want = np.full(buf.size, 0xA5, dtype=np.uint8)
    want_stats = np.zeros((len(maps), 256, 3), dtype=np.int64)
    for b, ((off, H, W, _), m) in enumerate(zip(host.tolist(), maps)):
        o, s = R.filter(m, group, rules, conn)
        want[off:off + H * W] = o.reshape(-1)
        want_stats[b] = s
    dbuf, dhost, dgroup = torch.from_numpy(buf).cuda(), host.cuda(), torch.from_numpy(group).cuda()
    roots, area = ops.label_components(dbuf, dhost, host, dgroup, conn)
    out = torch.full((buf.size,), 0xA5, dtype=torch.uint8, device="cuda")
    base = 0 if stats is None else stats.cpu().clone()
    for _ in range(times):
        got, stats = ops.filter_components(dbuf, dhost, host, dgroup, _rules_tensor(rules), roots, area, out=out, stats=stats)
    assert got is out and stats.dtype == torch.int64
    assert torch.equal(dbuf.cpu(), torch.from_numpy(buf)), "the input maps are not written"
    bad = (out.cpu() != torch.from_numpy(want)).nonzero().flatten().tolist()[:6]
    assert torch.equal(out.cpu(), torch.from_numpy(want)), [(i, int(out[i]), int(want[i])) for i in bad]
    assert torch.equal(stats.cpu(), base + times * torch.from_numpy(want_stats)), (stats.cpu() - base - times * want_stats).nonzero().tolist()[:6]
    return out, stats


def _pattern(name, H, W, rng):
    TW, TH = _tile()
    if name == "uniform":
        return np.full((H, W), 1, np.uint8)
    if name == "checkerboard":
        return R.checkerboard(H, W)
    if name == "serpentine":
        return R.serpentine(H, W)
    if name == "spiral":
        return R.spiral(H, W)
    if name == "vstripes":
        return R.stripes(H, W, True)
    if name == "hstripes":
        return R.stripes(H, W, False)
    if name == "diagonal":
        return R.diagonal(H, W, False, TH)
    if name == "antidiagonal":
        return R.diagonal(H, W, True, TH)
    if name == "random2":                                     # 8-connected site percolation sets in near 0.41, 4-connected near 0.59
        return R.random_map(rng, H, W, [1, 2], 0.62)
    raise KeyError(name)


PATTERNS = ["uniform", "checkerboard", "serpentine", "spiral", "vstripes", "hstripes", "diagonal", "antidiagonal", "random2"]


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", PATTERNS)
def test_every_shape_around_the_tile(name, conn):
    """one ragged batch of the 30 shapes (H and W at 1, tile - 1, tile, tile + 1, two tiles and a bit; single rows and
    columns among them) of one pattern, guard bytes of the neighbouring groups between the maps"""
    rng = np.random.default_rng(17)
    _label([_pattern(name, H, W, rng) for H, W in _shapes()], IDENT, conn, start=5, gap=3)


@pytest.mark.parametrize("conn", [4, 8])
def test_every_start_alignment_with_guard_bytes(conn):
    """the first image starts at every byte of a 16-byte line; a second one follows behind an odd gap.  Two values of one
    group: the kernels must compare group ids, not bytes"""
    TW, TH = _tile()
    rng = np.random.default_rng(19)
    maps = [R.random_map(rng, 3, TW + 5, [2, 3, 4], 0.5), R.random_map(rng, TH + 1, 19, [2, 3, 4, 7], 0.4)]
    for start in range(16):
        _label(maps, PAIRS, conn, start=start, gap=5)
        _filter(maps, PAIRS, {1: (4, 0, -1), 2: (0, 1, 9)}, conn, start=start, gap=5)


@pytest.mark.parametrize("conn", [4, 8])
def test_random_maps_below_and_above_percolation(conn):
    """2, 3 and 8 values, the first at a density that percolates (one component crosses every tile) and at one that
    does not, at the largest size of the shape test"""
    TW, TH = _tile()
    rng = np.random.default_rng(23)
    H, W = 2 * TH + 1, 2 * TW + 3
    maps = [R.random_map(rng, H, W, list(range(1, n + 1)), p) for n in (2, 3, 8) for p in (0.3, 0.7)]
    maps += [R.random_map(rng, H, W, list(range(1, n + 1))) for n in (2, 3, 8)]
    _label(maps, IDENT, conn, start=1, gap=2)


@pytest.mark.parametrize("conn", [4, 8])
def test_touching_images_do_not_connect(conn):
    """four images with no gap between them; the last row of one and the first row of the next hold the same value, and so
    do the bytes in front of the first and behind the last"""
    TW, TH = _tile()
    rng = np.random.default_rng(29)
    maps = []
    for H, W in ((3, 7), (TH + 1, 7), (2, TW + 1), (5, 5)):
        m = R.random_map(rng, H, W, [1, 2], 0.5)
        m[0] = m[-1] = 1
        maps.append(m)
    gr, ga = _label(maps, IDENT, conn, start=9, gap=0)
    assert int(gr[9]) == 0 and int(gr[9 + 21]) == 0, "every image's first pixel is its own root 0"
    _filter(maps, IDENT, {1: (0, 1, 2)}, conn, start=9, gap=0)


@pytest.mark.parametrize("conn", [4, 8])
def test_one_large_percolating_map(conn):
    """512 x 768: several dozen tiles merge through one component"""
    TW, TH = _tile()
    rng = np.random.default_rng(31)
    m = R.random_map(rng, 512, 768, [1, 2], 0.68 if conn == 4 else 0.5)
    gr, ga = _label([m], IDENT, conn, start=3, gap=1)
    assert int(ga.max()) > 40 * TW * TH, "one component spans several dozen tiles"


# ------------------------------------------------------------------------------------------------------------------ filter
def _blobs(H, W, value, boxes, background=0):
    m = np.full((H, W), background, np.uint8)
    for y, x, h, w in boxes:
        m[y:y + h, x:x + w] = value
    return m


@pytest.mark.parametrize("conn", [4, 8])
def test_min_area_at_the_exact_boundary(conn):
    """components of a - 1, a and a + 1 pixels with min_area = a: only the first goes; a = 6, and a = two tile widths + 1
    with components that cross two tile borders"""
    TW, TH = _tile()
    small = _blobs(9, 24, 6, [(1, 1, 1, 5), (3, 8, 2, 3), (6, 14, 1, 7)])
    out, stats = _filter([small], IDENT, {6: (6, 0, -1)}, conn)
    assert stats[0, 6].tolist() == [3, 1, 5]
    a = 2 * TW + 1
    wide = _blobs(7, 2 * TW + 3, 6, [(1, 0, 1, a - 1), (3, 0, 1, a), (5, 0, 1, a + 1)])
    out, stats = _filter([wide, small], IDENT, {6: (a, 0, 1)}, conn, start=2, gap=3)
    assert stats[0, 6].tolist() == [3, 1, a - 1] and stats[1, 6].tolist() == [3, 3, 18]


@pytest.mark.parametrize("conn", [4, 8])
def test_keep_largest_with_a_tie(conn):
    TW, TH = _tile()
    m = _blobs(TH + 6, TW + 9, 5, [(1, TW - 2, 2, 4), (TH - 1, 2, 4, 2), (TH + 3, TW + 1, 1, 7)])        # areas 8, 8, 7
    out, stats = _filter([m], IDENT, {5: (0, 1, -1)}, conn)
    assert stats[0, 5].tolist() == [3, 2, 15]
    assert (out[:m.size].cpu().numpy().reshape(m.shape)[1:3, TW - 2:TW + 2] == 5).all(), "of the two of 8 pixels the first stays"


@pytest.mark.parametrize("conn", [4, 8])
def test_fixed_and_neighbour_fill_without_cascade(conn):
    """a removed component beside another removed one takes the neighbour's INPUT value; column 0 takes the north
    neighbour; a component at the origin stays; rules on some groups only; group 255 is untouched"""
    m = np.full((8, 12), 10, np.uint8)          # group 5 (PAIRS): no rule
    m[0, 0:2] = 20                              # group 10 at the origin: would be removed, stays
    m[2, 3:5] = 30                              # group 15: removed, fixed fill 99
    m[2, 5:7] = 20                              # group 10: removed, neighbour fill = 30, the input value of the removed one
    m[5, 0] = 21                                # group 10 in column 0: north neighbour
    m[4, 0] = 31                                # ... which is itself removed (group 15): the input value 31
    m[6, 6:9] = 254                             # group 255: small, never touched
    m[7, 10] = 40                               # group 20: no rule
    rules = {10: (5, 0, -1), 15: (5, 0, 99), 255: (100, 0, 0)}
    out, stats = _filter([m], PAIRS, rules, conn, start=7, gap=4)
    got = out[7:7 + m.size].cpu().numpy().reshape(m.shape)
    assert got[2, 5] == 30 and got[5, 0] == 31 and got[4, 0] == 99 and got[0, 0] == 20 and got[6, 6] == 254 and got[7, 10] == 40
    assert stats[0, 10].tolist() == [3, 2, 3] and stats[0, 15].tolist() == [2, 2, 3] and stats[0, 255].tolist() == [1, 0, 0]
    # a second call adds to the same statistics
    _filter([m], PAIRS, rules, conn, start=7, gap=4, stats=stats, times=2)


@pytest.mark.parametrize("conn", [4, 8])
def test_filter_on_noisy_maps_matches_the_reference(conn):
    """every rule kind on maps with thousands of components: statistics and bytes"""
    TW, TH = _tile()
    rng = np.random.default_rng(37)
    maps = [R.random_map(rng, 2 * TH + 1, 2 * TW + 3, [2, 3, 4, 6, 9, 254], 0.3), R.random_map(rng, TH + 1, TW - 1, [2, 4, 5, 7]),
            R.checkerboard(TH, TW + 1, 4, 6), R.serpentine(TH + 1, TW + 1, 2, 4)]
    _filter(maps, PAIRS, {1: (3, 0, -1), 2: (0, 1, -1), 3: (7, 1, 0), 4: (2, 0, 254)}, conn, start=11, gap=6)


# ------------------------------------------------------------------------------------------- determinism and structure
def test_five_runs_give_identical_bytes():
    TW, TH = _tile()
    rng = np.random.default_rng(41)
    maps = [R.serpentine(2 * TH + 1, 2 * TW + 3), R.random_map(rng, 2 * TH + 1, 2 * TW + 3, [1, 2], 0.62)]
    first = None
    for _ in range(5):
        gr, ga = _label(maps, IDENT, 8, start=3, gap=2)
        out, stats = _filter(maps, IDENT, {1: (30, 1, -1), 2: (4, 0, 1)}, 8, start=3, gap=2)
        got = (gr, ga, out.cpu(), stats.cpu())
        if first is None:
            first = got
        assert all(torch.equal(a, b) for a, b in zip(first, got))


def test_launch_counters():
    from hrseg_amd import _lib, ops
    from hrseg_amd.Data import DevicePostprocess, RaggedLabels
    tree, cmap = _tree("tl")
    pp = DevicePostprocess(tree, cmap, 0, {"tooth": dict(min_area=4)})
    buf, host, _ = _pack([R.random_map(np.random.default_rng(43), 40, 50, [0, 127, 170, 212])], 0, 0)
    maps = RaggedLabels(torch.from_numpy(buf).cuda(), None, host.cuda(), host)
    pp.tables.device(torch.device("cuda", 0))
    torch.cuda.synchronize()
    assert (ops.LABEL_COMPONENTS_LAUNCHES, ops.FILTER_COMPONENTS_LAUNCHES) == (3, 3)
    families = ["label_components", "filter_components", "decode_labels", "score_labels", "decode_views", "augment_image"]
    before = {f: _lib.launch_count(f) for f in families}
    total = _lib.launch_count()
    clean = pp.apply(maps)
    after = {f: _lib.launch_count(f) for f in families}
    assert after["label_components"] == before["label_components"] + 3
    assert after["filter_components"] == before["filter_components"] + 3
    assert all(after[f] == before[f] for f in families[2:]) and _lib.launch_count() == total
    roots, area = pp.components(maps)
    assert _lib.launch_count("label_components") == before["label_components"] + 6
    assert _lib.launch_count("filter_components") == before["filter_components"] + 3
    assert clean.desc_host is host and clean.confidence is None and clean.labels.data_ptr() != maps.labels.data_ptr()
    m = buf.reshape(40, 50)
    group = np.array(pp.tables.group, dtype=np.uint8)
    want, stats = R.filter(m, group, {3: (4, 0, -1)}, 8)
    assert torch.equal(clean.labels.cpu(), torch.from_numpy(want.reshape(-1)))
    assert torch.equal(pp.last_stats.cpu()[0], torch.from_numpy(stats))
    r, a = R.label(m, group, 8)
    assert torch.equal(roots.cpu(), torch.from_numpy(r.reshape(-1))) and torch.equal(area.cpu(), torch.from_numpy(a.reshape(-1)))
    named = pp.stats_by_name()
    assert named[0]["tooth"] == tuple(stats[3].tolist()) and set(named[0]) == {"background", "upper", "tooth"}


# ----------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def small_model():
    from hrseg_amd.Models import models as PM
    tree, cmap = _tree("tl")
    return build_model(PM, "hrnet", True, tree, 64).cuda(), tree, cmap


def _images():
    rng = np.random.default_rng(47)
    return [_source(rng, 50, 70, 3), _source(rng, 60, 100, 1), _source(rng, 64, 64, 3)]


def test_predictor_without_postprocess_is_unchanged(small_model):
    from hrseg_amd import _lib
    from hrseg_amd import predictEval as PE
    model, tree, cmap = small_model
    args = argparse.Namespace(img_size=64, model_type=1, model_select=1)
    plain = PE.Predictor(model, tree, cmap, args)(_images())
    before = _lib.launch_count("label_components"), _lib.launch_count("filter_components")
    none = PE.Predictor(model, tree, cmap, args, postprocess=None)(_images())
    assert (_lib.launch_count("label_components"), _lib.launch_count("filter_components")) == before
    assert torch.equal(plain.labels, none.labels) and torch.equal(plain.desc_host, none.desc_host)


def test_predictor_with_postprocess_end_to_end(small_model):
    from hrseg_amd import predictEval as PE
    from hrseg_amd.Data import DevicePostprocess, DeviceScore
    model, tree, cmap = small_model
    args = argparse.Namespace(img_size=64, model_type=1, model_select=1)
    # whatever the untrained model draws, something goes: every component is too small, each group to another value
    rules = {"background": dict(min_area=10 ** 9, fill="upper"), "upper": dict(min_area=10 ** 9, fill="lower"),
             "lower": dict(min_area=10 ** 9, fill=0), "tooth": dict(min_area=10 ** 9, keep_largest=True, fill="background")}
    pp = DevicePostprocess(tree, cmap, 0, rules, connectivity=8)
    imgs = _images()
    raw = PE.Predictor(model, tree, cmap, args, want_confidence=True)(imgs)
    predictor = PE.Predictor(model, tree, cmap, args, want_confidence=True, postprocess=pp)
    clean = predictor(imgs)
    again = pp.apply(raw)
    assert torch.equal(clean.labels, again.labels) and again.confidence is raw.confidence
    # (the confidence of two forwards may differ in its last bits: the predictor hands its own decode's tensor through)
    assert clean.confidence is not None and clean.confidence.shape == raw.confidence.shape
    assert torch.equal(clean.desc_host, raw.desc_host)
    group = np.array(pp.tables.group, dtype=np.uint8)
    ref_rules = {0: (10 ** 9, 0, 212), 1: (10 ** 9, 0, 255), 2: (10 ** 9, 0, 0), 3: (10 ** 9, 1, 0)}
    want_stats = []
    for got, m in zip(clean.unpack(), raw.unpack()):
        want, stats = R.filter(m, group, ref_rules, 8)
        assert torch.equal(torch.from_numpy(got.copy()), torch.from_numpy(want))
        want_stats.append(stats)
    assert torch.equal(pp.last_stats.cpu(), torch.from_numpy(np.stack(want_stats)))          # (of pp.apply(raw), the same maps)
    assert int(pp.last_stats[:, :, 1].sum()) > 0 and not torch.equal(clean.labels, raw.labels), "the maps had something to clean"
    # score: the cleaned maps at the ground truth's sizes
    rng = np.random.default_rng(53)
    vals = np.array(sorted(R.name2pix(cmap).values()), dtype=np.uint8)
    labels = [rng.choice(vals, size=s) for s in ((50, 70), (60, 100), (33, 47))]
    scores = predictor.score(imgs, labels)
    maps = predictor.last_labels
    unclean = PE.Predictor(model, tree, cmap, args)
    unclean.score(imgs, labels)
    assert torch.equal(maps.labels, pp.apply(unclean.last_labels).labels)
    from hrseg_amd.Data.decode import pack_images
    gbuf, ghost = pack_images(labels)
    want = DeviceScore(tree, cmap).score(maps, (gbuf, ghost, ghost))
    assert torch.equal(scores.counts, want.counts) and torch.equal(scores.ignored, want.ignored)
