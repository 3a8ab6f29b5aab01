"""hrseg_border_weights (csrc/border_weight.hip) against the numpy brute force of tests/border_ref.py: labels, d2 and v are
compared exactly (v as bits).  Sizes around the tile of the search kernel, every channel-count instance edge, radii from 1
to the largest, and the patterns that single out one rule of the semantics each (include/hrseg.h, "border weights")."""
import numpy as np
import pytest
import torch

from tests import border_ref as BR

pytestmark = pytest.mark.gpu

BS, CS, RADII = (1, 3), (1, 4, 5, 16), (1, 2, 7, 15, 32)


@pytest.fixture(scope="module")
def ops():
    from hrseg_amd import ops as o
    assert torch.cuda.is_available()
    return o


def tile():
    from hrseg_amd import _lib
    return _lib.border_tile()


def sizes():
    TW, TH = tile()
    # the last two span three tiles in a row: one with W % 4 != 0 (byte staging), one with W % 4 == 0 (dword staging)
    return [(1, 1), (1, 70), (70, 1), (17, 19), (TH - 1, TW + 1), (TH, TW), (TH + 1, 2 * TW + 3), (2 * TH + 1, 2 * TW + 22),
            (2 * TH + 3, 2 * TW + 8)]


def grid_cases():
    """(H, W, B, C, radius): not the full product -- every value of each axis meets at least two values of each other axis"""
    out = []
    for i, (H, W) in enumerate(sizes()):
        for j in range(3):
            out.append((H, W, BS[(i + j) % 2], CS[(i // 2 + j) % 4], RADII[(i + 2 * j) % 5]))
    for j, r in enumerate(RADII):                    # every radius at every channel count somewhere, on a two-tile image
        out.append((21, 75, BS[j % 2], CS[(j // 2 + 2) % 4], r))
    return out


def test_the_grid_covers_every_axis():
    cases = grid_cases()
    axes = {"size": lambda c: c[:2], "B": lambda c: c[2], "C": lambda c: c[3], "radius": lambda c: c[4]}
    assert {c[2] for c in cases} == set(BS) and {c[3] for c in cases} == set(CS) and {c[4] for c in cases} == set(RADII)
    assert {c[:2] for c in cases} >= set(sizes()) and max(max(c[:2]) for c in cases) < 200
    assert any(W % 4 and W > 2 * tile()[0] for _, W, *_ in cases) and any(W % 4 == 0 and W > 2 * tile()[0] for _, W, *_ in cases)
    for a, fa in axes.items():
        for value in {fa(c) for c in cases}:
            for b, fb in axes.items():
                if a != b:
                    assert len({fb(c) for c in cases if fa(c) == value}) >= 2, (a, value, b)


def run(ops, t, radius, w0=10.0, sigma=None):
    """t (numpy [B,C,H,W]) through the device and the reference -> (labels, v, d2) of the reference, after exact comparison"""
    lut = BR.table(w0, sigma if sigma is not None else max(radius / 3.0, 0.5), radius)
    ref_labels, ref_v, ref_d2 = BR.weight_map(t, radius, lut)
    td, lutd = torch.from_numpy(t).cuda(), torch.from_numpy(lut).cuda()
    labels, v, d2 = ops.border_weights(td, radius, lutd, want_d2=True)
    what = (t.shape, radius)
    assert labels.dtype == torch.uint8 and v.dtype == torch.float32 and d2.dtype == torch.int32
    assert torch.equal(labels.cpu(), torch.from_numpy(ref_labels)), what
    assert torch.equal(d2.cpu(), torch.from_numpy(ref_d2)), what
    assert torch.equal(v.cpu().view(torch.int32), torch.from_numpy(ref_v).view(torch.int32)), what
    labels2, v2 = ops.border_weights(td, radius, lutd)                 # d2 = NULL: the same two maps
    assert torch.equal(labels2, labels) and torch.equal(v2.view(torch.int32), v.view(torch.int32)), what
    return ref_labels, ref_v, ref_d2


@pytest.mark.parametrize("H,W,B,C,radius", grid_cases())
def test_voronoi_blobs(ops, H, W, B, C, radius):
    lab = BR.voronoi(B, C, H, W, seed=H * 1000 + W + radius, nseeds=6)
    void = np.random.default_rng(radius).random((B, H, W)) < 0.05
    run(ops, BR.planes(lab, C, void=void), radius)


@pytest.mark.parametrize("H,W", [(17, 19), (1, 70), (33, 150)])
def test_checkerboard(ops, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    for C, radius in ((1, 1), (4, 7), (16, 32)):
        lab = np.broadcast_to(np.where((yy + xx) % 2 == 0, 0, C), (2, H, W))        # channel 0 on / nothing on
        _, v, d2 = run(ops, BR.planes(lab, C), radius, sigma=1.0)
        assert (d2 == 1).all() and (v == BR.table(10.0, 1.0, radius)[1]).all()


@pytest.mark.parametrize("H,W", [(1, 1), (16, 64), (40, 200)])
def test_uniform_image_takes_the_early_out(ops, H, W):
    for C, radius in ((1, 2), (5, 15), (16, 32)):
        labels, v, d2 = run(ops, np.ones((3, C, H, W), dtype=np.float32), radius)
        assert (labels == 0).all() and (d2 == 0).all() and (v == np.float32(1.0)).all()


@pytest.mark.parametrize("corner", [(0, 0), (0, -1), (-1, 0), (-1, -1)])
def test_one_pixel_in_a_corner_and_the_ring_at_the_radius(ops, corner):
    H, W, radius = 40, 70, 15
    lab = np.zeros((1, H, W), dtype=np.int64)
    lab[0][corner] = 2
    _, _, d2 = run(ops, BR.planes(lab, 4), radius)
    cy, cx = corner[0] % H, corner[1] % W
    yy, xx = np.mgrid[0:H, 0:W]
    dist = (yy - cy) ** 2 + (xx - cx) ** 2
    want = np.where(dist <= radius * radius, dist, 0)
    want[cy, cx] = 1                               # the odd pixel itself: its neighbours are the other label
    assert np.array_equal(d2[0], want)
    assert d2[0][(dist == 225)].tolist() == [225] * int((dist == 225).sum()) and (dist == 225).sum() >= 3      # (15,0), (0,15), (9,12), (12,9)
    assert (d2[0][dist > 225] == 0).all()


def test_void_stripes_between_two_labels(ops):
    H, W, radius = 20, 90, 7
    lab = np.zeros((2, H, W), dtype=np.int64)
    void = np.zeros((2, H, W), dtype=bool)
    for x0 in range(10, W, 20):                    # ... 0 | void x 3 | 1 | void x 3 | 0 ...
        lab[:, :, x0:x0 + 10] = 1
        void[:, :, x0 - 3:x0] = True
        void[:, :, x0 + 10:x0 + 13] = True
    labels, v, d2 = run(ops, BR.planes(lab, 2, void=void), radius)
    assert (labels[void] == 255).all() and (d2[void] == 0).all() and (v[void] == np.float32(1.0)).all()
    assert d2[0, 5, 6] == 16 and d2[0, 5, 10] == 16       # across the gap: 4 columns away on either side
    assert (d2[~void] > 0).sum() > 0 and d2[0, 5, 2] == 0


def test_first_channel_wins_and_nothing_on_is_label_c(ops):
    rng = np.random.default_rng(5)
    B, C, H, W = 2, 5, 19, 67
    t = BR.planes(BR.voronoi(B, C, H, W, seed=3), C)
    both = rng.random((B, H, W)) < 0.3
    t[:, 1][both] = 1.0
    t[:, 3][both] = 1.0                            # two (or three) channels on at one pixel
    labels, _, _ = run(ops, t, 7)
    assert (labels[both] <= 1).all()
    mix = rng.integers(-1, 1, (B, C, H, W)).astype(np.float32)          # -1 / 0 only: nothing is on anywhere
    labels, _, d2 = run(ops, mix, 7)
    assert set(np.unique(labels)) <= {C, 255} and (d2 == 0).all()


def test_a_nan_target_is_not_on_and_not_void(ops):
    B, C, H, W = 1, 4, 18, 66
    t = BR.planes(np.zeros((B, H, W), dtype=np.int64), C)
    t[0, 0, 9, 30] = np.nan                        # channel 0 was on: now nothing is -> label C, a border around it
    t[0, :, 3, 3] = -1.0
    t[0, 2, 3, 3] = np.nan                         # every other channel -1: still not void
    labels, _, d2 = run(ops, t, 2)
    assert labels[0, 9, 30] == C and labels[0, 3, 3] == C and d2[0, 9, 31] == 1 and d2[0, 3, 3] == 1


def test_images_of_a_batch_do_not_see_each_other(ops):
    B, C, H, W = 3, 4, 33, 70
    lab = BR.voronoi(B, C, H, W, seed=9, nseeds=7)
    lab[1] = 2                                     # a uniform image between two busy ones
    _, _, d2 = run(ops, BR.planes(lab, C), 32)
    assert (d2[1] == 0).all() and (d2[0] > 0).any() and (d2[2] > 0).any()
    alone = run(ops, BR.planes(lab[2:3], C), 32)[2]
    assert np.array_equal(alone[0], d2[2])


def test_a_border_on_every_tile_edge(ops):
    TW, TH = tile()
    H, W = 3 * TH + 1, 2 * TW + 3
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.broadcast_to((yy // TH + xx // TW) % 2, (2, H, W))
    for radius in (1, 7, 32):
        run(ops, BR.planes(lab, 4), radius)


def test_two_calls_give_the_same_bytes_and_count_two_launches(ops):
    from hrseg_amd import _lib
    t = torch.from_numpy(BR.planes(BR.voronoi(3, 5, 50, 150, seed=1), 5)).cuda()
    lut = torch.from_numpy(BR.table(10.0, 5.0, 15)).cuda()
    _lib.launch_count("border_weights", reset=True)
    a = ops.border_weights(t, 15, lut, want_d2=True)
    n1 = _lib.launch_count("border_weights")
    b = ops.border_weights(t, 15, lut, want_d2=True)
    n2 = _lib.launch_count("border_weights", reset=True)
    assert 1 <= n1 <= 2 and n2 - n1 == n1
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def test_border_weights_object(ops):
    from hrseg_amd.Metrics.border import BorderWeights
    bw = BorderWeights(10.0, 2.0, 5)
    t = BR.planes(BR.voronoi(2, 4, 30, 70, seed=4), 4)
    ref_labels, ref_v, _ = BR.weight_map(t, 5, bw.table())
    v = bw(torch.from_numpy(t).cuda())
    assert v is bw.last and tuple(v.shape) == (2, 30, 70) and bw.lut("cuda:0") is bw.lut(torch.device("cuda:0"))
    assert torch.equal(v.cpu().view(torch.int32), torch.from_numpy(ref_v).view(torch.int32))
    assert torch.equal(bw.labels.cpu(), torch.from_numpy(ref_labels))
    for bad, what in ((dict(radius=0), "radius"), (dict(radius=33), "radius")):
        with pytest.raises(ValueError, match=what):
            ops.border_weights(torch.from_numpy(t).cuda(), bad["radius"], bw.lut("cuda:0"))
    with pytest.raises(ValueError, match="lut has"):
        ops.border_weights(torch.from_numpy(t).cuda(), 4, bw.lut("cuda:0"))
