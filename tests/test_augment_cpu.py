"""Device input pipeline, the parts that need no GPU: the parameter sampler and table, the torch-CPU restatement of the
reference's transforms (tests/augment_ref.py) on known answers, and the ragged uint8 collate of the loader."""
import numpy as np
import pytest
import torch

from tests import augment_ref as R


def _aug():
    from hrseg_amd.Data import augment
    return augment


def test_sampler_ranges_and_rates():
    A = _aug()
    g = torch.Generator().manual_seed(123)
    n = 10000
    p = A.sample_params(n, g, hflip=True, vflip=False, affine=True)
    assert p["order"].shape == (n, 4)
    assert bool((p["order"].sort(dim=1).values == torch.arange(4)).all()), "every order is a permutation of 0..3"
    assert len({tuple(o) for o in p["order"].tolist()}) == 24
    for key, (lo, hi) in [("sigma", A.SIGMA), ("brightness", A.BRIGHTNESS), ("contrast", A.CONTRAST),
                          ("saturation", A.SATURATION), ("hue", A.HUE), ("angle", A.ANGLE), ("tx", A.TRANSLATE),
                          ("ty", A.TRANSLATE), ("scale", A.SCALE), ("shear", A.SHEAR)]:
        v = p[key]
        assert float(v.min()) >= lo and float(v.max()) <= hi, key
        assert float(v.min()) < lo + 0.01 * (hi - lo) and float(v.max()) > hi - 0.01 * (hi - lo), key
    assert abs(float(p["hflip"].double().mean()) - 0.5) <= 0.02
    assert not bool(p["vflip"].any()) and bool(p["affine"].all())
    q = A.sample_params(n, torch.Generator().manual_seed(123), vflip=True, affine=False)
    assert abs(float(q["vflip"].double().mean()) - 0.5) <= 0.02 and not bool(q["affine"].any())


def test_blur_taps_equal_the_formula():
    A = _aug()
    for sigma in (0.001, 0.37, 1.0, 2.0):
        t = torch.linspace(-12, 12, 25)
        k = torch.exp(-0.5 * (t / sigma) ** 2)
        k = k / k.sum()
        assert torch.equal(A.blur_taps(sigma), k)
        assert torch.equal(R.gaussian_kernel1d(sigma), k)
    g = torch.Generator().manual_seed(5)
    p = A.sample_params(3, g)
    table = A.pack_params(p, 62)
    for i in range(3):
        assert torch.equal(table[i, A.P_TAPS:A.P_TAPS + 25], A.blur_taps(float(p["sigma"][i])))


def test_param_table_matches_the_restated_affine_grid():
    A = _aug()
    p = A.sample_params(4, torch.Generator().manual_seed(9))
    S = 62
    table = A.pack_params(p, S)
    for i in range(4):
        d = R.sample_dict(p, i)
        m = R.inverse_affine_matrix(d["angle"], (d["tx"], d["ty"]), d["scale"], d["shear"])
        assert m == A.inverse_affine_matrix(d["angle"], d["tx"], d["ty"], d["scale"], d["shear"])
        theta = torch.tensor(m, dtype=torch.float32).reshape(1, 2, 3)
        rescaled = (theta.transpose(1, 2) / torch.tensor([0.5 * S, 0.5 * S])).reshape(6)
        assert torch.equal(table[i, A.P_THETA:A.P_THETA + 6], rescaled)
        assert table[i, A.P_ORDER:A.P_ORDER + 4].tolist() == [float(v) for v in d["order"]]
        flags = int(table[i, A.P_FLAGS])
        assert bool(flags & A.HFLIP) == d["hflip"] and bool(flags & A.WARP) and not flags & A.VFLIP


def _pattern(S=31, seed=0):
    return torch.rand(3, S, S, generator=torch.Generator().manual_seed(seed))


def test_blur_known_answers():
    const = torch.full((3, 40, 40), 0.3)
    assert float((R.gaussian_blur(const, 1.7) - 0.3).abs().max()) < 1e-6
    x = _pattern(40)
    assert torch.equal(R.gaussian_blur(x, 0.001), x)


def test_jitter_identity_and_hsv_round_trip():
    x = _pattern(33, 1)
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2]):
        y = R.color_jitter(x, order, 1.0, 1.0, 1.0, 0.0)
        assert float((y - x).abs().max()) <= 1e-6
    back = R.hsv2rgb(R.rgb2hsv(x))
    assert float((back - x).abs().max()) <= 1e-6
    gray = torch.full((3, 4, 4), 0.25)
    assert torch.equal(R.hsv2rgb(R.rgb2hsv(gray)), gray)


def test_integer_translation_moves_content_right_and_down():
    S = 31
    x = _pattern(S, 2)
    tx, ty = 3, 2
    m = R.inverse_affine_matrix(0.0, (tx, ty), 1.0, 0.0)
    out, _ = R.affine_nearest(x, m, [-1.0] * 3)
    assert torch.equal(out[:, ty:, tx:], x[:, :S - ty, :S - tx])
    assert bool((out[:, :ty, :] == -1).all()) and bool((out[:, :, :tx] == -1).all())


def test_angle_90_turns_clockwise():
    S = 9
    x = torch.zeros(1, S, S)
    x[0, 4, 6:] = 1.0          # a bar right of the centre ...
    x[0, 1, 4] = 2.0           # ... and a dot above it: asymmetric
    m = R.inverse_affine_matrix(90.0, (0.0, 0.0), 1.0, 0.0)
    out, _ = R.affine_nearest(x, m, [0.0])
    want = torch.rot90(x, k=-1, dims=(1, 2))      # clockwise on screen (rows grow downwards)
    assert torch.equal(out, want)
    assert bool((out[0, 6:, 4] == 1).all()), "the right-hand bar points down after a clockwise turn"
    assert float(out[0, 4, 7]) == 2.0, "the dot above the centre ends up on its right"


def _write_png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)


def test_png_pairs_collate_into_a_ragged_batch(tmp_path):
    from hrseg_amd.Data.loader import DeviceAugmentLoader, PngPairDataset, ragged_collate
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (17, 23, 3), dtype=np.uint8), rng.integers(0, 256, (9, 5), dtype=np.uint8)]
    labs = [rng.choice(np.array([0, 212, 255], dtype=np.uint8), size=(17, 23)), np.full((9, 5), 127, np.uint8)]
    ip, tp = [], []
    for i, (a, b) in enumerate(zip(imgs, labs)):
        ip.append(str(tmp_path / f"img{i}.png"))
        tp.append(str(tmp_path / f"lab{i}.png"))
        _write_png(ip[-1], a)
        _write_png(tp[-1], b)
    ds = PngPairDataset(ip, tp)
    assert len(ds) == 2
    for i in range(2):
        a, b = ds[i]
        assert a.dtype == np.uint8 and np.array_equal(a, imgs[i]) and np.array_equal(b, labs[i])
    batch = ragged_collate([ds[0], ds[1]])
    assert len(batch) == 2
    assert batch.desc.tolist() == [[0, 17, 23, 3], [17 * 23 * 3, 9, 5, 1]]
    assert batch.ldesc.tolist() == [[0, 17, 23, 1], [17 * 23, 9, 5, 1]]
    assert batch.src.dtype == torch.uint8 and batch.src.numel() == 17 * 23 * 3 + 45
    assert torch.equal(batch.src[:17 * 23 * 3], torch.from_numpy(imgs[0]).reshape(-1))
    assert torch.equal(batch.label[17 * 23:], torch.from_numpy(labs[1]).reshape(-1))

    class _Stub:
        device = torch.device("cpu")
    loader = DeviceAugmentLoader(ds, batch_size=2, shuffle=False, num_workers=0, augment=_Stub())
    assert len(loader) == 1 and loader.dataset is ds
    host = next(iter(loader.loader))
    assert host.desc_host.tolist() == batch.desc.tolist() and torch.equal(host.src, batch.src)
    with pytest.raises(ValueError):
        ragged_collate([(np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4), np.uint8))])
