"""CPU: the colour jitter of support crops (FEW_SHOT.NUM_SUPP_AUG = 3, data/datasets/coco.py:286-294, 447-452).
  * the numpy restatement tests/color_jitter_ref.py — the definition the device kernel is held to in tests/test_gpu_color_jitter.py —
    against tests/golden/color_jitter.npz (recorded through the reference's own method, tests/golden/make_golden_color_jitter.py) and
    against the installed Pillow, byte for byte;
  * dataset.FewShotCocoDataset(num_supp_aug=3): member order, order of draws, one `jitter` call per item, equal sizes inside a group,
    and that `num_supp_aug=None` changes nothing;
  * examples/train.py and the documents."""
import os

import numpy as np
import pytest

import color_jitter_ref as cj
import golden_utils as gu
from oneshotdet_amd import dataset, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, NumpyJitter = cj.CASES, cj.NumpyJitter


@pytest.fixture(scope="module")
def fixture():
    return gu.load("color_jitter.npz")


# ------------------------------------------------------------------------------------------------------------- the arithmetic
def test_fixture_holds_the_cases_and_no_more(fixture):
    assert list(fixture["names"]) == CASES
    assert sorted(fixture.keys()) == sorted(["names"] + ["%s.%s" % (n, k) for n in CASES for k in ("src", "seed", "factors", "out")])
    shapes = {n: fixture[n + ".src"].shape for n in CASES}
    assert [shapes[n] for n in CASES[:6]] == [(1, 1, 3), (2, 5, 3), (5, 2, 3), (3, 3, 3), (3, 40, 3), (37, 53, 3)]
    assert shapes["gradient127x131"] == (127, 131, 3)
    flat, low = fixture["flat.src"], fixture["lowcontrast.src"]
    assert flat.min() == flat.max() and int(low.max()) - int(low.min()) < 32
    path = os.path.join(ROOT, "tests", "golden", "color_jitter.npz")
    assert os.path.getsize(path) <= 256 * 1024
    assert os.path.getsize(path) <= max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f))
                                        for f in os.listdir(os.path.join(ROOT, "tests", "golden")) if f.startswith("case_") and f.endswith(".npz"))


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference_fixture(fixture, name):
    src, out, factors = fixture[name + ".src"], fixture[name + ".out"], fixture[name + ".factors"]
    assert src.dtype == out.dtype == np.uint8 and factors.dtype == np.float64 and factors.shape == (4,)
    # the factors are the four draws that follow np.random.seed(seed), in the order the reference makes them
    rs = np.random.RandomState(int(fixture[name + ".seed"]))
    np.testing.assert_array_equal(cj.draw_factors(rs), factors)
    assert (factors >= 0.1).all() and (factors < 2).all()
    np.testing.assert_array_equal(cj.color_jitter(src, factors), out)


def _pil_chain(a, factors):
    from PIL import Image, ImageEnhance
    im = Image.fromarray(a)
    for enh, f in zip((ImageEnhance.Color, ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Sharpness), factors):
        im = enh(im).enhance(float(f))
    return np.asarray(im)


def test_restatement_equals_the_installed_pillow():
    pytest.importorskip("PIL")
    rng = np.random.RandomState(5)
    edges = (0.1, 1.0, 2.0)
    n_bytes = 0
    for it in range(120):
        h, w = int(rng.randint(1, 34)), int(rng.randint(1, 34))
        a = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        if it % 4 == 1:
            a = (rng.randint(0, 224) + rng.randint(0, 32, (h, w, 3))).astype(np.uint8)          # low contrast
        if it % 8 == 3:
            a[:] = rng.randint(0, 256)                                                          # flat
        f = rng.uniform(0.1, 2, 4)
        if it % 2 == 0:
            f[it // 2 % 4] = edges[it // 8 % 3]                                                 # exactly 0.1, 1.0 and 2.0, at every step
        if it % 10 == 9:
            f[:] = edges[it // 10 % 3]
        if it % 6 == 5:
            f = rng.choice(np.round(np.arange(0.1, 2.05, 0.1), 1), 4)                           # short decimals: products next to integers
        np.testing.assert_array_equal(cj.color_jitter(a, f), _pil_chain(a, f), err_msg="%d x %d, factors %r" % (h, w, f))
        n_bytes += a.size
    assert n_bytes > 50000


def test_blend_branches():
    x = np.arange(256, dtype=np.uint8)
    np.testing.assert_array_equal(cj.blend(0, x, 1.0), x)
    np.testing.assert_array_equal(cj.blend(0, x, 2.0), np.minimum(2 * x.astype(int), 255))
    np.testing.assert_array_equal(cj.blend(255, x, 2.0), np.maximum(2 * x.astype(int) - 255, 0))
    np.testing.assert_array_equal(cj.blend(100, x, 0.0), np.full(256, 100))
    a = np.full((4, 5, 3), 255, dtype=np.uint8)
    np.testing.assert_array_equal(cj.color_jitter(a, [2, 2, 2, 2]), a)
    np.testing.assert_array_equal(cj.smooth(np.zeros((2, 7, 3), np.uint8) + 9), np.zeros((2, 7, 3), np.uint8) + 9)


# ------------------------------------------------------------------------------------------------------------- the dataset
class RecordingRng(object):
    """np.random.RandomState that remembers what was asked of it"""

    def __init__(self, seed):
        self.rs, self.calls, self.values = np.random.RandomState(seed), [], []

    def uniform(self, lo, hi):
        v = self.rs.uniform(lo, hi)
        self.calls.append((lo, hi))
        self.values.append(v)
        return v


def _dataset(**kw):
    coco, pix = gu.dataset_inputs()
    return dataset.FewShotCocoDataset(coco, lambda info: pix[info["id"]], is_train=True, supp_area_threshold=60.0, **kw)


@pytest.mark.parametrize("shot", [1, 2])
def test_dataset_yields_four_rows_per_support(shot):
    rng, jit = RecordingRng(11), NumpyJitter()
    ds = _dataset(shot=shot, num_supp_aug=3, jitter=jit, jitter_rng=rng)
    plain = _dataset(shot=shot, supp_aug=True)                     # the same private `random` stream: the same crops and flips
    assert ds.ids == plain.ids and ds.chosen_cats == plain.chosen_cats
    for idx in range(6):
        n_draws = len(rng.values)
        item, ref = ds[idx], plain[idx]
        supp = item["img_supp"]
        assert len(supp) == 4 * shot and item["img_neg_supp"] is supp and len(ref["img_supp"]) == 2 * shot
        assert len(jit.calls) == idx + 1                           # one call per item, all jittered members at once
        arrays, factors = jit.calls[-1]
        assert len(arrays) == 2 * shot and factors.shape == (2 * shot, 4) and factors.dtype == np.float64
        # eight draws per support: uniform(0.1, 2), the crop's four before the flip's four, one support after the other
        assert len(rng.values) == n_draws + 8 * shot and set(rng.calls) == {(0.1, 2)}
        np.testing.assert_array_equal(factors.reshape(-1), np.asarray(rng.values[n_draws:]))
        for s in range(shot):
            crop, flip, jcrop, jflip = supp[4 * s:4 * s + 4]
            np.testing.assert_array_equal(crop, ref["img_supp"][2 * s])
            np.testing.assert_array_equal(flip, ref["img_supp"][2 * s + 1])
            np.testing.assert_array_equal(flip, crop[:, ::-1])
            np.testing.assert_array_equal(arrays[2 * s], crop)
            np.testing.assert_array_equal(arrays[2 * s + 1], flip)
            # each support's OWN flip is jittered (coco.py:452 takes the first support's)
            np.testing.assert_array_equal(jcrop, cj.color_jitter(crop, factors[2 * s]))
            np.testing.assert_array_equal(jflip, cj.color_jitter(flip, factors[2 * s + 1]))
            assert not np.array_equal(jcrop, crop)
        sizes = [m.shape[:2] for m in supp]
        assert spec.group_query_sizes(sizes, 4) == sizes[::4]      # the model's equal-size rule accepts every group


def test_dataset_default_rng_is_a_private_numpy_stream():
    jit_a, jit_b = NumpyJitter(), NumpyJitter()
    a = _dataset(num_supp_aug=3, jitter=jit_a)
    np.random.seed(1)
    before = np.random.get_state()[1].copy()
    b = _dataset(num_supp_aug=3, jitter=jit_b, seed=6666)
    a[0], b[0]
    np.testing.assert_array_equal(jit_a.calls[0][1], jit_b.calls[0][1])
    np.testing.assert_array_equal(jit_a.calls[0][1].reshape(-1), np.random.RandomState(6666).uniform(0.1, 2, 8))
    np.testing.assert_array_equal(np.random.get_state()[1], before)          # the global stream is left alone ...
    g = _dataset(num_supp_aug=3, jitter=NumpyJitter(), jitter_rng=np.random)
    np.random.seed(77)
    g[0]
    np.testing.assert_array_equal(g.jitter.calls[0][1].reshape(-1), np.random.RandomState(77).uniform(0.1, 2, 8))      # ... unless asked for


@pytest.mark.parametrize("aug", [False, True])
def test_num_supp_aug_none_is_todays_dataset(aug):
    f = gu.load("dataset.npz")
    cfgs = [c for c in gu.DATASET_CONFIGS if bool(c[3]) == aug]
    assert cfgs
    name, is_train, shot, _, excl_train, excl_test, thr = cfgs[0]
    coco, pix = gu.dataset_inputs()

    def boom(*a):
        raise AssertionError("no jitter without num_supp_aug=3")
    ds = dataset.FewShotCocoDataset(coco, lambda info: pix[info["id"]], is_train=is_train, shot=shot,
                                    exclude_contiguous=excl_train if is_train else excl_test, supp_area_threshold=thr, supp_aug=aug,
                                    num_supp_aug=None, jitter=boom, jitter_rng=None)
    for idx in range(len(ds)):
        supp = ds[idx]["img_supp"]
        assert len(supp) == int(f["%s.%d.n_supp" % (name, idx)]) == shot * (2 if aug else 1)
        for k, crop in enumerate(supp):
            np.testing.assert_array_equal(crop, f["%s.%d.supp.%d" % (name, idx, k)])


@pytest.mark.parametrize("bad", [2, 4, 1, 0, -1, True, "3"])
def test_other_group_sizes_are_refused_by_name(bad):
    with pytest.raises(ValueError, match="NUM_SUPP_AUG"):
        _dataset(num_supp_aug=bad)


# ------------------------------------------------------------------------------------------------------------- example and documents
def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_example_takes_four_and_refuses_three():
    src = _read("examples", "train.py")
    assert "if supp_aug not in (1, 2, 4):" in src and "raise SystemExit(" in src
    assert "num_supp_aug=3 if supp_aug == 4 else None" in src and "supp_aug=supp_aug == 2" in src
    assert 'item["img_supp"][:supp_aug]' in src and "supp_aug=supp_aug, supp_aug_method=supp_aug_method" in src
    assert "colour" in src


def test_documents_name_the_feature():
    readme, design, integ = _read("README.md"), _read("DESIGN.md"), _read("INTEGRATION.md")
    assert "color_jitter.hip" in readme and "oneshotdet_hip_color_jitter.h" in readme
    assert "4.5n" in design and "osd_color_jitter_batch" in design and "profiles/color_jitter.md" in design
    not_built = design[design.index("Not built:"):]
    assert "colour-jitter" not in not_built[:not_built.index("\n\n")]
    assert "oneshotdet_hip_color_jitter.h" in integ and "num_supp_aug=3" in integ and "osd_color_jitter_batch" in integ
    assert os.path.exists(os.path.join(ROOT, "profiles", "color_jitter.md"))
    assert "bench_color_jitter.py" in _read("tools", "README.md") and os.path.exists(os.path.join(ROOT, "tools", "bench_color_jitter.py"))
