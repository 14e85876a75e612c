"""Host: the numpy restatement of PIL's 8-bit resampling (tests/preprocess_ref.py) against PIL's recorded outputs
(tests/golden/preprocess_pil.safetensors, tools/record_preprocess_golden.py) and, where PIL imports, against PIL itself; the plans,
coefficient tables, job rows and input checks of vtp_amd.Preprocess.  Nothing here needs a GPU.  Equality is bit equality: a
rounded integer has no tolerance."""
import os

import numpy as np
import pytest
import torch

import preprocess_ref as R
from vtp_amd import preprocess as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(R.cases())


@pytest.fixture(scope="module")
def fixture():
    from safetensors.numpy import load_file
    return load_file(os.path.join(ROOT, "tests", "golden", "preprocess_pil.safetensors"))


@pytest.fixture(scope="module")
def expected():
    return {name: R.expected(case) for name, case in R.cases().items()}


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def test_the_fixture_holds_every_case(fixture):
    want = {f"{name}.{i}" for name, case in R.cases().items() for i in range(len(case["images"]))}
    assert set(fixture) == want and len(want) == 57


def test_the_cases_are_the_ones_that_can_go_wrong(expected):
    c = R.cases()
    assert len(c) == 3 * len(R.RESIZES) + 5
    assert [x.shape[:2] for x in c["center_crop"]["images"]] == R.CC_SOURCES and c["zero_shot"]["images"] is c["center_crop"]["images"]
    assert (0, 0, 40, 52) in c["probe_train"]["boxes"] and any(b[2:] == (1, 1) for b in c["probe_train"]["boxes"])
    assert len(c["probe_train"]["boxes"]) == 8 and any(c["probe_train"]["flips"]) and not all(c["probe_train"]["flips"])
    for name in ("resize_17x23_to_40x31_bicubic", "resize_8x8_to_16x16_bicubic", "center_crop", "probe_eval", "probe_train"):
        before = list(R.CLAMPED)  # the bicubic overshoot reaches both ends of the clamp
        R.expected(c[name])
        assert R.CLAMPED[0] > before[0] and R.CLAMPED[1] > before[1], name


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_recorded_pil_output(fixture, expected, name):
    for i, e in enumerate(expected[name]):
        assert _same(e, fixture[f"{name}.{i}"]), (name, i)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_live_pil(expected, name):
    try:
        import PIL  # noqa: F401
    except ImportError:
        pytest.skip("PIL is not installed: the recorded outputs pin the restatement")
    for i, (e, p) in enumerate(zip(expected[name], R.pil_expected(R.cases()[name]))):
        assert _same(e, p), (name, i)


def test_restatement_equals_the_tokenizers_center_crop_arr(expected):
    try:
        from PIL import Image
    except ImportError:
        pytest.skip("PIL is not installed")
    from vtp_amd.tokenizer import center_crop_arr
    for img, e in zip(R.cases()["center_crop"]["images"], expected["center_crop"]):
        assert _same(np.asarray(center_crop_arr(Image.fromarray(img), R.S)), e)


@pytest.mark.parametrize("name", NAMES)
def test_job_rows_run_in_numpy_equal_the_restatement(expected, name):
    """the layout the device gets (job rows, tables, packed bytes), walked by a numpy copy of the kernels"""
    case = R.cases()[name]
    pp, plans = R.plans_for(P, case)
    pk = pp.pack(case["images"], plans)
    assert _same(R.run_jobs(pk), np.stack(expected[name]))


# ---- plans ----------------------------------------------------------------------------------------------------------------------
def test_plans_worked_examples():
    p = P.plan_center_crop(375, 500, 256)
    assert p.ops == (("resize", P.BICUBIC, 256, 341), ("crop", 0, 42, 256, 256)) and p.out_size() == (256, 256)
    p = P.plan_probe_eval(375, 500, 256, 224)
    assert p.ops == (("resize", P.BICUBIC, 256, 341), ("crop", 16, 58, 224, 224))  # round(58.5) is 58
    assert P.plan_zero_shot(375, 500, 256).ops == (("resize", P.BILINEAR, 256, 256),)
    p = P.plan_resized_crop(40, 52, (3, 5, 20, 30), 16, flip=True)
    assert p.ops == (("crop", 3, 5, 20, 30), ("resize", P.BICUBIC, 16, 16)) and p.flip
    assert P.plan_center_crop(1500, 2000, 256).ops[:2] == (("resize", P.BOX, 750, 1000), ("resize", P.BOX, 375, 500))


def test_plans_halvings_and_bankers_rounding():
    pp = P.Preprocess.center_crop(R.S)
    assert [p.halvings() for p in pp.plan(R.CC_SOURCES)] == R.CC_HALVINGS
    assert pp.plan([(67, 130)])[0].ops[-2:] == (("resize", P.BICUBIC, 16, 32), ("crop", 0, 8, 16, 16))  # the bicubic step is the identity
    # 11 * 12 / 8 = 16.5 rounds to 16 (half to even), not 17;  9 * 1.5 = 13.5 rounds to 14
    assert P.plan_center_crop(8, 11, 12).ops[0] == ("resize", P.BICUBIC, 12, 16)
    assert P.plan_center_crop(9, 8, 12).ops[0] == ("resize", P.BICUBIC, 14, 12)
    # probe_eval(20, 16): 30 x 47 -> 20 x 31, left = round(7.5) = 8;  20 x 25 -> 20 x 25, left = round(4.5) = 4
    assert [p.ops for p in P.Preprocess.probe_eval(20, 16).plan([(30, 47), (20, 25)])] == [
        (("resize", P.BICUBIC, 20, 31), ("crop", 2, 8, 16, 16)), (("resize", P.BICUBIC, 20, 25), ("crop", 2, 4, 16, 16))]


def test_probe_train_draw_repeats_from_state_dict():
    from vtp_amd.augment import _box
    pp = P.Preprocess.probe_train(16, seed=3, rank=1)
    sizes = [(40, 52), (17, 90), (300, 211)] * 3
    pp.plan(sizes)
    sd = pp.state_dict()
    a = pp.plan(sizes)
    other = P.Preprocess.probe_train(16, seed=0, rank=0)
    other.load_state_dict(sd)
    assert other.plan(sizes) == a and pp.plan(sizes) != a
    assert any(p.flip for p in a) and not all(p.flip for p in a)
    rng = np.random.default_rng([5, 2])  # the stream: get_params' box, then one random() for the flip, image by image
    want = []
    for H, W in sizes:
        box = _box(rng, H, W, (0.08, 1.0), (3 / 4, 4 / 3))
        want.append(P.plan_resized_crop(H, W, box, 16, rng.random() < 0.5))
    assert P.Preprocess.probe_train(16, seed=5, rank=2).plan(sizes) == want
    for p in want:
        assert p.ops[0][0] == "crop" and p.out_size() == (16, 16)


# ---- coefficient tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [P.BOX, P.BILINEAR, P.BICUBIC])
def test_coefficient_tables(filt):
    name = {v: k for k, v in P.FILTER_NAMES.items()}[filt]
    for size_in, out in [(53, 16), (23, 31), (95, 7), (8, 16), (300, 24), (211, 17), (1, 4), (9, 4), (2000, 256), (64, 32)]:
        xmin, n, K = P.coeffs(size_in, 0, size_in, out, filt)
        assert xmin.dtype == n.dtype == K.dtype == np.int32 and K.shape[0] == out
        assert (n >= 1).all() and (xmin >= 0).all() and (xmin + n <= size_in).all() and (n <= K.shape[1]).all()
        assert (np.abs(K.astype(np.int64).sum(1) - (1 << 22)) <= n).all()      # each coefficient is rounded once
        assert all((K[i, n[i]:] == 0).all() for i in range(out))
        assert (np.abs(K.astype(np.int64)).sum(1) <= 1.3 * (1 << 22)).all()    # |acc| < 2^31
        rx, rn, rK = R.coeffs(size_in, 0, size_in, out, name)                  # the restatement's own loop
        assert np.array_equal(xmin, rx) and np.array_equal(n, rn) and np.array_equal(K, rK)
    assert P.coeffs(64, 0, 64, 32, P.BOX)[2].tolist() == [[1 << 21, 1 << 21, 0]] * 32


def test_identity_table():
    xmin, n, K = P.coeffs(7, 0, 7, 7, P.IDENTITY)
    assert xmin.tolist() == list(range(7)) and n.tolist() == [1] * 7 and K.tolist() == [[1 << 22]] * 7
    assert all(((1 << 21) + p * (1 << 22)) >> 22 == p for p in range(256))
    with pytest.raises(ValueError):
        P.coeffs(7, 0, 7, 8, P.IDENTITY)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_bad_images_are_refused_on_the_host():
    pp = P.Preprocess.zero_shot(16)
    ok = np.zeros((9, 7, 3), np.uint8)
    for bad, match in [(np.zeros((9, 7, 3), np.float32), "uint8"), (torch.zeros(9, 7, 3), "uint8"), (np.zeros((9, 7), np.uint8), "H, W, 3"),
                       (np.zeros((9, 7, 4), np.uint8), "H, W, 3"), (np.zeros((0, 7, 3), np.uint8), "H, W, 3"),
                       (np.zeros((9, 0, 3), np.uint8), "H, W, 3"), ("x", "uint8")]:
        with pytest.raises(ValueError, match=match):
            pp([ok, bad])
    with pytest.raises(ValueError, match="empty"):
        pp.pack([], [])
    with pytest.raises(ValueError, match="plans"):
        pp.pack([ok, ok], pp.plan([(9, 7)]))
    with pytest.raises(ValueError, match="its plan is for"):
        pp.pack([ok], pp.plan([(7, 9)]))
    with pytest.raises(ValueError, match="the output is"):
        pp.pack([ok], P.Preprocess.zero_shot(8).plan([(9, 7)]))
    with pytest.raises(ValueError, match="H, W >= 1"):
        pp.plan([(0, 4)])
    with pytest.raises(ValueError):
        P.Preprocess.zero_shot(0)
    with pytest.raises(ValueError, match="std"):
        P.Preprocess.zero_shot(16, std=(1.0, 0.0, 1.0))


def test_a_crop_larger_than_the_resized_image_is_refused():
    with pytest.raises(ValueError, match="larger than the resized image"):
        P.Preprocess.probe_eval(resize=16, crop=20).plan([(30, 47)])
    with pytest.raises(ValueError, match="larger than the resized image"):
        P.plan_probe_eval(100, 10, 20, 21)           # 200 x 20: the crop fits one axis only
    pp = P.Preprocess.probe_train(16)
    img = np.zeros((40, 52, 3), np.uint8)
    for box in [(0, 0, 41, 52), (30, 0, 11, 5), (0, -1, 4, 4), (0, 0, 0, 4)]:
        with pytest.raises(ValueError, match="does not lie inside"):
            pp.pack([img], [P.plan_resized_crop(40, 52, box, 16)])
    with pytest.raises(ValueError, match="bad resize"):
        pp.pack([img], [P.Plan(40, 52, (("resize", 7, 16, 16),))])


def test_job_rows_that_leave_their_buffers_are_refused():
    case = R.cases()["center_crop"]
    pp, plans = R.plans_for(P, case)
    pk = pp.pack(case["images"], plans)
    args = (pk.src.numel(), pk.scratch_len, pk.B, pk.out_h, pk.out_w)
    P.check_jobs(pk.jobs, pk.tab, pk.launches, *args)
    n = len(pk.jobs)

    def broken(row, slot, value, tab=None, launches=None):
        jobs = pk.jobs.copy()
        if row is not None:
            jobs[row, slot] = value
        with pytest.raises(ValueError):
            P.check_jobs(jobs, pk.tab if tab is None else tab, pk.launches if launches is None else launches, *args)

    first_scratch = int(np.nonzero(pk.jobs[:, P.J_FLAGS] & P.F_SCRATCH)[0][0])
    broken(0, P.J_SRC, pk.src.numel() - 10)          # reads past the source bytes
    broken(0, P.J_SRC, -1)
    broken(first_scratch, P.J_SRC, pk.scratch_len)   # reads past the scratch
    broken(0, P.J_DST, pk.scratch_len - 1)           # writes past the scratch
    broken(0, P.J_DST, -3)
    broken(0, P.J_TS, 10 ** 6)
    broken(0, P.J_SY, 10 ** 6)
    broken(0, P.J_OH, 10 ** 4)
    broken(0, P.J_OW, 0)
    broken(0, P.J_BND, len(pk.tab) - 1)              # the table entry outside the table buffer
    broken(0, P.J_COEF, len(pk.tab) - 1)
    broken(0, P.J_BND, -2)
    broken(0, P.J_SUB, 1)                            # a tap in front of the buffer
    broken(0, P.J_KSIZE, 1)                          # more taps than coefficients per entry
    broken(1, P.J_BLOCK, 0)                          # not the numbering the kernels search
    broken(0, P.J_FLAGS, 8)
    broken(n - 1, P.J_DST, 0)                        # two endings for image 0, none for the last
    broken(n - 1, P.J_OH, 15)
    broken(first_scratch, P.J_SRC, int(pk.jobs[first_scratch, P.J_DST]))  # reads what it writes
    t = pk.tab.copy()
    b = int(pk.jobs[0, P.J_BND])
    t[b + 1] = 0                                     # a tap count of zero
    broken(None, 0, 0, tab=t)
    t = pk.tab.copy()
    t[b] = 10 ** 6                                   # a first tap far outside
    broken(None, 0, 0, tab=t)
    ln = pk.launches.copy()
    ln[0, 2] += 1                                    # a block with no job
    broken(None, 0, 0, launches=ln)
    ln = pk.launches.copy()
    ln[-1, 1] -= 1
    broken(None, 0, 0, launches=ln)
    with pytest.raises(ValueError):
        P.check_jobs(pk.jobs.astype(np.int32), pk.tab, pk.launches, *args)
    with pytest.raises(ValueError):
        P.check_jobs(pk.jobs, pk.tab, pk.launches, pk.src.numel() // 2, *args[1:])  # fewer source bytes than the jobs read


def test_apply_raises_without_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    pp = P.Preprocess.zero_shot(16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pp([np.zeros((9, 7, 3), np.uint8)])
    with pytest.raises(ValueError):                  # the checks come first, GPU or not
        pp([np.zeros((9, 7, 3), np.int16)])


def test_public_surface():
    import vtp_amd
    assert vtp_amd.Preprocess is P.Preprocess
    from vtp_amd import _lib
    assert "vtp_preprocess" in _lib.SIGNATURES
    from vtp_amd.tokenizer import VTP_Tokenizer
    assert callable(VTP_Tokenizer.images_from_decoded)
