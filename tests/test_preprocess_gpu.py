"""GPU: the preprocessing kernels (csrc/preprocess.hip: vtp_preprocess) and vtp_amd.Preprocess against the numpy restatement of
PIL's 8-bit resampling (tests/preprocess_ref.py, itself pinned to PIL by tests/test_preprocess_host.py).

For every case of preprocess_ref.cases() -- each filter up- and down-sampling, a 16-fold reduction, a skipped axis, width 1 and
height 1, the four chains as ragged batches, flip off and on:
  the uint8 output is torch.equal to the restatement's (a rounded integer has no tolerance);
  the f32 output is torch.equal to ops.u8_to_images of that uint8 output (padded to a width that kernel takes);
  the outputs are pre-filled with NaN / a byte sentinel and the scratch with a byte sentinel, in two runs with two different
  sentinels: every element is written, nothing depends on what the scratch held, and the two runs are bit-identical;
  the batch equals the same images run one at a time (the ragged job table).
Invalid input is tested on the host (test_preprocess_host.py): nothing here hands a kernel a bad table."""
import os

import numpy as np
import pytest
import torch

import preprocess_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(R.cases())


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _launch(pp, images, plans, sentinel):
    """pack on the host, then the launches through vtp_amd.ops with outputs and scratch pre-filled -> (f32, uint8) on the CPU"""
    from vtp_amd import ops
    pk = pp.pack(images, plans)
    out = torch.full((pk.B, 3, pk.out_h, pk.out_w), float("nan"), device=DEV)
    u8 = torch.full((pk.B, pk.out_h, pk.out_w, 3), sentinel, dtype=torch.uint8, device=DEV)
    scratch = torch.full((max(pk.scratch_len, 1),), sentinel, dtype=torch.uint8, device=DEV)
    ops.preprocess(pk.src.to(DEV), scratch, torch.from_numpy(pk.jobs.reshape(-1)).to(DEV), torch.from_numpy(pk.tab).to(DEV), pk.launches,
                   out, u8, R.MEAN, R.STD)
    torch.cuda.synchronize()
    return out.cpu(), u8.cpu()


def _normalise(u8):
    """ops.u8_to_images of uint8 [B, h, w, 3] (CPU) -> f32 [B, 3, h, w] (CPU); that kernel takes widths that are multiples of 4"""
    from vtp_amd import ops
    B, h, w, _ = u8.shape
    wp = (w + 3) // 4 * 4
    padded = torch.zeros(B, h, wp, 3, dtype=torch.uint8)
    padded[:, :, :w] = u8
    out = torch.empty(B, 3, h, wp, device=DEV)
    ops.u8_to_images(padded.to(DEV), out, R.MEAN, R.STD, False)
    return out.cpu()[:, :, :, :w].contiguous()


@pytest.fixture(scope="module")
def runs():
    """every case once: the restatement's bytes and the kernels' outputs with sentinel 0xA5"""
    _need_gpu()
    from vtp_amd import preprocess as P
    out = {}
    for name, case in R.cases().items():
        pp, plans = R.plans_for(P, case)
        f32, u8 = _launch(pp, case["images"], plans, 0xA5)
        out[name] = {"pp": pp, "plans": plans, "f32": f32, "u8": u8, "want": torch.from_numpy(np.stack(R.expected(case)))}
    return out


@pytest.mark.parametrize("name", NAMES)
def test_bytes_equal_the_restatement(runs, name):
    r = runs[name]
    assert r["u8"].shape == r["want"].shape
    diff = int((r["u8"] != r["want"]).sum())
    print(f"PREPROCESS {name:36s} images={len(r['plans'])} bytes={r['want'].numel()} differing={diff}")
    assert torch.equal(r["u8"], r["want"]), (name, diff)


@pytest.mark.parametrize("name", NAMES)
def test_floats_equal_u8_to_images(runs, name):
    r = runs[name]
    assert torch.isfinite(r["f32"]).all(), "an output element was not written"
    assert torch.equal(r["f32"], _normalise(r["u8"]))
    assert torch.equal(r["f32"][0], torch.from_numpy(R.to_float(r["u8"][0].numpy())))  # and ToTensor + Normalize in numpy's fp32


@pytest.mark.parametrize("name", NAMES)
def test_runs_repeat_and_ignore_what_the_buffers_held(runs, name):
    r = runs[name]
    f32, u8 = _launch(r["pp"], R.cases()[name]["images"], r["plans"], 0x5A)
    assert torch.equal(u8, r["u8"]) and torch.equal(f32, r["f32"])


@pytest.mark.parametrize("name", ["center_crop", "center_crop_flip", "probe_eval", "zero_shot", "probe_train"])
def test_batch_equals_one_image_at_a_time(runs, name):
    r = runs[name]
    images = R.cases()[name]["images"]
    pp = r["pp"]
    x, u8 = pp.apply(images, r["plans"], return_u8=True)  # the public path: pinned upload, the object's own scratch
    assert x.is_cuda and u8.is_cuda and x.dtype == torch.float32 and u8.dtype == torch.uint8
    assert torch.equal(u8.cpu(), r["want"]) and torch.equal(x.cpu(), r["f32"])
    assert torch.equal(pp.apply(images, r["plans"]).cpu(), r["f32"])
    for i, (img, plan) in enumerate(zip(images, r["plans"])):
        xi, ui = pp.apply([torch.from_numpy(img)], [plan], return_u8=True)  # a CPU tensor instead of an array
        assert torch.equal(ui.cpu()[0], r["want"][i]) and torch.equal(xi.cpu()[0], r["f32"][i]), (name, i)


def test_call_plans_and_runs_without_host_synchronisation(runs):
    from vtp_amd import Preprocess
    images = R.cases()["center_crop"]["images"]
    pp = Preprocess.center_crop(R.S)
    assert torch.equal(pp(images).cpu(), runs["center_crop"]["f32"])  # warm: the scratch exists
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x, u8 = pp(images, return_u8=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(x.cpu(), runs["center_crop"]["f32"]) and torch.equal(u8.cpu(), runs["center_crop"]["want"])
    half = Preprocess.zero_shot(R.S, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))  # another normalisation
    want = runs["zero_shot"]["want"].permute(0, 3, 1, 2).float().div(255).sub(0.5).div(0.5)
    assert torch.equal(half(images).cpu(), want)
    train = Preprocess.probe_train(R.S, seed=1)  # the drawn plans run
    sd = train.state_dict()
    a = train(images)
    train.load_state_dict(sd)
    assert a.shape == (len(images), 3, R.S, R.S) and torch.isfinite(a).all() and torch.equal(train(images), a)


def test_tokenizer_images_from_decoded(golden_sd, runs):
    from oracle.ref_stubs import TINY
    from vtp_amd import VTPConfig, VTPModel, VTP_Tokenizer
    m = VTPModel(VTPConfig(**TINY))
    m.load_state_dict(golden_sd, strict=True)
    tok = VTP_Tokenizer(m, img_size=R.S, normalize_type="imagenet")
    pick = [1, 2, 4]  # one halving, two halvings, up-sampling
    images = [R.cases()["center_crop"]["images"][i] for i in pick]
    try:
        from PIL import Image
        u8 = np.stack([tok.crop_to_u8(Image.fromarray(im)) for im in images])
    except ImportError:  # no PIL on this machine: its recorded outputs
        from safetensors.numpy import load_file
        g = load_file(os.path.join(ROOT, "tests", "golden", "preprocess_pil.safetensors"))
        u8 = np.stack([g[f"center_crop.{i}"] for i in pick])
    for flip in (False, True):
        assert torch.equal(tok.images_from_decoded(images, flip=flip), tok.images_from_u8(u8, flip=flip)), flip
