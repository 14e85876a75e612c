"""CPU-side checks of the linear segmentation probe (vtp_amd/segprobe.py, csrc/segprobe.hip): the fp64 restatement the GPU tests
compare against (tests/seg_ref.py) pinned to torch's own CPU ops, mIoU on a hand-written confusion matrix, the argument checks of
the three entry points, the register report of the kernels, and the export / CPU behaviour of the class."""
import ctypes
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

import seg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_restatement_matches_torch_cpu_ops_in_fp64(i):
    """upsampled logits == F.interpolate(bilinear, align_corners=False), loss == F.cross_entropy(ignore_index=255), G == the
    autograd gradient through both, 1e-12 relative, on every shape of the GPU tests"""
    B, h, w, Hl, Wl, C, K = R.CASES[i]
    X, W, b, labels = R.make_case(i, 1)
    z = (X.double() @ W.double().T + b.double()).view(B, h, w, C)
    r = R.loss_and_grad(z, labels)
    zt = z.permute(0, 3, 1, 2).clone().requires_grad_(True)
    up_t = F.interpolate(zt, size=(Hl, Wl), mode="bilinear", align_corners=False)
    assert float((r["up"].permute(0, 3, 1, 2) - up_t.detach()).abs().max()) <= 1e-12 * float(up_t.detach().abs().max())
    ok, oor = R.valid_mask(labels, C)
    assert r["n_valid"] == int(ok.sum()) > 0 and r["out_of_range"] == int(oor.sum())
    if i in (1, 2, 5):
        assert r["out_of_range"] > 0 and int((labels == 255).sum()) > 0  # the draw holds every kind of label
    target = torch.where(ok, labels.long(), torch.full_like(labels.long(), 255))  # torch refuses a target >= C: ours skips and counts it
    loss_t = F.cross_entropy(up_t, target, ignore_index=255)
    assert r["loss"] == pytest.approx(float(loss_t), rel=1e-12)
    (g_t,) = torch.autograd.grad(loss_t, zt)
    g_t = g_t.permute(0, 2, 3, 1)
    assert float((r["G"] - g_t).norm()) <= 1e-12 * float(g_t.norm())
    assert float(r["G"].sum(-1).abs().max()) <= 1e-15  # softmax minus one-hot sums to zero in every cell


def test_restatement_without_a_valid_pixel():
    X, W, b, labels = R.make_case(3, 1, all_ignored=True)
    B, h, w, Hl, Wl, C, K = R.CASES[3]
    r = R.loss_and_grad((X @ W.T + b).view(B, h, w, C), labels)
    assert r["loss"] == 0.0 and r["n_valid"] == 0 and not bool(r["G"].any())


def test_restatement_taps_clamp_at_both_edges():
    i0, i1, l0, l1 = R.taps(32, 2)  # scale 16: pixels 0..7 clamp to cell 0, pixels 24..31 sit on cell 1 twice
    assert i0[:8].tolist() == [0] * 8 and bool((l1[:8] == 0).all())
    assert i0[24:].tolist() == [1] * 8 and i1[24:].tolist() == [1] * 8
    assert float(R.tap_matrix(32, 2).sum(1).sub(1).abs().max()) <= 1e-15
    assert R.tap_matrix(2, 7).sum(0).eq(0).tolist() == [True, False, False, True, False, False, True]  # cells no pixel touches


def test_miou_on_a_hand_written_confusion_matrix():
    from vtp_amd.segprobe import miou_from_confusion
    #                 pred 0  1  2  3
    conf = torch.tensor([[5, 1, 0, 0],     # IoU 0 = 5 / (5 + 1 + 2)
                         [2, 3, 4, 0],     # IoU 1 = 3 / (3 + 2 + 4 + 1)
                         [0, 0, 0, 0],     # class 2: never a target but predicted 4 times: IoU 0 / 4 = 0, and it counts
                         [0, 0, 0, 0]])    # class 3: absent from targets and predictions alike: left out of the mean
    want = [5 / 8, 3 / 10, 0.0]
    m, iou, acc = R.miou(conf)
    assert iou[:3].tolist() == pytest.approx(want, rel=1e-15) and bool(iou[3].isnan())
    assert m == pytest.approx(sum(want) / 3, rel=1e-15) and acc == pytest.approx(8 / 15, rel=1e-15)
    m2, iou2, acc2 = miou_from_confusion(torch.stack([conf, torch.zeros_like(conf)]))
    assert float(m2[0]) == pytest.approx(m, rel=1e-15) and float(acc2[0]) == pytest.approx(acc, rel=1e-15)
    assert iou2[0, :3].tolist() == pytest.approx(want, rel=1e-15) and bool(iou2[0, 3].isnan())
    assert bool(m2[1].isnan()) and bool(iou2[1].isnan().all())  # nothing evaluated: no class to average


# ---------------------------------------------------------------------------------------------------------------- the library
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from vtp_amd import _lib
    return _lib.load()


def _refused(lib, fn, ok, changes):
    for i, v, msg in changes:
        a = list(ok)
        a[i] = v
        assert fn(*a) == -1 and msg in lib.vtp_last_error(), (fn.__name__, i, v, lib.vtp_last_error())


def test_argument_validation_needs_no_gpu(lib):
    p = ctypes.c_void_p(16)
    # ce: Z ldz labels B h w Hl Wl H C ignore lse conf loss call_counts totals workspace workspace_bytes stream
    ok = [p, 8, p, 2, 2, 2, 8, 8, 2, 4, 255, None, None, p, p, None, p, 1 << 20, None]
    _refused(lib, lib.vtp_seg_ce, ok, [(i, None, b"null") for i in (0, 2, 13, 14, 16)] +
             [(9, 0, b"C <= 255"), (9, 256, b"C <= 255"), (6, 0, b"Hl, Wl >= 1"), (7, 0, b"Hl, Wl >= 1"), (1, 7, b"ldz"), (3, 0, b"B"),
              (4, 0, b"h, w >= 1"), (17, 8, b"workspace")])
    assert lib.vtp_seg_ce_workspace_bytes(2, 2, 2, 8, 8, 2, 4) == (2 + 2) * 2 * 4  # one 32 x 32 tile per image: (H + 2) entries per workgroup
    assert lib.vtp_seg_ce_workspace_bytes(2, 2, 2, 0, 8, 2, 4) == -1 and b"Hl, Wl >= 1" in lib.vtp_last_error()
    assert lib.vtp_seg_ce_workspace_bytes(2, 2, 2, 8, 8, 2, 256) == -1 and b"C <= 255" in lib.vtp_last_error()
    # dlogits: Z ldz labels lse call_counts G ldg B h w Hl Wl H C ignore stream
    ok = [p, 8, p, p, p, p, 8, 2, 2, 2, 8, 8, 2, 4, 255, None]
    _refused(lib, lib.vtp_seg_dlogits, ok, [(i, None, b"null") for i in (0, 2, 3, 4, 5)] +
             [(13, 0, b"C <= 255"), (13, 256, b"C <= 255"), (10, 0, b"Hl, Wl >= 1"), (11, -1, b"Hl, Wl >= 1"), (1, 7, b"ldz"), (6, 7, b"ldg"),
              (8, 0, b"h, w >= 1")])
    # sgd: W bias mW mb G ldg X ldx lr M H C K momentum workspace workspace_bytes stream
    ok = [p, p, p, p, p, 8, p, 8, p, 2, 2, 4, 8, 0.9, p, 1 << 20, None]
    _refused(lib, lib.vtp_seg_sgd, ok, [(i, None, b"null") for i in (0, 1, 2, 3, 4, 6, 8, 14)] +
             [(11, 0, b"C <= 255"), (11, 256, b"C <= 255"), (12, 6, b"K % 4"), (7, 4, b"ldx >= K"), (7, 10, b"ldx % 4"), (5, 7, b"ldg"),
              (9, 0, b"M"), (6, ctypes.c_void_p(20), b"aligned"), (15, 64, b"workspace")])
    slice_rows = lib.vtp_seg_sgd_slice()
    assert slice_rows >= 64 and slice_rows % 64 == 0
    assert lib.vtp_seg_sgd_workspace_bytes(2 * slice_rows + 5, 8, 8) == 3 * 8 * (8 + 1) * 4
    assert lib.vtp_seg_sgd_workspace_bytes(4, 8, 6) == -1 and b"K % 4" in lib.vtp_last_error()
    # the grid of the weight step at B = 16, 32 x 32 cells, C = 150, K = 768, H = 1: at least one workgroup (4 tiles) per CU
    assert -(-(16 * 32 * 32) // slice_rows) * -(-150 // 64) * (768 // 64) >= 4 * 256


def test_segprobe_kernels_do_not_spill(lib):
    spec = importlib.util.spec_from_file_location("spill_report", os.path.join(ROOT, "tools", "spill_report.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    obj = os.path.join(ROOT, "vtp_amd", "lib", "segprobe.o")
    rows = {name: (vs, scr) for name, vs, ss, scr, *_ in sr.report_built(obj)}
    kernels = ("vtp::seg_ce_kernel", "vtp::seg_ce_fold_kernel", "vtp::seg_dlogits_kernel", "vtp::seg_wgrad_kernel", "vtp::seg_sgd_fold_kernel")
    for k in kernels:
        hit = [n for n in rows if n.startswith(k + "(")]
        assert hit, f"kernel {k} not in {obj}: {sorted(rows)}"
        assert rows[hit[0]] == (0, 0), f"{k}: {rows[hit[0]][0]} spilled VGPRs, {rows[hit[0]][1]} bytes of scratch"
    assert len(rows) == len(kernels), sorted(rows)


# ---------------------------------------------------------------------------------------------------------------- the class
def test_export_and_cpu_behaviour():
    import vtp_amd
    from vtp_amd.segprobe import SegProbe
    assert vtp_amd.SegProbe is SegProbe
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            SegProbe(None, [("a", 1, 0.1)], 3, embed_dim=4)
    probe = object.__new__(SegProbe)  # the checks below come before anything that needs the device
    probe.world, probe.n_max, probe.D = 1, 1, 4
    for call in (probe.step_features, probe.evaluate_features):
        with pytest.raises(ValueError, match="no CPU path"):
            call(torch.zeros(4, 4), (2, 2), torch.zeros(1, 8, 8, dtype=torch.uint8))
    probe.world = 2  # a faked process group
    with pytest.raises(NotImplementedError, match="Training is single-process in this pull request."):
        probe.step_features(torch.zeros(4, 4), (2, 2), torch.zeros(1, 8, 8, dtype=torch.uint8))
