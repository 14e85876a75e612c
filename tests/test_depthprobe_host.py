"""CPU-side checks of the linear depth probe (vtp_amd/depthprobe.py, csrc/depthprobe.hip): the fp64 restatement the GPU tests
compare against (tests/depth_ref.py) pinned to torch's own CPU ops, the metrics against their direct formulas, the argument checks
of every entry point, the register report of the kernels, and the export / error behaviour / checkpoint keys of the class."""
import ctypes
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

import depth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _torch_loss(zt, gt, C, lam=R.LAM):
    """the loss from torch's own ops on zt [B, C, h, w] (fp64, may require grad)"""
    Hl, Wl = gt.shape[1:]
    up = F.interpolate(zt, size=(Hl, Wl), mode="bilinear", align_corners=False)
    a = F.relu(up) + 0.1
    e = torch.linspace(R.MIN_DEPTH, R.MAX_DEPTH, C, dtype=F64).view(1, C, 1, 1)
    dhat = (a * e).sum(1) / a.sum(1)
    ok = (gt > 0) & (gt <= R.MAX_DEPTH)
    g = dhat[ok].log() - gt.to(F64)[ok].log()
    return up, dhat, torch.sqrt((g * g).mean() - lam * g.mean() ** 2)


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("variant", [None, "nan", "inf", "far"])
@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_restatement_matches_torch_cpu_ops_in_fp64(i, variant):
    """upsampled logits == F.interpolate(bilinear, align_corners=False), dhat == relu + normalise, loss == the formula on torch's
    ops, G == the autograd gradient through all of it, 1e-12 relative, on every shape of the GPU tests; a planted NaN / inf /
    too-far label is one valid pixel fewer and nothing else"""
    B, h, w, Hl, Wl, C, K = R.CASES[i]
    X, W, b, gt = R.make_case(i, 1, variant)
    z = (X.double() @ W.double().T + b.double()).view(B, h, w, C)
    r = R.loss_and_grad(z, gt)
    zt = z.permute(0, 3, 1, 2).clone().requires_grad_(True)
    up_t, dhat_t, loss_t = _torch_loss(zt, gt, C)
    assert float((r["up"].permute(0, 3, 1, 2) - up_t.detach()).abs().max()) <= 1e-12 * float(up_t.detach().abs().max())
    assert float((r["dhat"] - dhat_t.detach()).abs().max()) <= 1e-12 * R.MAX_DEPTH
    assert bool((r["dhat"] >= R.MIN_DEPTH).all()) and bool((r["dhat"] <= R.MAX_DEPTH).all())
    n_plain = int(R.valid_mask(R.make_case(i, 1)[3]).sum())
    assert r["n"] == n_plain - (variant is not None) and r["n"] > 0
    assert r["loss"] == pytest.approx(float(loss_t), rel=1e-12)
    (g_t,) = torch.autograd.grad(loss_t, zt)
    g_t = g_t.permute(0, 2, 3, 1)
    assert float((r["G"] - g_t).norm()) <= 1e-12 * float(g_t.norm()) and float(g_t.norm()) > 0
    assert bool(r["G"].isfinite().all())


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_restatement_without_a_valid_pixel(i):
    B, h, w, Hl, Wl, C, K = R.CASES[i]
    X, W, b, gt = R.make_case(i, 1, "all_invalid")
    r = R.loss_and_grad((X @ W.T + b).view(B, h, w, C), gt)
    assert r["loss"] == 0.0 and r["n"] == 0 and not bool(r["G"].any()) and bool(r["dhat"].isfinite().all())


def test_bin_centres_and_validity():
    e = R.bin_centres(256)
    assert float(e[0]) == R.MIN_DEPTH and float(e[-1]) == pytest.approx(R.MAX_DEPTH, rel=1e-15) and bool((e[1:] > e[:-1]).all())
    gt = torch.tensor([[[0.0, -1.0, 1e-6, 10.0, 10.000001, float("nan"), float("inf"), float("-inf")]]])
    assert R.valid_mask(gt).flatten().tolist() == [False, False, True, True, False, False, False, False]


def test_metrics_against_direct_formulas():
    from vtp_amd.depthprobe import METRICS, metrics_from_counters
    g = torch.Generator().manual_seed(0)
    gt = 0.5 + 9.0 * torch.rand(2, 9, 11, generator=g)
    gt[0, 0, :3] = torch.tensor([0.0, float("nan"), 11.0])
    d = (gt.nan_to_num(1.0) * torch.exp(0.3 * torch.randn(2, 9, 11, generator=g))).clamp(R.MIN_DEPTH, R.MAX_DEPTH)
    counts, sums = R.counters(d, gt)
    ok = R.valid_mask(gt)
    dd, tt = d.double()[ok], gt.double()[ok]
    n = dd.numel()
    assert int(counts[0]) == n == 2 * 9 * 11 - 3
    lg = dd.log() - tt.log()
    ratio = torch.maximum(dd / tt, tt / dd)
    want = dict(abs_rel=float(((dd - tt).abs() / tt).mean()), sq_rel=float(((dd - tt) ** 2 / tt).mean()),
                rmse=float(((dd - tt) ** 2).mean().sqrt()), rmse_log=float((lg ** 2).mean().sqrt()),
                log10=float((dd.log10() - tt.log10()).abs().mean()), silog=100.0 * float(lg.var(unbiased=False).sqrt()),
                d1=float((ratio < 1.25).double().mean()), d2=float((ratio < 1.25 ** 2).double().mean()),
                d3=float((ratio < 1.25 ** 3).double().mean()), valid=n)
    for got in (R.metrics(counts, sums), metrics_from_counters(counts, sums)):
        assert set(got) == set(METRICS) == set(want)
        for k, v in want.items():
            assert got[k] == pytest.approx(v, rel=1e-12), k
    assert 0 < want["d1"] < want["d2"] < want["d3"] <= 1
    with pytest.raises(RuntimeError, match="nothing evaluated"):
        metrics_from_counters(torch.zeros(4, dtype=torch.int64), torch.zeros(6, dtype=F64))


def test_the_recipe_meets_few_logits_within_their_rounding_bound_of_zero():
    """the two conditions of the cell-pass test on the reference alone, at the case where they are worst: near pairs (|z_p[c]| <=
    bz(p, c), docstring of tests/test_depthprobe_gpu.py) are at most 0.1 % of the valid pairs"""
    i = 2
    B, h, w, Hl, Wl, C, K = R.CASES[i]
    X, W, b, gt = R.make_case(i, 1)
    z = (X.double() @ W.double().T + b.double()).view(B, h, w, C)
    r = R.loss_and_grad(z, gt)
    bz = R.upsample(R.gamma(K + 1) * (X.double().abs() @ W.double().abs().T + b.double().abs()).view(B, h, w, C), Hl, Wl) \
        + R.gamma(8) * R.upsample(z.abs(), Hl, Wl)
    near = (r["up"].abs() <= bz) & r["valid"][..., None]
    assert int(near.sum()) <= 1e-3 * r["n"] * C


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
    # pix: Z ldz gt B h w Hl Wl H C min max lam dhat aux loss stats eval_counts eval_sums workspace workspace_bytes stream
    ok = [p, 512, p, 2, 2, 2, 8, 8, 2, 256, 0.001, 10.0, 0.85, None, None, p, p, None, None, p, 1 << 20, None]
    _refused(lib, lib.vtp_depth_pix, ok, [(0, None, b"null"), (15, None, b"null"), (16, None, b"null"), (19, None, b"null"),
                                          (2, None, b"dhat or gt"), (17, p, b"go together"), (18, p, b"go together"),
                                          (9, 1, b"2 <= C <= 1024"), (9, 1025, b"2 <= C <= 1024"), (6, 0, b"Hl, Wl >= 1"),
                                          (7, 0, b"Hl, Wl >= 1"), (1, 511, b"ldz"), (3, 0, b"B"), (4, 0, b"h, w >= 1"),
                                          (10, 0.0, b"min_depth"), (10, 10.0, b"min_depth"), (11, float("inf"), b"min_depth"),
                                          (10, float("nan"), b"min_depth"), (20, 8, b"workspace"), (19, ctypes.c_void_p(20), b"aligned")])
    pred = list(ok)  # prediction: no labels, only dhat
    pred[2], pred[13], pred[15], pred[16], pred[19], pred[20] = None, p, None, None, None, 0
    _refused(lib, lib.vtp_depth_pix, pred, [(14, p, b"need labels"), (17, p, b"need labels"), (9, 1, b"2 <= C <= 1024")])
    # one 32 x 32 tile per image; per workgroup: H heads x (6 fp64 sums + 3 i32 counts) + one i32 count
    assert lib.vtp_depth_pix_workspace_bytes(2, 2, 2, 8, 8, 2, 4, 0) == 2 * (2 * (6 * 8 + 3 * 4) + 4)
    assert lib.vtp_depth_pix_workspace_bytes(2, 2, 2, 8, 8, 2, 4, 1) == 3 * 2 * 2 * 8 * 8 * 4  # three fp32 planes [H, B, Hl, Wl]
    assert lib.vtp_depth_pix_workspace_bytes(2, 2, 2, 0, 8, 2, 4, 0) == -1 and b"Hl, Wl >= 1" in lib.vtp_last_error()
    assert lib.vtp_depth_pix_workspace_bytes(2, 2, 2, 8, 8, 2, 1025, 0) == -1 and b"C <= 1024" in lib.vtp_last_error()
    assert lib.vtp_depth_pix_workspace_bytes(16, 32, 32, 4096, 4096, 4, 256, 1) == -1 and b"2 GiB" in lib.vtp_last_error()
    # dlogits: Z ldz aux stats G ldg B h w Hl Wl H C min max lam stream
    ok = [p, 512, p, p, p, 512, 2, 2, 2, 8, 8, 2, 256, 0.001, 10.0, 0.85, None]
    _refused(lib, lib.vtp_depth_dlogits, ok, [(i, None, b"null") for i in (0, 2, 3, 4)] +
             [(12, 1, b"2 <= C <= 1024"), (12, 1025, b"2 <= C <= 1024"), (9, 0, b"Hl, Wl >= 1"), (10, -1, b"Hl, Wl >= 1"), (1, 511, b"ldz"),
              (5, 511, b"ldg"), (7, 0, b"h, w >= 1"), (13, -1.0, b"min_depth"), (14, 0.0005, b"min_depth")])
    # sgd: W bias mW mb G ldg X ldx lr M H C K momentum workspace workspace_bytes stream
    ok = [p, p, p, p, p, 512, p, 8, p, 2, 2, 256, 8, 0.9, p, 1 << 20, None]
    _refused(lib, lib.vtp_depth_sgd, ok, [(i, None, b"null") for i in (0, 1, 2, 3, 4, 6, 8, 14)] +
             [(11, 0, b"C <= 1024"), (11, 1025, b"C <= 1024"), (12, 6, b"K % 4"), (7, 4, b"ldx >= K"), (7, 10, b"ldx % 4"), (5, 511, b"ldg"),
              (9, 0, b"M"), (6, ctypes.c_void_p(20), b"aligned"), (15, 64, b"workspace")])
    for fn in (lib.vtp_depth_sgd, lib.vtp_seg_sgd):
        assert fn(*ok[:14], p, 64, None) == -1  # C = 256 or not, 64 bytes are too few
    assert b"vtp_seg_sgd" in lib.vtp_last_error() and b"C <= 255" in lib.vtp_last_error()  # vtp_seg_sgd still refuses 256 outputs ...
    assert lib.vtp_depth_sgd(*ok[:14], p, 64, None) == -1 and b"vtp_depth_sgd: workspace" in lib.vtp_last_error()  # ... vtp_depth_sgd does not
    slice_rows = lib.vtp_seg_sgd_slice()
    for M, N, K in ((2 * slice_rows + 5, 8, 8), (7, 1024, 132)):
        assert lib.vtp_depth_sgd_workspace_bytes(M, N, K) == lib.vtp_seg_sgd_workspace_bytes(M, N, K) == -(-M // slice_rows) * N * (K + 1) * 4
    assert lib.vtp_depth_sgd_workspace_bytes(4, 8, 6) == -1 and b"K % 4" in lib.vtp_last_error()


def test_depthprobe_kernels_do_not_spill(lib):
    spec = importlib.util.spec_from_file_location("spill_report", os.path.join(ROOT, "tools", "spill_report.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    obj = os.path.join(ROOT, "vtp_amd", "lib", "depthprobe.o")
    rows = {name: (vs, scr) for name, vs, ss, scr, *_ in sr.report_built(obj)}
    kernels = ("vtp::depth_pix_kernel", "vtp::depth_fold_kernel", "vtp::depth_dlogits_kernel")
    for k in kernels:
        hit = [n for n in rows if n.startswith(k + "(")]
        assert hit, f"kernel {k} not in {obj}: {sorted(rows)}"
        assert rows[hit[0]] == (0, 0), f"{k}: {rows[hit[0]][0]} spilled VGPRs, {rows[hit[0]][1]} bytes of scratch"
    assert len(rows) == len(kernels), sorted(rows)  # the weight step's kernels exist once, in segprobe.o


# ---------------------------------------------------------------------------------------------------------------- the class
def test_export_error_behaviour_and_checkpoint_keys():
    import vtp_amd
    from vtp_amd.depthprobe import DepthProbe
    from vtp_amd.heads import HeadStore
    assert vtp_amd.DepthProbe is DepthProbe
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            DepthProbe(None, [("a", 1, 0.1)], embed_dim=4)
    probe = object.__new__(DepthProbe)  # the checks below come before anything that needs the device
    probe.world, probe.n_max, probe.D, probe.Dc = 1, 1, 4, 4
    for call in (probe.step_features, probe.evaluate_features):
        with pytest.raises(ValueError, match="no CPU path"):
            call(torch.zeros(4, 4), (2, 2), torch.ones(1, 8, 8))
    with pytest.raises(ValueError, match="no CPU path"):
        probe.predict_features(torch.zeros(4, 4), (2, 2), (8, 8))
    probe.world = 2  # a faked process group
    with pytest.raises(NotImplementedError, match="Training is single-process in this pull request."):
        probe.step_features(torch.zeros(4, 4), (2, 2), torch.ones(1, 8, 8))
    # the checkpoint: SegProbe's keys, from a head store on the host
    heads = [("a", 1, 0.1), ("b", 2, 0.2)]
    probe.heads = HeadStore([(k, n, n * 4, (2 - n) * 4, lr) for k, n, lr in heads],
                            {k: (torch.randn(5, n * 4), torch.zeros(5)) for k, n, _ in heads}, "cpu")
    probe.keys, probe.steps = probe.heads.keys, 3
    sd = probe.state_dict()
    assert set(sd) == {f"{p}.{k}.{q}" for k in "ab" for p in ("heads", "momentum") for q in ("weight", "bias")} | {"steps"}
    assert int(sd["steps"]) == 3 and tuple(sd["heads.b.weight"].shape) == (5, 8)
    probe.steps = 0
    probe.load_state_dict(sd)
    assert probe.steps == 3
    with pytest.raises(KeyError, match="missing"):
        probe.load_state_dict({k: v for k, v in sd.items() if k != "momentum.a.bias"})

