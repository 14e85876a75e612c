"""GPU: the zero-shot kernels (csrc/zeroshot.hip: vtp_zs_class_mean / vtp_zs_topk, exact fp32 on the f32-input MFMA) and
vtp_amd.ZeroShot against fp64 on the CPU, and through the model against the fixture of the real tool.

Bounds.  gamma_n = n u / (1 - n u), u = 2^-24 (tests/probe_ref.py), is the a-priori error of a chain of n fp32 roundings in any
order: a product chain over D terms behind one rounding of scale * F obeys |err| <= gamma_{D+2} scale (|F| |Wt|^T) elementwise.
It is derived, not measured.  1e-5 (relative, Frobenius) is the project's bar for fp32 arithmetic against fp64
(tests/test_losses_gpu.py).  Ranks, counts and predictions are integers and are compared with equality: the dyadic inputs of
test 3 make every product and partial sum exact in fp32 (entries k / 8, |k| <= 4, scale 100: every product is a multiple of 1 / 16
of magnitude <= 25, every partial sum stays below 25 D <= 6500 < 2^13, so 17 significant bits suffice), which the test asserts
on the CPU before it looks at the GPU; test 4 recomputes ranks from the logits the kernel itself returned.

Printed on one MI355X: class mean relF 2.5e-08 ... 1.7e-07, row norms within 5.7e-08 of 1; logits at 0.009 ... 0.092 of the a-priori
bound (the largest at C = 4099, D = 40); through the model E_ours / E_ref = 0.93 (classifier) and 0.59 (logits) against the fixture,
relF 5.7e-08 and 3.0e-07 against the oracle's torch plumbing on the same model."""
import functools
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

import probe_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
BS = [1, 5, 33, 130]
CD = [(7, 40), (37, 132), (1000, 260)]
CASES = [(B, C, D) for C, D in CD for B in BS] + [(5, 4099, 40)]  # the last one: more classes than one LDS-resident row block holds
NAN = float("nan")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _sliced(x, pad=8, off=4):
    """x on the GPU as a column slice (offset `off`, row stride D + pad) of a wider NaN-poisoned matrix"""
    wide = torch.full((x.shape[0], x.shape[1] + pad), NAN, dtype=F32)
    wide[:, off:off + x.shape[1]] = x
    return wide.to(DEV)[:, off:off + x.shape[1]]


def _relF(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def rank_pred(z, y):
    """the stated rule on the CPU, exact comparisons: rank = #{z > z_t} + #{c < t : z == z_t} (C for a target outside [0, C)) and
    the first five classes of a stable sort by (-z, index)"""
    B, C = z.shape
    ok = (y >= 0) & (y < C)
    yc = y.clamp(0, C - 1)
    zt = z[torch.arange(B), yc][:, None]
    idx = torch.arange(C)[None]
    rank = (z > zt).sum(1) + ((z == zt) & (idx < yc[:, None])).sum(1)
    rank = torch.where(ok, rank, torch.full_like(rank, C))
    pred = torch.sort(-z, dim=1, stable=True).indices[:, :5]
    return rank.to(I32), pred.to(I32)


def counts_of(rank, y, C):
    ok = (y >= 0) & (y < C)
    per_class = torch.stack([torch.bincount(y[ok], minlength=C), torch.bincount(y[ok & (rank < 1)], minlength=C)]).to(I32)
    return torch.tensor([int((rank < 1).sum()), int((rank < 5).sum()), rank.shape[0]], dtype=I64), per_class


def run_topk(f, wt, y, scale=100.0, counts=None, outputs=True):
    """one call of the kernel; with outputs: logits in a NaN-poisoned [B, C + 3] buffer, rank, pred, per_class"""
    from vtp_amd import ops
    B, D = f.shape
    C = wt.shape[0]
    counts = torch.zeros(3, device=DEV, dtype=I64) if counts is None else counts
    out = dict(counts=counts)
    if outputs:
        out["wide"] = torch.full((B, C + 3), NAN, device=DEV, dtype=F32)
        out["rank"] = torch.full((B,), -7, device=DEV, dtype=I32)
        out["pred"] = torch.full((B, 5), -7, device=DEV, dtype=I32)
        out["per_class"] = torch.zeros(2, C, device=DEV, dtype=I32)
        ops.zs_topk(f, wt, y.to(DEV), scale, B, C, D, counts, out["per_class"], out["rank"], out["pred"], out["wide"][:, :C])
    else:
        ops.zs_topk(f, wt, y.to(DEV), scale, B, C, D, counts)
    out = {k: v.cpu() for k, v in out.items()}
    if outputs:
        out["logits"] = out["wide"][:, :C]
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. class mean
@pytest.mark.parametrize("C,T,D", [(1, 1, 4), (7, 3, 40), (10, 80, 132), (37, 5, 768)])
def test_class_mean_and_normalize(C, T, D):
    _gpu()
    from vtp_amd import ops
    feat = torch.randn(C * T, D, generator=torch.Generator().manual_seed(C + T + D))
    zero = 1 if C > 1 else None
    if zero is not None:
        feat[zero * T:(zero + 1) * T] = 0.0
    fs = _sliced(feat)
    assert fs.stride(0) == D + 8 and fs.storage_offset() == 4
    buf = torch.full((C + 2, D + 4), NAN, device=DEV, dtype=F32)
    ops.zs_class_mean(fs, buf[1:1 + C, :D], C, T, D, 1e-12)
    got = buf.cpu()
    w = got[1:1 + C, :D]
    m = feat.double().view(C, T, D).sum(1) / T
    ref = m / m.norm(dim=1, keepdim=True).clamp_min(1e-12)
    e = _relF(w, ref)
    norms = w.double().norm(dim=1)
    live = torch.ones(C, dtype=torch.bool)
    if zero is not None:
        live[zero] = False
        assert bool((w[zero] == 0).all()), "an all-zero class must give a zero row, not NaN"
    dn = float((norms[live] - 1).abs().max())
    print(f"CLASSMEAN C={C} T={T} D={D}: relF {e:.2e}  max |norm - 1| {dn:.2e}")
    assert e <= 1e-5
    assert dn <= 1e-6
    assert bool(got[0].isnan().all() and got[C + 1].isnan().all() and got[:, D:].isnan().all()), "wrote outside its rows"
    if C == 7:  # class batches fill one classifier call by call: rows [0, 3) and [3, 7) against all 7 at once, bitwise
        two = torch.full((C, D), NAN, device=DEV, dtype=F32)
        ops.zs_class_mean(fs[:3 * T], two[:3], 3, T, D, 1e-12)
        ops.zs_class_mean(fs[3 * T:], two[3:], 4, T, D, 1e-12)
        assert torch.equal(two.cpu(), w)


# ---------------------------------------------------------------------------------------------------------------- 2. logits
@functools.lru_cache(maxsize=None)
def real_case(B, C, D):
    g = torch.Generator().manual_seed(7 * B + C + D)
    f = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=1)
    wt = torch.nn.functional.normalize(torch.randn(C, D, generator=g), dim=1)
    y = torch.randint(0, C, (B,), generator=g)
    return f, wt, y


@pytest.mark.parametrize("B,C,D", CASES)
def test_logits_within_the_fp32_chain_bound(B, C, D):
    _gpu()
    f, wt, y = real_case(B, C, D)
    scale = 100.0
    got = run_topk(_sliced(f), _sliced(wt), y, scale)
    ref = scale * (f.double() @ wt.double().T)
    bound = R.gamma(D + 2) * scale * (f.double().abs() @ wt.double().abs().T)
    err = (got["logits"].double() - ref).abs()
    print(f"ZSLOGITS B={B} C={C} D={D}: max err/bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (B, C, D, float((err / bound).max()))
    assert bool(got["wide"][:, C:].isnan().all()), "wrote past column C"


@pytest.mark.parametrize("scale", [1.0, 100.0])
@pytest.mark.parametrize("B", [1, 33, 70])
def test_logits_have_the_bits_of_probe_logits_with_a_zero_bias(B, scale):
    """Both kernels run the k unit of csrc/wave_f32.h, so the optional logits output is vtp_probe_logits on the same F and W with a
    zero bias, bit for bit; with a scale, on (scale * F) formed in fp32 beforehand: "rounded once, then the product chain".
    D = 36 ends in a unit tail, D = 8 is less than one unit."""
    _gpu()
    from vtp_amd import ops
    for C in (7, 37, 100):
        for D in (8, 36, 100):
            f, wt, y = real_case(B, C, D)
            fd, wd = _sliced(f), wt.to(DEV)
            got = run_topk(fd, wd, y, scale)["logits"]
            want = torch.full((B, C), NAN, device=DEV, dtype=F32)
            scaled = fd if scale == 1.0 else _sliced(torch.tensor(scale, dtype=F32) * f)
            ops.probe_logits(scaled, wd, torch.zeros(C, device=DEV, dtype=F32), want, B, C, D)
            assert torch.equal(got.view(I32), want.cpu().view(I32)), (B, C, D, scale)


# ---------------------------------------------------------------------------------------------------------------- 3. exact ranks
@functools.lru_cache(maxsize=None)
def dyadic_case(B, C, D):
    """entries k / 8 with |k| <= 4; class 5 a copy of class 2; every second row of F its target's own classifier row; row 0 targets
    class 2 and row 1 class 5 with the same feature, so the duplicated column puts row 0 at rank 0 and row 1 at rank 1"""
    g = torch.Generator().manual_seed(1000 * B + C + D)
    f = torch.randint(-4, 5, (B, D), generator=g).float() / 8
    wt = torch.randint(-4, 5, (C, D), generator=g).float() / 8
    wt[5] = wt[2]
    y = torch.randint(0, C, (B,), generator=g)
    y[0] = 2
    if B > 1:
        y[1] = 5
    f[0::2] = wt[y[0::2]]
    if B > 1:
        f[1] = wt[5]
    z64 = (100.0 * f.double()) @ wt.double().T
    z32 = (100.0 * f) @ wt.T
    assert torch.equal(z32.double(), z64), "the dyadic data must make the fp32 product exact"
    assert float(z64.abs().max()) <= 25.0 * D
    return f, wt, y, z32


@pytest.mark.parametrize("B,C,D", CASES)
def test_exact_ranks_counts_and_predictions(B, C, D):
    _gpu()
    f, wt, y, z = dyadic_case(B, C, D)
    rank, pred = rank_pred(z, y)
    counts, per_class = counts_of(rank, y, C)
    ties = int(((z == z[torch.arange(B), y][:, None]).sum(1) > 1).sum())
    print(f"ZSEXACT B={B} C={C} D={D}: top-1 {int(counts[0])} top-5 {int(counts[1])} rows with a tie at the target {ties}")
    assert int(rank[0]) == 0 and (B == 1 or int(rank[1]) == 1) and ties >= min(B, 2)
    got = run_topk(_sliced(f), _sliced(wt), y, 100.0)
    assert torch.equal(got["logits"], z), "logits must equal the exact product bitwise"
    assert bool(got["wide"][:, C:].isnan().all())
    assert got["rank"].shape == (B,) and torch.equal(got["rank"], rank)
    assert torch.equal(got["counts"], counts)
    assert torch.equal(got["per_class"], per_class)
    assert torch.equal(got["pred"], pred)


# ---------------------------------------------------------------------------------------------------------------- 4. self-consistency
@pytest.mark.parametrize("B,C,D", CASES)
def test_ranks_follow_from_the_returned_logits(B, C, D):
    _gpu()
    f, wt, y = real_case(B, C, D)
    fd, wd = _sliced(f), _sliced(wt)
    got = run_topk(fd, wd, y, 100.0)
    rank, pred = rank_pred(got["logits"], y)
    assert torch.equal(got["rank"], rank)
    assert torch.equal(got["pred"], pred)
    counts, per_class = counts_of(rank, y, C)
    assert torch.equal(got["counts"], counts) and torch.equal(got["per_class"], per_class)
    for b in range(B):  # the target is among the first k predictions exactly when its rank is below k
        for k in (1, 5):
            assert (int(y[b]) in got["pred"][b, :k].tolist()) == (int(rank[b]) < k)
    bare = run_topk(fd, wd, y, 100.0, outputs=False)  # every optional output NULL: the same three numbers
    assert torch.equal(bare["counts"], counts)


# ---------------------------------------------------------------------------------------------------------------- 5. accumulation
def test_counts_accumulate_and_bad_targets_miss():
    _gpu()
    B, C, D = 33, 37, 132
    f, wt, y, z = dyadic_case(B, C, D)
    y = y.clone()
    y[3], y[4], y[32] = -1, C, C + 1000  # row 4 is a copy of its (former) target's row: still a miss
    rank, _ = rank_pred(z, y)
    assert int(rank[3]) == C and int(rank[4]) == C and int(rank[32]) == C
    c1, pc1 = counts_of(rank, y, C)
    f2, wt2, y2, z2 = dyadic_case(5, C, D)
    rank2, _ = rank_pred((100.0 * f2) @ wt.T, y2)
    c2, pc2 = counts_of(rank2, y2, C)
    from vtp_amd import ops
    counts = torch.tensor([7, 9, 11], device=DEV, dtype=I64)
    per_class = torch.zeros(2, C, device=DEV, dtype=I32)
    rk = torch.full((B,), -7, device=DEV, dtype=I32)
    wd = wt.to(DEV)
    ops.zs_topk(f.to(DEV), wd, y.to(DEV), 100.0, B, C, D, counts, per_class, rk)
    ops.zs_topk(f2.to(DEV), wd, y2.to(DEV), 100.0, 5, C, D, counts, per_class)
    assert torch.equal(rk.cpu(), rank)
    assert torch.equal(counts.cpu(), torch.tensor([7, 9, 11]) + c1 + c2)
    assert torch.equal(per_class.cpu(), pc1 + pc2)
    assert int(per_class[0].sum()) == B - 3 + 5 and int(per_class[1].sum()) == int(c1[0] + c2[0])


# ---------------------------------------------------------------------------------------------------------------- 6. through the model
def test_zero_shot_through_the_model_against_the_tool_fixture(golden_sd):
    """the zs.* part of tests/test_tools_gpu.py with ZeroShot in place of the tool's torch arithmetic"""
    _gpu()
    from safetensors.torch import load_file
    from oracle import tools_oracle as T
    from oracle.ref_stubs import TINY
    from vtp_amd import VTPConfig, VTPModel, ZeroShot
    tg = load_file(os.path.join(ROOT, "tests", "golden", "tools_tiny.safetensors"))
    images, targets = tg["in.images"], tg["in.targets"]
    tok = T.toy_tokenizer(TINY["text_vocab_size"], TINY["text_context_length"])
    C = len(T.CLASSNAMES)
    model = VTPModel(VTPConfig(**TINY))
    model.load_state_dict(golden_sd, strict=True)
    model = model.to(DEV).eval()
    zs = ZeroShot(model)
    with pytest.raises(RuntimeError, match="nothing evaluated"):
        zs.set_classifier(tg["out.zs.classifier"])
        zs.accuracy()
    W = zs.build_classifier(tok, T.CLASSNAMES, T.TEMPLATES, num_classes_per_batch=3)
    assert W.shape == tg["out.zs.classifier"].shape and W.data_ptr() == zs.Wt.data_ptr() and not W.is_contiguous()
    halves = [(images[:4], targets[:4]), (images[4:], targets[4:])]
    for im, y in halves:
        assert zs.update(im.to(DEV), y.to(DEV)) is None
    built = zs.counts()
    assert built[2] == 8 and zs.accuracy() == (built[0] / 8 * 100, built[1] / 8 * 100)
    # the same two batches with the optional outputs: logits and ranks of every row
    zs.reset()
    assert zs.counts() == (0, 0, 0)
    logits = torch.full((8, C), NAN, device=DEV)
    ranks = torch.full((8,), -7, device=DEV, dtype=I32)
    with torch.no_grad():
        for s, (im, y) in zip((slice(0, 4), slice(4, 8)), halves):
            zs.update_features(model.get_clip_image_feature(im.to(DEV), normalize=True), y.to(DEV), logits_out=logits[s], rank_out=ranks[s])
    assert zs.counts() == built
    ours = {"zs.classifier": W.cpu(), "zs.logits": logits.cpu()}
    # (a) against the fixture of the real tool on the real reference model, with tests/test_tools_gpu.py's bar
    noisy_model = T.OracleModel(golden_sd, 2, 2, 2, autocast_dtype=torch.bfloat16)
    noisy_clf = T.build_zero_shot_classifier(noisy_model, tok, T.CLASSNAMES, T.TEMPLATES, num_classes_per_batch=3, device="cpu")
    noisy = {"zs.classifier": noisy_clf, "zs.logits": T.zero_shot_evaluate(noisy_model, noisy_clf, halves, "cpu")[2]}
    for k in ("zs.classifier", "zs.logits"):
        ref = tg["out." + k]
        e, e_ref = _relF(ours[k], ref), _relF(noisy[k], ref)
        print(f"ZEROSHOT {k}: E_ours={e:.3e} E_ref={e_ref:.3e} ratio={e / e_ref:.2f}")
        assert ours[k].shape == ref.shape and e <= 1.5 * e_ref, (k, e, e_ref)
    # (b) against the oracle's torch plumbing driven by the same model: the two kernels alone
    clf_t = T.build_zero_shot_classifier(model, tok, T.CLASSNAMES, T.TEMPLATES, num_classes_per_batch=3, device=torch.device(DEV))
    _, _, logits_t = T.zero_shot_evaluate(model, clf_t, halves, torch.device(DEV))
    for k, a, b in (("classifier", ours["zs.classifier"], clf_t), ("logits", ours["zs.logits"], logits_t)):
        e = _relF(a, b)
        print(f"ZEROSHOT {k} against torch on the same model: relF {e:.2e}")
        assert e <= 1e-5, k
    rank_rule, _ = rank_pred(ours["zs.logits"], targets)
    assert torch.equal(ranks.cpu(), rank_rule)
    assert built == (int((rank_rule < 1).sum()), int((rank_rule < 5).sum()), 8)
    z = ours["zs.logits"]
    tied = ((z == z[torch.arange(8), targets][:, None]).sum(1) > 1).nonzero().flatten().tolist()
    if tied:
        print(f"ZEROSHOT rows with an exact tie at the target, compared by the stated rule: {tied}")
    else:
        a1, a5 = T.accuracy(z, targets, topk=(1, 5))
        assert (int(a1), int(a5)) == built[:2]
    # (c) the fixture's classifier adopted: the same counts where the fixture's logits rank the targets as ours do
    rank_fix, _ = rank_pred(tg["out.zs.logits"], targets)
    zs.set_classifier(tg["out.zs.classifier"])
    for im, y in halves:
        zs.update(im.to(DEV), y.to(DEV))
    adopted = zs.counts()
    print(f"ZEROSHOT top-1 / top-5 counts of 8: built {built[:2]} adopted classifier {adopted[:2]} "
          f"fixture {(int((rank_fix < 1).sum()), int((rank_fix < 5).sum()))} tool {tg['out.zs.top'].tolist()}")
    if torch.equal(rank_fix, rank_rule):
        assert adopted == built
    else:
        print(f"ZEROSHOT ranks differ between our logits and the fixture's (bf16 noise on near-ties): ours {rank_rule.tolist()} fixture {rank_fix.tolist()}")
    pc = zs.per_class_accuracy()
    assert pc.shape == (C,) and bool(pc[torch.bincount(targets, minlength=C) == 0].isnan().all())
    with pytest.raises(ValueError, match="MI355X"):
        zs.update(images[:4], targets[:4].to(DEV))


# ---------------------------------------------------------------------------------------------------------------- 7. two ranks
TWO = (130, 37, 132)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from vtp_amd import ZeroShot
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    f, wt, y, _ = dyadic_case(*TWO)
    zs = ZeroShot(None, group=dist.group.WORLD)
    zs.set_classifier(wt.T)
    half = TWO[0] // world
    sl = slice(rank * half, (rank + 1) * half)
    zs.update_features(f[sl].to(DEV), y[sl].to(DEV))
    out[rank] = (zs.counts(), zs.accuracy(), zs.per_class_accuracy())
    dist.destroy_process_group()


def test_two_ranks_sum_to_the_single_process_counts():
    _gpu()
    from vtp_amd import ZeroShot
    f, wt, y, z = dyadic_case(*TWO)
    rank, _ = rank_pred(z, y)
    want, _ = counts_of(rank, y, TWO[1])
    zs = ZeroShot(None)
    zs.set_classifier(wt.T)
    zs.update_features(f.to(DEV), y.to(DEV))
    one, one_pc = zs.counts(), zs.per_class_accuracy()
    assert one == tuple(int(v) for v in want)
    del zs
    torch.cuda.empty_cache()
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    for r in range(world):
        counts, acc, pc = out[r]
        assert counts == one and acc == (one[0] / one[2] * 100, one[1] / one[2] * 100)
        assert torch.equal(pc.nan_to_num(-1.0), one_pc.nan_to_num(-1.0))
