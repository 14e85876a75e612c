"""GPU checks of the Inception Score kernels (csrc/inception_score.hip: vtp_is_rows / vtp_is_accum), of InceptionScore,
InceptionFeatures.forward_taps and GenEval against the restatements of tests/is_ref.py and tests/fid_ref.py.

Bounds.  u = 2^-53.  vtp_is_rows forms p_c = exp(d_c) / Z from an exact d_c: one exp and one division (a few u), and Z, a sum of C
terms (C u at worst) -- |dp_c| <= 8 C u p_c, plus the smallest normal double for results in the subnormal range, which carry no
relative precision.  h adds the rounding of d_c - log Z, a product and C more adds per term: |dh| <= 8 C u sum_c |p_c (l_c - lse)|,
plus the same smallest normal double: a row whose every other class underflows (kind 2 below, at C = 8) has an h of 5e-311 made of
subnormal products, which no fp64 arithmetic forms to a relative bound (seen: error 1.8e-322 against a bound that rounds to 0).
The reference (is_ref.rows) works in 80-bit extended precision, so its own error is 2^-11 of these bounds.
vtp_is_accum: a chain of n fp64 adds, |err| <= gamma64(n) sum |terms| against the exact sum.
The end-to-end figures have no a-priori bound worth stating: the error of ours against fp64 must stay within twice that of the
restatement's own fp32 runs, both printed."""
import functools
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

import fid_ref as R
import is_ref as IR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
N_ROWS = 257
BIG = 1e30


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == F64 else torch.int32)


# ---------------------------------------------------------------------------------------------------------------- vtp_is_rows
@functools.lru_cache(maxsize=None)
def _rows_case(C):
    """N_ROWS + 5 rows of fp32 logits in five kinds, i % 5: 0 all equal; 1 one logit 80 above the rest; 2 a spread wide enough that
    some p underflow to 0 and one lands in the subnormal range; 3 magnitudes near 3e4; 4 ordinary -- and their reference"""
    g = torch.Generator().manual_seed(1000 + C)
    n = N_ROWS + 5
    l = torch.empty(n, C)
    for i in range(n):
        r = torch.randn(C, generator=g)
        j = [int(v) for v in torch.randperm(C, generator=g)[:3]]
        kind = i % 5
        if kind == 0:
            r = torch.full((C,), float(r[0]) * 10)
        elif kind == 1:
            r[j[0]] = float(r.max()) + 80
        elif kind == 2:
            r = r * 300
            top = float(r.max())
            r[j[0]], r[j[1]] = top - 1500, top - 720  # e^-1500 is 0 in fp64, e^-720 = 2e-313 is subnormal
            r[j[2]] = top + 1  # the maximum, away from the two
        elif kind == 3:
            r = 3e4 + 3 * r
        else:
            r = 3 * r
        l[i] = r
    p, h, mag = IR.rows(l.numpy())
    p64 = p.astype(np.float64)
    assert (p64[2::5] == 0).any(1).all() and ((p64[2::5] > 0) & (p64[2::5] < IR.TINY)).any(1).all()
    return l, p, h, mag


def _run_rows(l, C):
    """vtp_is_rows on the rows l; for C = 10 in a buffer 16 wide whose padded columns hold +1e30"""
    from vtp_amd import ops
    dev = _dev()
    B = l.shape[0]
    buf = torch.full((B, 16 if C == 10 else C), BIG)
    buf[:, :C] = l
    p = torch.full((B, C), -7.25, device=dev, dtype=F64)
    h = torch.full((B,), -7.25, device=dev, dtype=F64)
    ops.is_rows(buf.to(dev), C, p, h)
    return p, h


@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("C", [8, 10, 1000, 1008])
def test_is_rows_within_the_bound(C, B):
    l, pr, hr, mag = _rows_case(C)
    lo = B % 5  # B = 1 takes row 1 (one logit 80 above the rest), the others start at another kind each
    p, h = _run_rows(l[lo:lo + B], C)
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(h).all())
    pr, hr, mag = pr[lo:lo + B], hr[lo:lo + B], mag[lo:lo + B]
    dp = np.abs(p.cpu().numpy().astype(np.longdouble) - pr)
    dh = np.abs(h.cpu().numpy().astype(np.longdouble) - hr)
    bp, bh = 8 * C * IR.U64 * pr + IR.TINY, 8 * C * IR.U64 * mag + IR.TINY
    print(f"is_rows C={C} B={B}: max dp / bound {float((dp / bp).max()):.4f}, max dh / bound {float((dh / bh).max()):.4f}")
    assert (dp <= bp).all()
    assert (dh <= bh).all()


@pytest.mark.parametrize("C", [8, 10, 1000, 1008])
def test_is_rows_bits_do_not_depend_on_the_batch(C):
    l = _rows_case(C)[0]
    p, h = _run_rows(l[:N_ROWS], C)
    for i in (0, 1, 2, 3, 4, 256):  # every kind alone, and the last row of the last workgroup
        p1, h1 = _run_rows(l[i:i + 1], C)
        assert torch.equal(_bits(p1), _bits(p[i:i + 1])) and torch.equal(_bits(h1), _bits(h[i:i + 1])), i
    p2, h2 = _run_rows(l[:N_ROWS], C)
    assert torch.equal(_bits(p2), _bits(p)) and torch.equal(_bits(h2), _bits(h))


# ---------------------------------------------------------------------------------------------------------------- vtp_is_accum
def _exact(terms):
    """the sum over the leading axis of fp64 terms by a two-sum chain: the rounded total plus the collected rounding errors"""
    tot, low = torch.zeros_like(terms[0]), torch.zeros_like(terms[0])
    for p in terms:
        t = tot + p
        bp = t - tot
        low += (tot - (t - bp)) + (p - bp)
        tot = t
    return tot + low


@pytest.mark.parametrize("split", [50, 257, None])
@pytest.mark.parametrize("C", [10, 300])
def test_is_accum_bound_and_split_invariance(C, split):
    from vtp_amd import ops
    dev = _dev()
    l = 3 * torch.randn(N_ROWS, C, generator=torch.Generator().manual_seed(C))
    p = torch.empty(N_ROWS, C, device=dev, dtype=F64)
    h = torch.empty(N_ROWS, device=dev, dtype=F64)
    ops.is_rows(l.to(dev), C, p, h)
    step = N_ROWS if split is None else split
    slots = -(-N_ROWS // step)

    def run(updates):
        state = torch.zeros(slots + 1, 1 + C, device=dev, dtype=F64)  # one slot more than the rows reach: it must stay 0
        at = 0
        for m in updates:
            ops.is_accum(p[at:at + m], h[at:at + m], state, at, split)
            at += m
        assert at == N_ROWS
        return state

    state = run([N_ROWS])
    terms = torch.cat([h[:, None], p], 1).cpu()  # [rows, 1 + C]
    for s in range(slots):
        part = terms[s * step:(s + 1) * step]
        err = (state[s].cpu() - _exact(part)).abs()
        assert bool((err <= R.gamma64(part.shape[0]) * part.abs().sum(0)).all()), s
    assert float(state[slots].abs().max()) == 0
    again = run([1, 7, 64, 185])  # with split = 50 every update but the first straddles a boundary
    assert torch.equal(_bits(again), _bits(state))


# ---------------------------------------------------------------------------------------------------------------- InceptionScore
@functools.lru_cache(maxsize=None)
def _fc_case(C, n=300, D=2048):
    g = torch.Generator().manual_seed(100 + C)
    f = torch.randn(n, D, generator=g).abs()
    W = torch.randn(C, D, generator=g) * (6.0 / D ** 0.5)
    b = 0.1 * torch.randn(C, generator=g)
    return f, W, b


@pytest.mark.parametrize("C", [1000, 10])
def test_inception_score_end_to_end(C):
    from vtp_amd import InceptionScore, ops
    from vtp_amd.inception_score import pad_fc
    dev = _dev()
    f, W, b = _fc_case(C)
    want, want_std, _ = IR.inception_score(f.double() @ W.double().t() + b.double(), 128)
    assert 2 <= want <= C / 2, want  # well away from 1: otherwise the ratio below tests nothing
    e_32 = abs(IR.inception_score((f @ W.t() + b).double(), 128)[0] - want) / want

    isc = InceptionScore(W, b, split_size=128, device=dev, max_rows=64)
    fg = f.to(dev)
    wp, bp = pad_fc(W, b)
    ref = torch.empty(300, wp.shape[0], device=dev)
    ops.gemm_nt_f32(fg, wp.to(dev), ref, bias=bp.to(dev))
    lg = isc.logits(fg)
    assert lg.shape == (300, C) and torch.equal(_bits(lg), _bits(ref[:, :C]))

    isc.update(fg[:100])
    isc.update(fg[100:])
    assert isc.n == 300
    out = isc.result()
    assert set(out) == {"is", "is_std", "splits"} and out["splits"] == 3
    e_ours = abs(out["is"] - want) / want
    print(f"InceptionScore C={C}: IS {out['is']:.6f} (fp64 {want:.6f})  E_ours {e_ours:.3e}  E_32 {e_32:.3e}  ratio {e_ours / e_32:.3f}")
    assert e_ours <= 2 * e_32
    # is_std is a function of the same three split scores: the a-priori relative bound of the fp32 logits' K = 2048 chain, gamma_2049
    assert abs(out["is_std"] - want_std) <= R.gamma(2049) * want
    # on the device's own logits only the fp64 tail is left
    mean, std = IR.inception_score(lg.double().cpu(), 128)[:2]
    assert abs(out["is"] - mean) <= 1e-12 * mean and abs(out["is_std"] - std) <= 1e-12 * mean

    sd = isc.state_dict()
    other = InceptionScore(W, b, split_size=128, device=dev)
    other.load_state_dict(sd)
    assert other.n == 300 and other.result() == out
    with pytest.raises(ValueError, match="split_size"):
        InceptionScore(W, b, split_size=100, device=dev).load_state_dict(sd)
    isc.reset()
    assert isc.n == 0
    with pytest.raises(RuntimeError, match="no rows"):
        isc.result()
    isc.update(fg)  # one update instead of two: the same bits
    assert isc.result() == out
    one = InceptionScore(W, b, split_size=None, device=dev)
    one.update(fg)
    r = one.result()
    assert r["splits"] == 1 and r["is_std"] == 0.0
    assert abs(r["is"] - IR.inception_score(lg.double().cpu(), None)[0]) <= 1e-12 * r["is"]
    with pytest.raises(ValueError, match="no CPU path"):
        isc.update(f)


SHARD = 250  # rank 0 adds the rows [0, 250) (four slots of 64), rank 1 the rest (one slot): the ranks' states differ in size


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from vtp_amd import InceptionScore
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    f, W, b = _fc_case(10)
    isc = InceptionScore(W, b, split_size=64, device="cuda", group=dist.group.WORLD)
    isc.update((f[:SHARD] if rank == 0 else f[SHARD:]).to("cuda"))
    out[rank] = isc.result()
    dist.destroy_process_group()


def test_two_ranks_sum_their_slots():
    """each rank fills the slots in its own row order; result() sums [n_s | state] over the ranks: slot s holds rank 0's rows
    [64 s, 64 s + 64) and, for s = 0, rank 1's 50 rows"""
    from vtp_amd import InceptionScore
    from vtp_amd.inception_score import inception_score_from_sums
    dev = _dev()
    f, W, b = _fc_case(10)
    tables = []
    for part in (f[:SHARD], f[SHARD:]):
        isc = InceptionScore(W, b, split_size=64, device=dev)
        isc.update(part.to(dev))
        t = isc._gathered().numpy()
        tables.append(np.concatenate([t, np.zeros((4 - t.shape[0], t.shape[1]))]))
    both = tables[0] + tables[1]
    assert both[:, 0].tolist() == [114.0, 64.0, 64.0, 58.0]
    mean, std = inception_score_from_sums(both[:, 0], both[:, 1], both[:, 2:])
    want = {"is": mean, "is_std": std, "splits": 4}
    del isc
    torch.cuda.empty_cache()
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    for r in range(world):
        assert out[r] == want


# ---------------------------------------------------------------------------------------------------------------- forward_taps
@functools.lru_cache(maxsize=None)
def _weights():
    sd64 = R.seeded_state_dict(0, torch.float64)
    return sd64, {k: v.float() for k, v in sd64.items()}


def _rel(f, f64):
    return float((f.double().cpu() - f64).abs().max() / f64.abs().max())


@pytest.mark.parametrize("variant", ["torchvision", "pytorch_fid"])
def test_forward_taps_pool_bits_and_the_spatial_tap(variant):
    from vtp_amd import InceptionFeatures
    dev = _dev()
    sd64, sd32 = _weights()
    B, H, W = 3, 91, 107
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(B * H + W))
    s64 = IR.spatial_tap(sd64, x.double(), variant)
    e_cpu = _rel(IR.spatial_tap(sd32, x, variant), s64)
    e_gpu = _rel(IR.spatial_tap({k: v.to(dev) for k, v in sd32.items()}, x.to(dev), variant), s64)
    inc = InceptionFeatures(variant).reset_parameters(0).to(dev)
    pool, spatial = inc.forward_taps(x.to(dev))
    assert torch.equal(_bits(pool), _bits(inc(x.to(dev))))
    hw = (4, 5) if variant == "torchvision" else (17, 17)  # the input of Mixed_6d (tests/test_fid_host.py: Mixed_6a's output size)
    assert spatial.shape == s64.shape == (B, hw[0], hw[1], 7) and spatial.dtype == torch.float32 and spatial.is_contiguous()
    e_ours, e_ref = _rel(spatial, s64), max(e_cpu, e_gpu)
    print(f"forward_taps {variant}: E_ours {e_ours:.3e}  E_ref {e_ref:.3e} (cpu {e_cpu:.3e}, gpu {e_gpu:.3e})  ratio {e_ours / e_ref:.3f}")
    assert e_ours <= 2 * e_ref
    one = inc.forward_taps(x[1:2].to(dev))[1]  # an image's tap does not depend on its batch
    assert torch.equal(_bits(one[0]), _bits(spatial[1]))


def test_moved_and_reloaded_module_prepares_its_new_tap_weights():
    from vtp_amd import InceptionFeatures
    dev = _dev()
    x = torch.rand(1, 3, 80, 91, generator=torch.Generator().manual_seed(5)).to(dev)
    inc = InceptionFeatures().reset_parameters(0).to(dev)
    s0 = inc.forward_taps(x)[1]
    inc.cpu()
    inc.load_state_dict(R.seeded_state_dict(1))
    inc.to(dev)
    s1 = inc.forward_taps(x)[1]
    fresh = InceptionFeatures().reset_parameters(1).to(dev).forward_taps(x)[1]
    assert torch.equal(_bits(s1), _bits(fresh)) and not torch.equal(_bits(s1), _bits(s0))


# ---------------------------------------------------------------------------------------------------------------- GenEval
def _byte_images(seed, n, S=96):
    """smooth random byte images [n, S, S, 3]"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(n, 3, 8, 8, generator=g)
    img = F.interpolate(low, size=(S, S), mode="bicubic", align_corners=False) + 0.05 * torch.randn(n, 3, S, S, generator=g)
    return (img.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


VARIANT = "pytorch_fid"


@functools.lru_cache(maxsize=None)
def _gen_eval_case():
    """12 real and 10 generated byte images of 96 x 96 through GenEval in uneven batches, and its results (method "eig": a Frechet
    distance at D = 2023 / 2048 costs a second or more, scipy's matrix root three times that)"""
    from vtp_amd import GenEval, InceptionFeatures
    dev = _dev()
    inc = InceptionFeatures(VARIANT).reset_parameters(0).to(dev)
    _, W, b = _fc_case(10)
    sets = {"real": _byte_images(51, 12), "generated": _byte_images(52, 10)}
    real, gen = sets["real"].to(dev), sets["generated"].to(dev)
    ge = GenEval(inc, fc=(W, b), k=3, split_size=4)
    ge.add_real(real[:5])
    ge.add_real(real[5:])
    ge.add_generated(gen[:4])
    ge.add_generated(gen[4:])
    return inc, sets, real, gen, ge, ge.results("eig")


def test_gen_eval_equals_the_single_metric_classes_on_the_same_images():
    from vtp_amd import FID, InceptionScore, PrecisionRecall
    dev = _dev()
    inc, sets, real, gen, ge, out = _gen_eval_case()
    _, W, b = _fc_case(10)
    assert set(out) == {"fid", "sfid", "is", "is_std", "precision", "recall"}
    assert all(np.isfinite(v) for v in out.values())
    fid = FID(inc)
    f_real, f_gen = fid.features(real), fid.features(gen)
    fid.update_features(f_real, f_gen)
    assert out["fid"] == fid.result("eig")
    pr = PrecisionRecall(k=3)
    pr.add_real_features(f_real)
    pr.add_fake_features(f_gen)
    assert {k: out[k] for k in ("precision", "recall")} == pr.result()
    isc = InceptionScore(W, b, split_size=4, device=dev)
    isc.update(f_gen)
    r = isc.result()
    assert r["splits"] == 3 and (out["is"], out["is_std"]) == (r["is"], r["is_std"])


def test_gen_eval_sfid_against_the_fp64_restatement():
    """the spatial statistics and the distance against the fp64 restatement, held to twice the error the restatement's own fp32 runs
    (CPU and GPU) leave in the same figures (the margin of test_fid_update_against_the_fp64_pipeline)"""
    dev = _dev()
    inc, sets, real, gen, ge, out = _gen_eval_case()
    sd64, sd32 = _weights()
    sd32g = {k: v.to(dev) for k, v in sd32.items()}
    stats64, stats32 = {}, {"cpu": {}, "gpu": {}}
    for side, u8 in sets.items():
        x = u8.permute(0, 3, 1, 2).double() / 255
        n = x.shape[0]
        stats64[side] = R.statistics(IR.spatial_tap(sd64, x, VARIANT).reshape(n, -1).numpy())
        stats32["cpu"][side] = R.statistics(IR.spatial_tap(sd32, x.float(), VARIANT).reshape(n, -1).numpy())
        stats32["gpu"][side] = R.statistics(IR.spatial_tap(sd32g, x.float().to(dev), VARIANT).reshape(n, -1).cpu().numpy())
    rel = lambda a, a64: np.abs(a - a64).max() / np.abs(a64).max()
    for side in sets:
        mu64, s64 = stats64[side]
        assert mu64.shape == (2023,)  # 17 x 17 x 7
        e_mu = max(rel(stats32[w][side][0], mu64) for w in stats32)
        e_s = max(rel(stats32[w][side][1], s64) for w in stats32)
        mu, sigma = ge._spatial[side].mean_cov()
        o_mu, o_s = rel(mu, mu64), rel(sigma, s64)
        print(f"GenEval spatial {side}: mu E_ours {o_mu:.3e} E_ref {e_mu:.3e}; sigma E_ours {o_s:.3e} E_ref {e_s:.3e}")
        assert o_mu <= 2 * e_mu and o_s <= 2 * e_s
    sfid64 = R.frechet(*stats64["real"], *stats64["generated"])
    e_ref = max(abs(R.frechet(*stats32[w]["real"], *stats32[w]["generated"]) - sfid64) for w in stats32)
    e_ours = abs(out["sfid"] - sfid64)
    print(f"GenEval sfid {out['sfid']:.6f} (fp64 {sfid64:.6f})  E_ours {e_ours:.3e}  E_ref {e_ref:.3e}  ratio {e_ours / e_ref:.3f}")
    assert sfid64 > 0 and e_ours <= 2 * e_ref


def test_gen_eval_reference_statistics_in_place_of_real_images():
    from vtp_amd import GenEval
    inc, sets, real, gen, ge, out = _gen_eval_case()
    only = GenEval(inc, fc=None, k=3)
    only.set_reference(*ge.real.mean_cov())
    only.add_generated(gen)
    res = only.results("eig")
    assert set(res) == {"fid"} and res["fid"] == out["fid"]  # no real images: no precision, no recall, no sfid; no fc: no is
    with pytest.raises(ValueError):
        only.set_reference(np.zeros(7), np.zeros((7, 7)))
    with pytest.raises(ValueError, match="together"):
        only.set_reference(*ge.real.mean_cov(), mu_s=np.zeros(2023))
    only.reset()
    assert only.generated.n == 0
    with pytest.raises(RuntimeError, match="add_generated"):
        only.results()
