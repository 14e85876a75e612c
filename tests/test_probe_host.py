"""CPU-side checks of the linear probe (vtp_amd/probe.py, csrc/probe.hip): the sweep's head names and learning rates, the fp64
restatement the GPU tests compare against (tests/probe_ref.py) pinned to the REAL tool where the reference tree is present, the
argument checks of the three entry points, and the register report of the three kernels."""
import ctypes
import importlib.util
import os

import pytest
import torch

import probe_ref as R
from oracle.ref_stubs import reference_available

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the 13 rates of the tool's sweep times 128 / 256.  5e-6 and 1e-5 both print as 0.00001: the head created later (base rate 2e-5,
# scaled 1e-5) takes the key, as nn.ModuleDict does, and the reference trains 12 heads per feature group.
SCALED_128_1 = [("0_00001", 1e-5), ("0_00003", 2.5e-5), ("0_00005", 5e-5), ("0_00010", 1e-4), ("0_00025", 2.5e-4), ("0_00050", 5e-4),
                ("0_00100", 1e-3), ("0_00250", 2.5e-3), ("0_00500", 5e-3), ("0_01000", 1e-2), ("0_02500", 2.5e-2), ("0_05000", 5e-2)]
SCALED_128_8 = [("0_00004", 4e-5), ("0_00008", 8e-5), ("0_00020", 2e-4), ("0_00040", 4e-4), ("0_00080", 8e-4), ("0_00200", 2e-3),
                ("0_00400", 4e-3), ("0_00800", 8e-3), ("0_02000", 2e-2), ("0_04000", 4e-2), ("0_08000", 8e-2), ("0_20000", 0.2),
                ("0_40000", 0.4)]


def _expected(table):
    return [(f"classifier_{n}_blocks_avgpool_True_lr_{s}", n, True, lr) for n in (1, 4) for s, lr in table]


def _same(got, want):
    assert [h[:3] for h in got] == [h[:3] for h in want]
    for g, w in zip(got, want):
        assert g[3] == pytest.approx(w[3], rel=1e-12), (g, w)


@pytest.mark.parametrize("world,table,per_group", [(1, SCALED_128_1, 12), (8, SCALED_128_8, 13)])
def test_sweep_keys_and_learning_rates(world, table, per_group):
    from vtp_amd import probe
    heads = probe.resolve_heads(probe.sweep_heads(batch_size=128, world=world))
    assert len(heads) == 2 * per_group
    _same(heads, _expected(table))
    _same(R.sweep((1, 4), probe.DEFAULT_LEARNING_RATES, 128, world), _expected(table))
    assert len(probe.sweep_heads(batch_size=128, world=world)) == 26  # unresolved: every head the tool creates


@pytest.fixture(scope="module")
def tool():
    if not reference_available():
        pytest.skip("reference tree not present")
    from oracle.make_golden_tools import load_tool
    return load_tool("test_linear_probing_hf")


def _sample(B, T, D, n, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple((torch.randn(B, T, D, generator=g), torch.randn(B, D, generator=g)) for _ in range(n))


def _ref_rates(clfs, groups):
    lr_of = {}
    for g in groups:
        g["params"] = list(g["params"])
        lr_of[id(g["params"][0])] = g["lr"]
    return [(k, m.use_n_blocks, m.use_avgpool, lr_of[id(m.linear.weight)]) for k, m in clfs.classifiers_dict.items()]


@pytest.mark.parametrize("world", [1, 8])
def test_sweep_matches_the_tool(tool, monkeypatch, world):
    """keys, order, learning rates and -- under the same seed -- initial weights equal setup_linear_classifiers' (:221-254)"""
    from vtp_amd import probe
    D, C = 8, 5
    monkeypatch.setattr(tool, "get_world_size", lambda: world)
    torch.manual_seed(3)
    clfs, groups = tool.setup_linear_classifiers(_sample(2, 3, D, 4, 0), (1, 4), tool.DEFAULT_LEARNING_RATES, 128, C, torch.device("cpu"))
    assert tuple(probe.DEFAULT_LEARNING_RATES) == tuple(tool.DEFAULT_LEARNING_RATES)
    heads = probe.sweep_heads(batch_size=128, world=world)
    _same(probe.resolve_heads(heads), _ref_rates(clfs, groups))
    _same(R.sweep((1, 4), tool.DEFAULT_LEARNING_RATES, 128, world), _ref_rates(clfs, groups))
    torch.manual_seed(3)
    init = probe.init_heads(heads, D, C)
    assert list(init) == list(clfs.classifiers_dict.keys())
    for k, m in clfs.classifiers_dict.items():
        assert torch.equal(init[k][0], m.linear.weight.data) and torch.equal(init[k][1], m.linear.bias.data), k


def test_restatement_matches_the_tool(tool, monkeypatch):
    """tests/probe_ref.py in fp64 against AllClassifiers + SGD + CosineAnnealingLR + CrossEntropyLoss in fp32: 4 steps, 2 groups of 3
    heads, B = 8, D = 16, C = 7.  1e-5 = the project's bar for fp32 arithmetic against fp64 (tests/test_losses_gpu.py)."""
    B, T, D, C, n_max, steps = 8, 5, 16, 7, 2, 4
    monkeypatch.setattr(tool, "get_world_size", lambda: 1)
    torch.manual_seed(1)
    clfs, groups = tool.setup_linear_classifiers(_sample(B, T, D, n_max, 0), (1, 2), (0.1, 0.5, 2.0), 256, C, torch.device("cpu"))
    heads = _ref_rates(clfs, groups)
    assert len(heads) == 6
    ref = R.RefProbe(heads, {k: (m.linear.weight.data, m.linear.bias.data) for k, m in clfs.classifiers_dict.items()}, D, 0.9, steps)
    opt = torch.optim.SGD(groups, momentum=0.9, weight_decay=0)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, steps, eta_min=0)
    crit = torch.nn.CrossEntropyLoss()
    for s in range(steps):
        feats = _sample(B, T, D, n_max, 10 + s)
        labels = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(20 + s))
        out = clfs(feats)
        losses = {k: crit(v, labels) for k, v in out.items()}
        opt.zero_grad()
        sum(losses.values()).backward()
        opt.step()
        sched.step()
        mine = ref.step(R.x_all_of(feats, n_max), labels)
        for k in losses:
            assert mine[k] == pytest.approx(float(losses[k].detach()), rel=1e-5), (s, k)
    for k, m in clfs.classifiers_dict.items():
        for got, want in ((ref.W[k], m.linear.weight.data.double()), (ref.b[k], m.linear.bias.data.double())):
            assert float((got - want).norm() / want.norm()) <= 1e-5, k
        assert ref.evaluate(R.x_all_of(feats, n_max), labels)[k] == int((m(feats).argmax(dim=1) == labels).sum())


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from vtp_amd import _lib
    return _lib.load()


def test_argument_validation_needs_no_gpu(lib):
    p = ctypes.c_void_p(16)
    err = lambda: lib.vtp_last_error()
    # logits: X ldx W bias logits ldl B N K
    assert lib.vtp_probe_logits(None, 8, p, p, p, 8, 2, 8, 8, None) == -1 and b"null" in err()
    assert lib.vtp_probe_logits(p, 8, p, p, None, 8, 2, 8, 8, None) == -1 and b"null" in err()
    assert lib.vtp_probe_logits(p, 8, p, p, p, 8, 2, 8, 6, None) == -1 and b"K % 4" in err()
    assert lib.vtp_probe_logits(p, 4, p, p, p, 8, 2, 8, 8, None) == -1 and b"ldx >= K" in err()
    assert lib.vtp_probe_logits(p, 10, p, p, p, 8, 2, 8, 8, None) == -1 and b"ldx % 4" in err()
    assert lib.vtp_probe_logits(p, 8, p, p, p, 7, 2, 8, 8, None) == -1 and b"ldl" in err()
    assert lib.vtp_probe_logits(p, 8, p, p, p, 8, 0, 8, 8, None) == -1
    assert lib.vtp_probe_logits(ctypes.c_void_p(20), 8, p, p, p, 8, 2, 8, 8, None) == -1 and b"aligned" in err()
    # ce: logits ldl labels B H C inv_rows loss correct dlogits
    assert lib.vtp_probe_ce(None, 8, p, 2, 2, 4, 0.5, p, None, None, None) == -1 and b"null" in err()
    assert lib.vtp_probe_ce(p, 8, None, 2, 2, 4, 0.5, p, None, None, None) == -1 and b"null" in err()
    assert lib.vtp_probe_ce(p, 8, p, 2, 2, 4, 0.5, None, None, None, None) == -1 and b"null" in err()
    assert lib.vtp_probe_ce(p, 8, p, 2, 2, 0, 0.5, p, None, None, None) == -1 and b"C >= 1" in err()
    assert lib.vtp_probe_ce(p, 7, p, 2, 2, 4, 0.5, p, None, None, None) == -1 and b"ldl" in err()
    # sgd: W bias mW mb dlogits ldl X ldx lr B H C K momentum
    ok = [p, p, p, p, p, 8, p, 8, p, 2, 2, 4, 8, 0.9, None]
    for i in (0, 1, 2, 3, 4, 6, 8):
        a = list(ok)
        a[i] = None
        assert lib.vtp_probe_sgd(*a) == -1 and b"null" in err(), i
    for i, v, msg in ((12, 6, b"K % 4"), (7, 4, b"ldx >= K"), (7, 10, b"ldx % 4"), (11, 0, b"C >= 1"), (5, 7, b"ldl"), (9, 0, b"B")):
        a = list(ok)
        a[i] = v
        assert lib.vtp_probe_sgd(*a) == -1 and msg in err(), (i, err())


def test_probe_kernels_do_not_spill(lib):
    spec = importlib.util.spec_from_file_location("spill_report", os.path.join(ROOT, "tools", "spill_report.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    obj = os.path.join(ROOT, "vtp_amd", "lib", "probe.o")
    rows = {name: vs for name, vs, *_ in sr.report_built(obj)}
    for k in ("vtp::probe_logits_kernel", "vtp::probe_ce_kernel", "vtp::probe_sgd_kernel"):
        hit = [n for n in rows if n.startswith(k + "(")]
        assert hit, f"kernel {k} not in {obj}: {sorted(rows)}"
        assert rows[hit[0]] == 0, f"{k}: {rows[hit[0]]} spilled VGPRs"
    assert len(rows) == 3, sorted(rows)


def test_cpu_tensors_raise_and_export():
    import vtp_amd
    from vtp_amd.probe import LinearProbe
    assert vtp_amd.LinearProbe is LinearProbe
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            LinearProbe(None, [("a", 1, True, 0.1)], 3, embed_dim=4)
