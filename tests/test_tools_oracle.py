"""CPU: the restated evaluation-tool plumbing (oracle/tools_oracle.py) against (a) the committed golden fixture
written from the REAL tools/test_*_hf.py functions driving the real reference VTPModel, with the oracle model behind the method
surface, and (b) the outputs of the real tool functions themselves (tests/golden/ref_pins.safetensors)."""
import os

import pytest
import torch
from safetensors.torch import load_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tg():
    return load_file(os.path.join(ROOT, "tests", "golden", "tools_tiny.safetensors"))


def test_restated_tools_on_the_oracle_model_reproduce_the_reference_tools(tg, golden_sd):
    from oracle import tools_oracle as T
    from oracle.ref_stubs import TINY
    m = T.OracleModel(golden_sd, 2, 2, 2)
    out = T.run_all(m, torch.device("cpu"), tg["in.images"], tg["in.targets"], TINY["text_vocab_size"], TINY["text_context_length"])
    assert set("out." + k for k in out) == set(k for k in tg if k.startswith("out."))
    for k, v in out.items():
        ref = tg["out." + k]
        assert v.shape == ref.shape, k
        err = float((v.float() - ref.float()).norm() / (ref.float().norm() + 1e-30))
        assert err < 2e-5, (k, err)  # fp32 vs fp32: summation order only
    assert torch.equal(out["zs.top"], tg["out.zs.top"])


def test_toy_tokenizer_layout():
    from oracle import tools_oracle as T
    tok = T.toy_tokenizer(512, 16)
    ids = tok(["a photo of a great white shark.", "x " * 40])
    assert ids.shape == (2, 16) and int(ids[0, 0]) == 510 and int(ids[0].max()) == 511 and int(ids[0].argmax()) == 8
    assert int(ids[1].argmax()) == 15 and (ids[1, 1:15] > 0).all() and (ids < 512).all()
    assert torch.equal(tok(["tench"]), tok(["tench"]))


def test_restated_tools_against_the_live_reference_tools(tg, golden_sd):
    """the real tool functions' own outputs on the reference model (recorded by oracle/make_golden_refpins.py) against the
    restatement's fixture (the checks oracle/make_golden_tools.py makes while it writes it) and against the restatement run now"""
    from oracle import tools_oracle as T
    from oracle.make_golden_refpins import digest, load, seen
    from oracle.ref_stubs import TINY
    g, meta = load()
    real = {k[len("tools/"):]: v for k, v in g.items() if k.startswith("tools/")}  # large ones at fixed sampled positions
    sha = {k[len("sha256/"):]: v for k, v in meta["tools"].items() if k.startswith("sha256/")}

    def vs(k, got):
        assert list(got.shape) == meta["tools"]["shapes"][k], k
        return seen(got, real[k]), real[k]

    assert torch.allclose(*vs("zs.classifier", tg["out.zs.classifier"]), atol=1e-6)
    assert torch.equal(real["zs.top"].float(), tg["out.zs.top"].float())
    for k in ("lp.patch0", "lp.cls0", "lp.patch1", "lp.cls1", "lp.input_1_avg", "lp.input_2"):
        assert digest(tg["out." + k]) == sha[k], k  # bit for bit
    assert abs(float(real["lp.avg_loss"]) - float(tg["out.lp.losses"].mean())) < 1e-5
    assert torch.allclose(*vs("lp.w_after", tg["out.lp.w_after"]), atol=1e-6)
    assert torch.allclose(real["rec.psnr"], tg["out.rec.psnr"].double(), atol=1e-4)
    out = T.run_all(T.OracleModel(golden_sd, 2, 2, 2), torch.device("cpu"), tg["in.images"], tg["in.targets"], TINY["text_vocab_size"],
                    TINY["text_context_length"])
    assert T.accuracy(out["zs.logits"], tg["in.targets"], topk=(1, 5)) == real["zs.accuracy"].tolist()
    assert out["zs.top"].tolist() == real["zs.top"].tolist()
    for k in ("zs.classifier", "lp.patch0", "lp.cls0", "lp.patch1", "lp.cls1", "lp.input_1_avg", "lp.input_2", "lp.w_after"):
        a, b = vs(k, out[k])
        err = float((a.float() - b.float()).norm() / (b.float().norm() + 1e-30))
        assert err < 2e-5, (k, err)  # fp32 vs fp32: summation order only
    assert abs(float(out["lp.losses"].mean()) - float(real["lp.avg_loss"])) < 1e-5
    assert torch.allclose(out["rec.psnr"].double(), real["rec.psnr"], atol=1e-3)
