"""CPU-side checks of the zero-shot evaluation (vtp_amd/zeroshot.py, csrc/zeroshot.hip): the caption lists handed to the tokenizer
against the restated tool (oracle/tools_oracle.py::build_zero_shot_classifier), the argument checks of the two entry points, and
what the class does without a GPU."""
import ctypes

import pytest
import torch

from oracle import tools_oracle as T


class _SpyTokenizer:
    def __init__(self):
        self.calls = []

    def __call__(self, texts):
        self.calls.append(list(texts))
        return torch.zeros(len(texts), 4, dtype=torch.long)


class _FakeModel:
    """seeded CPU features, one row per caption"""

    def __init__(self, D=8):
        self.D, self.g = D, torch.Generator().manual_seed(0)

    def get_clip_text_feature(self, tokens, normalize=True):
        f = torch.randn(tokens.shape[0], self.D, generator=self.g)
        return torch.nn.functional.normalize(f, dim=1) if normalize else f


@pytest.mark.parametrize("n", [1, 3, 10])
def test_caption_batches_feed_the_tokenizer_what_the_tool_feeds_it(n):
    from vtp_amd.zeroshot import caption_batches
    spy = _SpyTokenizer()
    clf = T.build_zero_shot_classifier(_FakeModel(), spy, T.CLASSNAMES, T.TEMPLATES, num_classes_per_batch=n, device="cpu")
    assert clf.shape == (8, len(T.CLASSNAMES))
    ours = list(caption_batches(T.CLASSNAMES, T.TEMPLATES, n))
    assert [texts for _, texts in ours] == spy.calls
    assert [c0 for c0, _ in ours] == list(range(0, len(T.CLASSNAMES), n))
    assert len(ours) == -(-len(T.CLASSNAMES) // n)
    last = len(T.CLASSNAMES) - ours[-1][0]
    assert len(ours[-1][1]) == last * len(T.TEMPLATES) and (n != 3 or last == 1)  # 7 classes in threes: a short last batch
    assert ours[0][1][:3] == ["a photo of a tench.", "a blurry photo of the tench.", "art of the tench."]  # templates vary fastest
    with pytest.raises(ValueError):
        list(caption_batches(T.CLASSNAMES, T.TEMPLATES, 0))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from vtp_amd import _lib
    return _lib.load()


def test_argument_validation_needs_no_gpu(lib):
    p = ctypes.c_void_p(16)
    err = lambda: lib.vtp_last_error()
    # class mean: feat ldf Wt ldw C T D eps
    assert lib.vtp_zs_class_mean(None, 8, p, 8, 2, 3, 8, 1e-12, None) == -1 and b"null" in err()
    assert lib.vtp_zs_class_mean(p, 8, None, 8, 2, 3, 8, 1e-12, None) == -1 and b"null" in err()
    assert lib.vtp_zs_class_mean(p, 8, p, 8, 2, 0, 8, 1e-12, None) == -1 and b"T >= 1" in err()
    assert lib.vtp_zs_class_mean(p, 8, p, 8, 0, 3, 8, 1e-12, None) == -1
    assert lib.vtp_zs_class_mean(p, 8, p, 8, 2, 3, 6, 1e-12, None) == -1 and b"D % 4" in err()
    assert lib.vtp_zs_class_mean(p, 4, p, 8, 2, 3, 8, 1e-12, None) == -1 and b"ldf" in err()
    assert lib.vtp_zs_class_mean(p, 8, p, 10, 2, 3, 8, 1e-12, None) == -1 and b"ldw % 4" in err()
    assert lib.vtp_zs_class_mean(ctypes.c_void_p(20), 8, p, 8, 2, 3, 8, 1e-12, None) == -1 and b"aligned" in err()
    # topk: F ldf Wt ldw targets scale B C D counts per_class rank pred logits ldl
    ok = [p, 8, p, 8, p, 100.0, 2, 7, 8, p, None, None, None, None, 0, None]
    for i in (0, 2, 4):
        a = list(ok)
        a[i] = None
        assert lib.vtp_zs_topk(*a) == -1 and b"null" in err(), i
    for i, v, msg in ((8, 6, b"D % 4"), (7, 4, b"C >= 5"), (6, 0, b"B >= 1"), (1, 4, b"ldf"), (3, 10, b"ldw % 4")):
        a = list(ok)
        a[i] = v
        assert lib.vtp_zs_topk(*a) == -1 and msg in err(), (i, err())
    a = list(ok)
    a[13], a[14] = p, 6  # logits given with a row stride below C
    assert lib.vtp_zs_topk(*a) == -1 and b"ldl" in err()
    a = list(ok)
    a[0] = ctypes.c_void_p(20)
    assert lib.vtp_zs_topk(*a) == -1 and b"aligned" in err()


def test_no_cpu_path_and_export():
    import vtp_amd
    from vtp_amd.zeroshot import ZeroShot
    assert vtp_amd.ZeroShot is ZeroShot
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ZeroShot(None)


def test_accuracy_before_any_update_raises():
    """accuracy() is percent(count, n) of the device counters; with nothing evaluated it raises instead of dividing by zero"""
    from vtp_amd import zeroshot
    with pytest.raises(RuntimeError, match="nothing evaluated"):
        zeroshot.percent(0, 0)
    assert zeroshot.percent(1, 8) == 1 / 8 * 100
    if torch.cuda.is_available():
        zs = zeroshot.ZeroShot(None)
        zs.set_classifier(torch.eye(8)[:, :6])
        with pytest.raises(RuntimeError, match="nothing evaluated"):
            zs.accuracy()
