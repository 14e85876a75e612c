"""The Inception Score of vtp_amd.InceptionScore (csrc/inception_score.hip) and the sFID tap of InceptionFeatures.forward_taps restated
on the CPU.  Not a test module; imported by tests/test_inception_score_host.py and tests/test_inception_score_gpu.py.

inception_score() is written from the definition (Salimans et al. 2016): softmax, p (log p - log mean p), splits.  rows() is the
per-row reference of vtp_is_rows in 80-bit extended precision (numpy's longdouble on x86-64: a 64-bit significand, unit roundoff
2^-64), so that its own error -- a few 2^-64 per exp / log and C adds -- is 2^-11 of the fp64 bound the kernel is held to."""
import numpy as np
import torch
import torch.nn.functional as F

import fid_ref as R

U64 = 2.0 ** -53
TINY = 2.0 ** -1022  # the smallest normal double: below it a result carries no relative precision


def inception_score(logits, split_size=None):
    """(mean, population std, per-split scores) of exp(KL_s) over the splits of the rows, in the dtype of logits (give fp64).
    KL_s = mean_i sum_c p_ic (log p_ic - log m_c) with m_c = mean_i p_ic; a class nobody gives any probability contributes 0"""
    logits = torch.as_tensor(logits)
    n = logits.shape[0]
    step = n if split_size is None else int(split_size)
    scores = []
    for lo in range(0, n, step):
        part = logits[lo:lo + step]
        p, logp = torch.softmax(part, 1), torch.log_softmax(part, 1)
        m = p.mean(0, keepdim=True)
        terms = torch.where(p > 0, p * (logp - torch.log(torch.where(m > 0, m, torch.ones_like(m)))), torch.zeros_like(p))
        scores.append(torch.exp(terms.sum(1).mean()))
    scores = torch.stack(scores)
    return float(scores.mean()), float(scores.std(unbiased=False)), scores


def rows(logits):
    """(p [B, C], h [B], mag [B]) as longdouble arrays: the softmax of every row, h = sum_c p_c (l_c - lse) and mag = sum_c
    |p_c (l_c - lse)|.  log Z = log1p(sum over all columns but the first maximum of exp(l - max)): a row that is certain of one
    class keeps the entropy term of that class"""
    assert np.finfo(np.longdouble).nmant >= 63, "rows() needs the 80-bit long double of x86-64"
    l = np.asarray(logits, dtype=np.float32).astype(np.longdouble)
    at = np.arange(l.shape[0])
    j = l.argmax(1)  # the first maximum
    d = l - l[at, j][:, None]
    e = np.exp(d)
    rest = e.copy()
    rest[at, j] = 0
    z = rest.sum(1)
    log_z = np.log1p(z)
    p = e / (1 + z)[:, None]
    t = p * (d - log_z[:, None])
    return p, t.sum(1), np.abs(t).sum(1)


def sums(logits, split_size=None):
    """(n [s], H [s], S [s, C]) as fp64 arrays: the sums InceptionScore keeps per split, from rows()"""
    p, h, _ = rows(logits)
    n = p.shape[0]
    step = n if split_size is None else int(split_size)
    cuts = range(0, n, step)
    return (np.array([min(step, n - lo) for lo in cuts], dtype=np.float64),
            np.array([h[lo:lo + step].sum() for lo in cuts], dtype=np.float64),
            np.stack([p[lo:lo + step].sum(0) for lo in cuts]).astype(np.float64))


class _Reached(Exception):
    pass


class _UpTo(list):
    """a trace that ends the restated network once the named activation is there: the layers behind it are not needed"""

    def __init__(self, name):
        super().__init__()
        self.name = name

    def append(self, item):
        super().append(item)
        if item[0] == self.name:
            raise _Reached


def spatial_tap(sd, x, variant="torchvision"):
    """[B, h, w, 7] in the dtype of sd and x: the first 7 filters of Mixed_6d.branch1x1 (the bare convolution, no BatchNorm, no ReLU)
    on the input of Mixed_6d, which is the output of Mixed_6c in the restated network of fid_ref"""
    trace = _UpTo("Mixed_6c")
    try:
        R.features(sd, x, variant, trace)
    except _Reached:
        pass
    name, act = trace[-1]
    assert name == "Mixed_6c" and act.shape[1] == 768
    return F.conv2d(act, sd["Mixed_6d.branch1x1.conv.weight"][:7]).permute(0, 2, 3, 1).contiguous()
