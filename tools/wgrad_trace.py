"""Every C call of a few tiny eager training steps, as text that two trees can be diffed by: the vtp_* attributes of the object
_lib.load() returns are replaced with recording wrappers (nothing of the package is patched, so the tool runs on any tree with this
C ABI).  One line per call: the name, every integer / float argument, every pointer as the ordinal of its first appearance in the
case.  For the grouped weight-gradient launches also the problem table and the work-item list, copied back from the device, the
table's pointers numbered the same way.  Cases (two steps each): the grouped path with the patch-embed problem held for block 0,
packed captions (a device token count), tail rows as two groups and as one mixed item list, and the per-layer path under stochastic
depth, LayerScale and a token count below 256.
Usage (GPU box): python tools/wgrad_trace.py --out wgrad_trace.txt [--case NAME]; the wall time of each case goes to stdout."""
import argparse
import ctypes
import gc
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vtp_amd import VTP, VTPConfig, VTPModel, VTPTrainer, _lib

DEV = "cuda"
TINY = dict(image_size=64, vision_embed_dim=128, vision_depth=2, vision_num_heads=2, text_embed_dim=128, text_depth=2,
            text_num_heads=2, text_vocab_size=512, text_context_length=16, decoder_embed_dim=128, decoder_depth=2, decoder_num_heads=2)
GROUPED = ("vtp_gemm_tn_grouped", "vtp_gemm_tn_grouped_limit", "vtp_gemm_tn_grouped_items")


class Recorder:
    def __init__(self, lib):
        self.lib, self.lines, self.ptrs, self.tables = lib, [], {}, {}
        path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
        self.hip = ctypes.CDLL(path)  # (already loaded: libvtp_hip.so links against it)
        self.hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        for name, types in _lib.SIGNATURES.items():
            setattr(lib, name, self._wrap(name, getattr(lib, name), types))

    def ptr(self, p):
        p = int(p or 0)
        return "null" if p == 0 else f"p{self.ptrs.setdefault(p, len(self.ptrs))}"

    def fetch(self, p, n, width, ctype):
        """n x width integers at device address p (static tables: read once, behind everything queued so far)"""
        if (p, n) not in self.tables:
            torch.cuda.synchronize()
            buf = (ctype * (n * width))()
            assert self.hip.hipMemcpy(buf, p, ctypes.sizeof(buf), 2) == 0  # 2: device to host
            self.tables[(p, n)] = [list(buf[i * width:(i + 1) * width]) for i in range(n)]
        return self.tables[(p, n)]

    def _wrap(self, name, fn, types):
        def call(*args):
            words = [self.ptr(a) if t is ctypes.c_void_p else repr(a) for a, t in zip(args, types)]
            self.lines.append(f"{name} " + " ".join(words))
            if name in GROUPED:
                for r in self.fetch(args[0], args[1], 16, ctypes.c_int64):  # GroupProblem: four pointers, twelve integers
                    self.lines.append("  problem " + " ".join([self.ptr(v) for v in r[:4]] + [str(v) for v in r[4:]]))
            if name == "vtp_gemm_tn_grouped_items":
                for r in self.fetch(args[4], args[5], 8, ctypes.c_int32):
                    self.lines.append("  item " + " ".join(map(str, r)))
            return fn(*args)
        return call

    def begin(self, case):
        self.ptrs = {}
        self.lines.append(f"=== {case}")


def _seeded(m, seed):
    torch.manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            if p.ndim <= 1 and p.numel() > 1:
                p.add_(0.05 * torch.randn_like(p))
    return m.to(DEV)


def _images(B, R, seed):
    return torch.randn(B, 3, R, R, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _captions(lengths, T, vocab, seed):
    ids = torch.randint(1, vocab - 1, (len(lengths), T), generator=torch.Generator().manual_seed(seed))
    for b, n in enumerate(lengths):
        ids[b, n - 1] = vocab - 1  # EOT: the arg-max
        ids[b, n:] = 0
    return ids.to(DEV)


def rec(B, R, steps, **kw):
    cfg = {k: kw.pop(k) for k in list(kw) if k.endswith("init_values") or k.endswith("_depth")}
    torch.manual_seed(8)
    m = _seeded(VTPModel(VTPConfig(**dict(TINY, image_size=R, **cfg))), 9)
    tr, img = VTPTrainer(m, lr=1e-3, weight_decay=0.0, **kw), _images(B, R, 3)
    for _ in range(steps):
        tr.step_rec(img)


def captions(steps):
    torch.manual_seed(4)
    m = _seeded(VTPModel(VTPConfig(**dict(TINY, vision_depth=1, decoder_depth=1, text_context_length=77))), 5)
    tr, img, ids = VTPTrainer(m, lr=5e-4, weight_decay=0.0), _images(4, 64, 2), _captions((9, 77, 40, 23), 77, 512, 1)
    for _ in range(steps):
        tr.step(img, ids)
    assert m._text.stack.varlen is not None, "the packed path was not taken"


def ssl(B, n_local, steps):
    """the student's list forward has B * 17 lead rows, 2 B * 17 global and n_local * B * 5 local rows; its last block keeps the lead
    rows, the class rows and the masked patches padded to a multiple of 64"""
    torch.manual_seed(0)
    cfg = VTPConfig(**dict(TINY, text_depth=1, text_vocab_size=64, text_context_length=8, decoder_depth=1))
    m = _seeded(VTP(cfg, dino_out_dim=512, dino_hidden_dim=128, dino_bottleneck_dim=64), 1)
    tr = VTPTrainer(m, lr=5e-4, weight_decay=0.0)
    g = torch.Generator().manual_seed(6)
    gc_, lc = torch.randn(2 * B, 3, 64, 64, generator=g).to(DEV), torch.randn(n_local * B, 3, 32, 32, generator=g).to(DEV)
    masks = np.random.default_rng(7).random((2 * B, 16)) < 0.4
    txt = torch.randint(1, 60, (B, 8), generator=g)
    txt[:, 5] = 63
    p = tr.prepare_ssl(gc_, lc, masks, pad_to=64)
    for _ in range(steps):
        tr.step(_images(B, 64, 3), txt.to(DEV), p)
    c = m._trunk.ctx()
    assert c.Mc < c.M, "the tail row plan was not taken"
    return f"M = {c.M}, Mc = {c.Mc}"


CASES = {
    "rec_grouped_M514": lambda n: rec(2, 256, n),
    "rec_captions_308_text_rows": captions,
    "ssl_tail_two_groups": lambda n: ssl(4, 4, n),                 # 284 and 156 rows: no multiples of 8
    "ssl_tail_mixed_items": lambda n: ssl(8, 2, n),                # 488 and 296 rows, VTP_GEMM4W_TN=1 (set in main)
    "rec_stochastic_depth": lambda n: rec(5, 64, n, vision_depth=3, drop_rate=0.4, decoder_drop_rate=0.4, drop_seed=3),
    "rec_layerscale": lambda n: rec(4, 64, n, vision_depth=3, vision_init_values=0.5, decoder_init_values=0.3),
    "rec_M17": lambda n: rec(1, 64, n),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--case", action="append", choices=list(CASES))
    ap.add_argument("--steps", type=int, default=2)
    a = ap.parse_args()
    gc.disable()  # tensors are freed where their last reference goes, on every tree alike: the caching allocator repeats its addresses
    r = Recorder(_lib.load())
    for name in a.case or CASES:
        os.environ.pop("VTP_GEMM4W_TN", None)
        if name == "ssl_tail_mixed_items":
            os.environ["VTP_GEMM4W_TN"] = "1"
        r.begin(name)
        n0, t0 = len(r.lines), time.perf_counter()
        note = CASES[name](a.steps)
        torch.cuda.synchronize()
        grouped = sum(ln.startswith(GROUPED) for ln in r.lines[n0:])
        print(f"# {name}: {time.perf_counter() - t0:.2f} s, {len(r.lines) - n0} lines, {grouped} grouped launches {note or ''}", flush=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(r.lines) + "\n")


if __name__ == "__main__":
    main()
