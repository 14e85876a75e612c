"""Where the resident attention forward kernel spends its time: per (workgroup, wave) s_memrealtime stamps (vtp_attn_debug) at
start, first data, barrier, end of the key loop, stores, odd-tile share and merge -> µs since the wave's start (stamps x 10 ns),
per wave of one workgroup (head 3 of image 5).   AT_B=<images> python tools/attn_timing.py"""
import os
import sys

os.environ.setdefault("VTP_DIAG", "1")  # vtp_attn_debug: process-global hooks of production kernels
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vtp_amd import _lib, ops

HEAD, IMAGE = 3, 5
PHASES = ("first data", "barrier", "key loop", "stores", "odd tile", "merge")


def main():
    B, N, h = int(os.environ.get("AT_B", "64")), 257, 12
    assert B > IMAGE, "the workgroup printed is head 3 of image 5"
    D = 64 * h
    lib = _lib.load()
    torch.manual_seed(0)
    qkv = torch.randn(B * N, 3 * D, device="cuda").to(torch.bfloat16)
    o = torch.empty(B * N, D, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B * h * N, device="cuda")

    def fwd():
        ops.attn_fwd(qkv, qkv[:, D:], qkv[:, 2 * D:], o, lse, B, N, h, N * 3 * D, 3 * D, N * D, D, 0.125, False)

    for _ in range(3):
        fwd()
    tbuf = torch.zeros(B * h, 16, 8, dtype=torch.int64, device="cuda")  # [workgroup = image x heads + head][16 waves][8]
    try:
        _lib.check(lib.vtp_attn_debug(tbuf.data_ptr(), 0, 0, 0), "vtp_attn_debug")
        fwd()
        torch.cuda.synchronize()
    finally:
        lib.vtp_attn_debug(None, 0, 0, 0)
    t = tbuf[IMAGE * h + HEAD].cpu()
    for w in range(16):
        if t[w, 0] == 0:
            continue
        print(f"[attn timing] wave {w}: " + "  ".join(f"{nm} {(int(t[w, i + 1]) - int(t[w, 0])) / 100.0:.2f}"
                                                    for i, nm in enumerate(PHASES) if t[w, i + 1] > 0) + "  (us)")


if __name__ == "__main__":
    main()
