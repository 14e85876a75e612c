#!/usr/bin/env python
"""Times the fp32 inference forward on one MI355X (seeded weights and inputs):

    gemm   vtp_gemm_nt_f32 at the shapes the VTP-B path runs at B = 32, 256 x 256 (M = 8192 decoder rows / 8224 trunk rows) and at
           4096^3: TFLOP/s against the 157.3 TFLOP/s peak of v_mfma_f32_32x32x2_f32 and the 122 TFLOP/s of an untuned LDS-tiled kernel
    attn   vtp_attn_fwd_f32 at B = 32, 12 heads, N = 257 / 256 / 77 (causal)
    path   trunk, decoder and text forward per batch: the fp32 path, the bf16 path (same calls, switch off) and the oracle's fp32
           formulation run by torch on the same GPU (oracle/vtp_oracle.py: F.linear / F.scaled_dot_product_attention in fp32 through
           torch's BLAS and SDPA back ends -- the only other fp32 implementation there is)

Without --what each part runs as a child process of its own under its own time limit, one after the other; the first that fails ends
the run.  Timings are HIP events around --iters calls after warm-up of the same shapes; --rounds windows are printed (median, min,
max), so the spread is on the page."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF, UNTUNED_TF = 157.3, 122.0


def _windows(fn, iters, rounds, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3 / iters)
    return out


def _line(res, t):
    res.update(median_us=statistics.median(t) * 1e6, min_us=min(t) * 1e6, max_us=max(t) * 1e6)
    if "flop" in res:
        res["tflops_median"] = res["flop"] / statistics.median(t) * 1e-12
        res["of_peak"] = res["tflops_median"] / PEAK_TF
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


def run_gemm(a):
    import torch
    from vtp_amd import ops
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    shapes = [(M, N, K, epi) for M in (8192, 8224) for N, K, epi in
              ((2304, 768, "plain"), (768, 768, "resid"), (2048, 768, "swiglu"), (768, 2048, "resid"))] + [(4096, 4096, 4096, "plain")]
    for M, N, K, epi in shapes:
        A = (torch.rand(M, K, generator=g) * 2 - 1).to(dev)
        W = (torch.rand(N, K, generator=g) * 2 - 1).to(dev)
        W2 = (torch.rand(N, K, generator=g) * 2 - 1).to(dev) if epi == "swiglu" else None
        bias = torch.zeros(N, device=dev)
        C, R = torch.empty(M, N, device=dev), (torch.zeros(M, N, device=dev) if epi == "resid" else None)
        kw = dict(plain=dict(bias=bias), resid=dict(bias=bias, resid=R, epi=ops.F32_RESID),
                  swiglu=dict(w2=W2, bias=bias, bias2=bias, epi=ops.F32_SWIGLU))[epi]
        t = _windows(lambda: ops.gemm_nt_f32(A, W, C, **kw), a.iters, a.rounds, a.warmup)
        flop = 2.0 * M * N * K * (2 if epi == "swiglu" else 1)  # SwiGLU with hidden width N multiplies by w1 and by w2
        _line({"what": "gemm", "M": M, "N": N, "K": K, "epi": epi, "flop": flop}, t)
    print(json.dumps({"what": "gemm", "note": f"peak {PEAK_TF} TFLOP/s; untuned LDS-tiled kernel of the programming guide at 4096^3: {UNTUNED_TF}"}))


def run_attn(a):
    import torch
    from vtp_amd import ops
    dev = "cuda"
    for B, heads, N, causal in ((32, 12, 257, False), (32, 12, 256, False), (32, 12, 77, True)):
        D = heads * 64
        qkv = torch.randn(B * N, 3 * D, device=dev)
        o = torch.empty(B * N, D, device=dev)
        t = _windows(lambda: ops.attn_fwd_f32(qkv, qkv[:, D:], qkv[:, 2 * D:], o, B, N, heads, N * 3 * D, 3 * D, N * D, D, 0.125, causal),
                     a.iters, a.rounds, a.warmup)
        flop = 4.0 * B * heads * N * N * 64 * (0.5 if causal else 1.0)
        _line({"what": "attn", "B": B, "heads": heads, "N": N, "causal": causal, "flop": flop}, t)


def run_path(a):
    import torch
    from oracle import vtp_oracle as O
    from vtp_amd import VTPConfig, VTPModel
    dev = "cuda"
    torch.manual_seed(0)
    cfg = VTPConfig()  # VTP-B
    m = VTPModel(cfg).to(dev).eval()
    B = a.batch
    g = torch.Generator().manual_seed(1)
    img = torch.randn(B, 3, 256, 256, generator=g).to(dev)
    text = torch.randint(0, cfg.text_vocab_size, (B, cfg.text_context_length), generator=g).to(dev)
    lat = m.get_reconstruction_latents(img)
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    hv, hd, ht = cfg.vision_num_heads, cfg.decoder_num_heads, cfg.text_num_heads
    calls = {"trunk": lambda: m.get_reconstruction_latents(img), "decoder": lambda: m.get_latents_decoded_images(lat),
             "text": lambda: m.get_clip_text_feature(text)}
    torch_calls = {"trunk": lambda: O.reconstruction_latents(sd, img, hv), "decoder": lambda: O.decoder_forward(sd, lat, hd),
                   "text": lambda: O.clip_text_feature(sd, text, ht)}
    for name, fn in calls.items():
        m.disable_fp32_forward()
        t16 = _windows(fn, a.iters, a.rounds, a.warmup)
        _line({"what": "path", "tower": name, "impl": "ours bf16", "B": B}, t16)
        m.enable_fp32_forward((name,))
        t32 = _windows(fn, max(a.iters // 4, 1), a.rounds, 2)
        _line({"what": "path", "tower": name, "impl": "ours fp32", "B": B, "x_bf16": statistics.median(t32) / statistics.median(t16)}, t32)
        m.disable_fp32_forward()
        with torch.no_grad():
            tt = _windows(torch_calls[name], max(a.iters // 4, 1), a.rounds, 2)
        _line({"what": "path", "tower": name, "impl": "torch fp32 (oracle formulation)", "B": B,
               "x_ours_fp32": statistics.median(tt) / statistics.median(t32)}, tt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["gemm", "attn", "path"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    a = ap.parse_args()
    if a.what is None:
        for what in ("gemm", "attn", "path"):
            cmd = [sys.executable, os.path.abspath(__file__), "--what", what, "--iters", str(a.iters), "--rounds", str(a.rounds),
                   "--warmup", str(a.warmup), "--batch", str(a.batch)]
            try:
                rc = subprocess.run(cmd, timeout=a.limit).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit(f"fp32_forward_bench: --what {what} ran into its {a.limit} s limit")
            if rc != 0:
                raise SystemExit(f"fp32_forward_bench: --what {what} failed (rc={rc})")
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fp32_forward_bench needs the MI355X: there is nothing to time on a CPU")
    {"gemm": run_gemm, "attn": run_attn, "path": run_path}[a.what](a)


if __name__ == "__main__":
    main()
