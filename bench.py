#!/usr/bin/env python
"""bench.py -- VTP training-step throughput on MI355X (the BASELINE.json metric).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus N --steps K --warmup W          (no launcher in the environment: re-runs itself under the next form)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = one full optimizer step of the hot path on one batch of synthetic 256x256 images already resident in HBM
(forward, loss, backward, gradient all-reduce, fused AdamW, bf16 weight refresh).  Default workload: VTP-Base f16d64,
32 images per GPU (BASELINE config 3's per-GPU shard; weak scaling), all three objectives: reconstruction (L1; LPIPS with
--perceptual-weight), contrastive (InfoNCE with feature all-gather) and self-supervised (DINO + iBOT, EMA teacher);
config.workload says exactly what ran.  Rank 0 prints ONE JSON line.

Inside the timed region, EVERY step draws fresh block-wise iBOT masks (vtp_amd.data.collate_ssl_masks, host numpy), builds
the SSL index plan (VTPTrainer.prepare_ssl) and copies it to the device -- one batch ahead of the step that consumes it, as a
prefetching loader does (the draw for step k + 1 is issued while the GPU runs step k; K timed steps = K draws): the captured
hipGraph is keyed by the padded masked-token buffer size (the collate's `upperbound`, vtp.py:432-439) and serves every draw.  The image / caption / crop
tensors stay resident in HBM (the contract's "inputs already resident").

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line.  With --full it goes on, after the timed
steps (their figures do not change), with what takes runs of its own: `lpips_on` repeats the measurement (fewer steps) with the
perceptual term of north_star switched on, `separate_passes` with rec and clip on different input tensors, and further on the line:
  roofline     -- the dominant kernel (gemm_nt bf16 MFMA GEMM): algorithmic FLOPs (2*M*N*K per launch) / average launch
                  duration measured with HIP events on the launch stream over one instrumented step run right after
                  the timed region (kept out of it so event overhead cannot inflate `value`); peak = 2.5 PFLOP/s dense
                  bf16 (MI355X_MICROARCH.md).  `step_frac` is the whole-step figure of BASELINE.md §4
                  (images/s/GPU x GFLOP/image / 2.5e6).
  cpu_baseline -- the CPU oracle (oracle/vtp_oracle.py, kind "port": a PyTorch-fp32 restatement of the reference, which
                  is itself PyTorch) running the same train step on the host cores on a bounded sample.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0

_SMALL = dict(vision_embed_dim=384, vision_depth=12, vision_num_heads=6, text_embed_dim=384, text_depth=12,
              text_num_heads=6, decoder_embed_dim=384, decoder_depth=12, decoder_num_heads=6)
_LARGE = dict(vision_embed_dim=1024, vision_depth=24, vision_num_heads=16, text_embed_dim=1024, text_depth=24,
              text_num_heads=16, decoder_embed_dim=1024, decoder_depth=24, decoder_num_heads=16)
PEAK_FP8_TFLOPS = 5000.0
ROLL = {}   # N > 1: result of the rank roll-call all-reduce (ranks seen, backend, RCCL version) -> `comm` of the JSON line
# forward-only workloads (no optimizer step): BASELINE config 5
FORWARD_WORKLOADS = {
    "vtp_large_fp8_fwd": (_LARGE, 64, 256),   # VTP-L encode -> decode, fp8 (e4m3) MFMA GEMMs, 64 img/GPU
}
WORKLOADS = {
    # name: (config kwargs, per-GPU batch, resolution, objectives)
    "vtp_base_full": (dict(), 32, 256, ("rec", "clip", "ssl")),  # BASELINE config 3: contrastive + SSL + recon
    "vtp_base_rec_clip": (dict(), 32, 256, ("rec", "clip")),
    "vtp_base_rec": (dict(), 32, 256, ("rec",)),
    "vtp_small_rec": (_SMALL, 64, 256, ("rec",)),               # BASELINE config 2
    "vtp_large_full_512": (_LARGE, 16, 512, ("rec", "clip", "ssl")),  # BASELINE config 4: long sequences (N = 1025)
}


def synthetic_captions(B, T, vocab, device, seed):
    """ids ~ U{1..vocab-3}, SOT = vocab-2 first, EOT = vocab-1 at a random length in [8, T-1], zeros after
    (so the argmax pooling of text_transformer.py:222-224 hits EOT)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, vocab - 2, (B, T), generator=g)
    ids[:, 0] = vocab - 2
    ln = torch.randint(8, T, (B,), generator=g)
    ar = torch.arange(T)[None, :]
    ids = torch.where(ar < ln[:, None], ids, torch.zeros_like(ids))
    ids[torch.arange(B), ln] = vocab - 1
    return ids.to(device)


def synthetic_crops(B, res, device, seed, local_res=96, n_local=8):
    """2 global crops at res^2 + 8 local crops at 96^2 per image (DINOv2 convention, unpinned)."""
    g = torch.Generator(device=device).manual_seed(seed)
    gc = torch.randn(2 * B, 3, res, res, device=device, generator=g)
    lc = torch.randn(n_local * B, 3, local_res, local_res, device=device, generator=g)
    return gc, lc


class MaskStream:
    """Fresh iBOT masks per step: half of the global crops masked block-wise at ratios stratified over (0.1, 0.5) (the
    DINOv2 collate, vtp_amd/data.py); `upperbound` is the same for every draw, so one captured graph serves them all."""

    def __init__(self, B, res, seed):
        import numpy as np
        from vtp_amd.data import collate_ssl_masks
        self.rng = np.random.default_rng(seed)
        self.n, self.grid, self.collate = 2 * B, (res // 16, res // 16), collate_ssl_masks

    def draw(self):
        d = self.collate(self.n, self.grid, 0.5, (0.1, 0.5), self.rng)
        return d["masks"], d["upperbound"]


DUMP_SAMPLE = 1 << 20      # --dump-outputs: elements kept of a larger array (the same seeded subset on every run)
DUMP_PARAM_SAMPLE = 2048   # elements kept per parameter tensor of the updated weights
DUMP_LIMIT = 64 << 20      # bytes written in all


def _sample(t, n, seed):
    """t flattened; more than n elements: the n at fixed seeded positions (sorted), so two runs pick the same ones"""
    flat = t.detach().reshape(-1)
    if flat.numel() <= n:
        return flat
    idx = torch.randint(0, flat.numel(), (n,), generator=torch.Generator().manual_seed(seed)).sort().values
    return flat[idx.to(flat.device)]


def dump_outputs(path, arrays):
    """--dump-outputs DIR: writes DIR/<name>.npy for every array (float64 stays float64, everything else float32)"""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    host = {}
    for name, t in arrays.items():
        t = _sample(t, DUMP_SAMPLE, 0)
        host[name] = t.double().cpu().numpy() if t.dtype == torch.float64 else t.float().cpu().numpy()
    total = sum(a.nbytes for a in host.values())
    assert total <= DUMP_LIMIT, f"--dump-outputs: {total} bytes > {DUMP_LIMIT}"
    for name, a in host.items():
        np.save(os.path.join(path, name + ".npy"), a)
    print(f"[bench] wrote {len(host)} arrays ({total / 1e6:.2f} MB) to {path}", file=sys.stderr, flush=True)


def param_sample(model):
    """the weights after the step: DUMP_PARAM_SAMPLE seeded elements of every floating-point state-dict tensor, in state-dict order"""
    parts = [_sample(v, DUMP_PARAM_SAMPLE, i).float() for i, v in enumerate(model.state_dict().values()) if v.is_floating_point()]
    return torch.cat(parts)


def text_fwd_gflop(D, L, T):
    return (L * (2 * T * 12 * D * D + 4 * T * T * D) + 2 * D * D) / 1e9


def vit_fwd_gflop(D, H, L, N, hw, enc: bool):
    """BASELINE.md §4 / SURVEY.md §8d algorithmic FLOPs of one forward, per image."""
    f = L * (2 * N * (4 * D * D + 3 * D * H) + 4 * N * N * D)
    if enc:
        f += 2 * hw * 768 * D + 2 * N * D * 64
    else:
        f += 2 * hw * 64 * D + 2 * hw * D * 768
    return f / 1e9


def cpu_baseline(model, B_cpu, res, clip, do_ssl, n_fp32=5, n_bf16=3):
    """The CPU oracle (kind "port": oracle/vtp_oracle.py is a PyTorch restatement of the reference, itself PyTorch) timed on
    the host cores on a bounded sample of the SAME workload: one full train step (fwd + every loss that ran on the GPU + autograd
    bwd + AdamW) at a scaled-down batch in fp32 and under torch.autocast("cpu", bf16) (bounded: see below)."""
    from oracle import vtp_oracle as O
    import numpy as np
    from vtp_amd.data import collate_ssl_masks
    cfg = model.config
    sd = {k: v.detach().float().cpu().clone() if v.dtype == torch.float32 else v.detach().cpu().clone()
          for k, v in model.state_dict().items()}
    train_pref = ("trunk.", "pixel_decoder.") + (("visual_proj.", "text_transformer.", "token_embedding.", "positional_embedding",
                                                   "ln_final.", "text_projection", "logit_scale") if clip else ()) \
        + (("dino_head.",) if do_ssl else ())
    keys = [k for k in sd if sd[k].dtype == torch.float32 and k.startswith(train_pref)]
    for k in keys:
        sd[k].requires_grad_(True)
    opt = torch.optim.AdamW([sd[k] for k in keys], lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05)
    g = torch.Generator().manual_seed(99)
    img = torch.randn(B_cpu, 3, res, res, generator=g)
    txt = synthetic_captions(B_cpu, cfg.text_context_length, cfg.text_vocab_size, "cpu", 98)
    hv, hd, ht = cfg.vision_num_heads, cfg.decoder_num_heads, cfg.text_num_heads
    if do_ssl:
        gc = torch.randn(2 * B_cpu, 3, res, res, generator=g)
        lc = torch.randn(8 * B_cpu, 3, 96, 96, generator=g)
        masks = collate_ssl_masks(2 * B_cpu, (res // 16, res // 16), 0.5, (0.1, 0.5), np.random.default_rng(97))["masks"]
        K = sd["dino_head.last_layer.weight_v"].shape[0]
        c_d, c_i = torch.zeros(K), torch.zeros(K)
    n_thr = torch.get_num_threads()

    def step():
        opt.zero_grad(set_to_none=True)
        if clip:
            l1, lc_ = O.rec_clip_train_loss(sd, img, txt, hv, hd, ht)
            loss = l1 + lc_
        else:
            loss = O.rec_train_loss(sd, img, hv, hd)
        if do_ssl:
            t_out, s_out = O.ssl_outputs(sd, gc, lc, masks, hv)
            loss = loss + O.ssl_loss(t_out, s_out, masks, c_d, c_i, 8)
        loss.backward()
        opt.step()

    def timed(autocast, n_warm, n_timed):
        import contextlib
        ctx = (lambda: torch.autocast("cpu", dtype=torch.bfloat16)) if autocast else contextlib.nullcontext
        ts = []
        for i in range(n_warm + n_timed):
            t0 = time.perf_counter()
            with ctx():
                step()
            if i >= n_warm:
                ts.append(time.perf_counter() - t0)
        raw = list(ts)
        ts.sort()
        return ts[len(ts) // 2], len(ts), raw

    # SURVEY.md §8d asks for bs 8, 2 warm-up + 10 timed steps in fp32 AND under bf16 autocast; the full step (K = 65536 prototypes, 10
    # crops per image) costs ~7 s per image on a 128-thread host, so that protocol would be ~25 minutes.  Bounded sample (task contract:
    # tens of seconds of CPU work per leg): batch 2, fp32 1 warm-up + 5 timed steps, bf16 autocast 1 warm-up + 3 timed steps (round 5;
    # round 4 timed 2 + 1) -- the median is the reported `value`, every sample is in the line.
    t32, n32, s32 = timed(False, 1, n_fp32)
    t16, n16, s16 = timed(True, 1, n_bf16)
    auto = {"value": round(B_cpu / t16, 3), "unit": "images/sec", "steps": n16, "ms_per_step": round(t16 * 1e3, 1),
            "samples_ms": [round(t * 1e3, 1) for t in s16],
            "note": 'same step under torch.autocast("cpu", dtype=torch.bfloat16), 1 warm-up'}
    objs = "L1" + ("+CLIP" if clip else "") + ("+DINO/iBOT (K=%d prototypes, 2 global + 8 local crops/img, EMA-teacher fwd)" % K if do_ssl else "")
    return {"value": round(B_cpu / t32, 3), "unit": "images/sec", "cores": n_thr, "host_cpus": os.cpu_count(), "kind": "port",
            "kind_note": "the oracle (oracle/vtp_oracle.py, pinned to the real reference by tests/test_oracle_vs_reference.py and the "
                         "golden fixtures); the reference tree itself does not travel to the GPU box and ships no loss / optimizer",
            "sample": f"median of {n32} fp32 train steps (fwd + {objs} loss + bwd + AdamW) of the same model at batch {B_cpu} "
                      f"after 1 warm-up step; SURVEY §8d's bs-8 / 10-step protocol is ~25 min of host time and is not run",
            "samples_ms_fp32": [round(t * 1e3, 1) for t in s32],
            "bf16_autocast": auto, "ms_per_step_fp32": round(t32 * 1e3, 1), "threads": n_thr}


def e2e_parity(model, res, dev):
    """north_star's "encode / decode outputs within 1e-3 of the reference": per op that holds (tests/test_kernels_gpu.py); end to end
    the reference's OWN bf16-autocast path deviates from its fp32 path by more than that, so the line carries both numbers -- ours and
    the reference algorithm's (the oracle under torch.autocast on this GPU) against the oracle in fp32, same weights, 4 images.
    Part of the oracle leg of the bench (the oracle is the checker here, nothing timed)."""
    from oracle import vtp_oracle as O
    cfg = model.config
    hv, hd = cfg.vision_num_heads, cfg.decoder_num_heads
    img = torch.randn(4, 3, res, res, device=dev, generator=torch.Generator(device=dev).manual_seed(2025))
    with torch.no_grad():
        lat = model.get_reconstruction_latents(img)
        rec = model.get_latents_decoded_images(lat)
        sd = {k: v.detach() for k, v in model.state_dict().items()}
        lat_r = O.reconstruction_latents(sd, img, hv)
        rec_r = O.decoder_forward(sd, lat_r, hd)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            lat_b = O.reconstruction_latents(sd, img, hv).float()
            rec_b = O.decoder_forward(sd, lat_b, hd).float()
    mx = lambda a, b: float((a.float() - b.float()).abs().max())
    rl = lambda a, b: float((a.float() - b.float()).norm() / b.float().norm())
    return {"images": 4, "latents_max_abs": {"ours": round(mx(lat, lat_r), 5), "reference_bf16_autocast": round(mx(lat_b, lat_r), 5)},
            "reconstruction_max_abs": {"ours": round(mx(rec, rec_r), 5), "reference_bf16_autocast": round(mx(rec_b, rec_r), 5)},
            "latents_rel": {"ours": round(rl(lat, lat_r), 6), "reference_bf16_autocast": round(rl(lat_b, lat_r), 6)},
            "reconstruction_rel": {"ours": round(rl(rec, rec_r), 6), "reference_bf16_autocast": round(rl(rec_b, rec_r), 6)},
            "note": "vs the oracle in fp32 on this GPU (stock PyTorch kernels); training-step parity at this geometry: "
                    "tests/test_parity_bench_gpu.py"}


def bench_forward(args, world, rank, dev):
    """BASELINE config 5: VTP-L encode -> decode throughput with the linear maps on the fp8 (e4m3) MFMA path; the bf16 path of the
    same model is timed beside it and the output difference is reported (random-init weights, synthetic images).  Independent
    images: ranks are replicas with their own batch, no data-path collective."""
    from vtp_amd import VTPConfig, VTPModel, ops
    cfg_kw, B, res = FORWARD_WORKLOADS[args.workload]
    B = args.batch or B
    torch.manual_seed(0)
    model = VTPModel(VTPConfig(**cfg_kw)).to(dev).eval()
    img = torch.randn(B, 3, res, res, device=dev, generator=torch.Generator(device=dev).manual_seed(1234 + rank))

    def sync():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    def one_step():
        lat = model.get_reconstruction_latents(img)
        return lat, model.get_latents_decoded_images(lat)

    def timed(steps, warmup):
        for _ in range(warmup):
            one_step()
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = one_step()
        sync()
        el = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            el = float(t)
        return el, out

    el_bf16, err, recs = None, None, []
    with torch.no_grad():
        n_bf16 = max(2, args.steps // 2)
        if args.full:
            el_bf16, (lat_b, rec_b) = timed(n_bf16, max(1, args.warmup // 2))
        model.enable_fp8_forward(img[: min(B, 16)])
        el, (lat_8, rec_8) = timed(args.steps, args.warmup)
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, {"latents": lat_8, "reconstruction": rec_8})
        if args.full:
            rec_same = model.get_latents_decoded_images(lat_b)
            rel = lambda a, b: float((a - b).norm() / b.norm())
            err = {"latents_rel": round(rel(lat_8, lat_b), 5), "decoder_rel_same_latents": round(rel(rec_same, rec_b), 5),
                   "end_to_end_rel": round(rel(rec_8, rec_b), 5)}
            # roofline of the dominant kernel: HIP events around every fp8 GEMM launch of one extra pass (rank 0)
            orig = ops.gemm_nt_fp8

            def probe(a8, b8, c, **kw):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                orig(a8, b8, c, **kw)
                e1.record()
                recs.append((2.0 * kw["M"] * kw["N"] * kw["K"], e0, e1))

            ops.gemm_nt_fp8 = probe
            try:
                one_step()
                torch.cuda.synchronize()
            finally:
                ops.gemm_nt_fp8 = orig
    c = model.config
    hw = (res // 16) ** 2
    from vtp_amd.config import swiglu_hidden
    enc = vit_fwd_gflop(c.vision_embed_dim, swiglu_hidden(c.vision_embed_dim), c.vision_depth, hw + 1, hw, True)
    dec = vit_fwd_gflop(c.decoder_embed_dim, swiglu_hidden(c.decoder_embed_dim), c.decoder_depth, hw, hw, False)
    ips = world * B * args.steps / el
    out = {"metric": "images/sec/node VTP-L f16d64 fp8 forward encode->decode 256x256", "value": round(ips, 2), "unit": "images/sec",
           "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(el / args.steps * 1e3, 3),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "fp8 e4m3 GEMM operands (per-tensor scales), fp32 accumulation, bf16 attention / fp32 residual", "data": "synthetic",
           "config": {"workload": f"{args.workload}: get_reconstruction_latents + get_latents_decoded_images of VTP-L (1024/24/16 trunk and "
                                  f"pixel decoder), {B} img/GPU @ {res}x{res}, random-init weights, activation scales calibrated on 16 images",
                      "per_gpu_batch": B, "global_batch": world * B, "resolution": res, "parallelism": f"dp{world} (replicas)",
                      "fwd_gflop_per_image": round(enc + dec, 1)},
           "bf16_path": {"value": round(world * B * n_bf16 / el_bf16, 2), "unit": "images/sec", "ms_per_step": round(el_bf16 / n_bf16 * 1e3, 3)}
           if args.full else None,
           "fp8_vs_bf16": err,
           "step_tflops_per_gpu": round(ips / world * (enc + dec) / 1e3, 1)}
    if rank == 0:
        out["roofline"] = None
        if args.full:
            fl = sum(r[0] for r in recs)
            ms = sum(r[1].elapsed_time(r[2]) for r in recs)
            ach = fl / (ms * 1e-3) / 1e12
            out["roofline"] = {"bound": "mfma", "kernel": "vtp::gemm8p_kernel<.., VAR=8> (v_mfma_f32_32x32x64_f8f6f4, e4m3 x e4m3)",
                               "achieved": round(ach, 1), "peak": PEAK_FP8_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / PEAK_FP8_TFLOPS, 4),
                               "traffic": None, "launches_per_step": len(recs), "gemm_ms_per_step": round(ms, 3)}
        out["cpu_baseline"] = None  # reported on the default workload (the reference has no fp8 path)
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


def self_launch(n: int):
    """`python bench.py --gpus N` started WITHOUT a launcher (no WORLD_SIZE in the environment): re-run the same command line
    under `python -m torch.distributed.run`, one rank per GPU, rendezvous on 127.0.0.1 and a free port; rank 0's JSON line goes
    to this process's stdout unchanged and the launcher's exit code is ours.  The torchrun form of the docstring keeps working
    (it sets WORLD_SIZE, so this function is never reached)."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    # host side of a rank = mask collate + launch enqueue: N ranks must not each spin up one OpenMP thread per host core
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n) // n)))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print(f"[bench] no launcher in the environment: re-running under torch.distributed.run with {n} ranks (port {port}, "
          f"OMP_NUM_THREADS={env['OMP_NUM_THREADS']})", file=sys.stderr, flush=True)
    raise SystemExit(subprocess.call(cmd, env=env))


def gemm_roofline(args, trainer, img, txt, ssl, rank):
    """--full: one extra step after the timed region, launched eagerly; rank 0 returns the roofline below, other ranks None"""
    from vtp_amd import ops
    # ---- dominant-kernel roofline: one instrumented step, HIP events (recorded on the launch stream) around every launch of
    # the MFMA GEMM family -- gemm_nt (forward / dgrad) and gemm_tn (wgrad) are the same kernel template (rank 0)
    roof = None
    recs = []
    import vtp_amd.engine as eng
    orig_nt, orig_tn, orig_qkv, orig_dsw = ops.gemm_nt, ops.gemm_tn, ops.gemm_qkv_rope, ops.gemm_dgrad_swiglu

    def timed(fn):
        def run(a, b, c, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(a, b, c, **kw)
            e1.record()
            M = kw["M"] if kw.get("M") is not None else a.shape[0]
            K = kw["K"] if kw.get("K") is not None else a.shape[1]
            N = kw["N"] if kw.get("N") is not None else b.shape[0]
            epi, sp = kw.get("epi", 0), kw.get("splits", 1)
            # algorithmic HBM bytes: operands once + result once (+ residual read; SwiGLU: x12 and hidden; GELU: pre-activation and output)
            out_b = {ops.EPI_BF16: 2.0, ops.EPI_F32: 4.0 + (4.0 if kw.get("resid") is not None else 0.0), ops.EPI_SWIGLU: 3.0,
                     ops.EPI_GELU: 4.0 if kw.get("c2") is not None else 2.0, ops.EPI_F32_ATOMIC: 8.0, ops.EPI_F32_SLAB: 4.0 * sp}.get(epi, 4.0)
            recs.append((2.0 * M * N * K, e0, e1, (fn.__name__, M, N, K, epi, sp), 2.0 * K * (M + N) + out_b * M * N))
        return run

    def timed_qkv(a, w, bias, c, M, N, K, *rest):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        orig_qkv(a, w, bias, c, M, N, K, *rest)
        e1.record()
        recs.append((2.0 * M * N * K, e0, e1, ("gemm_qkv_rope", M, N, K, 0, 1), 2.0 * K * (M + N) + 2.0 * M * N))

    def timed_dsw(dy, wT, x12, dx12, M, H, K):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        orig_dsw(dy, wT, x12, dx12, M, H, K)
        e1.record()
        recs.append((2.0 * M * H * K, e0, e1, ("gemm_dgrad_swiglu", M, H, K, 0, 1), 2.0 * K * (M + H) + 8.0 * M * H))  # + x12 read, dx12 written

    orig_grp = ops.WgradGroup.launch

    def timed_grp(self, kernel=None):  # the block's grouped weight-gradient launch: sum of 2 N K tokens over its problems
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        orig_grp(self, kernel)
        e1.record()
        fl = sum(2.0 * r[7] * r[8] * self.Ktok for r in self.rows)
        by = sum(2.0 * self.Ktok * (r[7] + r[8]) + 4.0 * r[7] * r[8] * (2 if r[12] else 1) for r in self.rows)  # dy + x read, dW written (+ read: C +=)
        recs.append((fl, e0, e1, ("gemm_tn_grouped", len(self.rows), self.ntiles, self.Ktok, 1, self.splits), by))

    if rank == 0:
        ops.gemm_nt, ops.gemm_tn, ops.gemm_qkv_rope, ops.gemm_dgrad_swiglu = timed(orig_nt), timed(orig_tn), timed_qkv, timed_dsw
        ops.WgradGroup.launch = timed_grp
    trainer.use_graphs = False   # events cannot sit inside a replayed graph: this step launches eagerly
    overlap_was = eng.OVERLAP.enabled
    eng.OVERLAP.enabled = False  # per-kernel durations: no second stream sharing the CUs while a GEMM is timed
    # (without the side streams the step announces its gradient buckets in finer pieces; the rank-sharded optimizer ties chunk
    # ownership to the bucket layout and refuses a changed one -- this one untimed step after the measurement may re-assign it)
    shard_layout_was = getattr(trainer, "_shard_layout", None)
    trainer._shard_layout = None
    try:
        trainer.step(img, txt, ssl)  # every rank takes the step (it contains the collectives); rank 0 times its GEMMs
        torch.cuda.synchronize()
    finally:
        trainer._shard_layout = shard_layout_was
        ops.gemm_nt, ops.gemm_tn, ops.gemm_qkv_rope, ops.gemm_dgrad_swiglu = orig_nt, orig_tn, orig_qkv, orig_dsw
        ops.WgradGroup.launch = orig_grp
        eng.OVERLAP.enabled = overlap_was
    if rank == 0:
        fl = sum(r[0] for r in recs)
        ms = sum(r[1].elapsed_time(r[2]) for r in recs)
        ach = fl / (ms * 1e-3) / 1e12
        if os.environ.get("VTP_BENCH_GEMM_TABLE"):  # per-shape in-situ table of the instrumented step (tuning aid)
            tab = {}
            for f, a, b, key, _by in recs:
                t = tab.setdefault(key, [0, 0.0, 0.0])
                t[0] += 1
                t[1] += a.elapsed_time(b)
                t[2] += f
            with open(os.environ["VTP_BENCH_GEMM_TABLE"], "w") as fh:
                for key, (n, t, f) in sorted(tab.items(), key=lambda kv: -kv[1][1]):
                    fh.write(f"{key[0]:14s} M={key[1]:6d} N={key[2]:6d} K={key[3]:6d} epi={key[4]} splits={key[5]:2d}  calls={n:3d}  "
                             f"total={t:7.3f} ms  avg={t / n * 1e3:7.1f} us  {f / t / 1e9:7.1f} TF/s\n")
        traffic, traffic_src, mfma_util, pmc_extra = None, None, None, None
        pmc = next((q for q in (os.path.join(ROOT, "profiles", f"r0{r}_pmc_summary.json") for r in (6, 5, 4, 3, 2, 1)) if os.path.exists(q)), "")
        if pmc and args.workload == "vtp_base_full" and not args.batch:
            try:  # HBM bytes per launch and SQ counters of the same kernels from the committed rocprofv3 --pmc passes of this command
                d = json.load(open(pmc))
                by, n, busy, gui = 0.0, 0, 0.0, 0.0
                for fam in ("gemm_nt", "gemm_tn", "gemm8p_nt", "gemm8p_tn", "gemm8p_grouped_tn", "gemm8h_nt", "gemm4w_nt", "gemm4w_grouped_tn"):
                    if fam not in d:
                        continue
                    # FETCH_SIZE / WRITE_SIZE are KiB; gfx950 FETCH_SIZE tallies 128-B requests at 64 B (x2, MI355X_MICROARCH.md HBM)
                    by += 1024.0 * (2.0 * d[fam]["FETCH_SIZE"]["sum"] + d[fam]["WRITE_SIZE"]["sum"])
                    n += d[fam]["FETCH_SIZE"]["dispatches"]
                    if "SQ_VALU_MFMA_BUSY_CYCLES" in d[fam]:
                        busy += d[fam]["SQ_VALU_MFMA_BUSY_CYCLES"]["sum"]
                        gui += d[fam]["GRBM_GUI_ACTIVE"]["sum"]
                traffic, traffic_src = round(by / n), f"profiles/{os.path.basename(pmc)} (separate --pmc passes; bytes per launch)"
                if gui > 0:
                    # matrix-pipe busy cycles / SIMD-cycles while the kernels ran (tools/pmc_summarize.py `derived`: GRBM_GUI_ACTIVE is
                    # summed over the 8 XCDs; 1024 SIMDs); attention alongside, from the same pass
                    mfma_util = round(busy / (gui / 8.0 * 1024.0), 4)
                    pmc_extra = {k: {m: d[k][m] for m in ("mfma_util", "valu_busy", "lds_bank_conflict_frac") if m in d[k]}
                                 for k in ("gemm8p_nt", "gemm8h_nt", "gemm4w_nt", "gemm4w_grouped_tn", "gemm8p_grouped_tn", "gemm_nt", "attn_fwd", "attn_bwd_fused") if k in d}
            except (KeyError, ValueError, ZeroDivisionError):
                pass
        # algorithmic HBM bytes of the same launches: every operand read once, every result written once (+ the residual / pre-
        # activation reads of the fused epilogues) -- what `traffic` is to be compared with
        alg = sum(r[4] for r in recs if len(r) > 4 and r[4])
        # the MIXED floor of the same launches: per launch max(FLOP / dense bf16 MFMA peak, algorithmic bytes / the
        # 6.3 TB/s a streaming copy achieves) -- what the family would take if every launch sat on whichever roof bounds it
        HBM_ACHIEVABLE = 6.3e12
        mixed_ms = sum(max(r[0] / (PEAK_BF16_TFLOPS * 1e12), r[4] / HBM_ACHIEVABLE) for r in recs) * 1e3
        mfma_ms = sum(r[0] for r in recs) / (PEAK_BF16_TFLOPS * 1e12) * 1e3
        hbm_bound = sum(1 for r in recs if r[4] / HBM_ACHIEVABLE > r[0] / (PEAK_BF16_TFLOPS * 1e12))
        # HBM floors of the step's other kernel families from the same counter passes (bytes per step / 6.3 TB/s) beside their kernel
        # time in the committed rocprofv3 --stats summary of the round (single stream): attention, norms, optimizer lane
        other = None
        try:
            if pmc:
                d = json.load(open(pmc))
                rnd = os.path.basename(pmc)[:3]
                stats = os.path.join(ROOT, "profiles", f"{rnd}_kernel_stats_full_eager_b32.csv")
                tms = {}
                if os.path.exists(stats):
                    import csv as _csv
                    rows_ = list(_csv.DictReader(open(stats)))
                    nst = max(1, min(int(r_["Calls"]) for r_ in rows_ if "dino_ce_kernel" in r_["Name"])) if any("dino_ce_kernel" in r_["Name"] for r_ in rows_) else 1
                    for fam in ("attn_fwd", "attn_bwd_fused", "norm_fwd", "norm_bwd", "adamw", "prep_weights"):
                        tms[fam] = sum(float(r_["TotalDurationNs"]) for r_ in rows_ if fam in r_["Name"]) / nst / 1e6
                other = {}
                for fam in ("attn_fwd", "attn_bwd_fused", "norm_fwd", "norm_bwd", "adamw", "prep_weights"):
                    if fam in d and "FETCH_SIZE" in d[fam]:
                        steps_pmc = max(1, d["dino_ce"]["FETCH_SIZE"]["dispatches"]) if "dino_ce" in d else 1
                        byt = 1024.0 * (2.0 * d[fam]["FETCH_SIZE"]["sum"] + d[fam]["WRITE_SIZE"]["sum"]) / steps_pmc
                        other[fam] = {"hbm_bytes_per_step": round(byt), "hbm_floor_ms": round(byt / HBM_ACHIEVABLE * 1e3, 3),
                                      "kernel_ms_per_step": round(tms[fam], 3) if fam in tms else None,
                                      "frac_of_floor": round(byt / HBM_ACHIEVABLE * 1e3 / tms[fam], 3) if tms.get(fam) else None}
        except (KeyError, ValueError, ZeroDivisionError, OSError):
            other = None
        roof = {"bound": "mfma", "kernel": "vtp::gemm8p_kernel<...> + vtp::gemm4w_grouped_tn_kernel + vtp::gemm4w_kernel<...> + vtp::gemm8h_kernel<...> + vtp::gemm_nt_kernel<...> (the bf16 MFMA 32x32x16 GEMM family: NT fwd/dgrad, TN wgrad incl. the per-block grouped launches; 256x256 8-phase, one-wave-per-SIMD and 128x256 kernels, ring tile configs, all epilogues)",
                "achieved": round(ach, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / PEAK_BF16_TFLOPS, 4),
                "traffic": traffic, "traffic_source": traffic_src,
                "pmc_replayed": traffic is not None,  # traffic / mfma_util / pmc_by_kernel come from the committed rocprofv3 --pmc passes of this
                # command (profiles/), NOT from this run: hardware counters cannot be read from inside the process
                "algorithmic_bytes_per_launch_avg": round(alg / len(recs)) if alg else None,
                "traffic_over_algorithmic": round(traffic / (alg / len(recs)), 3) if (traffic and alg) else None,
                "mfma_util": mfma_util, "mfma_util_note": "SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 XCDs x 1024 SIMDs) of the GEMM family, "
                "rocprofv3 --pmc pass of this command (profiles/); x sustained clock / 2.4 GHz = fraction of the data-sheet peak",
                "pmc_by_kernel": pmc_extra, "launches_per_step": len(recs),
                "avg_launch_us": round(ms * 1e3 / len(recs), 2), "gemm_ms_per_step": round(ms, 3),
                "flop_per_launch_avg": fl / len(recs),
                "mixed_floor_ms": round(mixed_ms, 3), "mfma_floor_ms": round(mfma_ms, 3), "frac_of_mixed_floor": round(mixed_ms / ms, 4),
                "launches_hbm_bound_at_the_floor": hbm_bound,
                "mixed_floor_note": "sum over the instrumented step's launches of max(2MNK / 2.5 PFLOP/s, algorithmic bytes / 6.3 TB/s); "
                "frac_of_mixed_floor = that / gemm_ms_per_step",
                "other_families_hbm_floor": other,
                "other_families_note": "bytes per step = 2 x FETCH_SIZE + WRITE_SIZE of the committed --pmc passes (replayed, like `traffic`); "
                "kernel_ms_per_step from the committed rocprofv3 --stats CSV of the same round (eager, single stream)"}
    return roof


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="vtp_base_full", choices=sorted(WORKLOADS) + sorted(FORWARD_WORKLOADS))
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch (default: workload's)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline measurement, also run what takes runs of its own: the instrumented roofline step, the "
                         "LPIPS-on and separate-pass measurements, the end-to-end parity and CPU-oracle legs (forward workload: the "
                         "bf16-path timing, the fp8-vs-bf16 errors and the roofline pass).  Off: set up, warm up, time, dump, print")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the end-to-end parity and CPU-oracle legs")
    ap.add_argument("--cpu-batch", type=int, default=2, help="images per CPU-oracle step (the full step costs ~8 s per image on a 128-thread host)")
    ap.add_argument("--cpu-steps", type=int, default=5, help="timed fp32 steps of the CPU-oracle leg (bf16-autocast leg: half of it)")
    ap.add_argument("--cpu-survey-protocol", action="store_true", help="SURVEY 8d's CPU protocol: batch 8, 10 timed fp32 steps (5 bf16-autocast) -- "
                    "about 25 minutes of host time on a 128-thread box, so NOT the default (the driver's run keeps batch 2, 5 + 3 steps)")
    ap.add_argument("--bucket-blocks", type=int, default=3, help="transformer blocks per gradient bucket (= per hipGraph segment / optimizer-lane update)")
    ap.add_argument("--no-lpips-run", action="store_true", help="--full without the second measurement with the perceptual term on")
    ap.add_argument("--no-graphs", action="store_true", help="eager kernel launches instead of hipGraph segment replay")
    ap.add_argument("--no-separate-run", action="store_true",
                    help="--full without the extra measurement with a separate reconstruction input (rec and clip as separate trunk passes)")
    ap.add_argument("--shard-optimizer", action="store_true",
                    help="N > 1: reduce-scatter + rank-sharded AdamW + parameter all-gather instead of all-reduce + replicated AdamW")
    ap.add_argument("--grad-dtype", default="fp32", choices=["fp32", "bf16"], help="gradient bucket dtype (bf16: --shard-optimizer only)")
    ap.add_argument("--dist-timeout", type=int, default=600, help="seconds before a stuck collective aborts the job (no silent hang)")
    ap.add_argument("--prototypes", type=int, default=65536, help="DINO head out_dim K (DINOv2 default 65536; unpinned)")
    ap.add_argument("--perceptual-weight", type=float, default=0.0,
                    help="> 0: add the LPIPS perceptual term (VGG16, seeded random weights: vgg.pth is a download) to the rec loss")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed to DIR/<name>.npy (rank 0; large arrays as a fixed "
                         "seeded sample): train workloads the losses and a sample of the updated weights, forward workloads the "
                         "latents and reconstructions")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(args.gpus)
    # VTP_BENCH_BACKEND=gloo + VTP_BENCH_SHARE_GPU=1: control-flow rehearsal of the N > 1 path on a one-GPU box (all ranks on
    # device 0, gloo collectives); never used for reported numbers -- config.parallelism records it
    backend = os.environ.get("VTP_BENCH_BACKEND", "nccl")
    if os.environ.get("VTP_BENCH_SHARE_GPU") == "1":
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as dist
        import datetime
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("NCCL_DEBUG", "VERSION")               # RCCL prints its version banner on rank 0
        os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "1")  # a timed-out collective tears the process down (no hang)
        # RCCL's channels are workgroups that hold a CU each while a collective runs, and the step's one-workgroup-per-CU GEMMs (160 KiB
        # of LDS) cannot share a CU with them: a launch that needs every CU then takes a second round.  The step's gradient traffic (1.28 GB
        # in ~35 ms of backward) needs ~65 GB/s, so half of RCCL's usual channel count is plenty: cap it at 32 and leave those 32 CUs out of the
        # GEMM grids (4 CUs of 32 per XCD; 224 of 256 CUs cost the step 1.5 % when nothing else runs, profiles/r06_dyn_tiles.log).  Both only as
        # defaults: the environment of the launch wins.  INTEGRATION.md "Running beside RCCL".
        os.environ.setdefault("NCCL_MAX_NCHANNELS", "32")
        os.environ.setdefault("VTP_GEMM_CUS", "224")
        tmo = datetime.timedelta(seconds=args.dist_timeout)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, timeout=tmo)
        else:
            dist.init_process_group(backend, timeout=tmo)
        # every rank must have arrived with the same idea of the job before any timing starts
        seen = torch.zeros(world, dtype=torch.int32, device=dev)
        seen[rank] = 1 + local
        dist.all_reduce(seen)
        ROLL["ranks_seen"] = int((seen > 0).sum())
        ROLL["backend"] = backend
        if rank == 0:
            ver = ".".join(str(v) for v in torch.cuda.nccl.version()) if backend == "nccl" else "-"
            ROLL["rccl_version"] = ver
            print(f"[bench] {world} ranks up (backend {backend}, RCCL {ver}); local devices {[int(v) - 1 for v in seen.tolist()]}",
                  file=sys.stderr, flush=True)

    from vtp_amd import VTP, VTPConfig, VTPModel, VTPTrainer, ops
    if args.workload in FORWARD_WORKLOADS:
        return bench_forward(args, world, rank, dev)
    cfg_kw, B, res, objectives = WORKLOADS[args.workload]
    clip, do_ssl = "clip" in objectives, "ssl" in objectives
    B = args.batch or B
    img = torch.randn(B, 3, res, res, device=dev, generator=torch.Generator(device=dev).manual_seed(1234 + rank))

    crops = synthetic_crops(B, res, dev, 777 + rank) if do_ssl else None
    mask_stream = MaskStream(B, res, 555 + rank) if do_ssl else None
    state = {"n_masked": [], "Ts": set()}

    def build_trainer(use_graphs: bool, perceptual_weight: float):
        torch.manual_seed(0)
        model = (VTP(VTPConfig(**cfg_kw), dino_out_dim=args.prototypes) if do_ssl else VTPModel(VTPConfig(**cfg_kw))).to(dev)
        lp = None
        if perceptual_weight > 0:
            from vtp_amd import LPIPS
            lp = LPIPS().reset_parameters(0).to(dev)
        trainer = VTPTrainer(model, lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05, use_graphs=use_graphs, lpips=lp, bucket_blocks=args.bucket_blocks,
                             perceptual_weight=perceptual_weight, shard_optimizer=args.shard_optimizer and world > 1,
                             grad_dtype=args.grad_dtype if (args.shard_optimizer and world > 1) else "fp32")
        txt = synthetic_captions(B, model.config.text_context_length, model.config.text_vocab_size, dev, 4321 + rank) if clip else None
        return model, lp, trainer, txt

    # seconds of host time in: mask draw | prepare_ssl (work) | step() enqueue | prepare_ssl's wait for a free pinned staging slot
    # (back-pressure of the 4-slot ring: the host is that far AHEAD of the GPU -- idle time, not work)
    host_t = state.setdefault("host_t", [0.0, 0.0, 0.0, 0.0])

    img_rec = torch.randn(B, 3, res, res, device=dev, generator=torch.Generator(device=dev).manual_seed(4242 + rank))
    state["separate"] = False  # True: the reconstruction objective sees its own tensor -> its own trunk pass (reference accounting)

    def draw_batch(trainer):
        """fresh masks -> index plan -> pinned pack -> H2D enqueue: what a loader worker + collate does for one batch"""
        t0 = time.perf_counter()
        masks, upper = mask_stream.draw()
        t1 = time.perf_counter()
        ssl = trainer.prepare_ssl(crops[0], crops[1], masks, upperbound=upper)
        state["n_masked"].append(ssl["plan"]["n_masked"])
        state["Ts"].add(ssl["plan"]["Ts"])
        state["last_plan"] = ssl["plan"]
        t2 = time.perf_counter()
        wait_s, trainer._stager.wait_s = trainer._stager.wait_s, 0.0
        host_t[0] += t1 - t0
        host_t[1] += t2 - t1 - wait_s
        host_t[3] += wait_s
        return ssl

    def one_step(trainer, txt):
        """the step as a training loop with a prefetching loader runs it: the optimizer step on the batch drawn during the previous
        step, then the draw of the next batch (fresh masks -> index plan -> H2D) while the GPU runs this one.  Every step draws exactly
        one batch; the first timed step consumes the batch drawn by the last warm-up step, the last timed step draws one that the next
        step would consume."""
        ssl = None
        if do_ssl:
            ssl = state.pop("next_ssl", None) or draw_batch(trainer)
        t0 = time.perf_counter()
        out = trainer.step(img, txt, ssl, reconstruction_image=img_rec if state["separate"] else None)
        host_t[2] += time.perf_counter() - t0
        if do_ssl:
            state["next_ssl"] = draw_batch(trainer)
        return out

    def sync():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    def measure(perceptual_weight: float, steps: int, warmup: int, separate: bool = False):
        state["separate"] = separate
        state.pop("next_ssl", None)
        model, lp, trainer, txt = build_trainer(not args.no_graphs, perceptual_weight)
        launch = "eager" if args.no_graphs else ("one hipGraph per step" if trainer.single_graph else "hipGraph segments (collectives between them)")
        try:
            for _ in range(warmup):
                one_step(trainer, txt)
            sync()
        except RuntimeError as e:  # a capture problem must not cost the measurement: same step, eager launches
            if args.no_graphs:
                raise
            print(f"[bench] hipGraph path failed ({str(e)[:200]}); falling back to eager launches", file=sys.stderr, flush=True)
            launch = "eager (hipGraph capture failed on this configuration)"
            model, lp, trainer, txt = build_trainer(False, perceptual_weight)
            for _ in range(warmup):
                one_step(trainer, txt)
            sync()
        trainer.time_comm = world > 1  # HIP events around every point where the main stream waits for a collective
        trainer.bucketer.comm_bytes = 0
        host_t[:] = [0.0, 0.0, 0.0, 0.0]
        t0 = time.perf_counter()
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]  # per-step spread (one event record per step: free)
        marks[0].record()
        # VTP_BENCH_THIEF=n (with VTP_DIAG=1; an experiment, never the line of record): a do-nothing kernel holds n CUs on a side stream
        # for the whole timed region -- the footprint of RCCL's channels beside the step, on one GPU (tools/cu_thief.py)
        thief_n = int(os.environ.get("VTP_BENCH_THIEF", "0") or 0)
        if thief_n:
            from vtp_amd import _lib as _l
            thief_stream = torch.cuda.Stream()
        for i in range(steps):
            if thief_n:
                _l.check(_l.load().vtp_cu_thief(thief_n, 4000000, None, thief_stream.cuda_stream), "vtp_cu_thief")  # 40 ms each, back to back
            loss, closs = one_step(trainer, txt)
            marks[i + 1].record()
        state["host_split_ms"] = [round(v * 1e3 / steps, 3) for v in host_t]
        state["host_ms_per_step"] = round((time.perf_counter() - t0) * 1e3 / steps, 3)  # enqueue time: << ms_per_step unless host-bound
        sync()
        elapsed = time.perf_counter() - t0
        per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
        state["per_step_ms"] = [round(marks[i].elapsed_time(marks[i + 1]), 2) for i in range(steps)]
        state["step_ms_spread"] = {"min": round(per[0], 3), "median": round(per[len(per) // 2], 3), "max": round(per[-1], 3)}
        if world > 1:
            state["comm"] = {**ROLL, "exposed_ms_per_step": round(trainer.comm_exposed_ms() / steps, 3),
                             "payload_mb_per_step": round(trainer.bucketer.comm_bytes / steps / 1e6, 1),
                             "gradient_exchange": ("reduce-scatter (" + args.grad_dtype + ") + rank-sharded AdamW + fp32 parameter all-gather")
                             if trainer.shard_optimizer else "bucketed fp32 all-reduce + replicated AdamW"}
            trainer.time_comm = False
        if world > 1:
            t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            elapsed = float(t)
        return model, lp, trainer, txt, launch, elapsed, loss, closs

    model, lp, trainer, txt, launch, elapsed, loss, closs = measure(args.perceptual_weight, args.steps, args.warmup)
    if args.dump_outputs and rank == 0:  # before the instrumented step below changes the weights again
        outs = {"rec_loss": loss.reshape(-1), "clip_loss": closs.reshape(-1)}
        if do_ssl:
            outs["ssl_loss"] = trainer.ssl_loss_sum.reshape(-1)
        if lp is not None:
            outs["lpips"] = trainer.lpips_val
        outs["params_sample"] = param_sample(model)
        dump_outputs(args.dump_outputs, outs)
    state["host_ms_main"], state["host_split_main"] = state.get("host_ms_per_step"), state.get("host_split_ms")
    state["spread_main"] = state.get("step_ms_spread")
    state["per_step_main"] = state.get("per_step_ms")
    if rank == 0:
        print(f"[bench] per-step ms (HIP events on the main stream): {state.get('per_step_ms')}", file=sys.stderr, flush=True)
    state["comm_main"] = state.pop("comm", None)  # rank 0's main-stream waits (the second, LPIPS-on measurement overwrites "comm")
    ssl = None
    if do_ssl and args.full:  # the batch of the instrumented step below
        masks, upper = mask_stream.draw()
        ssl = trainer.prepare_ssl(crops[0], crops[1], masks, upperbound=upper)
    loss_val, closs_val = float(loss), float(closs)
    ssl_loss_val = float(trainer.ssl_loss_sum) if do_ssl else 0.0

    roof = gemm_roofline(args, trainer, img, txt, ssl, rank) if args.full else None
    if world > 1:
        sync()

    c = model.config
    hw = (res // 16) ** 2
    from vtp_amd.config import swiglu_hidden
    enc = vit_fwd_gflop(c.vision_embed_dim, swiglu_hidden(c.vision_embed_dim), c.vision_depth, hw + 1, hw, True)
    dec = vit_fwd_gflop(c.decoder_embed_dim, swiglu_hidden(c.decoder_embed_dim), c.decoder_depth, hw, hw, False)
    tflop = text_fwd_gflop(c.text_embed_dim, c.text_depth, c.text_context_length) if clip else 0.0
    gflop_img = 3.0 * (enc + dec + tflop)            # executed: one shared trunk pass serves rec and clip
    gflop_ref = 3.0 * (enc + dec) + (3.0 * (enc + tflop) if clip else 0.0)  # BASELINE.md accounting (separate passes)
    ssl_info = None
    if do_ssl:
        hw_l = (96 // 16) ** 2
        loc = vit_fwd_gflop(c.vision_embed_dim, swiglu_hidden(c.vision_embed_dim), c.vision_depth, hw_l + 1, hw_l, True) \
            - 2 * (hw_l + 1) * c.vision_embed_dim * 64 / 1e9
        enc_nb = enc - 2 * (hw + 1) * c.vision_embed_dim * 64 / 1e9   # SSL passes do not use the bottleneck
        ssl_trunk = 3.0 * (2 * enc_nb + 8 * loc) + 2 * enc_nb          # student fwd+bwd (2 global + 8 local) + teacher fwd
        dh = model.dino_cfg
        tok_flop = 2.0 * (dh["in_dim"] * dh["hidden"] + dh["hidden"] ** 2 + dh["hidden"] * dh["bott"] + dh["bott"] * dh["K"])
        pl = state["last_plan"]   # Ts and Tm follow from the collate's upperbound: the same for every draw
        head = (3.0 * pl["Ts"] + (2 * B + pl["Tm"])) * tok_flop / 1e9 / B   # student fwd+bwd + teacher fwd, per image
        gflop_img += ssl_trunk + head
        gflop_ref += ssl_trunk + head
        nm = state["n_masked"]
        ssl_info = {"prototypes": dh["K"], "masks": "fresh block-wise iBOT masks every step (host collate + index plan + H2D inside the timed region, one batch ahead of the step that consumes it: a prefetching loader)",
                    "masked_tokens_min_mean_max": [min(nm), round(sum(nm) / len(nm), 1), max(nm)], "masked_token_buffer_rows": pl["Tm"],
                    "graph_keys_seen": len(state["Ts"]), "student_head_rows": pl["Ts"],
                    "global_crops": 2, "local_crops": 8, "local_res": 96, "ssl_loss": round(ssl_loss_val, 4)}
    lpips_info = None
    if lp is not None:  # two VGG forwards (decoded + target) and one input-gradient pass
        lp_g = 3.0 * lp.forward_gflop(res, res)
        gflop_img += lp_g
        gflop_ref += lp_g
        lpips_info = {"weight": args.perceptual_weight, "train_gflop_per_image": round(lp_g, 1),
                      "mean_lpips": round(float(trainer.lpips_val.mean()), 5), "weights": "seeded random (vgg.pth unavailable offline)"}
    ips = world * B * args.steps / elapsed
    lpips_on = None
    if args.full and args.perceptual_weight == 0 and not args.no_lpips_run and args.workload.startswith("vtp_base"):
        # the same step with the perceptual (LPIPS / VGG16) term of north_star switched on: fewer steps, same protocol
        del trainer, model
        torch.cuda.empty_cache()
        st2, wu2 = max(4, args.steps // 2), max(2, args.warmup // 2)
        m2, lp2, tr2, _, launch2, el2, _, _ = measure(1.0, st2, wu2)
        lp_g = 3.0 * lp2.forward_gflop(res, res)
        ips2 = world * B * st2 / el2
        lpips_on = {"value": round(ips2, 2), "unit": "images/sec", "ms_per_step": round(el2 / st2 * 1e3, 3), "steps": st2, "warmup": wu2,
                    "perceptual_weight": 1.0, "launch": launch2, "train_gflop_per_image": round(gflop_img + lp_g, 1),
                    "step_frac": round(ips2 / world * (gflop_img + lp_g) / 1e3 / PEAK_BF16_TFLOPS, 4),
                    "mean_lpips": round(float(tr2.lpips_val.mean()), 5), "weights": "seeded random VGG16 (vgg.pth is a download)"}
        model = m2
    separate = None
    if args.full and clip and not args.no_separate_run and args.workload.startswith("vtp_base"):
        # the reference's accounting EXECUTED: `image` and `reconstruction_image` are different tensors (vtp.py:323-338), so the
        # reconstruction objective runs its own trunk pass (one more item of the list forward) -- gflop_ref per image
        try:
            del trainer
        except NameError:
            pass
        model = None
        torch.cuda.empty_cache()
        st3, wu3 = max(4, args.steps // 2), max(2, args.warmup // 2)
        m3, _, tr3, _, launch3, el3, _, _ = measure(args.perceptual_weight, st3, wu3, separate=True)
        ips3 = world * B * st3 / el3
        separate = {"value": round(ips3, 2), "unit": "images/sec", "ms_per_step": round(el3 / st3 * 1e3, 3), "steps": st3, "warmup": wu3,
                    "launch": launch3, "train_gflop_per_image": round(gflop_ref, 1),
                    "step_tflops_per_gpu": round(ips3 / world * gflop_ref / 1e3, 1),
                    "step_frac": round(ips3 / world * gflop_ref / 1e3 / PEAK_BF16_TFLOPS, 4),
                    "note": "rec and clip on different input tensors: two lead items in the list forward (separate trunk passes)"}
        model = m3
        del tr3
    out = {
        "metric": {"vtp_base": "images/sec/node VTP-B f16d64 256x256 train step", "vtp_smal": "images/sec/node VTP-S f16d64 256x256 train step",
                   "vtp_larg": "images/sec/node VTP-L f16d64 512x512 train step"}[args.workload[:8]],
        "value": round(ips, 2), "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "config": {"workload": f"{args.workload}: full optimizer step (fwd + {' + '.join(objectives)} losses + bwd + bucketed grad "
                               f"all-reduce{' + feature all-gather/reduce-scatter' if clip else ''} + fused AdamW"
                               f"{' + EMA teacher' if do_ssl else ''}) of trunk + pixel_decoder{' + text tower' if clip else ''}"
                               f"{' + DINO head + EMA teacher trunk (2 global + 8 local-96 crops/img, iBOT masks)' if do_ssl else ''}, "
                               f"{B} img/GPU @ {res}x{res}{', 77-token synthetic captions' if clip else ''}, random-init weights; "
                               "rec and clip share one trunk pass (identical activations at drop rate 0); "
                               + ("LPIPS perceptual term included" if lp is not None else "LPIPS term not included (--perceptual-weight)"),
                   "launch": launch, "global_batch": world * B, "per_gpu_batch": B, "resolution": res, "parallelism": f"dp{world}" + ("" if backend == "nccl" else f" ({backend} rehearsal, shared GPU)"),
                   "train_gflop_per_image": round(gflop_img, 1),
                   "reference_accounting_gflop_per_image": round(gflop_ref, 1)},
        "loss": round(loss_val, 5), "clip_loss": round(closs_val, 5), "step_ms_spread": state.get("spread_main"), "host_enqueue_ms_per_step": state.get("host_ms_main"), "host_split_ms": state.get("host_split_main"),
        "host_split_legend": ["mask collate", "prepare_ssl work (index plan + pinned pack + H2D enqueue)", "step() enqueue",
                              "prepare_ssl back-pressure wait (host ahead of the GPU: idle, not work)"], "ssl": ssl_info, "lpips": lpips_info, "lpips_on": lpips_on, "separate_passes": separate,
        "comm": state.get("comm_main"),
        "step_tflops_per_gpu": round(ips / world * gflop_img / 1e3, 1),
        "step_frac": round(ips / world * gflop_img / 1e3 / PEAK_BF16_TFLOPS, 4),
    }
    if rank == 0:
        out["roofline"] = roof
        if args.full and world == 1 and not args.no_cpu_baseline:
            e2e = e2e_parity(model, res, dev)  # (before the CPU leg: the model's weights are still on the device)
            if args.cpu_survey_protocol:
                args.cpu_batch, args.cpu_steps = 8, 10
            out["cpu_baseline"] = cpu_baseline(model, args.cpu_batch, res, clip, do_ssl, n_fp32=args.cpu_steps, n_bf16=max(1, (args.cpu_steps + 1) // 2))
            out["cpu_baseline"]["e2e_vs_oracle_fp32"] = e2e
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
