#!/usr/bin/env python
"""What per-parameter-group scales (VTPTrainer(param_groups=...)) cost, on one MI355X, in one process:

  kernel -- vtp_adamw_ema_dev_grouped against vtp_adamw_ema_dev (masked) over the whole flat buffer of the benchmark model, with the
            trainer's own index / flag tables; launches of the two alternate round by round, HIP events around each round;
  step   -- bench.py's default step (VTP-B, 32 images, rec + clip + DINO/iBOT, one hipGraph per step, a fresh mask draw per step) with
            layerwise_lr_decay(decay=0.9) on and off: two trainers in the process, timed in alternating blocks.

Every figure comes with the spread of its own repeats (min .. max of the round medians / block means): a difference inside the spread of
the masked kernel / the step without groups is not a difference.  Prints one JSON line; --out also writes it to a file.

    python tools/param_groups_cost.py --rounds 7 --steps 20 --out param_groups_cost.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def kernel_cost(trainer, rounds, launches):
    from vtp_amd import ops
    st = trainer.store
    n = st.numel // 4 * 4
    g = torch.Generator(device=st.device).manual_seed(1)
    p, t = st.flat_p[:n].detach().clone(), st.flat_p[:n].detach().clone()
    gr = torch.randn(n, device=st.device, generator=g) * 1e-3
    m, v = torch.zeros(n, device=st.device), torch.zeros(n, device=st.device)
    hyper = torch.zeros(16, device=st.device)
    hyper[:10] = torch.tensor([1e-4, 0.9, 0.95, 1e-8, 0.05, 0.1, 0.2, 1.0, 0.0, 0.994])
    tab, group4, nodecay4 = trainer.group_tab, trainer._group4[:n // 4], trainer.nodecay4[:n // 4]
    run = {"masked": lambda: ops.adamw_ema_dev(p, gr, m, v, t, n, hyper, nodecay4),
           "grouped": lambda: ops.adamw_ema_dev_grouped(p, gr, m, v, t, n, hyper, group4, tab, tab.shape[0])}
    for f in run.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in run}
    for r in range(rounds):
        for k in (("masked", "grouped") if r % 2 == 0 else ("grouped", "masked")):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                run[k]()
            b.record()
            b.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3 / launches)
    bytes_moved = n * 4 * 9 + n // 4  # p, m, v, teacher read and written, g read, one byte per float4
    out = {k: dict(spread(v), unit="us per launch") for k, v in us.items()}
    out["elements"], out["table_rows"] = n, int(tab.shape[0])
    out["gbytes_per_s"] = {k: bytes_moved / (out[k]["median"] * 1e-6) / 1e9 for k in us}
    out["grouped_over_masked"] = out["grouped"]["median"] / out["masked"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7, help="alternating rounds (kernel) / blocks per variant (step)")
    ap.add_argument("--launches", type=int, default=20, help="kernel launches per round")
    ap.add_argument("--steps", type=int, default=20, help="steps per timed block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--decay", type=float, default=0.9)
    ap.add_argument("--prototypes", type=int, default=65536)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("param_groups_cost.py measures on the GPU: no device found")
    import bench
    from vtp_amd import VTP, VTPConfig, VTPTrainer
    from vtp_amd.train import layerwise_lr_decay
    dev = torch.device("cuda", 0)
    cfg_kw, B, res, _ = bench.WORKLOADS["vtp_base_full"]
    img = torch.randn(B, 3, res, res, device=dev, generator=torch.Generator(device=dev).manual_seed(1234))
    crops = bench.synthetic_crops(B, res, dev, 777)

    def build(groups: bool):
        torch.manual_seed(0)
        model = VTP(VTPConfig(**cfg_kw), dino_out_dim=args.prototypes).to(dev)
        pg = layerwise_lr_decay(list(model._engine().offsets), model.config.vision_depth, args.decay) if groups else None
        tr = VTPTrainer(model, lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05, use_graphs=True, param_groups=pg)
        txt = bench.synthetic_captions(B, model.config.text_context_length, model.config.text_vocab_size, dev, 4321)
        return {"trainer": tr, "txt": txt, "masks": bench.MaskStream(B, res, 555), "next": None}

    def draw(v):
        masks, upper = v["masks"].draw()
        return v["trainer"].prepare_ssl(crops[0], crops[1], masks, upperbound=upper)

    def block(v, steps):
        """bench.py's one_step: the step on the batch drawn during the previous one, then the next draw"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            ssl = v["next"] or draw(v)
            v["trainer"].step(img, v["txt"], ssl)
            v["next"] = draw(v)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    variants = {"groups_on": build(True)}
    res_line = {"device": torch.cuda.get_device_name(0), "workload": "vtp_base_full", "batch": B, "decay": args.decay,
                "groups": len(variants["groups_on"]["trainer"].param_groups),
                "kernel_adamw_ema": kernel_cost(variants["groups_on"]["trainer"], args.rounds, args.launches)}
    if not args.skip_step:
        variants["groups_off"] = build(False)
        for v in variants.values():
            block(v, args.warmup)
        ms = {k: [] for k in variants}
        for r in range(args.rounds):
            for k in (("groups_off", "groups_on") if r % 2 == 0 else ("groups_on", "groups_off")):
                ms[k].append(block(variants[k], args.steps))
        res_line["step_ms"] = {k: dict(spread(v), blocks=[round(x, 4) for x in v]) for k, v in ms.items()}
        res_line["step_ms"]["on_over_off"] = res_line["step_ms"]["groups_on"]["median"] / res_line["step_ms"]["groups_off"]["median"]
        res_line["graphs_captured"] = {k: len(v["trainer"]._graphs) for k, v in variants.items()}
    line = json.dumps(res_line)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
