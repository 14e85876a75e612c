#!/usr/bin/env python
"""What VTPTrainer(skip_nonfinite=True) costs on top of max_grad_norm=inf, on one MI355X, in one process: bench.py's default step
(VTP-B, 32 images, rec + clip + DINO/iBOT, one hipGraph per step, a fresh mask draw per step) with two trainers, guard off and guard
on, timed in alternating blocks.  Both measure the norm (the guard needs the clipping machinery); the guard adds one scalar load per
update workgroup and the one-thread tail of the finalize.

Every figure comes with the spread of its own blocks (min .. max of the block means): a difference inside the spread of the step
without the guard is not a difference.  Prints one JSON line; --out also writes it to a file.

    python tools/skip_nonfinite_cost.py --rounds 7 --steps 20 --out skip_nonfinite_cost.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7, help="blocks per variant")
    ap.add_argument("--steps", type=int, default=20, help="steps per timed block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--prototypes", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("skip_nonfinite_cost.py measures on the GPU: no device found")
    import bench
    from vtp_amd import VTP, VTPConfig, VTPTrainer
    dev = torch.device("cuda", 0)
    cfg_kw, B, res, _ = bench.WORKLOADS["vtp_base_full"]
    img = torch.randn(B, 3, res, res, device=dev, generator=torch.Generator(device=dev).manual_seed(1234))
    crops = bench.synthetic_crops(B, res, dev, 777)

    def build(guard: bool):
        torch.manual_seed(0)
        model = VTP(VTPConfig(**cfg_kw), dino_out_dim=args.prototypes).to(dev)
        tr = VTPTrainer(model, lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05, use_graphs=True, max_grad_norm=float("inf"),
                        skip_nonfinite=guard)
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

    variants = {"guard_off": build(False), "guard_on": build(True)}
    for v in variants.values():
        block(v, args.warmup)
    ms = {k: [] for k in variants}
    for r in range(args.rounds):
        for k in (("guard_off", "guard_on") if r % 2 == 0 else ("guard_on", "guard_off")):
            ms[k].append(block(variants[k], args.steps))
    on = variants["guard_on"]["trainer"]
    res_line = {"device": torch.cuda.get_device_name(0), "workload": "vtp_base_full", "batch": B, "max_grad_norm": "inf",
                "step_ms": {k: dict(spread(v), blocks=[round(x, 4) for x in v]) for k, v in ms.items()},
                "graphs_captured": {k: len(v["trainer"]._graphs) for k, v in variants.items()},
                "guard_on_counters": dict(zip(("applied_steps", "skipped_steps", "skip_now"), on._skip_state[:3].tolist())),
                "guard_on_attempted_steps": on.step_no}
    res_line["step_ms"]["on_over_off"] = res_line["step_ms"]["guard_on"]["median"] / res_line["step_ms"]["guard_off"]["median"]
    line = json.dumps(res_line)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
