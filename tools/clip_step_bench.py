#!/usr/bin/env python3
"""FusedAdamEMA.step() alone on DiT-B/2 by device events: with and without max_grad_norm, the non-finite guard on (the f16
configuration) and off (bf16).  Four optimisers over one model and one gradient buffer, interleaved rounds in ONE process with the order
rotated, no synchronisation inside a round; prints medians, minima and maxima as one JSON line ("Gradient-norm
clipping"; profiles/grad_clip_step_b2.json).

    python tools/clip_step_bench.py [--rounds 40] [--warmup 8] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="DiT-B/2")
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import mapdit_amd  # noqa: F401
    from mapdit_amd.diffusion import create_diffusion
    from mapdit_amd.optim import FusedAdamEMA
    from mapdit_amd.src.models import DIT_MODELS

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = DIT_MODELS[args.model](in_channels=4, input_size=32, num_classes=1000).to(dev).train()
    model.gemm_precision = "bf16"
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(8, 4, 32, 32, device=dev, generator=g)
    y = torch.randint(0, 1000, (8,), device=dev, generator=g)
    t = torch.randint(0, 1000, (8,), device=dev)
    create_diffusion("").training_losses(model, x, t, dict(y=y))["loss"].mean().backward()      # fills the flat gradient buffer
    torch.cuda.synchronize()

    configs = {"guard_off": dict(nonfinite_guard=False), "guard_off_clip": dict(nonfinite_guard=False, max_grad_norm=1.0),
               "guard_on": dict(nonfinite_guard=True), "guard_on_clip": dict(nonfinite_guard=True, max_grad_norm=1.0)}
    opts = {k: FusedAdamEMA(model, lr=1e-4, **kw) for k, kw in configs.items()}
    times = {k: [] for k in opts}
    for r in range(args.warmup + args.rounds):
        marks = {}
        order = list(opts)[r % 4:] + list(opts)[:r % 4]
        for k in order:                                # the queue stays ahead of the device: no synchronisation inside a round
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            opts[k].step()
            b.record()
            marks[k] = (a, b)
        torch.cuda.synchronize()
        if r >= args.warmup:
            for k, (a, b) in marks.items():
                times[k].append(a.elapsed_time(b))
    out = {"model": args.model, "parameters": model._pflat.numel(), "grad_bytes": model._gflat.numel() * 4, "rounds": args.rounds}
    out.update({k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in times.items()})
    out["norm"], out["coef"], out["refused"] = opts["guard_on_clip"].grad_norm(), opts["guard_on_clip"].clip_coef(), opts["guard_on_clip"].overflow_steps()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
