#!/usr/bin/env python3
"""What gradient accumulation costs per optimiser step: DiT-B/2, bf16, 256 samples as 4 micro-batches of 64, through the facade.

    python tools/accum_bench.py [--tree DIR] [--tag NAME] [--steps 20] [--warmup 5] [--micro 4] [--micro-batch 64] [--out FILE]

One optimiser step = zero_grad(), `micro` x (training_losses on a fresh micro-batch, .mean(), backward()) - the backwards after the first
find p.grad set and accumulate - and the fused Adam + EMA step with grad_scale 1 / micro; HIP events around each whole step.  Appends one
JSON line: median / min / max of the step in ms, the allocation peak above the resident state, and the tag.

--tree DIR imports the package from another checkout (its own built library), so that the same driver times a build that accumulates
by copying the flat gradient buffer (clone, backward, add) against one whose engine accumulates in place.  Run the older tree twice
first: the spread of its two medians is what a difference has to exceed.
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--tag", default="this")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--micro", type=int, default=4)
    ap.add_argument("--micro-batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_accum_b2_4x64.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))

    import torch
    import mapdit_amd
    from mapdit_amd.diffusion import create_diffusion
    from mapdit_amd.optim import FusedAdamEMA, create_lr_lambda
    from mapdit_amd.src.models import DIT_MODELS
    assert os.path.abspath(mapdit_amd._lib.LIB_PATH).startswith(os.path.abspath(args.tree)), mapdit_amd._lib.LIB_PATH
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = DIT_MODELS["DiT-B/2"](in_channels=4, input_size=32, num_classes=1000).to(dev).train()
    model.gemm_precision = "bf16"
    diffusion = create_diffusion(timestep_respacing="")
    opt = FusedAdamEMA(model, lr=1e-2, betas=(0.9, 0.99), ema_stds=(0.05, 0.1), lr_lambda=create_lr_lambda(2666, 40000),
                       grad_scale=1.0 / args.micro)
    g = torch.Generator(device=dev).manual_seed(1)
    n = args.micro_batch

    def step():
        opt.zero_grad()
        for _ in range(args.micro):
            x = torch.randn(n, 4, 32, 32, device=dev, generator=g)
            y = torch.randint(0, 1000, (n,), device=dev, generator=g)
            t = torch.randint(0, diffusion.num_timesteps, (n,), device=dev)
            diffusion.training_losses(model, x, t, dict(y=y))["loss"].mean().backward()
        opt.step()

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for a, b in ev:
        a.record()
        step()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    assert all(torch.isfinite(p).all() for p in model.parameters())
    line = dict(tag=args.tag, model="DiT-B/2", precision="bf16", micro_steps=args.micro, micro_batch=n, steps=args.steps,
                ms_per_step_median=round(statistics.median(ms), 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4),
                peak_above_resident_mib=round((torch.cuda.max_memory_allocated() - resident) / 2 ** 20, 1),
                grad_buffer_mib=round(model._gflat.numel() * 4 / 2 ** 20, 1))
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
