#!/usr/bin/env python3
"""Likelihood evaluation cost: calc_bpd_loop (bits per dimension) of DiT-B/2 at 256 samples on a '50' schedule, per timestep,
next to the eval forward alone at the same shape (the loop's per-timestep work = one randn draw, q_sample, the forward and one
mapdit_obj_vb_terms launch).

    python tools/bpd_bench.py [--model DiT-B/2] [--n 256] [--respacing 50] [--repeats 3]
Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats` the stats give the bound kernel's own time.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mapdit_amd  # noqa: E402,F401
from mapdit_amd.diffusion import create_diffusion  # noqa: E402
from mapdit_amd.src.models import DIT_MODELS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="DiT-B/2")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--respacing", default="50")
    ap.add_argument("--repeats", type=int, default=3, help="timed calc_bpd_loop runs (the best is reported)")
    ap.add_argument("--precision", choices=["bf16", "f16", "bf16x3"], default="f16")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = DIT_MODELS[args.model](in_channels=4, input_size=32, num_classes=1000).to(dev).eval().requires_grad_(False)
    model.gemm_precision = args.precision
    d = create_diffusion(args.respacing)
    T = d.num_timesteps
    x0 = torch.rand(args.n, 4, 32, 32, device=dev) * 2 - 1
    y = torch.randint(0, 1000, (args.n,), device=dev)
    kw = dict(y=y)

    def timed(fn, reps):
        best = float("inf")
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        return best

    with torch.no_grad():
        d.calc_bpd_loop(model.forward, x0, model_kwargs=kw)                  # warm-up (engine workspace, weight images)
        loop = timed(lambda: d.calc_bpd_loop(model.forward, x0, model_kwargs=kw), args.repeats)

        def forwards():
            for i in range(T)[::-1]:
                model.forward(x0, torch.full((args.n,), d.timestep_map[i], device=dev), y)
        fwd = timed(forwards, args.repeats)
        r = d.calc_bpd_loop(model.forward, x0, model_kwargs=kw)
    per_loop, per_fwd = 1e3 * loop / T, 1e3 * fwd / T
    print(json.dumps({"metric": f"calc_bpd_loop per timestep, {args.model}, {args.n} samples, respacing '{args.respacing}'",
                      "ms_per_timestep_bpd_loop": per_loop, "ms_per_timestep_eval_forward": per_fwd,
                      "overhead_pct": 100 * (per_loop / per_fwd - 1), "timesteps": T, "dtype": args.precision,
                      "mean_total_bpd": float(r["total_bpd"].mean())}))


if __name__ == "__main__":
    main()
