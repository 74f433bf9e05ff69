#!/usr/bin/env python3
"""Counter-based sampler noise: what the fused ancestral step costs beside today's.

    python tools/bench_sample_rng.py [--model DiT-XL/2] [--images 128] [--runs 3] [--replays 50]
one captured ancestral step (classifier-free guidance at 1.5, 2 x --images rows, 250-step schedule) of two GraphedSamplers in one
process and one build: rng=None - the torch generator's randn_like, mapdit_psample_step and the copy back, launch for launch what the
sampler has always captured - and rng=SampleRNG, the in-place mapdit_psample_step_counter.  Device events around --replays replays,
--runs runs of each, alternating; median and range per step.  The step counter is reset before every run, so every timed step draws
noise.

    python tools/bench_sample_rng.py --kernels [--iters 100]
the step's pointwise tail alone at the same shape: randn_like + mapdit_psample_step + copy against mapdit_psample_step_counter,
--iters repetitions captured into one graph each (launches this short cannot be enqueued from Python as fast as they run).  The 4 MiB
tensors stay in the last-level cache between repetitions: a cost figure, not a memory rate.

Each mode prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mapdit_amd  # noqa: E402,F401
from mapdit_amd import _lib as L  # noqa: E402
from mapdit_amd.diffusion import create_diffusion  # noqa: E402
from mapdit_amd.sample_rng import SampleRNG  # noqa: E402
from mapdit_amd.sampling import GraphedSampler  # noqa: E402
from mapdit_amd.src.models import DIT_MODELS  # noqa: E402

DEV = torch.device("cuda", 0)


def window(fn, count):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(count):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / count


def summary(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "ms": ms}


def steps(args):
    torch.manual_seed(0)
    model = DIT_MODELS[args.model](in_channels=4, input_size=32, num_classes=1000).to(DEV).eval().requires_grad_(False)
    model.gemm_precision = args.precision
    n = args.images
    d = create_diffusion("250")
    rng = SampleRNG(0, DEV)
    index = list(range(n))
    z = rng.latents(index + index, (4, 32, 32))
    y = torch.cat([rng.labels(index, 1000), torch.full((n,), 1000, device=DEV)])
    samplers = {"torch": GraphedSampler(model, d, z.shape, y, cfg_scale=args.cfg_scale),
                "counter": GraphedSampler(model, d, z.shape, y, cfg_scale=args.cfg_scale, rng=rng)}
    samplers["counter"].index.copy_(torch.tensor(index + index, device=DEV))
    assert args.replays < d.num_timesteps, "every timed step must be one that draws noise (t > 0)"
    ms = {k: [] for k in samplers}
    for r in range(args.runs + 1):                               # the first round is the warm-up
        for k, s in samplers.items():
            s.img.copy_(z)
            s.t.fill_(d.num_timesteps - 1)
            torch.cuda.synchronize()
            t = window(s.graph.replay, args.replays)
            if r:
                ms[k].append(t)
    out = {"metric": f"one captured ancestral step, {args.model}, cfg {args.cfg_scale}, batch 2x{n}, {args.replays} replays per run",
           "dtype": args.precision, **{k: summary(v) for k, v in ms.items()}}
    out["counter_minus_torch_ms"] = out["counter"]["ms_median"] - out["torch"]["ms_median"]
    out["spread_ms"] = max(v["ms_max"] - v["ms_min"] for v in (out["torch"], out["counter"]))
    print(json.dumps(out))


def kernels(args):
    g = torch.Generator(device=DEV).manual_seed(0)
    N, per = 2 * args.images, 4 * 32 * 32
    d = create_diffusion("250")
    tab = d._tables(DEV)
    mo = torch.randn(N, 2 * per, device=DEV, generator=g)
    img = torch.randn(N, per, device=DEV, generator=g)
    t = torch.full((N,), 100, device=DEV, dtype=torch.int64)
    index = torch.arange(N, device=DEV, dtype=torch.int64)
    lib = L.lib()

    def unfused():                                               # the tail of GraphedSampler._step without an rng
        noise = torch.randn_like(img)
        nxt = torch.empty_like(img)
        lib.psample_step(mo.data_ptr(), img.data_ptr(), noise.data_ptr(), t.data_ptr(), tab.data_ptr(), d.num_timesteps, 0, nxt.data_ptr(), None,
                         N, per, L.cur_stream())
        img.copy_(nxt)

    def fused():
        lib.psample_step_counter(mo.data_ptr(), img.data_ptr(), 0, index.data_ptr(), t.data_ptr(), tab.data_ptr(), d.num_timesteps, 0,
                                 img.data_ptr(), None, N, per, L.cur_stream())

    graphs = {}
    for name, fn in (("unfused", unfused), ("fused", fused)):
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream(DEV).wait_stream(side)
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(args.iters):
                fn()
    ms = {k: [] for k in graphs}
    for r in range(args.runs + 1):
        for k, gr in graphs.items():
            t_ms = window(gr.replay, args.replays) / args.iters
            if r:
                ms[k].append(t_ms)
    out = {"metric": f"pointwise tail of one ancestral step, {N} x {per} fp32", "repetitions_per_window": args.iters * args.replays,
           **{k: summary(v) for k, v in ms.items()}}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--model", default="DiT-XL/2")
    ap.add_argument("--images", type=int, default=128, help="images per batch (the guidance batch is twice as many rows)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--iters", type=int, default=100, help="--kernels: repetitions captured into one graph")
    ap.add_argument("--cfg-scale", type=float, default=1.5)
    ap.add_argument("--precision", choices=["bf16", "f16"], default="f16")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample_rng.py measures on the MI355X: no GPU found")
    if args.kernels:
        kernels(args)
    else:
        steps(args)


if __name__ == "__main__":
    main()
