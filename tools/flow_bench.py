#!/usr/bin/env python3
"""Rectified flow: device time of its pointwise chain and wall time of its captured sampler.

    python tools/flow_bench.py --loss [--n 256] [--rounds 10] [--iters 100] [--replays 20]
the three launches around the model of one training step, flow objective against the default diffusion objective, on DiT-B/2 shapes
(N x 4 x 32 x 32 latents, an 8-channel model output), interleaved in one process: device events around `replays` replays of a
hipGraph that holds `iters` back-to-back repetitions of a chain, `rounds` alternations, median and range.  Bytes are counted from the
shapes; the 4 MiB tensors stay in the last-level cache between repetitions, so the rates are not HBM rates.

    python tools/flow_bench.py --chains 5 [--model DiT-XL/2] [--images 128]
whole captured chains with classifier-free guidance: dpm++ at 20 steps, flow-heun at 20 steps and flow-euler at 39 steps (the same 39
model evaluations), alternating, median of --chains runs after one warm-up run each.  A cost figure, not a quality claim.

Each mode prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mapdit_amd  # noqa: E402,F401
from mapdit_amd import _lib as L  # noqa: E402
from mapdit_amd.diffusion import create_diffusion  # noqa: E402
from mapdit_amd.flow import create_flow  # noqa: E402
from mapdit_amd.sampling import GraphedSampler  # noqa: E402
from mapdit_amd.src.models import DIT_MODELS  # noqa: E402


def loss_chain(args):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    N, C, S = args.n, 4, 32
    per = C * S * S
    x0, eps = (torch.randn(N, C, S, S, device=dev, generator=g) for _ in range(2))
    mo = torch.randn(N, 2 * C, S, S, device=dev, generator=g)
    t = torch.randint(0, 1000, (N,), device=dev, generator=g)
    gl = torch.full((N,), 1.0 / N, device=dev)
    xt, G, dout = torch.empty_like(x0), torch.empty_like(mo), torch.empty_like(mo)
    loss, mse, vb = (torch.empty(N, device=dev) for _ in range(3))
    flow, diff = create_flow(), create_diffusion("")
    sig, tab = flow._tables(dev), diff._tables(dev)
    lib, st = L.lib(), L.cur_stream()
    p = lambda v: v.data_ptr()

    def flow_chain():                                            # (st: the stream current when the chain is enqueued, set below)
        lib.flow_q_sample(p(x0), p(eps), p(t), p(sig), 1000, p(xt), N, per, st)
        lib.flow_loss_fwd(p(mo), p(x0), p(eps), p(loss), p(G), N, per, 2, st)
        lib.obj_loss_bwd(p(G), p(gl), None, None, p(dout), N, per, 2, st)

    def diffusion_chain():
        lib.q_sample(p(x0), p(eps), p(t), p(tab), 1000, p(xt), N, per, st)
        lib.loss_fwd(p(mo), p(x0), p(xt), p(eps), p(t), p(tab), 1000, p(mse), p(vb), p(loss), p(G), N, per, st)
        lib.loss_bwd(p(G), p(gl), None, None, p(dout), N, per, st)

    # `iters` repetitions of a chain are captured into one hipGraph: three launches of ~10 us each cannot be enqueued from Python as
    # fast as the device runs them, and a window timed around eager launches would measure the host
    graphs = {}
    for name, fn in (("flow", flow_chain), ("diffusion", diffusion_chain)):
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            st = L.cur_stream()
            fn()                                                     # warm-up: code objects
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            st = L.cur_stream()
            for _ in range(args.iters):
                fn()

    def timed(graph):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.replays):
            graph.replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / (args.iters * args.replays)

    for g_ in graphs.values():
        timed(g_)
    ms = {"flow": [], "diffusion": []}
    for _ in range(args.rounds):
        ms["flow"].append(timed(graphs["flow"]))
        ms["diffusion"].append(timed(graphs["diffusion"]))
    e = 4 * N * per                                              # bytes of one [N, C, H, W] fp32 tensor
    bytes_moved = {
        # q_sample: x0, eps -> xt;  loss_fwd: model_out (first C channels), x0, eps -> G (2C, the second C zeros);  bwd: G -> dout (2C each)
        "flow": {"q_sample": 3 * e, "loss_fwd": 3 * e + 2 * e, "loss_bwd": 4 * e},
        # loss_fwd reads model_out (2C), x0, xt, eps and writes G (2C)
        "diffusion": {"q_sample": 3 * e, "loss_fwd": 5 * e + 2 * e, "loss_bwd": 4 * e},
    }
    out = {"metric": f"pointwise chain of one training step (q_sample + loss_fwd + loss_bwd), {N} x {C} x {S} x {S}, model output {2 * C} channels",
           "chains_per_window": args.iters * args.replays, "rounds": args.rounds}
    for k in ms:
        med = statistics.median(ms[k])
        total = sum(bytes_moved[k].values())
        out[k] = {"ms_median": med, "ms_min": min(ms[k]), "ms_max": max(ms[k]), "ms": ms[k], "bytes": bytes_moved[k], "bytes_total": total,
                  "gb_per_s_at_median": total / med / 1e6}
    out["flow_over_diffusion"] = out["flow"]["ms_median"] / out["diffusion"]["ms_median"]
    print(json.dumps(out))


def chains(args):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = DIT_MODELS[args.model](in_channels=4, input_size=32, num_classes=1000).to(dev).eval().requires_grad_(False)
    model.gemm_precision = args.precision
    n = args.images
    z = torch.randn(n, 4, 32, 32, device=dev)
    z = torch.cat([z, z], 0)
    y = torch.cat([torch.randint(0, 1000, (n,), device=dev), torch.full((n,), 1000, device=dev)])
    flow = create_flow()
    samplers = {"dpm++ 20": GraphedSampler(model, create_diffusion(""), z.shape, y, cfg_scale=args.cfg_scale, sampler="dpm++", num_steps=20),
                "flow-heun 20": GraphedSampler(model, flow, z.shape, y, cfg_scale=args.cfg_scale, sampler="flow", num_steps=20, order=2),
                "flow-euler 39": GraphedSampler(model, flow, z.shape, y, cfg_scale=args.cfg_scale, sampler="flow", num_steps=39, order=1)}
    times = {k: [] for k in samplers}
    for r in range(args.chains + 1):                             # the first round is the warm-up
        for k, s in samplers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.sample(z)
            torch.cuda.synchronize()
            if r:
                times[k].append(time.perf_counter() - t0)
    out = {"metric": f"whole captured chain, {args.model}, cfg {args.cfg_scale}, batch 2x{n}", "dtype": args.precision}
    for k, s in samplers.items():
        med = statistics.median(times[k])
        out[k] = {"model_evaluations": s.num_replays, "s_per_batch_median": med, "s_per_batch": times[k], "ms_per_evaluation": 1e3 * med / s.num_replays}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loss", action="store_true")
    ap.add_argument("--n", type=int, default=256, help="--loss: samples of the batch")
    ap.add_argument("--images", type=int, default=128, help="--chains: images per batch (the CFG batch is twice as many rows)")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100, help="--loss: chain repetitions captured into one graph")
    ap.add_argument("--replays", type=int, default=20, help="--loss: graph replays per timed window")
    ap.add_argument("--chains", type=int, default=0)
    ap.add_argument("--model", default="DiT-XL/2")
    ap.add_argument("--cfg-scale", type=float, default=1.5)
    ap.add_argument("--precision", choices=["bf16", "f16"], default="bf16")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flow_bench.py measures on the MI355X: no GPU found")
    if args.loss:
        loss_chain(args)
    if args.chains > 0:
        chains(args)
    if not args.loss and args.chains <= 0:
        ap.error("pass --loss and / or --chains K")


if __name__ == "__main__":
    main()
