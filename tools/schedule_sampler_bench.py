#!/usr/bin/env python3
"""What the loss-second-moment schedule sampler costs per training step ("Loss-aware timestep sampling";
profiles/schedule_sampler_b2.json).  Four legs, each printed as one JSON line:

  device   sample() + update_with_local_losses() of LossSecondMomentResampler at N draws, T timesteps, H losses per timestep on a
           warmed-up history (the prepare kernel runs inside the next sample()): device events around blocks of --block iterations with
           no synchronisation inside a block, and the host's enqueue time for the same blocks.
  graph    the same iterations captured into one graph and replayed: the device's time without launch gaps.
  host     the reference's algorithm restated on the host for the same device tensors (reference diffusion/timestep_sampler.py:92-103,
           139-147, 53-58): one .item() per timestep and one per loss, the numpy history update, weights() and np.random.choice; a host
           clock, which is the right one for a path that synchronises per element.
  step     the training step of train.py (fresh synthetic batch, timesteps, losses, backward, fused Adam / EMA) on --model at --batch
           samples: `randint` (the default path: torch.randint and the unweighted mean) and `lsm` (--schedule-sampler loss-second-moment:
           sample, losses, update, weighted mean), alternating blocks of --block steps in ONE process, device events per block.

    python tools/schedule_sampler_bench.py [--legs device,graph,host,step] [--modes randint,lsm] [--out FILE]

`--modes randint` runs on a checkout that has no timestep_sampler module (the parent's step on the same box: copy this file there).
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(v):
    return dict(median_ms=round(statistics.median(v), 5), min_ms=round(min(v), 5), max_ms=round(max(v), 5), blocks=len(v))


def warmed_sampler(T, H, dev, seed=0):
    from mapdit_amd.diffusion.timestep_sampler import LossSecondMomentResampler
    s = LossSecondMomentResampler(types.SimpleNamespace(num_timesteps=T), history_per_term=H)
    rng = np.random.default_rng(seed)
    s.load_state_dict({"loss_history": rng.lognormal(-2.0, 1.0, size=(T, H)).astype(np.float32).astype(np.float64),
                       "loss_counts": np.full(T, H, dtype=np.int64)})
    s.sample(1, dev)                                   # uploads the state
    return s


def leg_device(args, dev):
    s = warmed_sampler(args.T, args.H, dev)
    losses = torch.rand(args.N, device=dev) + 0.01
    dev_ms, host_ms = [], []
    for r in range(args.warmup + args.rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for _ in range(args.block):
            t, w = s.sample(args.N, dev)
            s.update_with_local_losses(t, losses)
        b.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        if r >= args.warmup:
            dev_ms.append(a.elapsed_time(b) / args.block)
            host_ms.append((t1 - t0) * 1e3 / args.block)
    return {"leg": "device", "N": args.N, "T": args.T, "H": args.H, "block": args.block, "launches_per_step": 4,
            "what": "torch.rand + prepare + draw + update per iteration", "device_events_per_step": summary(dev_ms),
            "host_enqueue_per_step": summary(host_ms)}


def leg_graph(args, dev):
    """The device leg's iterations captured into ONE graph (every per-step argument is a device pointer) and replayed: the device's time
    without launch gaps."""
    s = warmed_sampler(args.T, args.H, dev)
    losses = torch.rand(args.N, device=dev) + 0.01
    t, w = s.sample(args.N, dev)
    s.update_with_local_losses(t, losses)              # (the table is dirty at the start of the capture, as at the end of every iteration)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(args.graph_block):
            t, w = s.sample(args.N, dev)
            s.update_with_local_losses(t, losses)
    graph_ms = []
    for r in range(args.warmup + args.rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        if r >= args.warmup:
            graph_ms.append(a.elapsed_time(b) / args.graph_block)
    return {"leg": "graph", "N": args.N, "T": args.T, "H": args.H, "graph_block": args.graph_block, "launches_per_step": 4,
            "what": "the device leg's iterations captured into one graph, device events around a replay", "graph_replay_per_step": summary(graph_ms)}


def leg_host(args, dev):
    """The reference's per-step work on the host, for tensors that live on the device as its training loop's do."""
    T, H = args.T, args.H
    rng = np.random.default_rng(0)
    hist = rng.lognormal(-2.0, 1.0, size=(T, H))
    counts = np.full(T, H, dtype=np.int64)
    losses = torch.rand(args.N, device=dev) + 0.01
    ms = []
    for r in range(args.warmup + args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        # sample (timestep_sampler.py:53-58)
        w = np.sqrt(np.mean(hist ** 2, axis=-1))
        w /= np.sum(w)
        w *= 1 - 0.001
        w += 0.001 / T
        p = w / np.sum(w)
        idx = np.random.choice(T, size=(args.N,), p=p)
        t = torch.from_numpy(idx).long().to(dev)
        wt = torch.from_numpy(1 / (T * p[idx])).float().to(dev)
        # update_with_local_losses (:99-103) for one rank, update_with_all_losses (:139-147)
        ts = [x.item() for x in t]
        ls = [x.item() for x in losses]
        for tt, loss in zip(ts, ls):
            if counts[tt] == H:
                hist[tt, :-1] = hist[tt, 1:]
                hist[tt, -1] = loss
            else:
                hist[tt, counts[tt]] = loss
                counts[tt] += 1
        torch.cuda.synchronize()
        if r >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    del wt
    return {"leg": "host", "N": args.N, "T": T, "H": H, "read_backs_per_step": 2 * args.N,
            "what": "the reference's sample + update on the host, device idle otherwise", "host_clock_per_step": summary(ms)}


def leg_step(args, dev):
    import mapdit_amd  # noqa: F401
    from mapdit_amd.diffusion import create_diffusion
    from mapdit_amd.optim import FusedAdamEMA
    from mapdit_amd.src.models import DIT_MODELS
    modes = args.modes.split(",")
    torch.manual_seed(0)
    model = DIT_MODELS[args.model](in_channels=4, input_size=32, num_classes=1000).to(dev).train()
    model.gemm_precision = args.precision
    opt = FusedAdamEMA(model, lr=1e-4, betas=(0.9, 0.99), ema_stds=(0.05, 0.1))
    diffusion = create_diffusion("")
    sampler = warmed_sampler(diffusion.num_timesteps, 10, dev) if "lsm" in modes else None
    g = torch.Generator(device=dev).manual_seed(1)
    n = args.batch

    def step(mode):
        x = torch.randn(n, 4, 32, 32, device=dev, generator=g)
        y = torch.randint(0, 1000, (n,), device=dev, generator=g)
        if mode == "randint":
            t = torch.randint(0, diffusion.num_timesteps, (n,), device=dev)
            loss = diffusion.training_losses(model, x, t, dict(y=y))["loss"].mean()
        else:
            t, w = sampler.sample(n, dev)
            losses = diffusion.training_losses(model, x, t, dict(y=y))
            sampler.update_with_local_losses(t, losses["loss"].detach())
            loss = (losses["loss"] * w).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()

    times = {m: [] for m in modes}
    for r in range(args.warmup + args.rounds):
        order = modes[r % len(modes):] + modes[:r % len(modes)]
        for m in order:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.step_block):
                step(m)
            b.record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[m].append(a.elapsed_time(b) / args.step_block)
    out = {"leg": "step", "model": args.model, "precision": args.precision, "batch": n, "steps_per_block": args.step_block,
           "what": "train.py's step, device events per block, modes alternating in one process"}
    out.update({m: summary(v) for m, v in times.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="device,graph,host,step")
    ap.add_argument("--modes", default="randint,lsm")
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--H", type=int, default=10)
    ap.add_argument("--block", type=int, default=200, help="sampler iterations per timed block (device leg)")
    ap.add_argument("--graph-block", type=int, default=50, help="sampler iterations captured into the replayed graph (graph leg)")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default="DiT-B/2")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--step-block", type=int, default=10, help="training steps per timed block (step leg)")
    ap.add_argument("--tag", default=None, help="copied into every line (which checkout this is)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X: there is no CPU path and no fallback"
    dev = torch.device("cuda", 0)
    for leg in args.legs.split(","):
        line = {"device": leg_device, "graph": leg_graph, "host": leg_host, "step": leg_step}[leg](args, dev)
        if args.tag:
            line["tag"] = args.tag
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
