#!/usr/bin/env python3
"""The data pipeline of train.py, host loader against the device-resident data set, on a data set the tool writes itself.

    python tools/data_bench.py [--samples 65536] [--rounds 3] [--out profiles/data_pipeline_b2.json] [--legs batch,loader,train]

The data set is random tensors in the reference's four-file layout (N x 4 x 32 x 32 means and stds, labels, stats) in a temporary
directory that is removed at the end.  Three legs:
  batch    device time of one DeviceLatentDataset.batch() call at 256 and at 32 samples, `--rounds` times each way: device events
           around `--calls` back-to-back eager calls (what a training loop pays: the host enqueues two allocations and a launch), and
           around 5 replays of a graph that holds `--graph-calls` calls (the launches alone; they revisit the same steps, so at 32
           samples their 105 MB of rows stay in the last-level cache); bytes are counted from the shapes (means + stds read, x
           written, per sample 3 x C x H x W x 4)
  loader   samples per second of train.py's host path on its own - LatentDataset behind a DataLoader with --num-workers 4, pinned,
           batches of 256 copied to the device - by the host clock around whole batches that end in a device synchronise
  train    train.py steps per second, --data-loader host and device ALTERNATING in fresh processes, `--rounds` each: DiT-B/2 at
           256 samples and DiT-S/2 at 32 (the per-rank shape of an 8-GPU run), bf16; the figure of a run is the median of its log
           windows after the first (which holds start-up)
Every figure is reported as median and range over the rounds.  None is a pass condition.  Prints one JSON line and writes --out.
"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mapdit_amd  # noqa: E402,F401
from mapdit_amd import train  # noqa: E402
from mapdit_amd.data import DeviceLatentDataset  # noqa: E402


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}


def write_set(path, n):
    g = torch.Generator().manual_seed(0)
    torch.save(torch.randn(n, 4, 32, 32, generator=g), os.path.join(path, "posterior_means.pt"))
    torch.save(torch.rand(n, 4, 32, 32, generator=g) * 0.5, os.path.join(path, "posterior_stds.pt"))
    torch.save(torch.randint(0, 1000, (n,), generator=g), os.path.join(path, "labels.pt"))
    torch.save({"mean": torch.zeros(4), "std": torch.ones(4)}, os.path.join(path, "stats.pt"))


def leg_batch(path, args):
    dev = torch.device("cuda", 0)
    ds = DeviceLatentDataset(path, dev, seed=0)
    out = {}
    for B in (256, 32):
        for s in range(20):
            ds.batch(s, B)                                               # warm-up: code object, allocator
        torch.cuda.synchronize()
        us = []
        for r in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for s in range(args.calls):
                ds.batch(r * args.calls + s, B)
            b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / args.calls)
        # the same calls captured into one graph: the launches back to back, without the host's enqueueing between them
        graph, keep = torch.cuda.CUDAGraph(), []
        with torch.cuda.graph(graph):
            for s in range(args.graph_calls):
                keep.append(ds.batch(s, B))
        graph.replay()
        torch.cuda.synchronize()
        gus = []
        for r in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(5):
                graph.replay()
            b.record()
            torch.cuda.synchronize()
            gus.append(a.elapsed_time(b) * 1e3 / (5 * args.graph_calls))
        moved = 3 * B * 4 * 32 * 32 * 4
        out[f"batch_{B}"] = {"us_per_call_eager": spread(us), "us_per_call_in_graph": spread(gus), "bytes_per_call": moved,
                             "gb_per_s_in_graph_at_median": moved / statistics.median(gus) / 1e3}
    return out


def leg_loader(path, args):
    dev = torch.device("cuda", 0)
    ds = train.LatentDataset(path)
    loader = torch.utils.data.DataLoader(ds, batch_size=256, num_workers=4, shuffle=True, pin_memory=True, drop_last=True)
    rates = []
    for r in range(args.rounds + 1):                                     # round 0 starts the workers: not counted
        it = iter(loader)
        for _ in range(8):
            x, y = next(it)
        torch.cuda.synchronize()
        t0, n = time.perf_counter(), 0
        for _ in range(args.loader_batches):
            x, y = next(it)
            x, y = x.to(dev, non_blocking=True), y.to(dev, non_blocking=True)
            n += x.shape[0]
        torch.cuda.synchronize()
        if r:
            rates.append(n / (time.perf_counter() - t0))
        del it
    return {"host_loader_workers4_samples_per_s": spread(rates)}


def train_run(path, results, model, batch, loader, steps, every):
    cmd = [sys.executable, "-m", "mapdit_amd.train", "--data-path", path, "--results-dir", results, "--model", model, "--batch-size", str(batch),
           "--precision", "bf16", "--num-steps", str(steps), "--log-every", str(every), "--ckpt-every", "1000000", "--ema-snapshot-every", "1000000",
           "--num-lin-warmup", "1", "--start-decay", str(steps), "--data-loader", loader]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=420)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    sps = [float(v) for v in re.findall(r"train steps/sec: (\d+\.\d+)", r.stdout)]
    return statistics.median(sps[1:])


def leg_train(path, args):
    out = {}
    results = tempfile.mkdtemp(prefix="data_bench_results_")
    try:
        for model, batch, steps, every in (("DiT-B/2", 256, args.steps_b2, args.steps_b2 // 4), ("DiT-S/2", 32, args.steps_s2, args.steps_s2 // 4)):
            runs = {"host": [], "device": []}
            for _ in range(args.rounds):
                for loader in ("host", "device"):                        # interleaved: a drift of the machine hits both
                    runs[loader].append(train_run(path, results, model, batch, loader, steps, every))
                    print(f"{model} {batch} {loader}: {runs[loader][-1]:.2f} steps/s", file=sys.stderr, flush=True)
            key = f"{model.replace('/', '-')}_bf16_{batch}"
            out[key] = {"steps_per_s_host": spread(runs["host"]), "steps_per_s_device": spread(runs["device"]),
                        "device_over_host_at_median": statistics.median(runs["device"]) / statistics.median(runs["host"])}
    finally:
        shutil.rmtree(results, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--graph-calls", type=int, default=100)
    ap.add_argument("--loader-batches", type=int, default=200)
    ap.add_argument("--steps-b2", type=int, default=80)
    ap.add_argument("--steps-s2", type=int, default=400)
    ap.add_argument("--legs", default="batch,loader,train")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_pipeline_b2.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("data_bench.py measures on the GPU: no device visible")
    path = tempfile.mkdtemp(prefix="data_bench_set_")
    try:
        write_set(path, args.samples)
        res = {"data_set": f"{args.samples} x 4 x 32 x 32 fp32 means and stds (random), labels < 1000", "rounds": args.rounds,
               "device": torch.cuda.get_device_name(0)}
        legs = args.legs.split(",")
        if "train" in legs:                                              # first: this process has not opened the device's memory yet
            res["train"] = leg_train(path, args)
        if "loader" in legs:
            res["loader"] = leg_loader(path, args)
        if "batch" in legs:
            res["batch"] = leg_batch(path, args)
    finally:
        shutil.rmtree(path, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
