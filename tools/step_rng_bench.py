#!/usr/bin/env python3
"""The counter-based step draws and --resume, measured.

    python tools/step_rng_bench.py [--rounds 3] [--out profiles/step_rng_b2.json] [--legs train,resume,draw]

  draw    device time of one mapdit_step_draw call at count 256, per 4096 with the outputs a default step uses (eps, t, drop; 4 MB
          written), against the torch calls it replaces (torch.randn_like + torch.randint + torch.rand < p): device events around 5
          replays of a graph that holds `--graph-calls` calls (the launches alone), and around `--calls` eager calls (what a loop pays);
          the floor is 4 MB over the HBM rate
  train   train.py --synthetic steps per second on DiT-B/2 at 256 samples, bf16, --step-rng torch and counter ALTERNATING in fresh
          processes, `--rounds` each; the figure of a run is the median of its log windows after the first (which holds start-up)
  resume  wall time of a fresh process from start to its first logged step, for --resume from a DiT-B/2 checkpoint against a new run, and
          the checkpoint's size with the keys --resume needs ("ema", "train_state") against the reference's two
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
from mapdit_amd.step_rng import StepRNG  # noqa: E402

HBM_BYTES_PER_S = 8.0e12                                                  # MI355X HBM3E, specified peak (a float4 copy reaches 6.3e12)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}


def timed(fn, calls, graph_calls, rounds):
    """(us per call eager, us per call inside a graph) of fn(i)."""
    for i in range(20):
        fn(i)
    torch.cuda.synchronize()
    eager, graphed = [], []
    for r in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(calls):
            fn(r * calls + i)
        b.record()
        torch.cuda.synchronize()
        eager.append(a.elapsed_time(b) * 1e3 / calls)
    graph, keep = torch.cuda.CUDAGraph(), []
    with torch.cuda.graph(graph):
        for i in range(graph_calls):
            keep.append(fn(i))
    graph.replay()
    torch.cuda.synchronize()
    for r in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(5):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        graphed.append(a.elapsed_time(b) * 1e3 / (5 * graph_calls))
    return spread(eager), spread(graphed)


def leg_draw(args):
    dev = torch.device("cuda", 0)
    rng, x = StepRNG(0, dev), torch.zeros(256, 4, 32, 32, device=dev)

    def counter(i):
        return rng.draw(i, 0, 256, per=4096, T=1000, drop_prob=0.1, want=("eps", "t", "drop"))

    def torch_calls(i):
        return torch.randn_like(x), torch.randint(0, 1000, (256,), device=dev), torch.rand(256, device=dev) < 0.1

    out = {}
    for name, fn in (("counter", counter), ("torch", torch_calls)):
        eager, graphed = timed(fn, args.calls, args.graph_calls, args.rounds)
        out[name] = {"us_per_call_eager": eager, "us_per_call_in_graph": graphed}
    moved = 256 * 4096 * 4 + 2 * 256 * 8
    out["bytes_written"] = moved
    out["hbm_floor_us"] = moved / HBM_BYTES_PER_S * 1e6
    out["counter_over_floor_in_graph"] = out["counter"]["us_per_call_in_graph"]["median"] / out["hbm_floor_us"]
    out["counter_over_torch_in_graph"] = out["counter"]["us_per_call_in_graph"]["median"] / out["torch"]["us_per_call_in_graph"]["median"]
    return out


def train_cmd(results, extra, steps, every):
    return [sys.executable, "-m", "mapdit_amd.train", "--synthetic", "--model", "DiT-B/2", "--batch-size", "256", "--precision", "bf16",
            "--num-steps", str(steps), "--log-every", str(every), "--ema-snapshot-every", "1000000", "--num-lin-warmup", "1",
            "--start-decay", "1000000"] + (["--results-dir", results] if results else []) + extra


def run(cmd):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=420)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout, time.perf_counter() - t0


def leg_train(args):
    results, runs = tempfile.mkdtemp(prefix="step_rng_bench_"), {"torch": [], "counter": []}
    try:
        for _ in range(args.rounds):
            for mode in ("torch", "counter"):                            # interleaved: a drift of the machine hits both
                out, _ = run(train_cmd(results, ["--step-rng", mode, "--ckpt-every", "1000000"], args.steps, args.steps // 4))
                sps = [float(v) for v in re.findall(r"train steps/sec: (\d+\.\d+)", out)]
                runs[mode].append(statistics.median(sps[1:]))
                print(f"DiT-B/2 256 --step-rng {mode}: {runs[mode][-1]:.2f} steps/s", file=sys.stderr, flush=True)
    finally:
        shutil.rmtree(results, ignore_errors=True)
    return {"steps_per_s_torch": spread(runs["torch"]), "steps_per_s_counter": spread(runs["counter"]),
            "ms_per_step_torch_at_median": 1e3 / statistics.median(runs["torch"]), "ms_per_step_counter_at_median": 1e3 / statistics.median(runs["counter"]),
            "counter_over_torch_at_median": statistics.median(runs["counter"]) / statistics.median(runs["torch"])}


def leg_resume(args):
    results = tempfile.mkdtemp(prefix="step_rng_bench_")
    try:
        out, _ = run(train_cmd(results, ["--step-rng", "counter", "--ckpt-every", "4"], 4, 4))
        exp = os.path.join(results, os.listdir(results)[0])
        ckpt = os.path.join(exp, "checkpoints", "0000004.pt")
        full = torch.load(ckpt, map_location="cpu", weights_only=True)
        plain = os.path.join(results, "plain.pt")
        torch.save({"model": full["model"], "opt": full["opt"]}, plain)
        sizes = {"checkpoint_bytes": os.path.getsize(ckpt), "checkpoint_bytes_model_and_opt_only": os.path.getsize(plain)}
        del full
        os.remove(plain)
        fresh, resumed = [], []
        for r in range(args.rounds):                                     # a process that logs its first step and ends: start-up + 1 step
            fresh.append(run(train_cmd(results, ["--step-rng", "counter", "--ckpt-every", "1000000"], 1, 1))[1])
            resumed.append(run([sys.executable, "-m", "mapdit_amd.train", "--resume", ckpt, "--num-steps", "5", "--log-every", "1",
                                "--ckpt-every", "1000000"])[1])
        return {**sizes, "process_wall_s_new_run_one_step": spread(fresh), "process_wall_s_resume_one_step": spread(resumed),
                "resume_minus_new_at_median_s": statistics.median(resumed) - statistics.median(fresh)}
    finally:
        shutil.rmtree(results, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--graph-calls", type=int, default=100)
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--legs", default="train,resume,draw")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_rng_b2.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("step_rng_bench.py measures on the GPU: no device visible")
    res, legs = {"rounds": args.rounds, "device": torch.cuda.get_device_name(0)}, args.legs.split(",")
    if "train" in legs:                                                  # first: this process has not opened the device's memory yet
        res["train"] = leg_train(args)
    if "resume" in legs:
        res["resume"] = leg_resume(args)
    if "draw" in legs:
        res["draw"] = leg_draw(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
