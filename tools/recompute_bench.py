#!/usr/bin/env python3
"""What activation recompute costs and saves: DiT-B/2, 256 samples, bf16, synthetic inputs (the benchmark's shape), one process.

    python tools/recompute_bench.py [--steps 20] [--warmup 5] [--rounds 2] [--out profiles/recompute_bench_b2_n256.jsonl]

For each level (none / mlp / block; DiT.activation_recompute) in turn, `rounds` times over so that drift of the box reaches every level
alike: `warmup` + `steps` training steps (bench.py's step: fresh batch, training_losses, backward, fused Adam + EMA; HIP events around
each whole step), the training forward alone (mapdit_engine_forward with save=1: no weight pass, no loss) and the fc1 launches of those
forwards through the MAPDIT_PROF_FC1_FWD hook.  One JSON line per level: medians, the training workspace, and the cost the code predicts
from the `none` line OF THE SAME RUN - a re-run issues the forward's launches and nothing else, so

    mlp   = none + depth x one fc1 launch
    block = none + one forward (the whole forward is taken: conditioning, patch embedding and final layer are < 2 % of it)

`added_over_predicted` above 1.10 means the level costs more than its launches explain (look at a kernel trace of its own then).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
MODEL, BATCH, PRECISION = "DiT-B/2", 256, "bf16"
LEVELS = ["none", "mlp", "block"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recompute_bench_b2_n256.jsonl"))
    args = ap.parse_args()

    import torch
    import mapdit_amd  # noqa: F401
    from mapdit_amd import _lib as L
    from mapdit_amd.diffusion import create_diffusion
    from mapdit_amd.optim import FusedAdamEMA, create_lr_lambda
    from mapdit_amd.src.models import DIT_MODELS
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = DIT_MODELS[MODEL](in_channels=4, input_size=32, num_classes=1000).to(dev).train()
    model.gemm_precision = PRECISION
    diffusion = create_diffusion(timestep_respacing="")
    opt = FusedAdamEMA(model, lr=1e-2, betas=(0.9, 0.99), ema_stds=(0.05, 0.1), lr_lambda=create_lr_lambda(2666, 40000))
    g = torch.Generator(device=dev).manual_seed(1)

    def events(n):
        return [torch.cuda.Event(enable_timing=True) for _ in range(n)]

    def batch():
        return (torch.randn(BATCH, 4, 32, 32, device=dev, generator=g), torch.randint(0, 1000, (BATCH,), device=dev, generator=g),
                torch.randint(0, diffusion.num_timesteps, (BATCH,), device=dev))

    def step():
        x, y, t = batch()
        loss = diffusion.training_losses(model, x, t, dict(y=y))["loss"].mean()
        opt.zero_grad()
        loss.backward()
        opt.step()

    def timed_steps(n):
        ev = events(n + 1)
        ev[0].record()
        for i in range(n):
            step()
            ev[i + 1].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]

    res = {lv: {"step_ms": [], "forward_ms": [], "fc1_ms": [], "fc1_launches": 0, "workspace_bytes": None} for lv in LEVELS}
    for _ in range(args.rounds):
        for lv in LEVELS:
            model.activation_recompute = lv          # (the next training forward rebuilds the training runtime at this level)
            timed_steps(args.warmup)
            r = res[lv]
            r["step_ms"] += timed_steps(args.steps)
            rt = model._rt[True]
            assert rt.recompute == lv
            r["workspace_bytes"] = rt.workspace.numel()
            # the training forward alone, on the weight images of the last step, with every fc1 launch bracketed
            x, y, t = batch()
            out = torch.empty(BATCH, 8, 32, 32, device=dev)
            fwd = lambda: rt.lib.engine_forward(rt.handle, x.data_ptr(), t.data_ptr(), y.data_ptr(), BATCH, 1, out.data_ptr(), L.cur_stream())
            for _ in range(3):
                fwd()
            ev = events(args.steps + 1)
            ev[0].record()
            for i in range(args.steps):
                fwd()
                ev[i + 1].record()
            torch.cuda.synchronize()
            r["forward_ms"] += [ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps)]
            L.lib().engine_profile_begin(rt.handle, L.PROF_FC1_FWD, model.depth * 5)
            for _ in range(5):
                fwd()
            cnt, tot = C.c_int(0), C.c_double(0.0)
            L.lib().engine_profile_end(rt.handle, C.byref(cnt), C.byref(tot))
            r["fc1_ms"].append(tot.value / cnt.value)
            r["fc1_launches"] = model.depth
            rt.generation += 1                       # (those forwards replaced the saved activations of the last autograd forward)

    med = statistics.median
    base = res["none"]
    lines = []
    for lv in LEVELS:
        r = res[lv]
        s, f, c = med(r["step_ms"]), med(r["forward_ms"]), med(r["fc1_ms"])
        predicted = {"none": 0.0, "mlp": model.depth * med(base["fc1_ms"]), "block": med(base["forward_ms"])}[lv]
        added = s - med(base["step_ms"])
        lines.append({"model": MODEL, "batch": BATCH, "precision": PRECISION, "level": lv, "steps": len(r["step_ms"]), "rounds": args.rounds,
                      "workspace_bytes": r["workspace_bytes"], "step_ms": round(s, 4), "step_ms_min": round(min(r["step_ms"]), 4),
                      "forward_ms": round(f, 4), "fc1_ms_per_launch": round(c, 4), "fc1_launches_per_forward": r["fc1_launches"],
                      "step_over_none": round(s / med(base["step_ms"]), 4), "added_ms": round(added, 4),
                      "predicted_added_ms": round(predicted, 4),
                      "added_over_predicted": round(added / predicted, 4) if predicted else None,
                      "workspace_over_none": round(r["workspace_bytes"] / base["workspace_bytes"], 4)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + "\n")
            print(json.dumps(ln), flush=True)


if __name__ == "__main__":
    main()
