#!/usr/bin/env python3
"""What the input-latent gradient costs: DiT-B/2 at 256 samples, bf16 and f16, one box, one session.

    python tools/time_input_grad.py --parent-tree DIR [--rounds 2] [--steps 20] [--warmup 5] [--out profiles/input_grad_timing.json]

DIR is a BUILT checkout of the parent commit (git worktree / git archive + make -C map-dit_amd/csrc); without it (a) is skipped.

 (a) the plain training step (bench.py's step: fresh batch, training_losses, backward, fused Adam + EMA) of the parent tree and of this
     tree, in fresh processes that alternate parent / this tree, `rounds` times: medians of the per-step device-event times.  They must
     agree within the box spread tools/README.md's A/B drivers work with (about 4 %).
 (b) the same step with x_t.requires_grad (model.input_gradients = True), interleaved with the plain step in ONE process: the added
     cost is mapdit_patch_embed_bwd_x (one pass over the 100 MB gradient of the patch embedding output) and one 4 MB allocation.
 (c) the backward alone (device events around out.backward(dout) of an eval-mode saved forward): full backward, full backward + dx,
     input-only backward (frozen weights), interleaved in the same process.

Every worker is a fresh child process (the parent process never opens the GPU); each warms up every shape it times and reports
medians.  One JSON document goes to --out and a summary to stdout.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODEL, BATCH = "DiT-B/2", 256


def worker(args):
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import mapdit_amd  # noqa: F401
    from mapdit_amd.diffusion import create_diffusion
    from mapdit_amd.optim import FusedAdamEMA, create_lr_lambda
    from mapdit_amd.src.models import DIT_MODELS
    assert torch.cuda.is_available(), "needs an MI355X"
    assert os.path.abspath(mapdit_amd.__file__).startswith(os.path.abspath(args.tree)), mapdit_amd.__file__
    dev = torch.device("cuda", 0)
    res = {}

    def events(n):
        return [torch.cuda.Event(enable_timing=True) for _ in range(n)]

    for precision in args.precisions.split(","):
        torch.manual_seed(0)
        model = DIT_MODELS[MODEL](in_channels=4, input_size=32, num_classes=1000).to(dev).train()
        model.gemm_precision = precision
        diffusion = create_diffusion(timestep_respacing="")
        opt = FusedAdamEMA(model, lr=1e-2, betas=(0.9, 0.99), ema_stds=(0.05, 0.1), lr_lambda=create_lr_lambda(2666, 40000))
        g = torch.Generator(device=dev).manual_seed(1)
        with_x = lambda xt, t, **kw: model(xt.requires_grad_(True), t, **kw)       # x_t is a leaf: dL/dx_t lands in its .grad

        def step(xgrad=False):
            x = torch.randn(BATCH, 4, 32, 32, device=dev, generator=g)
            y = torch.randint(0, 1000, (BATCH,), device=dev, generator=g)
            t = torch.randint(0, diffusion.num_timesteps, (BATCH,), device=dev)
            loss = diffusion.training_losses(with_x if xgrad else model, x, t, dict(y=y))["loss"].mean()
            opt.zero_grad()
            loss.backward()
            opt.step()

        def timed_steps(n, xgrad=False):
            ev = events(n + 1)
            ev[0].record()
            for i in range(n):
                step(xgrad)
                ev[i + 1].record()
            torch.cuda.synchronize()
            return [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]

        if args.worker == "plain":
            timed_steps(args.warmup)
            res[precision] = {"plain_ms": timed_steps(args.steps)}
            continue
        # ---- (b): plain step / step with x.requires_grad, alternating blocks in one process
        model.input_gradients = True
        timed_steps(args.warmup)
        timed_steps(args.warmup, True)
        plain, xg = [], []
        for _ in range(4):
            plain += timed_steps(args.steps // 4 + 1)
            xg += timed_steps(args.steps // 4 + 1, True)
        # ---- (c): the backward alone
        model.eval()
        x = torch.randn(BATCH, 4, 32, 32, device=dev, generator=g)
        y = torch.randint(0, 1000, (BATCH,), device=dev, generator=g)
        t = torch.randint(0, 1000, (BATCH,), device=dev)
        dout = torch.randn(BATCH, 8, 32, 32, device=dev, generator=g) / BATCH

        def backward_ms(frozen, xgrad):
            model.requires_grad_(not frozen)
            xx = x.clone().requires_grad_(xgrad)
            out = model(xx, t, y)
            a, b = events(2)
            a.record()
            out.backward(dout)
            b.record()
            torch.cuda.synchronize()
            for p in model.parameters():
                p.grad = None
            return a.elapsed_time(b)

        kinds = {"full": (False, False), "full_dx": (False, True), "input_only": (True, True)}
        for k in kinds.values():
            for _ in range(3):
                backward_ms(*k)
        bw = {k: [] for k in kinds}
        for _ in range(args.steps):
            for k, v in kinds.items():
                bw[k].append(backward_ms(*v))
        res[precision] = {"plain_ms": plain, "xgrad_ms": xg, **{f"bwd_{k}_ms": v for k, v in bw.items()}}
        del model, opt
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(res))


def run_worker(kind, tree, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", kind, "--tree", tree, "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--precisions", args.precisions]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.worker_timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"worker {kind} on {tree} failed with status {r.returncode}: nothing more is started")
    print(f"   worker {kind} on {tree}: done", flush=True)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def med(v):
    return statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precisions", default="bf16,f16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_grad_timing.json"))
    ap.add_argument("--worker", choices=["plain", "extras"], default=None)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--worker-timeout", type=int, default=420)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    doc = {"model": MODEL, "batch": BATCH, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "plain": [], "extras": None}
    if args.parent_tree:
        for r in range(args.rounds):
            for tag, tree in (("parent", args.parent_tree), ("this", ROOT)):
                doc["plain"].append({"round": r, "tree": tag, **run_worker("plain", tree, args)})
    doc["extras"] = run_worker("extras", ROOT, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    for prec in args.precisions.split(","):
        print(f"== {MODEL} @ {BATCH}, {prec}")
        for tag in ("parent", "this"):
            runs = [med(d[prec]["plain_ms"]) for d in doc["plain"] if d["tree"] == tag]
            if runs:
                print(f"   (a) plain step, {tag:6s} tree: median per run {', '.join(f'{v:.3f}' for v in runs)} ms -> {med(runs):.3f} ms")
        e = doc["extras"][prec]
        p, x = med(e["plain_ms"]), med(e["xgrad_ms"])
        print(f"   (b) same process: plain {p:.3f} ms, x.requires_grad {x:.3f} ms ({x - p:+.3f} ms)")
        f_, fd, io = med(e["bwd_full_ms"]), med(e["bwd_full_dx_ms"]), med(e["bwd_input_only_ms"])
        print(f"   (c) backward alone: full {f_:.3f} ms, full + dx {fd:.3f} ms, input-only {io:.3f} ms ({io / f_:.2f} x full)")


if __name__ == "__main__":
    main()
