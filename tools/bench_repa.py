"""Device time of REPA (map-dit_amd/repa.py, train.py --repa-features) on DiT-B/2, bf16, 256 samples:

 * the training step - forward, loss, backward, optimiser step(s) - with and without the alignment term (synthetic:768 features, the
   projector at its default width 2048, the tap after 4 blocks), the same loop in both cases;
 * the head's own forward and backward on a [256 x 256, 768] hidden state;
 * the rate of ``dinov2 tokens`` at ViT-B/14 shapes (random weights), grid 16: images per second through ``DinoV2Features.tokens``.

HIP events on the stream after warm-up, the median of --rounds.  By arithmetic the head adds 6 M (D H + H H + H P) = 6 x 65,536 x
(768 x 2048 + 2048^2 + 2048 x 768) = 2.9 TFLOP to the step's 35.

    python tools/bench_repa.py [--samples 256] [--steps 5] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def time_events(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters                                   # ms per call


def step_time(n, steps, rounds, repa, prec="bf16", feat_dim=768, hidden=2048):
    from mapdit_amd.diffusion import create_diffusion
    from mapdit_amd.optim import FusedAdamEMA
    from mapdit_amd.repa import RepaHead
    from mapdit_amd.src.models import DIT_MODELS
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = DIT_MODELS["DiT-B/2"](in_channels=4, input_size=32, num_classes=1000).to(dev).train()
    model.gemm_precision = prec
    opt = FusedAdamEMA(model, lr=1e-4)
    diffusion = create_diffusion(timestep_respacing="")
    head = head_opt = feats = None
    if repa:
        model.hidden_tap = 3
        head = RepaHead(model.hidden_size, feat_dim, hidden=hidden, precision=prec).to(dev)
        head_opt = FusedAdamEMA(head, lr=1e-4, ema_stds=())
        feats = torch.randn(n, 256, feat_dim, device=dev).half()
    x, y = torch.randn(n, 4, 32, 32, device=dev), torch.randint(0, 1000, (n,), device=dev)

    def step():
        t = torch.randint(0, diffusion.num_timesteps, (n,), device=dev)
        loss = diffusion.training_losses(model, x, t, dict(y=y))["loss"].mean()
        if head is not None:
            loss = loss + 0.5 * head.loss(model.tapped_hidden, feats).mean()
            head_opt.zero_grad()
        opt.zero_grad()
        loss.backward()
        opt.step()
        if head_opt is not None:
            head_opt.step()
    ms = [time_events(step, 2 if r == 0 else 0, steps) for r in range(rounds)]
    return statistics.median(ms), ms


def head_time(n, rounds, prec="bf16", dim=768, feat_dim=768, hidden=2048):
    from mapdit_amd.repa import RepaHead
    dev = torch.device("cuda", 0)
    head = RepaHead(dim, feat_dim, hidden=hidden, precision=prec).to(dev)
    hid, feats = torch.randn(n, 256, dim, device=dev), torch.randn(n, 256, feat_dim, device=dev).half()
    g = torch.full((n,), 0.5 / n, device=dev)
    saved = head._forward(hid, feats)
    fwd = statistics.median(time_events(lambda: head._forward(hid, feats), 1, 3) for _ in range(rounds))
    bwd = statistics.median(time_events(lambda: head._backward(saved, g, True), 1, 3) for _ in range(rounds))
    return fwd, bwd


def tokens_rate(n, rounds, prec="f16"):
    import dinov2_reference as R
    import mapdit_amd.dinov2 as D
    sd = R.make_state_dict(768, 12, 3072, seed=3)
    net = D.DinoV2Features.from_state_dict(sd, "cuda", precision=prec, max_batch=n, image_size=224)
    img = torch.randint(0, 256, (n, 256, 256, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).cuda()
    ms = statistics.median(time_events(lambda: net.tokens(img, out16=True), 1, 2) for _ in range(rounds))
    return ms, 1e3 * n / ms


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--samples", type=int, default=256)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--tokens-images", type=int, default=64)
    p.add_argument("--out", type=str, default=None)
    args = p.parse_args()
    n = args.samples
    res = {"samples": n, "device": torch.cuda.get_device_name(0), "head_tflop": 6 * n * 256 * (768 * 2048 + 2048 * 2048 + 2048 * 768) / 1e12}
    base, base_all = step_time(n, args.steps, args.rounds, repa=False)
    print(f"step without --repa-features: {base:.2f} ms {['%.2f' % v for v in base_all]}", flush=True)
    with_, with_all = step_time(n, args.steps, args.rounds, repa=True)
    print(f"step with synthetic:768:      {with_:.2f} ms {['%.2f' % v for v in with_all]}  (+{100 * (with_ / base - 1):.1f} %)", flush=True)
    fwd, bwd = head_time(n, args.rounds)
    print(f"head alone: forward {fwd:.2f} ms, backward {bwd:.2f} ms ({res['head_tflop']:.2f} TFLOP: {res['head_tflop'] / (fwd + bwd) * 1e3:.0f} TFLOP/s)", flush=True)
    tms, rate = tokens_rate(args.tokens_images, args.rounds)
    print(f"dinov2 tokens, ViT-B/14, grid 16, f16: {tms:.2f} ms for {args.tokens_images} images = {rate:.0f} images/s", flush=True)
    res.update(step_ms=base, step_ms_all=base_all, step_repa_ms=with_, step_repa_ms_all=with_all, overhead=with_ / base - 1, head_fwd_ms=fwd,
               head_bwd_ms=bwd, tokens_ms=tms, tokens_images=args.tokens_images, tokens_images_per_s=rate)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
