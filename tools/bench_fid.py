"""Device time of the native FID pieces (map-dit_amd/fid.py) on random weights.

Feature extraction: images per second for --n uint8 images of --size x --size, both operand formats (HIP events on the stream, after
warm-up; the resize to 299 x 299 is part of it).  --torch runs the same network as plain torch.nn.functional fp16 calls on the same
GPU (folded weights, NCHW, what pytorch-fid would execute in half precision) in a child process under its own time limit: MIOpen's
first-run kernel search can be slow; if the child does not finish, that is reported and the native numbers stand alone.
Statistics: the time of a --samples-sample pass of mapdit_inc_stats_accumulate in batches of --n, and of the host Fréchet solve at
D = 2048.

    python tools/bench_fid.py [--n 64] [--size 256] [--rounds 3] [--samples 10000] [--torch] [--torch-timeout 300] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

GMACS_PER_IMAGE = 5.73          # Inception-v3 at 299 x 299, the published count (the classifier head is 0.002 of it)


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


def torch_features_fp16(units, weights, x):
    """The network as plain torch.nn.functional calls on fp16 tensors: x [N, 3, 299, 299] -> [N, 2048].  units: fid.conv_units();
    weights: name -> (w, b) folded, fp16 on the device."""
    it = iter(units)

    def u(t):
        name, _, _, _, stride, pad = next(it)
        w, b = weights[name]
        return F.relu(F.conv2d(t, w, b, stride, pad))
    avg = lambda t: F.avg_pool2d(t, 3, 1, 1, count_include_pad=False)  # noqa: E731
    x = u(u(u(x)))
    x = F.max_pool2d(x, 3, 2)
    x = u(u(x))
    x = F.max_pool2d(x, 3, 2)
    for _ in range(3):                                                 # Mixed_5b / 5c / 5d
        x = torch.cat([u(x), u(u(x)), u(u(u(x))), u(avg(x))], 1)
    x = torch.cat([u(x), u(u(u(x))), F.max_pool2d(x, 3, 2)], 1)       # Mixed_6a
    for _ in range(4):                                                 # Mixed_6b .. 6e
        x = torch.cat([u(x), u(u(u(x))), u(u(u(u(u(x))))), u(avg(x))], 1)
    x = torch.cat([u(u(x)), u(u(u(u(x)))), F.max_pool2d(x, 3, 2)], 1)  # Mixed_7a
    for pool in (avg, lambda t: F.max_pool2d(t, 3, 1, 1)):             # Mixed_7b / 7c
        b1 = u(x)
        b3 = u(x)
        b3 = torch.cat([u(b3), u(b3)], 1)
        bd = u(u(x))
        bd = torch.cat([u(bd), u(bd)], 1)
        x = torch.cat([b1, b3, bd, u(pool(x))], 1)
    assert next(it, None) is None
    return x.float().mean(dim=(2, 3))


def torch_child(args):
    import inception_reference as R
    import mapdit_amd.fid as FID
    folded = FID.fold_state_dict(R.init_state_dict(seed=3))
    weights = {k: (w.half().cuda(), b.half().cuda()) for k, (w, b) in folded.items()}
    units = FID.conv_units()
    img = torch.randint(0, 256, (args.n, args.size, args.size, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).cuda()

    def run():
        x = F.interpolate(img.permute(0, 3, 1, 2).float(), size=(299, 299), mode="bilinear", align_corners=False) / 255.0 * 2.0 - 1.0
        return torch_features_fp16(units, weights, x.half())
    with torch.no_grad():
        ms = [time_events(run, 2, 3) for _ in range(args.rounds)]
    print(json.dumps({"torch_fp16_ms": statistics.median(ms), "torch_fp16_ms_all": ms}))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=64)
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--samples", type=int, default=10_000)
    p.add_argument("--torch", action="store_true")
    p.add_argument("--torch-timeout", type=int, default=300)
    p.add_argument("--torch-child", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("--out", type=str, default=None)
    args = p.parse_args()
    if args.torch_child:
        return torch_child(args)

    import inception_reference as R
    import mapdit_amd.fid as FID
    res = {"n": args.n, "size": args.size, "device": torch.cuda.get_device_name(0)}
    sd = R.init_state_dict(seed=3)
    img = torch.randint(0, 256, (args.n, args.size, args.size, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).cuda()
    for prec in ("f16", "bf16"):
        net = FID.InceptionFeatures.from_state_dict(sd, "cuda", precision=prec, max_batch=args.n)
        ms = [time_events(lambda: net.features(img), 2, 3) for _ in range(args.rounds)]
        m = statistics.median(ms)
        res[prec] = {"ms": m, "ms_all": ms, "images_per_s": 1e3 * args.n / m, "tflops": 2 * GMACS_PER_IMAGE * args.n / m}
        print(f"features {prec}: {m:.2f} ms for {args.n} images of {args.size} x {args.size} = {res[prec]['images_per_s']:.0f} images/s "
              f"({res[prec]['tflops']:.1f} TFLOP/s at {GMACS_PER_IMAGE} GMACs per image)", flush=True)
        del net

    feat = torch.rand(args.samples, 2048, device="cuda")
    def stats_pass():
        st = FID.FeatureStats(2048, "cuda")
        for i in range(0, args.samples, args.n):
            st.update(feat[i:i + args.n])
        return st
    ms = [time_events(stats_pass, 1, 1) for _ in range(args.rounds)]
    res["stats_pass_ms"] = statistics.median(ms)
    print(f"statistics: {res['stats_pass_ms']:.1f} ms for {args.samples} samples in batches of {args.n}", flush=True)
    mu1, s1 = stats_pass().mean_cov()
    mu2, s2 = FID.FeatureStats(2048, "cuda").update(feat[: args.samples // 2] * 1.1).mean_cov()
    t = time.perf_counter()
    d = FID.frechet_distance(mu1, s1, mu2, s2)
    res["frechet_host_s"] = time.perf_counter() - t
    print(f"frechet_distance at D = 2048 on the host: {res['frechet_host_s']:.2f} s (value {d:.4f}, {os.cpu_count()} CPUs visible, "
          f"{torch.get_num_threads()} torch threads)", flush=True)

    if args.torch:
        cmd = [sys.executable, os.path.abspath(__file__), "--torch-child", "--n", str(args.n), "--size", str(args.size), "--rounds", str(args.rounds)]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.torch_timeout)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
            if out.returncode == 0 and line:
                res.update(json.loads(line[-1]))
                res["native_f16_over_torch_fp16"] = res["torch_fp16_ms"] / res["f16"]["ms"]
                print(f"torch.nn.functional fp16: {res['torch_fp16_ms']:.2f} ms = {1e3 * args.n / res['torch_fp16_ms']:.0f} images/s; "
                      f"native f16 is {res['native_f16_over_torch_fp16']:.2f} x its speed")
            else:
                res["torch_fp16_error"] = (out.stderr or out.stdout)[-400:]
                print("torch child failed:", res["torch_fp16_error"])
        except subprocess.TimeoutExpired:
            res["torch_fp16_error"] = f"no result within {args.torch_timeout} s"
            print("torch child:", res["torch_fp16_error"])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
