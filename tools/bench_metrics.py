"""Device time of the metrics beside the FID (map-dit_amd/metrics.py on csrc/manifold.hip) against the same arithmetic as plain torch
fp32 calls on the same GPU.

precision_recall at --sizes REALxFAKE (default 10000x10000 and 50000x10000) with D = --dim features drawn like the test fixture
(relu of eight Gaussian clusters), and kid at its defaults (100 subsets of 1000) on the first pair.  The torch side is what a user
without the library would write: squared row norms, ``x @ y.T`` in row blocks of --block, ``topk`` for the radii, comparisons and
sums for the counts; for KID a gather and three 1000 x 1000 products per subset, the polynomial and the sums in fp64.  HIP events on
the stream after --warmup calls, --rounds timed calls each, the median reported; TFLOP/s counts the Gram products only (2 N M D per
pass: two radius passes and three count passes for precision / recall, three products per KID subset).

inception_score at --isc-samples x 1008 x --dim (two Gram passes: 4 N C D flop) against ``softmax(x @ W.T)`` in row blocks of --block
with fp64 sums, and the feature network on --tap-images images of 64 x 64 (random weights: the time does not depend on them) with and
without the spatial tap of sFID.  --cases picks among pr, kid, isc, tap.

    python tools/bench_metrics.py [--cases pr,kid,isc,tap] [--sizes 10000x10000,50000x10000] [--dim 2048] [--rounds 3] [--warmup 1]
                                  [--block 4096] [--isc-samples 50000] [--tap-images 64] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def time_events(fn, warmup, rounds):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def features(n, dim, seed, spread):
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.randn(8, dim, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    which = torch.randint(0, 8, (n,), device="cuda", generator=g)
    return torch.relu(0.5 * centres[which] + spread * torch.randn(n, dim, device="cuda", generator=g)).contiguous()


# ---- the same arithmetic as plain torch calls ----------------------------------------------------------------------------------------
def _blocks(q, r, nq, nr, block):
    for i in range(0, q.shape[0], block):
        yield i, torch.clamp_min(nq[i:i + block, None] + nr[None, :] - 2.0 * (q[i:i + block] @ r.T), 0.0)


def torch_radii(x, k, block):
    n, out = (x.double() ** 2).sum(1).float(), []
    for i, d in _blocks(x, x, n, n, block):
        rows = torch.arange(d.shape[0], device=x.device)
        d[rows, i + rows] = float("inf")
        out.append(d.topk(k, dim=1, largest=False).values[:, k - 1])
    return torch.cat(out)


def torch_count(q, r, rad, mode, block):
    nq, nr = (q.double() ** 2).sum(1).float(), (r.double() ** 2).sum(1).float()
    return torch.cat([(d <= (rad[None, :] if mode == "ref" else rad[i:i + d.shape[0], None])).sum(1) for i, d in _blocks(q, r, nq, nr, block)])


def torch_precision_recall(real, fake, k, block):
    r_real, r_fake = torch_radii(real, k, block), torch_radii(fake, k, block)
    in_real, in_fake = torch_count(fake, real, r_real, "ref", block), torch_count(real, fake, r_fake, "ref", block)
    covered = torch_count(real, fake, r_real, "query", block)
    return {"precision": int((in_real > 0).sum()) / len(fake), "recall": int((in_fake > 0).sum()) / len(real),
            "density": int(in_real.sum()) / (k * len(fake)), "coverage": int((covered > 0).sum()) / len(real)}


def torch_kid(real, fake, subsets, m, seed):
    import numpy as np
    import mapdit_amd.metrics as M
    D, est = real.shape[1], []
    sums = []
    for ir, jf in M.kid_subsets(len(real), len(fake), subsets, m, seed):
        x, y = real[torch.from_numpy(ir).cuda()], fake[torch.from_numpy(jf).cuda()]
        kxx, kyy, kxy = (((a @ b.T).double() / D + 1.0) ** 3 for a, b in ((x, x), (y, y), (x, y)))
        sums.append(torch.stack([kxx.sum() - kxx.diagonal().sum(), kyy.sum() - kyy.diagonal().sum(), kxy.sum()]))
    for row in torch.stack(sums).cpu().numpy():
        est.append(M.mmd2_unbiased(*row, m))
    return float(np.mean(est)), float(np.std(est))


def torch_inception_score(x, w, split, block):
    import numpy as np
    import mapdit_amd.metrics as M
    scores = []
    for i in range(0, len(x), split):
        part = x[i:i + split]
        ent, marg = torch.zeros((), dtype=torch.float64, device=x.device), torch.zeros(len(w), dtype=torch.float64, device=x.device)
        for j in range(0, len(part), block):
            logp = torch.log_softmax(part[j:j + block] @ w.T, dim=1)
            prob = logp.exp()
            ent += (prob * logp).double().sum()
            marg += prob.double().sum(0)
        scores.append(M.inception_score_from_sums(float(ent), marg.cpu().numpy(), len(part)))
    return float(np.mean(scores)), float(np.std(scores))


def random_inception(device, precision="f16"):
    """The feature network on He-scaled random weights (folded form: no BatchNorm to fold)."""
    import math
    from mapdit_amd import fid as FID
    g = torch.Generator().manual_seed(0)
    folded = {name: (torch.randn(cout, cin, kh, kw, generator=g, dtype=torch.float64) * math.sqrt(2.0 / (cin * kh * kw)),
                     torch.full((cout,), 0.05, dtype=torch.float64)) for name, cin, cout, (kh, kw), _, _ in FID.conv_units()}
    return FID.InceptionFeatures(folded, device, precision, max_batch=64)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--cases", default="pr,kid,isc,tap")
    p.add_argument("--isc-samples", type=int, default=50000)
    p.add_argument("--isc-split", type=int, default=5000)
    p.add_argument("--tap-images", type=int, default=64)
    p.add_argument("--sizes", default="10000x10000,50000x10000", help="REALxFAKE pairs")
    p.add_argument("--dim", type=int, default=2048)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--block", type=int, default=4096)
    p.add_argument("--kid-subsets", type=int, default=100)
    p.add_argument("--kid-subset-size", type=int, default=1000)
    p.add_argument("--no-torch", action="store_true")
    p.add_argument("--out", type=str, default=None)
    args = p.parse_args()
    import mapdit_amd.metrics as M
    torch.backends.cuda.matmul.allow_tf32 = False                         # the comparison is fp32 arithmetic
    D = args.dim
    res = {"device": torch.cuda.get_device_name(0), "dim": D, "rounds": args.rounds, "warmup": args.warmup, "pr": [], "kid": None}
    cases = [c.strip() for c in args.cases.split(",") if c.strip()]
    if "isc" in cases:
        n, C = args.isc_samples, 1008
        g = torch.Generator(device="cuda").manual_seed(3)
        x = (torch.randn(n, D, device="cuda", generator=g).abs() * 0.4).contiguous()
        w = (torch.randn(C, D, device="cuda", generator=g) * 0.03).contiguous()
        tflop = 4.0 * n * C * D / 1e12
        ms, all_ms = time_events(lambda: M.inception_score(x, w, None, args.isc_split), args.warmup, args.rounds)
        row = {"samples": n, "classes": C, "split_size": args.isc_split, "tflop": tflop, "native_ms": ms, "native_ms_all": all_ms,
               "native_tflops": tflop / ms * 1e3, "native": M.inception_score(x, w, None, args.isc_split)}
        print(f"inception_score {n} x {C} x {D}: native {ms:.1f} ms = {row['native_tflops']:.1f} TFLOP/s {row['native']}", flush=True)
        if not args.no_torch:
            tms, tall = time_events(lambda: torch_inception_score(x, w, args.isc_split, args.block), args.warmup, args.rounds)
            row.update(torch_ms=tms, torch_ms_all=tall, torch_tflops=tflop / 2 / tms * 1e3, torch=torch_inception_score(x, w, args.isc_split, args.block),
                       torch_over_native=tms / ms)
            print(f"    torch fp32 in blocks of {args.block} (one product, not two): {tms:.1f} ms {row['torch']}; native is "
                  f"{row['torch_over_native']:.2f} x its speed", flush=True)
        res["isc"] = row
        del x, w
    if "tap" in cases:
        net = random_inception("cuda")
        img = torch.randint(0, 256, (args.tap_images, 64, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4)).cuda()
        ms0, all0 = time_events(lambda: net.features(img), args.warmup, args.rounds)
        ms1, all1 = time_events(lambda: net.features(img, spatial=True), args.warmup, args.rounds)
        res["tap"] = {"images": args.tap_images, "features_ms": ms0, "features_ms_all": all0, "features_tap_ms": ms1, "features_tap_ms_all": all1,
                      "tap_over_plain": ms1 / ms0}
        print(f"feature pass, {args.tap_images} images: {ms0:.2f} ms without the tap, {ms1:.2f} ms with it ({ms1 / ms0:.4f} x)", flush=True)
        del net, img
    first = None
    for pair in (args.sizes.split(",") if "pr" in cases or "kid" in cases else []):
        nr, nf = (int(v) for v in pair.lower().split("x"))
        real, fake = features(nr, D, 1, 0.55), features(nf, D, 2, 0.5)
        first = first or (real, fake)
        if "pr" not in cases:
            break
        tflop = 2.0 * D * (nr * nr + nf * nf + 3.0 * nr * nf) / 1e12
        ms, all_ms = time_events(lambda: M.precision_recall(real, fake, 3), args.warmup, args.rounds)
        row = {"real": nr, "fake": nf, "tflop": tflop, "native_ms": ms, "native_ms_all": all_ms, "native_tflops": tflop / ms * 1e3,
               "native": M.precision_recall(real, fake, 3)}
        print(f"precision_recall {nr} x {nf}, D = {D}: native {ms:.1f} ms = {row['native_tflops']:.1f} TFLOP/s {row['native']}", flush=True)
        if not args.no_torch:
            tms, tall = time_events(lambda: torch_precision_recall(real, fake, 3, args.block), args.warmup, args.rounds)
            row.update(torch_ms=tms, torch_ms_all=tall, torch_tflops=tflop / tms * 1e3, torch=torch_precision_recall(real, fake, 3, args.block),
                       torch_over_native=tms / ms)
            print(f"    torch fp32 in blocks of {args.block}: {tms:.1f} ms = {row['torch_tflops']:.1f} TFLOP/s {row['torch']}; "
                  f"native is {row['torch_over_native']:.2f} x its speed", flush=True)
        res["pr"].append(row)
        del real, fake
    real, fake = first or (torch.empty(0, D), torch.empty(0, D))
    m, s = args.kid_subset_size, args.kid_subsets
    if "kid" in cases and m <= min(len(real), len(fake)):
        tflop = 2.0 * D * 3 * m * m * s / 1e12
        ms, all_ms = time_events(lambda: M.kid(real, fake, s, m), args.warmup, args.rounds)
        res["kid"] = {"subsets": s, "subset_size": m, "tflop": tflop, "native_ms": ms, "native_ms_all": all_ms, "native_tflops": tflop / ms * 1e3,
                      "native": M.kid(real, fake, s, m)}
        print(f"kid {s} x {m}: native {ms:.1f} ms = {res['kid']['native_tflops']:.1f} TFLOP/s {res['kid']['native']}", flush=True)
        if not args.no_torch:
            tms, tall = time_events(lambda: torch_kid(real, fake, s, m, 0), args.warmup, args.rounds)
            res["kid"].update(torch_ms=tms, torch_ms_all=tall, torch_tflops=tflop / tms * 1e3, torch=torch_kid(real, fake, s, m, 0),
                              torch_over_native=tms / ms)
            print(f"    torch fp32: {tms:.1f} ms = {res['kid']['torch_tflops']:.1f} TFLOP/s {res['kid']['torch']}; "
                  f"native is {res['kid']['torch_over_native']:.2f} x its speed", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
