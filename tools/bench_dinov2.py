"""Device time of the native DINOv2 features (map-dit_amd/dinov2.py) for ViT-L/14 shapes on random weights.

Features: --n uint8 images of --size x --size through ``DinoV2Features.features`` (the antialiased resize to 224 included), both
operand formats, HIP events on the stream after warm-up, the median of --rounds.  The per-kernel split times every kernel of the walk
alone, through the C ABI on buffers of the walk's shapes, and multiplies by the number of its launches: linears (patch embed, qkv,
proj, fc1, fc2), attention, pointwise (prepare, embed, LayerNorm, GELU, residual).  --torch runs the same network as plain
torch.nn.functional fp16 calls on the same GPU (interpolate, layer_norm, linear, scaled_dot_product_attention, gelu) in a child
process under its own time limit; if the child does not finish, that is reported and the native numbers stand alone.

FLOPs per image (2 per multiply-add), T = 1 + (224 / 14)^2 = 257, D = 1024, F = 4096, depth 24:
    patch embed 2 * 256 * 588 * D;  per block  2 T D (3 D) + 2 T D D + 4 T D F  (linears)  +  4 T T D  (QK^T and PV)
    = 0.308 + 24 * (6.468 + 0.271) = 162.0 GFLOP.

    python tools/bench_dinov2.py [--n 64] [--size 256] [--rounds 3] [--torch] [--torch-timeout 300] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DIM, DEPTH, MLP, HEADS, SIZE, T = 1024, 24, 4096, 16, 224, 257
FLOPS_PER_IMAGE = 2 * 256 * 588 * DIM + DEPTH * (2 * T * DIM * 3 * DIM + 2 * T * DIM * DIM + 4 * T * DIM * MLP + 4 * T * T * DIM)


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


def images(n, size):
    return torch.randint(0, 256, (n, size, size, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).cuda()


def torch_features_fp16(w, pos, img):
    """The network as plain torch.nn.functional calls on fp16 tensors: img uint8 [N, H, W, 3] -> [N, D]."""
    x = F.interpolate(img.permute(0, 3, 1, 2).float(), size=(SIZE, SIZE), mode="bicubic", antialias=True, align_corners=False) / 255.0
    x = ((x - x.new_tensor([0.485, 0.456, 0.406])[None, :, None, None]) / x.new_tensor([0.229, 0.224, 0.225])[None, :, None, None]).half()
    N, g = x.shape[0], SIZE // 14
    x = x.reshape(N, 3, g, 14, g, 14).permute(0, 2, 4, 1, 3, 5).reshape(N, g * g, 588)
    x = F.linear(x, w["patch_embed.proj.weight"].reshape(DIM, 588), w["patch_embed.proj.bias"])
    x = torch.cat([w["cls_token"].expand(N, 1, DIM), x], dim=1) + pos
    for i in range(DEPTH):
        p = f"blocks.{i}."
        h = F.layer_norm(x, (DIM,), w[p + "norm1.weight"], w[p + "norm1.bias"], 1e-6)
        q, k, v = F.linear(h, w[p + "attn.qkv.weight"], w[p + "attn.qkv.bias"]).reshape(N, T, 3, HEADS, 64).permute(2, 0, 3, 1, 4)
        a = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(N, T, DIM)
        x = x + w[p + "ls1.gamma"] * F.linear(a, w[p + "attn.proj.weight"], w[p + "attn.proj.bias"])
        h = F.layer_norm(x, (DIM,), w[p + "norm2.weight"], w[p + "norm2.bias"], 1e-6)
        h = F.linear(F.gelu(F.linear(h, w[p + "mlp.fc1.weight"], w[p + "mlp.fc1.bias"])), w[p + "mlp.fc2.weight"], w[p + "mlp.fc2.bias"])
        x = x + w[p + "ls2.gamma"] * h
    return F.layer_norm(x[:, 0], (DIM,), w["norm.weight"], w["norm.bias"], 1e-6).float()


def torch_child(args):
    import dinov2_reference as R
    import mapdit_amd.dinov2 as D
    sd = R.make_state_dict(DIM, DEPTH, MLP, seed=3)
    w = {k: v.half().cuda() for k, v in sd.items()}
    pos = D.interpolate_pos_embed(sd["pos_embed"], SIZE // 14).half().cuda()[None]
    img = images(args.n, args.size)
    with torch.no_grad():
        ms = [time_events(lambda: torch_features_fp16(w, pos, img), 2, 3) for _ in range(args.rounds)]
    print(json.dumps({"torch_fp16_ms": statistics.median(ms), "torch_fp16_ms_all": ms}))


def kernel_split(n, size, prec, rounds):
    """ms per features call spent in each kernel family: one launch of every distinct shape timed alone, times its count."""
    import mapdit_amd._lib as L
    lib = L.lib()
    fn = lambda name: getattr(lib, name + ("_f16" if prec == "f16" else ""))       # noqa: E731
    dt = torch.float16 if prec == "f16" else torch.bfloat16
    M, st = n * T, L.cur_stream()
    z16 = lambda *s: (0.1 * torch.randn(*s, device="cuda")).to(dt)                 # noqa: E731
    img = images(n, size)
    rows, x, y = z16(n * 256, L.VIT_PATCH_K), torch.randn(M, DIM, device="cuda"), torch.randn(M, DIM, device="cuda")
    h, qkv, f = z16(M, DIM), z16(M, 3 * DIM), z16(M, MLP)
    wp, wq, wo, w1, w2 = z16(DIM, L.VIT_PATCH_K), z16(3 * DIM, DIM), z16(DIM, DIM), z16(MLP, DIM), z16(DIM, MLP)
    bias, g, pos = torch.zeros(MLP, device="cuda"), torch.ones(DIM, device="cuda"), torch.zeros(T, DIM, device="cuda")
    K16, K32 = L.VIT_OUT_16, L.VIT_OUT_F32
    P = lambda t: t.data_ptr()                                                     # noqa: E731

    def ms(call):
        return statistics.median(time_events(call, 2, 5) for _ in range(rounds))
    lin = {"patch": (1, lambda: fn("vit_linear")(P(rows), P(wp), P(bias), P(y), K32, n * 256, L.VIT_PATCH_K, DIM, st)),
           "qkv": (DEPTH, lambda: fn("vit_linear")(P(h), P(wq), P(bias), P(qkv), K16, M, DIM, 3 * DIM, st)),
           "proj": (DEPTH, lambda: fn("vit_linear")(P(h), P(wo), P(bias), P(y), K32, M, DIM, DIM, st)),
           "fc1": (DEPTH, lambda: fn("vit_linear")(P(h), P(w1), P(bias), P(f), K16, M, DIM, MLP, st)),
           "fc2": (DEPTH, lambda: fn("vit_linear")(P(f), P(w2), P(bias), P(y), K32, M, MLP, DIM, st))}
    pw = {"prepare": (1, lambda: fn("vit_prepare")(P(img), L.VIT_IMG_U8_NHWC, P(rows), n, size, size, SIZE, st)),
          "embed": (1, lambda: lib.vit_embed(P(y), P(g), P(pos), P(x), n, T, DIM, st)),
          "layernorm": (2 * DEPTH, lambda: fn("vit_layernorm")(P(x), DIM, P(g), P(bias), 1e-6, P(h), K16, M, DIM, st)),
          "gelu": (DEPTH, lambda: fn("vit_gelu")(P(f), P(f), M * MLP, st)),
          "residual": (2 * DEPTH, lambda: fn("vit_residual")(P(x), P(y), K32, P(bias), M, DIM, st))}
    out = {"linears": {k: c * ms(call) for k, (c, call) in lin.items()},
           "attention": DEPTH * ms(lambda: fn("vit_attention")(P(qkv), P(h), n, T, HEADS, 64, st)),
           "pointwise": {k: c * ms(call) for k, (c, call) in pw.items()}}
    out["linears_ms"], out["pointwise_ms"] = sum(out["linears"].values()), sum(out["pointwise"].values())
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=64)
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--torch", action="store_true")
    p.add_argument("--torch-timeout", type=int, default=300)
    p.add_argument("--torch-child", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("--out", type=str, default=None)
    args = p.parse_args()
    if args.torch_child:
        return torch_child(args)

    import dinov2_reference as R
    import mapdit_amd.dinov2 as D
    res = {"n": args.n, "size": args.size, "device": torch.cuda.get_device_name(0), "gflop_per_image": FLOPS_PER_IMAGE / 1e9}
    sd = R.make_state_dict(DIM, DEPTH, MLP, seed=3)
    img = images(args.n, args.size)
    for prec in ("f16", "bf16"):
        net = D.DinoV2Features.from_state_dict(sd, "cuda", precision=prec, max_batch=args.n)
        ms = [time_events(lambda: net.features(img), 1, 2) for _ in range(args.rounds)]
        m = statistics.median(ms)
        res[prec] = {"ms": m, "ms_all": ms, "images_per_s": 1e3 * args.n / m, "tflops": FLOPS_PER_IMAGE * args.n / m / 1e9}
        print(f"features {prec}: {m:.2f} ms for {args.n} images of {args.size} x {args.size} = {res[prec]['images_per_s']:.0f} images/s "
              f"({res[prec]['tflops']:.1f} TFLOP/s at {FLOPS_PER_IMAGE / 1e9:.1f} GFLOP per image)", flush=True)
        del net
    res["split_f16"] = kernel_split(args.n, args.size, "f16", args.rounds)
    s = res["split_f16"]
    print(f"split f16 (ms per call): linears {s['linears_ms']:.2f}, attention {s['attention']:.2f}, pointwise {s['pointwise_ms']:.2f}", flush=True)

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
