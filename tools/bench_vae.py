"""Device time of the native VAE decoder (mapdit_vae_decode) on random weights of the default config.

For N latents of each --latents size and both operand formats: device time per image (HIP events on the stream, after warm-up),
the achieved TFLOP/s from a FLOP count computed here from the config, and the two heaviest layers on their own (3 x 3 convolutions
512 -> 512 at 64 x 64 and 128 -> 128 at 256 x 256, N images each).  --torch runs the same network as plain torch.nn.functional calls in
fp16 on the same GPU (what the diffusers package would execute) in a child process under its own time limit: MIOpen's first-run kernel
search can be slow; if the child does not finish, that is reported and the native numbers stand alone.

    python tools/bench_vae.py [--n 16] [--latents 32,16] [--rounds 3] [--torch] [--torch-timeout 300] [--out FILE]

--encode measures the encoder (mapdit_vae_encode) instead: device time per image for N images of each --images size (128, 256), both
operand formats, from a fp32 NCHW batch and from uint8 through mapdit_vae_prepare_u8, with the FLOP count of the encoder; --torch then
runs the encoder as plain torch.nn.functional fp16 calls in the child process.

    python tools/bench_vae.py --encode [--n 16] [--images 128,256] [--rounds 3] [--torch] [--out FILE]
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

DEFAULT = dict(block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=4, out_channels=3)


def decoder_flops(cfg, h, w):
    """FLOPs (2 per multiply-add) of one decode of an h x w latent: every conv / linear and the two attention products."""
    ch = list(reversed(cfg["block_out_channels"]))
    lat, px, c0 = cfg["latent_channels"], h * w, ch[0]
    macs = px * lat * lat + px * 9 * lat * c0
    res = lambda p, ci, co: p * 9 * ci * co + p * 9 * co * co + (p * ci * co if ci != co else 0)  # noqa: E731
    macs += 2 * res(px, c0, c0)
    macs += 4 * px * c0 * c0 + 2 * px * px * c0                        # q, k, v, out; q k^T and p v
    cin = c0
    for i, c in enumerate(ch):
        for _ in range(cfg["layers_per_block"] + 1):
            macs += res(px, cin, c)
            cin = c
        if i < len(ch) - 1:
            px *= 4
            macs += px * 9 * c * c
    macs += px * 9 * cin * cfg["out_channels"]
    return 2 * macs


def encoder_flops(cfg, H, W):
    """FLOPs (2 per multiply-add) of one encode of an H x W image: every conv / linear and the two attention products."""
    ch = list(cfg["block_out_channels"])
    px, lat2 = H * W, 2 * cfg["latent_channels"]
    res = lambda p, ci, co: p * 9 * ci * co + p * 9 * co * co + (p * ci * co if ci != co else 0)  # noqa: E731
    macs = px * 9 * cfg["out_channels"] * ch[0]
    cin = ch[0]
    for i, c in enumerate(ch):
        for _ in range(cfg["layers_per_block"]):
            macs += res(px, cin, c)
            cin = c
        if i < len(ch) - 1:
            px //= 4
            macs += px * 9 * c * c
    macs += 2 * res(px, cin, cin) + 4 * px * cin * cin + 2 * px * px * cin
    macs += px * 9 * cin * lat2 + px * lat2 * lat2
    return 2 * macs


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


def torch_decode_fp16(sd, z, cfg, groups=32):
    """The same network as plain torch.nn.functional calls on fp16 tensors (NCHW, like the diffusers modules)."""
    A = "decoder.mid_block.attentions.0."
    conv = lambda x, n, p: F.conv2d(x, sd[n + ".weight"], sd[n + ".bias"], padding=p)  # noqa: E731
    gn = lambda x, n: F.group_norm(x, groups, sd[n + ".weight"], sd[n + ".bias"], 1e-6)  # noqa: E731

    def resnet(x, p):
        h = conv(F.silu(gn(x, p + ".norm1")), p + ".conv1", 1)
        h = conv(F.silu(gn(h, p + ".norm2")), p + ".conv2", 1)
        return (conv(x, p + ".conv_shortcut", 0) if p + ".conv_shortcut.weight" in sd else x) + h
    x = conv(conv(z, "post_quant_conv", 0), "decoder.conv_in", 1)
    x = resnet(x, "decoder.mid_block.resnets.0")
    n, c, hh, ww = x.shape
    t = gn(x, A + "group_norm").reshape(n, c, hh * ww).transpose(1, 2)
    q, k, v = (F.linear(t, sd[A + f"{m}.weight"], sd[A + f"{m}.bias"]) for m in ("to_q", "to_k", "to_v"))
    o = F.scaled_dot_product_attention(q[:, None], k[:, None], v[:, None])[:, 0]
    x = x + F.linear(o, sd[A + "to_out.0.weight"], sd[A + "to_out.0.bias"]).transpose(1, 2).reshape(n, c, hh, ww)
    x = resnet(x, "decoder.mid_block.resnets.1")
    nb = len(cfg["block_out_channels"])
    for i in range(nb):
        for j in range(cfg["layers_per_block"] + 1):
            x = resnet(x, f"decoder.up_blocks.{i}.resnets.{j}")
        if i < nb - 1:
            x = conv(F.interpolate(x, scale_factor=2.0, mode="nearest"), f"decoder.up_blocks.{i}.upsamplers.0.conv", 1)
    return conv(F.silu(gn(x, "decoder.conv_norm_out")), "decoder.conv_out", 1)


def torch_encode_fp16(sd, x, cfg, groups=32):
    """The encoder as plain torch.nn.functional calls on fp16 tensors (NCHW, like the diffusers modules); returns the moments."""
    A = "encoder.mid_block.attentions.0."
    conv = lambda t, n, p: F.conv2d(t, sd[n + ".weight"], sd[n + ".bias"], padding=p)  # noqa: E731
    gn = lambda t, n: F.group_norm(t, groups, sd[n + ".weight"], sd[n + ".bias"], 1e-6)  # noqa: E731

    def resnet(t, p):
        h = conv(F.silu(gn(t, p + ".norm1")), p + ".conv1", 1)
        h = conv(F.silu(gn(h, p + ".norm2")), p + ".conv2", 1)
        return (conv(t, p + ".conv_shortcut", 0) if p + ".conv_shortcut.weight" in sd else t) + h
    t = conv(x, "encoder.conv_in", 1)
    nb = len(cfg["block_out_channels"])
    for i in range(nb):
        for j in range(cfg["layers_per_block"]):
            t = resnet(t, f"encoder.down_blocks.{i}.resnets.{j}")
        if i < nb - 1:
            d = f"encoder.down_blocks.{i}.downsamplers.0.conv"
            t = F.conv2d(F.pad(t, (0, 1, 0, 1)), sd[d + ".weight"], sd[d + ".bias"], stride=2)
    t = resnet(t, "encoder.mid_block.resnets.0")
    n, c, hh, ww = t.shape
    u = gn(t, A + "group_norm").reshape(n, c, hh * ww).transpose(1, 2)
    q, k, v = (F.linear(u, sd[A + f"{m}.weight"], sd[A + f"{m}.bias"]) for m in ("to_q", "to_k", "to_v"))
    o = F.scaled_dot_product_attention(q[:, None], k[:, None], v[:, None])[:, 0]
    t = t + F.linear(o, sd[A + "to_out.0.weight"], sd[A + "to_out.0.bias"]).transpose(1, 2).reshape(n, c, hh, ww)
    t = resnet(t, "encoder.mid_block.resnets.1")
    return conv(conv(F.silu(gn(t, "encoder.conv_norm_out")), "encoder.conv_out", 1), "quant_conv", 0)


def run_torch_encode(args):
    import vae_encoder_reference as E
    dev = torch.device("cuda")
    sd = {k: v.to(dev, torch.float16) for k, v in E.init_encoder_state_dict(DEFAULT, seed=1).items()}
    out = []
    for s in args.images:
        x = (torch.rand(args.n, 3, s, s, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev, torch.float16)
        with torch.no_grad():
            ms = [time_events(lambda: torch_encode_fp16(sd, x, DEFAULT), 2, 3) for _ in range(args.rounds)]
        line = dict(leg="torch_fp16_encode", image=s, n=args.n, ms_per_image=statistics.median(ms) / args.n,
                    ms_per_image_range=[min(ms) / args.n, max(ms) / args.n], tflops=encoder_flops(DEFAULT, s, s) * args.n / (statistics.median(ms) * 1e-3) / 1e12)
        print(json.dumps(line), flush=True)
        out.append(line)
    return out


def run_native_encode(args):
    import vae_encoder_reference as E
    from mapdit_amd.vae import VAEEncoder
    dev = torch.device("cuda")
    sd = E.init_encoder_state_dict(DEFAULT, seed=1)
    out = []
    for prec in ("f16", "bf16"):
        enc = VAEEncoder.from_state_dict(sd, dev, precision=prec, max_batch=args.n)
        for s in args.images:
            u8 = torch.randint(0, 256, (args.n, s, s, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8).to(dev)
            x = ((u8.float() / 255 - 0.5) / 0.5).permute(0, 3, 1, 2).contiguous()
            for src, t in (("f32_nchw", x), ("uint8", u8)):
                ms = [time_events(lambda: enc.encode(t), 2, 3) for _ in range(args.rounds)]
                line = dict(leg="native_encode", precision=prec, input=src, image=s, n=args.n, ms_per_image=statistics.median(ms) / args.n,
                            ms_per_image_range=[min(ms) / args.n, max(ms) / args.n], gflop_per_image=encoder_flops(DEFAULT, s, s) / 1e9,
                            tflops=encoder_flops(DEFAULT, s, s) * args.n / (statistics.median(ms) * 1e-3) / 1e12,
                            workspace_mib=enc.workspace_bytes(args.n, s, s) / 2 ** 20)
                print(json.dumps(line), flush=True)
                out.append(line)
    return out


def run_torch(args):
    import vae_reference as R
    dev = torch.device("cuda")
    sd = {k: v.to(dev, torch.float16) for k, v in R.init_state_dict(DEFAULT, seed=1).items()}
    out = []
    for s in args.latents:
        z = (3 * torch.randn(args.n, 4, s, s, generator=torch.Generator().manual_seed(3))).to(dev, torch.float16)
        with torch.no_grad():
            ms = [time_events(lambda: torch_decode_fp16(sd, z, DEFAULT), 2, 3) for _ in range(args.rounds)]
        line = dict(leg="torch_fp16", latent=s, n=args.n, ms_per_image=statistics.median(ms) / args.n, ms_per_image_range=[min(ms) / args.n, max(ms) / args.n],
                    tflops=decoder_flops(DEFAULT, s, s) * args.n / (statistics.median(ms) * 1e-3) / 1e12)
        print(json.dumps(line), flush=True)
        out.append(line)
    return out


def run_native(args):
    import mapdit_amd
    import vae_reference as R
    from mapdit_amd.vae import VAEDecoder
    L = mapdit_amd._lib
    dev = torch.device("cuda")
    sd = R.init_state_dict(DEFAULT, seed=1)
    out = []
    for prec in ("f16", "bf16"):
        dec = VAEDecoder.from_state_dict(sd, dev, precision=prec, max_batch=args.n)
        for s in args.latents:
            z = (3 * torch.randn(args.n, 4, s, s, generator=torch.Generator().manual_seed(3))).to(dev)
            ms = [time_events(lambda: dec.decode(z), 2, 3) for _ in range(args.rounds)]
            line = dict(leg="native", precision=prec, latent=s, n=args.n, ms_per_image=statistics.median(ms) / args.n,
                        ms_per_image_range=[min(ms) / args.n, max(ms) / args.n], gflop_per_image=decoder_flops(DEFAULT, s, s) / 1e9,
                        tflops=decoder_flops(DEFAULT, s, s) * args.n / (statistics.median(ms) * 1e-3) / 1e12,
                        workspace_mib=dec.workspace_bytes(args.n, s, s) / 2 ** 20)
            print(json.dumps(line), flush=True)
            out.append(line)
        # the two heaviest layers alone
        dt = torch.float16 if prec == "f16" else torch.bfloat16
        fn = L.lib().vae_conv_f16 if prec == "f16" else L.lib().vae_conv
        for cch, hw in ((512, 64), (128, 256)):
            x = torch.randn(args.n, hw, hw, cch, device=dev).to(dt)
            wgt = (torch.randn(cch, 3, 3, cch, device=dev) * (9 * cch) ** -0.5).to(dt)
            bias = torch.zeros(cch, device=dev)
            y = torch.empty(args.n, hw, hw, cch, device=dev)
            a = L.VaeConv(x.data_ptr(), L.VAE_IN_16, wgt.data_ptr(), bias.data_ptr(), None, y.data_ptr(), L.VAE_OUT_F32, args.n, hw, hw, cch, cch, 3, 0)
            ms = [time_events(lambda: fn(C.byref(a), L.cur_stream()), 2, 5) for _ in range(args.rounds)]
            fl = 2 * args.n * hw * hw * 9 * cch * cch
            line = dict(leg="conv3x3", precision=prec, channels=cch, size=hw, n=args.n, ms=statistics.median(ms), ms_range=[min(ms), max(ms)],
                        tflops=fl / (statistics.median(ms) * 1e-3) / 1e12)
            print(json.dumps(line), flush=True)
            out.append(line)
            del x, wgt, y
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=16)
    p.add_argument("--latents", type=lambda s: [int(v) for v in s.split(",")], default=[32, 16])
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--encode", action="store_true", help="measure the encoder (images to posterior latents) instead of the decoder")
    p.add_argument("--images", type=lambda s: [int(v) for v in s.split(",")], default=[128, 256], help="--encode: image sizes")
    p.add_argument("--torch", action="store_true", help="also time the plain-torch fp16 network (child process, own time limit)")
    p.add_argument("--torch-only", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("--torch-timeout", type=float, default=300.0)
    p.add_argument("--out", type=str, default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), "bench_vae.py measures on the GPU; there is no CPU path"
    if args.torch_only:
        (run_torch_encode if args.encode else run_torch)(args)
        return
    lines = (run_native_encode if args.encode else run_native)(args)
    if args.torch:
        cmd = [sys.executable, os.path.abspath(__file__), "--torch-only", "--n", str(args.n), "--latents", ",".join(map(str, args.latents)), "--rounds", str(args.rounds)]
        if args.encode:
            cmd += ["--encode", "--images", ",".join(map(str, args.images))]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.torch_timeout)
            got = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
            for ln in got:
                print(json.dumps(ln), flush=True)
            lines += got
            if r.returncode != 0:
                lines.append(dict(leg="torch_fp16", error=f"exit status {r.returncode}", stderr=r.stderr[-400:]))
                print(json.dumps(lines[-1]), flush=True)
        except subprocess.TimeoutExpired as e:
            done = [json.loads(ln) for ln in (e.stdout or b"").decode().splitlines() if ln.startswith("{")]
            lines += done + [dict(leg="torch_fp16", error=f"did not finish within {args.torch_timeout:.0f} s", finished=len(done))]
            for ln in lines[-len(done) - 1:]:
                print(json.dumps(ln), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
