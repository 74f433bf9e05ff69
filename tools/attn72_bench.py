#!/usr/bin/env python3
"""Micro-benchmark of the head_dim-72 attention kernels, by default on the DiT-XL/2 sampling shape (256 rows of the CFG batch x 16 heads,
256 tokens): the forward on normalised q, k, its raw-q/k form (inference), the training form that writes the normalised rows back
(beyond 256 tokens: the normalisation pass + the tiled forward), and the two backward forms (head-major dq^, dk^, dv; the Jacobian exit
straight into dqkv).  --tokens 1024: DiT-XL/2 on 64x64 latents (256-token key / query tiles).  TFLOP/s count 2 products forward, 5 backward
(the two-pass backward executes 7).
    python tools/attn72_bench.py [--batch 256] [--heads 16] [--tokens 256] [--iters 20] [--f16]"""
import argparse, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mapdit_amd  # noqa: E402
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--heads", type=int, default=16)
ap.add_argument("--tokens", type=int, default=256)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--f16", action="store_true")
a = ap.parse_args()
lib = mapdit_amd._lib.lib()
B, H, T, hd = a.batch, a.heads, a.tokens, 72
D = H * hd
dt = torch.float16 if a.f16 else torch.bfloat16
sfx = "_f16" if a.f16 else ""
g = torch.Generator(device="cuda").manual_seed(0)
rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
q, k, v = rn(B * H, T, hd).to(dt), rn(B * H, T, hd).to(dt), rn(B * H, T, hd).to(dt)
o = torch.empty(B * T, D, device="cuda", dtype=dt)
lse = torch.empty(B * H, T, device="cuda")
scales = torch.empty(2, B * H, T, device="cuda")
st = torch.cuda.current_stream().cuda_stream
p = lambda t: t.data_ptr()
dO = rn(B * T, D).to(dt)
delta = torch.empty(B * H, T, device="cuda")
dqn, dkn, dv = (torch.empty(B * H, T, hd, device="cuda", dtype=dt) for _ in range(3))
dqkv = torch.empty(B * T, 3 * D, device="cuda", dtype=dt)
F = lambda n: getattr(lib, n + sfx)
F("attn_cos_fwd_rawqk_save")(p(q), p(k), p(v), p(o), p(lse), p(scales), B, T, H, hd, st)       # q, k normalised, scales / o / lse valid from here on
cases = [("fwd (normalised q, k)", 4.0, lambda: F("attn_cos_fwd")(p(q), p(k), p(v), p(o), p(lse), B, T, H, hd, st)),
         ("bwd two-pass (dq^, dk^, dv)", 10.0, lambda: F("attn_cos_bwd")(p(q), p(k), p(v), p(dO), p(o), p(lse), p(delta), p(dqn), p(dkn), p(dv), B, T, H, hd, st)),
         ("bwd two-pass, Jacobian exit", 10.0, lambda: F("attn_cos_bwd_fused")(p(q), p(k), p(v), p(dO), p(o), p(lse), p(delta), p(scales), p(dqkv), B, T, H, hd, st)),
         ("q, k normalisation pass", 0.0, lambda: F("qk_cos_normalize")(p(q), p(k), p(scales), B, T, H, hd, st)),
         ("fwd raw (inference)", 4.0, lambda: getattr(lib, "attn_cos_fwd_rawqk" + sfx)(p(q), p(k), p(v), p(o), p(lse), B, T, H, hd, st)),
         ("fwd raw + save (training)", 4.0, lambda: getattr(lib, "attn_cos_fwd_rawqk_save" + sfx)(p(q), p(k), p(v), p(o), p(lse), p(scales), B, T, H, hd, st))]
print(f"head_dim 72, {B} x {H} heads, {T} tokens, {'f16' if a.f16 else 'bf16'}, {a.iters} launches each")
for name, fl, fn in cases:
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / a.iters * 1e3
    pairs = B * H * (T // 256) ** 2 if T % 256 == 0 else 0
    per = f"   {us * 1e3 / pairs:7.1f} ns per 256 x 256 tile pair" if pairs and fl else ""
    print(f"{name:30s} {us:9.1f} us   {fl * T * T * hd * B * H / us / 1e6:7.1f} TFLOP/s{per}")
