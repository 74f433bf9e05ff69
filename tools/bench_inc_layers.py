"""Device time of mapdit_inc_conv alone on fifteen of the Inception network's layer shapes at N = 64 (16-bit output, ReLU), both operand
formats: best of three rounds of twenty launches, in microseconds, one JSON line.  MAPDIT_LIB selects another build for an A/B.

    python tools/bench_inc_layers.py
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import mapdit_amd  # noqa: E402

L = mapdit_amd._lib
N = 64
LAYERS = [  # H, Cin, Cout, kh, kw, st, ph, pw, in_f32
    (299, 3, 32, 3, 3, 2, 0, 0, True),
    (149, 32, 32, 3, 3, 1, 0, 0, False),
    (147, 32, 64, 3, 3, 1, 1, 1, False),
    (73, 64, 80, 1, 1, 1, 0, 0, False),
    (73, 80, 192, 3, 3, 1, 0, 0, False),
    (35, 192, 64, 1, 1, 1, 0, 0, False),
    (35, 48, 64, 5, 5, 1, 2, 2, False),
    (35, 64, 96, 3, 3, 1, 1, 1, False),
    (35, 288, 384, 3, 3, 2, 0, 0, False),
    (17, 768, 192, 1, 1, 1, 0, 0, False),
    (17, 128, 128, 1, 7, 1, 0, 3, False),
    (17, 192, 192, 7, 1, 1, 3, 0, False),
    (8, 1280, 320, 1, 1, 1, 0, 0, False),
    (8, 448, 384, 3, 3, 1, 1, 1, False),
    (8, 2048, 448, 1, 1, 1, 0, 0, False),
]
out = {}
for prec, dt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
    fn = getattr(L.lib(), "inc_conv" + ("_f16" if prec == "f16" else ""))
    for (H, Cin, Cout, kh, kw, st, ph, pw, f32) in LAYERS:
        Ho = (H + 2 * ph - kh) // st + 1
        Wo = (H + 2 * pw - kw) // st + 1
        x = torch.randn(N, H, H, Cin, device="cuda").to(torch.float32 if f32 else dt)
        w = (torch.randn(Cout, kh, kw, Cin, device="cuda") * (kh * kw * Cin) ** -0.5).to(dt)
        b = torch.zeros(Cout, device="cuda")
        y = torch.empty(N, Ho, Wo, Cout, device="cuda", dtype=dt)
        a = L.IncConv(x.data_ptr(), L.INC_IN_F32 if f32 else L.INC_IN_16, w.data_ptr(), b.data_ptr(), y.data_ptr(), L.INC_OUT_16, N, H, H, Cin, Cout, kh, kw,
                      st, ph, pw, 1, Cout, 0)
        best = 1e9
        for _ in range(3):
            for _ in range(3):
                fn(C.byref(a), L.cur_stream())
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn(C.byref(a), L.cur_stream())
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / 20 * 1e3)
        out[f"{prec} {H} {Cin}->{Cout} {kh}x{kw} s{st}"] = best
        del x, w, y
print(json.dumps(out))
