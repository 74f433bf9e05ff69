"""The three kernel families of the VAE decoder (csrc/vae.hip) one by one against fp64, in both 16-bit operand formats.

Convolution: the reference is an fp64 conv of the ALREADY ROUNDED operands, so what is left is fp32 accumulation:
|out - ref| <= (k^2 Cin + 2) 2^-23 S with S = conv(|x|, |w|) + |bias| + |res| - the bound for any summation order with one bit of slack
for the MFMA's internal rounding.  An indexing error (a halo read across an image row or across samples) is off by O(1)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMATS = {"f16": (torch.float16, "_f16", 2.0 ** -10), "bf16": (torch.bfloat16, "", 2.0 ** -7)}      # dtype, symbol suffix, one unit in the last place


def _lib():
    import mapdit_amd
    return mapdit_amd._lib


def _fn(name, fmt):
    return getattr(_lib().lib(), name + FORMATS[fmt][1])


def _pack(w, dt):
    return w.permute(0, 2, 3, 1).contiguous().to(dt)


def run_conv(fmt, x_nhwc, *, in_kind, wp, bias, res, N, H, W, Cin, Cout, k, up2, out_kind):
    L = _lib()
    if out_kind == L.VAE_OUT_F32_NCHW:
        out = torch.full((N, Cout, H, W), float("nan"), device=DEV)
    else:
        out = torch.full((N, H, W, Cout), float("nan"), device=DEV, dtype=FORMATS[fmt][0] if out_kind == L.VAE_OUT_16 else torch.float32)
    a = L.VaeConv(x_nhwc.data_ptr(), in_kind, wp.data_ptr(), bias.data_ptr(), None if res is None else res.data_ptr(), out.data_ptr(), out_kind,
                  N, H, W, Cin, Cout, k, up2)
    _fn("vae_conv", fmt)(C.byref(a), L.cur_stream())
    torch.cuda.synchronize()
    return out


CONV_CASES = [
    # (N, H, W, Cin, Cout, k), options
    ((2, 5, 7, 64, 64, 3), {}),                                   # odd sizes; 35 pixels per sample: one M tile holds both samples
    ((3, 20, 20, 64, 128, 3), {}),                                # tiles that straddle rows and samples mid-image
    ((1, 8, 8, 128, 64, 3), {"res": True}),
    ((2, 8, 12, 64, 64, 3), {"up2": True, "f32": True}),          # from a fp32 [2, 4, 6, 64] input
    ((2, 8, 8, 4, 64, 3), {"f32": True}),                         # conv_in
    ((1, 9, 8, 64, 3, 3), {"nchw": True}),                        # conv_out
    ((2, 4, 6, 128, 64, 1), {"f32": True, "res": True}),          # shortcut
    ((1, 4, 6, 4, 4, 1), {}),
    ((1, 8, 8, 512, 512, 3), {}),                                 # the production K
]


def _conv_case(fmt, shape, opts, seed=0):
    """Inputs of one case, its fp64 reference (NHWC or NCHW like the kernel's output) and the bound."""
    L = _lib()
    N, H, W, Cin, Cout, k = shape
    dt = FORMATS[fmt][0]
    g = torch.Generator().manual_seed(seed)
    up2 = 1 if opts.get("up2") else 0
    Hs, Ws = (H // 2, W // 2) if up2 else (H, W)
    x = torch.randn(N, Hs, Ws, Cin, generator=g)                                      # NHWC
    w = (torch.rand(Cout, Cin, k, k, generator=g) * 2 - 1) * (3.0 / (Cin * k * k)) ** 0.5
    bias = (torch.rand(Cout, generator=g) * 2 - 1) * 0.1
    res = torch.randn(N, H, W, Cout, generator=g) if opts.get("res") else None
    xr, wr = x.to(dt).double(), w.to(dt).double()                                     # the operands as the MFMA sees them
    xin = x.to(DEV) if opts.get("f32") else x.to(dt).to(DEV)
    xc = xr.permute(0, 3, 1, 2)
    if up2:
        xc = F.interpolate(xc, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(xc, wr, bias.double(), padding=k // 2)
    S = F.conv2d(xc.abs(), wr.abs(), None, padding=k // 2) + bias.double().abs().reshape(1, -1, 1, 1)
    if res is not None:
        ref = ref + res.double().permute(0, 3, 1, 2)
        S = S + res.double().abs().permute(0, 3, 1, 2)
    bound = (k * k * Cin + 2) * 2.0 ** -23 * S
    nchw = bool(opts.get("nchw"))
    if not nchw:
        ref, bound = ref.permute(0, 2, 3, 1), bound.permute(0, 2, 3, 1)
    args = dict(in_kind=L.VAE_IN_F32 if opts.get("f32") else L.VAE_IN_16, wp=_pack(w, dt).to(DEV), bias=bias.to(DEV),
                res=None if res is None else res.to(DEV), Cin=Cin, Cout=Cout, k=k, up2=up2, out_kind=L.VAE_OUT_F32_NCHW if nchw else L.VAE_OUT_F32)
    return xin, args, ref, bound


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("shape, opts", CONV_CASES, ids=[("x".join(map(str, s)) + "".join("-" + o for o in sorted(op))) for s, op in CONV_CASES])
def test_conv_against_fp64_of_the_rounded_operands(fmt, shape, opts):
    N, H, W = shape[:3]
    xin, args, ref, bound = _conv_case(fmt, shape, opts)
    out = run_conv(fmt, xin, N=N, H=H, W=W, **args)
    assert torch.isfinite(out).all()
    err = (out.double().cpu() - ref).abs()
    worst = float((err / bound).max())
    print(f"conv {fmt} {shape} {sorted(opts)}: max |err| {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("shape", [CONV_CASES[0][0], CONV_CASES[1][0]], ids=["2x5x7", "3x20x20"])
def test_conv_sample_alone_equals_its_slice_of_the_batch(fmt, shape):
    """M = N H W is flattened: a 128-row tile holds the end of one sample and the start of the next.  A halo taken from the flat index
    would leak the neighbour sample's rows into the border; each sample run alone (where that neighbour does not exist) shows it."""
    N, H, W = shape[:3]
    xin, a, _, _ = _conv_case(fmt, shape, {})
    batch = run_conv(fmt, xin, N=N, H=H, W=W, **a)
    for n in range(N):
        alone = run_conv(fmt, xin[n:n + 1].contiguous(), N=1, H=H, W=W, **a)
        assert torch.equal(alone[0], batch[n]), n


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_conv_16_bit_store_and_refusals(fmt):
    """The stacked q / k / v projection writes 16-bit operands: the fp32 bound plus one unit in the last place of the format."""
    L = _lib()
    shape = (2, 4, 6, 64, 192, 1)
    N, H, W, Cin, Cout, k = shape
    xin, a, ref, bound = _conv_case(fmt, shape, {}, seed=3)
    out = run_conv(fmt, xin, N=N, H=H, W=W, **dict(a, out_kind=L.VAE_OUT_16))
    err = (out.double().cpu() - ref).abs()
    assert float((err / (bound + FORMATS[fmt][2] * ref.abs())).max()) <= 1.0
    with pytest.raises(L.MapditError, match="k=5"):
        run_conv(fmt, xin, N=N, H=H, W=W, **dict(a, k=5))
    with pytest.raises(L.MapditError, match="even"):
        run_conv(fmt, xin, N=N, H=5, W=W, **dict(a, up2=1))


# ---- GroupNorm -----------------------------------------------------------------------------------------------------------------------
def run_groupnorm(fmt, x, gamma, beta, silu, G, split, eps=1e-6):
    """split: pass the scratch that selects the two-stage form (partial sums per 1,024-pixel chunk); without it one workgroup per (sample, group)."""
    N, HW, Cc = x.shape
    out = torch.full((N, HW, Cc), float("nan"), device=DEV, dtype=FORMATS[fmt][0])
    stats = torch.full((N, G, 2), float("nan"), device=DEV)
    scratch = torch.full((N * ((HW + 1023) // 1024) * G * 2,), float("nan"), device=DEV, dtype=torch.float64) if split else None
    _fn("vae_groupnorm", fmt)(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, silu, out.data_ptr(), stats.data_ptr(), N, HW, Cc, G,
                              None if scratch is None else scratch.data_ptr(), 0 if scratch is None else scratch.numel() * 8, _lib().cur_stream())
    torch.cuda.synchronize()
    return out, stats


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("mean, std", [(0.5, 2.0), (1000.0, 1.0)], ids=["N(0.5,4)", "N(1000,1)"])
@pytest.mark.parametrize("split", [False, True], ids=["one-launch", "split"])
@pytest.mark.parametrize("shape", [(2, 5, 7, 64, 32), (1, 16, 16, 512, 32), (2, 4, 6, 128, 32), (2, 33, 32, 64, 32)], ids=lambda s: "x".join(map(str, s)))
def test_groupnorm(fmt, silu, mean, std, shape, split):
    """(2, 33, 32, 64, 32): 1,056 pixels - two chunks of the split form, the second one short - and two channels per group, so that one
    thread's four channels belong to two groups."""
    N, H, W, Cc, G = shape
    g = torch.Generator().manual_seed(7)
    x = (mean + std * torch.randn(N, H * W, Cc, generator=g)).float()
    gamma, beta = 1 + 0.2 * torch.randn(Cc, generator=g), 0.2 * torch.randn(Cc, generator=g)
    xd = x.double().reshape(N, H * W, G, Cc // G)
    m64 = xd.mean(dim=(1, 3))
    r64 = 1.0 / torch.sqrt(xd.var(dim=(1, 3), unbiased=False) + 1e-6)
    xhat_g = ((xd - m64[:, None, :, None]) * r64[:, None, :, None]).reshape(N, H * W, Cc) * gamma.double()
    t = xhat_g + beta.double()
    y64 = F.silu(t) if silu else t
    out, stats = run_groupnorm(fmt, x.to(DEV), gamma.to(DEV), beta.to(DEV), silu, G, split)
    out2, stats2 = run_groupnorm(fmt, x.to(DEV), gamma.to(DEV), beta.to(DEV), silu, G, split)
    assert torch.equal(out, out2) and torch.equal(stats, stats2)                       # fixed summation order, no atomics
    stats = stats.double().cpu()
    e_mean = float((stats[..., 0] - m64).abs().max())
    e_rstd = float(((stats[..., 1] - r64) / r64).abs().max())
    print(f"groupnorm {fmt} {shape} silu={silu} mean={mean} split={split}: mean err {e_mean:.3e} (bound {4 * 2.0 ** -24 * float(x.abs().max()):.3e}), rstd rel err {e_rstd:.3e}")
    assert e_mean <= 4 * 2.0 ** -24 * float(x.abs().max())
    assert e_rstd <= 1e-5                                                              # a one-pass fp32 E[x^2] - E[x]^2 misses this by percents at mean 1000
    assert torch.isfinite(out).all()
    bound = FORMATS[fmt][2] * y64.abs() + 2.0 ** -18 * (xhat_g.abs() + beta.double().abs()) + (1e-3 if mean == 1000.0 else 0.0)
    worst = float(((out.double().cpu() - y64).abs() / bound).max())
    print(f"    output: worst err / bound {worst:.3f}")
    assert worst <= 1.0


# ---- softmax -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("variant", ["plain", "pm80", "plus100"])
@pytest.mark.parametrize("rows, T", [(24, 24), (64, 64), (256, 1024)])
def test_softmax(fmt, variant, rows, T):
    g = torch.Generator().manual_seed(9)
    s = torch.randn(rows, T, generator=g)
    if variant == "pm80":
        s[:, 1::7] = 80.0
        s[:, 3::11] = -80.0
    elif variant == "plus100":
        s[torch.arange(rows), torch.randint(0, T, (rows,), generator=g)] = 100.0        # exp(100) overflows fp32 without the max subtraction
    ref = torch.softmax(s.double(), dim=-1)
    p = torch.full((rows, T), float("nan"), device=DEV, dtype=FORMATS[fmt][0])
    sd = s.to(DEV)
    _fn("vae_softmax", fmt)(sd.data_ptr(), T, p.data_ptr(), T, rows, T, _lib().cur_stream())
    torch.cuda.synchronize()
    assert torch.isfinite(p).all()
    pd = p.double().cpu()
    ulp = FORMATS[fmt][2]
    worst = float(((pd - ref).abs() / (ulp * ref + 2.0 ** -16)).max())
    rowsum = float((pd.sum(-1) - 1).abs().max())
    print(f"softmax {fmt} {variant} {rows}x{T}: worst err / bound {worst:.3f}, max |rowsum - 1| {rowsum:.3e}")
    assert worst <= 1.0
    assert rowsum <= min(T * ulp / 2, 2e-2)                                             # T 2^-11 (fp16) / T 2^-8 (bf16), capped
