"""The encoder's kernels (csrc/vae.hip) one by one: the stride-2 downsample convolution in both operand formats, the posterior head,
the image preparation and the latent statistics.

conv_down: the reference is an fp64 convolution of the ALREADY ROUNDED operands - literally F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2) -
so what is left is fp32 accumulation: |out - ref| <= (9 Cin + 2) 2^-23 S with S the same convolution of the absolute values + |bias|,
the bound of tests/test_vae_kernels_gpu.py (derived, not measured).  A wrong pad side or a halo taken from the flat index is off by O(1)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMATS = {"f16": (torch.float16, "_f16"), "bf16": (torch.bfloat16, "")}      # dtype, symbol suffix


def _lib():
    import mapdit_amd
    return mapdit_amd._lib


def run_conv_down(fmt, x, *, in_kind, wp, bias, N, Hin, Win, Cin, Cout, H=None, W=None, k=3, up2=0):
    L = _lib()
    H, W = Hin // 2 if H is None else H, Win // 2 if W is None else W
    out = torch.full((N, H, W, Cout), float("nan"), device=DEV)
    a = L.VaeConv(x.data_ptr(), in_kind, wp.data_ptr(), bias.data_ptr(), None, out.data_ptr(), L.VAE_OUT_F32, N, H, W, Cin, Cout, k, up2)
    getattr(L.lib(), "vae_conv_down" + FORMATS[fmt][1])(C.byref(a), Hin, Win, L.cur_stream())
    torch.cuda.synchronize()
    return out


DOWN_CASES = [
    # (N, Hin, Win, Cin, Cout), fp32 input
    ((2, 5, 7, 64, 64), False),                # odd sizes (the pad row / column is never touched); both samples in one M tile
    ((3, 20, 20, 64, 128), False),             # tiles that straddle rows and samples; the last window reads the zero row and column
    ((1, 8, 8, 128, 128), False),              # the wide tile
    ((2, 4, 6, 64, 64), True),                 # 2 x 3 outputs: every output touches a border
    ((1, 6, 8, 8, 8), False),                  # the plain path
    ((1, 8, 8, 512, 512), False),              # the production K
]


def _down_case(fmt, shape, f32, seed=0):
    L = _lib()
    N, Hin, Win, Cin, Cout = shape
    dt = FORMATS[fmt][0]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Hin, Win, Cin, generator=g)                                    # NHWC
    w = (torch.rand(Cout, Cin, 3, 3, generator=g) * 2 - 1) * (3.0 / (Cin * 9)) ** 0.5
    bias = (torch.rand(Cout, generator=g) * 2 - 1) * 0.1
    xr, wr = x.to(dt).double().permute(0, 3, 1, 2), w.to(dt).double()                 # the operands as the MFMA sees them
    ref = F.conv2d(F.pad(xr, (0, 1, 0, 1)), wr, bias.double(), stride=2)
    S = F.conv2d(F.pad(xr.abs(), (0, 1, 0, 1)), wr.abs(), None, stride=2) + bias.double().abs().reshape(1, -1, 1, 1)
    bound = (9 * Cin + 2) * 2.0 ** -23 * S
    args = dict(in_kind=L.VAE_IN_F32 if f32 else L.VAE_IN_16, wp=w.permute(0, 2, 3, 1).contiguous().to(dt).to(DEV), bias=bias.to(DEV), Cin=Cin, Cout=Cout)
    return (x.to(DEV) if f32 else x.to(dt).to(DEV)), args, ref.permute(0, 2, 3, 1), bound.permute(0, 2, 3, 1)


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("shape, f32", DOWN_CASES, ids=["x".join(map(str, s)) + ("-f32" if f else "") for s, f in DOWN_CASES])
def test_conv_down_against_fp64_of_the_rounded_operands(fmt, shape, f32):
    N, Hin, Win = shape[:3]
    xin, args, ref, bound = _down_case(fmt, shape, f32)
    out = run_conv_down(fmt, xin, N=N, Hin=Hin, Win=Win, **args)
    assert out.shape == ref.shape == (N, Hin // 2, Win // 2, shape[4])
    assert torch.isfinite(out).all()
    err = (out.double().cpu() - ref).abs()
    worst = float((err / bound).max())
    print(f"conv_down {fmt} {shape} f32={f32}: max |err| {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("shape", [DOWN_CASES[0][0], DOWN_CASES[1][0]], ids=["2x5x7", "3x20x20"])
def test_conv_down_sample_alone_equals_its_slice_of_the_batch(fmt, shape):
    N, Hin, Win = shape[:3]
    xin, a, _, _ = _down_case(fmt, shape, False)
    batch = run_conv_down(fmt, xin, N=N, Hin=Hin, Win=Win, **a)
    for n in range(N):
        alone = run_conv_down(fmt, xin[n:n + 1].contiguous(), N=1, Hin=Hin, Win=Win, **a)
        assert torch.equal(alone[0], batch[n]), n


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_conv_down_refusals(fmt):
    L = _lib()
    shape = (2, 4, 6, 64, 64)
    xin, a, _, _ = _down_case(fmt, shape, False)
    with pytest.raises(L.MapditError, match="k=1"):
        run_conv_down(fmt, xin, N=2, Hin=4, Win=6, k=1, **a)
    with pytest.raises(L.MapditError, match="up2=1"):
        run_conv_down(fmt, xin, N=2, Hin=4, Win=6, up2=1, **a)
    with pytest.raises(L.MapditError, match="2 x 3 expected"):
        run_conv_down(fmt, xin, N=2, Hin=4, Win=6, H=3, W=3, **a)              # H != Hin / 2


# ---- posterior head ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_logvar", [True, False])
def test_posterior_head(with_logvar):
    N, hw, Lc = 3, 35, 4                                                       # 420 outputs: no multiple of the workgroup size
    g = torch.Generator().manual_seed(5)
    mom = torch.empty(N, hw, 2 * Lc)
    mom[..., :Lc] = torch.randperm(N * hw * Lc, generator=g).reshape(N, hw, Lc).float() * 0.37 - 70.0      # a different value in every element
    raw = torch.rand(N, hw, Lc, generator=g) * 24 - 12 + torch.arange(N * hw * Lc).reshape(N, hw, Lc) * 1e-4  # distinct as well
    special = torch.tensor([-40.0, -30.0, -29.999, 0.0, 19.999, 20.0, 25.0])
    raw.reshape(-1)[torch.arange(7) * 53 + 11] = special
    mom[..., Lc:] = raw
    mean = torch.full((N, Lc, hw), float("nan"), device=DEV)
    std, logvar = torch.full_like(mean, float("nan")), torch.full_like(mean, float("nan"))
    L = _lib()
    md = mom.to(DEV)
    L.lib().vae_posterior(md.data_ptr(), mean.data_ptr(), std.data_ptr(), logvar.data_ptr() if with_logvar else None, N, hw, Lc, L.cur_stream())
    torch.cuda.synchronize()
    assert torch.equal(mean.cpu(), mom[..., :Lc].transpose(1, 2).contiguous())              # bit-equal, transposed
    lv = torch.clamp(raw, -30.0, 20.0).transpose(1, 2).contiguous()
    if with_logvar:
        assert torch.equal(logvar.cpu(), lv)
        assert set(special.clamp(-30, 20).tolist()) <= set(logvar.cpu().reshape(-1).tolist())
    else:
        assert torch.isnan(logvar).all()                                                    # NULL: not written
    want = torch.exp(0.5 * lv.double())
    rel = float(((std.double().cpu() - want).abs() / want).max())
    print(f"posterior std: max rel err {rel:.3e} (bound 1e-6)")
    assert rel <= 1e-6
    # NaN propagates (a clamp written with fminf / fmaxf would turn it into a bound)
    md[0, 0, Lc] = float("nan")
    md[0, 1, 0] = float("nan")
    L.lib().vae_posterior(md.data_ptr(), mean.data_ptr(), std.data_ptr(), None, N, hw, Lc, L.cur_stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(std[0, 0, 0])) and bool(torch.isnan(mean[0, 0, 1])) and int(torch.isnan(std).sum()) == 1 and int(torch.isnan(mean).sum()) == 1


# ---- image preparation ----------------------------------------------------------------------------------------------------------------
def _prepare(u8, flip):
    L = _lib()
    N, H, W, Cc = u8.shape
    out = torch.full((N, H, W, Cc), float("nan"), device=DEV)
    ud = u8.to(DEV)
    fd = None if flip is None else flip.to(DEV)
    L.lib().vae_prepare_u8(ud.data_ptr(), None if fd is None else fd.data_ptr(), out.data_ptr(), N, H, W, Cc, L.cur_stream())
    torch.cuda.synchronize()
    return out.cpu()


def _torch_prepare(u8):
    return (u8.float().div(255) - 0.5) / 0.5                                   # ToTensor + Normalize(0.5, 0.5), on the CPU


def test_prepare_u8_all_byte_values_bit_equal():
    u8 = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16, 1)
    got = _prepare(u8, None)
    assert torch.equal(got, _torch_prepare(u8))
    one_multiply = u8.float() * (2.0 / 255.0) - 1.0                            # the form the contract excludes: it is not the same function
    assert int((one_multiply != _torch_prepare(u8)).sum()) > 0


def test_prepare_u8_flip_per_sample():
    g = torch.Generator().manual_seed(6)
    u8 = torch.randint(0, 256, (3, 5, 7, 3), generator=g, dtype=torch.uint8)
    want = _torch_prepare(u8)
    flipped = want.clone()
    flipped[1] = torch.flip(want[1:2], dims=[2])[0]                            # [N, H, W, C]: dim 2 is the width
    assert torch.equal(_prepare(u8, torch.tensor([0, 1, 0], dtype=torch.uint8)), flipped)
    assert torch.equal(_prepare(u8, torch.tensor([0, 7, 0], dtype=torch.uint8)), flipped)      # any non-zero byte
    assert torch.equal(_prepare(u8, None), want)                                # flip = NULL: nothing mirrored
    assert torch.equal(_prepare(u8, torch.zeros(3, dtype=torch.uint8)), want)


# ---- latent statistics -----------------------------------------------------------------------------------------------------------------
def _stats(means, stds, chunks):
    L = _lib()
    N, Lc, h, w = means.shape
    acc = torch.zeros(Lc, 3, dtype=torch.float64, device=DEV)
    i = 0
    for n in chunks:
        m, s = means[i:i + n].contiguous().to(DEV), stds[i:i + n].contiguous().to(DEV)
        L.lib().vae_stats_accumulate(m.data_ptr(), s.data_ptr(), n, Lc, h * w, acc.data_ptr(), L.cur_stream())
        i += n
    assert i == N
    cm, cs = torch.full((Lc,), float("nan"), device=DEV), torch.full((Lc,), float("nan"), device=DEV)
    L.lib().vae_stats_finish(acc.data_ptr(), C.c_double(float(N * h * w)), cm.data_ptr(), cs.data_ptr(), Lc, L.cur_stream())
    torch.cuda.synchronize()
    return acc.cpu(), cm.cpu(), cs.cpu()


def test_latent_statistics():
    g = torch.Generator().manual_seed(8)
    spread = torch.tensor([1.0, 0.5, 2.0, 1.5])
    offset = torch.tensor([3.0, -1.5, 1.0, 4.5])                               # of the order of the spread, |offset| <= 3 x spread
    means = (offset[None, :, None, None] + spread[None, :, None, None] * torch.randn(37, 4, 5, 7, generator=g)).float()
    stds = (0.05 + 1.95 * torch.rand(37, 4, 5, 7, generator=g)).float()
    # download_data.py:56-58 in fp64, two-pass
    m64, s64 = means.double(), stds.double()
    mean = m64.mean(dim=[0, 2, 3])
    var = s64.square().mean(dim=[0, 2, 3]) + (m64 - mean[None, :, None, None]).square().mean(dim=[0, 2, 3])
    std = var.sqrt()
    acc1, cm1, cs1 = _stats(means, stds, [37])
    acc3, cm3, cs3 = _stats(means, stds, [16, 16, 5])
    n = 37 * 35
    for acc in (acc1, acc3):
        am = acc[:, 0] / n
        astd = (acc[:, 2] / n + acc[:, 1] / n - am * am).sqrt()
        e_m, e_s = float(((am - mean) / mean).abs().max()), float(((astd - std) / std).abs().max())
        print(f"latent statistics from the fp64 sums: mean rel err {e_m:.3e}, std rel err {e_s:.3e} (bound 1e-9)")
        assert e_m <= 1e-9 and e_s <= 1e-9
    # the stored results are the fp32 roundings of those fp64 values
    for cm, cs in ((cm1, cs1), (cm3, cs3)):
        assert float(((cm.double() - mean).abs() / mean.abs()).max()) <= 2.0 ** -24 + 1e-9
        assert float(((cs.double() - std).abs() / std).max()) <= 2.0 ** -24 + 1e-9
    acc3b, cm3b, cs3b = _stats(means, stds, [16, 16, 5])
    assert torch.equal(acc3, acc3b) and torch.equal(cm3, cm3b) and torch.equal(cs3, cs3b)   # fixed order, no atomics
