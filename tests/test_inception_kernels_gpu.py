"""The kernels of csrc/inception.hip one by one against fp64, at the smallest shapes that reach every guard: the implicit-GEMM
convolution (K granules that span taps and run past K, the column guard, the row guard, channel slices), the plain first-layer
kernel, the three pools, the global average, the resize and the fp64 statistics.

Convolution tolerance.  The reference multiplies the same 16-bit operands in fp64; a product of two 16-bit values is exact in fp32,
so the kernel differs by its fp32 accumulation alone: |err| <= K u sum|x||w| to first order with u = 2^-24, whatever the order of
the K additions.  The tests allow 2 K u sum|x||w| (the sum of absolute products from an fp64 convolution of the absolute values)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


def _L():
    import mapdit_amd
    return mapdit_amd._lib


def _fn(name, prec):
    return getattr(_L().lib(), name + ("_f16" if prec == "f16" else ""))


def _rt(t, prec):
    return t.to(torch.float32).to(DTYPES[prec]).to(torch.float64)


def _conv(prec, x, w, b, stride=1, pad=(0, 0), relu=True, in_f32=False, out16=False, ld=None, coff=0, out=None):
    """x fp64 [N, Cin, H, W] and w fp64 [Cout, Cin, kh, kw] holding 16-bit-representable values -> the kernel's output buffer
    [N, Ho, Wo, ld] (fp32, or the operand format with out16)."""
    L = _L()
    N, Cin, H, W = x.shape
    Cout, _, kh, kw = w.shape
    Ho, Wo = (H + 2 * pad[0] - kh) // stride + 1, (W + 2 * pad[1] - kw) // stride + 1
    ld = Cout if ld is None else ld
    xd = x.permute(0, 2, 3, 1).contiguous().to(torch.float32 if in_f32 else DTYPES[prec]).to(DEV)
    wd = w.permute(0, 2, 3, 1).contiguous().to(DTYPES[prec]).to(DEV)
    bd = b.to(torch.float32).to(DEV)
    if out is None:
        out = torch.zeros(N, Ho, Wo, ld, dtype=DTYPES[prec] if out16 else torch.float32, device=DEV)
    assert out.shape == (N, Ho, Wo, ld) and out.is_contiguous()
    a = L.IncConv(xd.data_ptr(), L.INC_IN_F32 if in_f32 else L.INC_IN_16, wd.data_ptr(), bd.data_ptr(), out.data_ptr(),
                  L.INC_OUT_16 if out16 else L.INC_OUT_F32, N, H, W, Cin, Cout, kh, kw, stride, pad[0], pad[1], int(relu), ld, coff)
    _fn("inc_conv", prec)(C.byref(a), L.cur_stream())
    torch.cuda.synchronize()
    return out


def _ref_conv(x, w, b, stride, pad, relu=True):
    """fp64 result [N, Ho, Wo, Cout] of the same operands, the bias as fp32 holds it, and the tolerance 2 K u sum|x||w| per element."""
    b = b.to(torch.float32).to(torch.float64)
    y = F.conv2d(x, w, b, stride, pad)
    y = F.relu(y) if relu else y
    K = w.shape[1] * w.shape[2] * w.shape[3]
    tol = 2 * K * 2.0 ** -24 * (F.conv2d(x.abs(), w.abs(), b.abs(), stride, pad)) + 1e-30
    return y.permute(0, 2, 3, 1), tol.permute(0, 2, 3, 1)


def _operands(prec, N, Cin, H, W, Cout, kh, kw, seed):
    g = torch.Generator().manual_seed(seed)
    x = _rt(torch.randn(N, Cin, H, W, generator=g, dtype=torch.float64), prec)
    w = _rt(torch.randn(Cout, Cin, kh, kw, generator=g, dtype=torch.float64) / (Cin * kh * kw) ** 0.5, prec)
    b = 0.3 * torch.randn(Cout, generator=g, dtype=torch.float64)
    return x, w, b


CASES = {
    # name: (N, Cin, H, W, Cout, kh, kw, stride, (pad_h, pad_w), fp32 input)
    "first layer 3x3 s2 valid 3->32 (plain path, odd extent)": (2, 3, 9, 9, 32, 3, 3, 2, (0, 0), True),
    "1x1 80->48 (K tail granule, column guard, M = 35)": (1, 80, 5, 7, 48, 1, 1, 1, (0, 0), False),
    "5x5 pad 2 48->64 (a K tile spans taps)": (2, 48, 6, 6, 64, 5, 5, 1, (2, 2), False),
    "1x7 pad (0,3) 128->128": (1, 128, 9, 9, 128, 1, 7, 1, (0, 3), False),
    "7x1 pad (3,0) 128->128": (1, 128, 9, 9, 128, 7, 1, 1, (3, 0), False),
    "3x3 s2 valid 96->96": (2, 96, 9, 9, 96, 3, 3, 2, (0, 0), False),
    "1x1 16->16, M = 129 (one row past a tile)": (1, 16, 3, 43, 16, 1, 1, 1, (0, 0), False),
    "1x3 pad (0,1) 32->80, 3x1 twin below": (1, 32, 4, 5, 80, 1, 3, 1, (0, 1), False),
    "3x1 pad (1,0) 32->80": (1, 32, 4, 5, 80, 3, 1, 1, (1, 0), False),
}


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_conv_against_fp64(case, prec):
    N, Cin, H, W, Cout, kh, kw, stride, pad, in_f32 = CASES[case]
    x, w, b = _operands(prec, N, Cin, H, W, Cout, kh, kw, seed=len(case))
    ref, tol = _ref_conv(x, w, b, stride, pad)
    out = _conv(prec, x, w, b, stride, pad, in_f32=in_f32).cpu().double()
    assert out.shape == ref.shape
    err = (out - ref).abs()
    print(f"{case} {prec}: out {tuple(out.shape)}, max err {float(err.max()):.2e}, max err / tol {float((err / tol).max()):.3f}")
    assert bool((ref > 0).any()) and bool((ref == 0).any())            # the ReLU cuts some and passes some
    assert bool((err <= tol).all())
    # without the ReLU, same call
    ref2, tol2 = _ref_conv(x, w, b, stride, pad, relu=False)
    out2 = _conv(prec, x, w, b, stride, pad, relu=False, in_f32=in_f32).cpu().double()
    assert bool(((out2 - ref2).abs() <= tol2).all()) and bool((out2 < 0).any())


@pytest.mark.parametrize("out16", [False, True])
@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_conv_writes_its_channel_slice_only(prec, out16):
    """3 x 3 stride 2 valid, 96 -> 96 on 2 x 9 x 9, at c_off 32 of a 160-wide buffer full of a sentinel: the other 64 channels keep
    their bits.  16-bit output: the fp32 result rounded once (half an ulp of the format on top of the accumulation bound)."""
    x, w, b = _operands(prec, 2, 96, 9, 9, 96, 3, 3, seed=21)
    ref, tol = _ref_conv(x, w, b, 2, (0, 0))
    dt = DTYPES[prec] if out16 else torch.float32
    sentinel = torch.full((2, 4, 4, 160), -7.25, dtype=dt, device=DEV)
    out = _conv(prec, x, w, b, 2, (0, 0), out16=out16, ld=160, coff=32, out=sentinel.clone())
    assert torch.equal(out[..., :32], sentinel[..., :32]) and torch.equal(out[..., 128:], sentinel[..., 128:])
    got = out[..., 32:128].cpu().double()
    if out16:
        tol = tol + ref.abs() * (2.0 ** -11 if prec == "f16" else 2.0 ** -8)
    assert bool(((got - ref).abs() <= tol).all()) and not bool((got == -7.25).any())


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_conv_is_batch_independent(prec):
    """One image alone against the same image at index 1 of 3 (rows 49..97 of the 147: another place in the tile, a second tile
    behind it): the same bits.  3 x 3 pad 1 and the 1 x 7 form, 64 -> 96 on 7 x 7."""
    for kh, kw, pad in ((3, 3, (1, 1)), (1, 7, (0, 3))):
        x, w, b = _operands(prec, 3, 64, 7, 7, 96, kh, kw, seed=31)
        three = _conv(prec, x, w, b, 1, pad)
        alone = _conv(prec, x[1:2], w, b, 1, pad)
        assert torch.equal(three[1], alone[0]), (kh, kw)
        assert not torch.equal(three[0], alone[0])


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("N, H, W, Cin, Cout, k", [
    (2, 5, 7, 64, 64, 3),            # the 64 tile both ways; a sample boundary inside a tile
    (1, 8, 8, 128, 128, 3),          # mapdit_vae_conv takes the 128 tile, mapdit_inc_conv the 64 tile: the two tile forms give the same bits
    (2, 4, 6, 64, 64, 1),
], ids=["2x5x7-64-64-3x3", "1x8x8-128-128-3x3", "2x4x6-64-64-1x1"])
def test_vae_conv_and_inc_conv_are_one_convolution(prec, N, H, W, Cin, Cout, k):
    """The two entry points run the same kernels (csrc/conv.hip): the same 16-bit operands, one packed [Cout][ky][kx][Cin] weight, bias,
    no ReLU, no residual, fp32 output, "same" padding through mapdit_vae_conv and pad k / 2 through mapdit_inc_conv - equal bits."""
    L = _L()
    x, w, b = _operands(prec, N, Cin, H, W, Cout, k, k, seed=61)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DTYPES[prec]).to(DEV)
    wd = w.permute(0, 2, 3, 1).contiguous().to(DTYPES[prec]).to(DEV)
    bd = b.to(torch.float32).to(DEV)
    via_vae = torch.full((N, H, W, Cout), float("nan"), device=DEV)
    via_inc = torch.full((N, H, W, Cout), float("nan"), device=DEV)
    va = L.VaeConv(xd.data_ptr(), L.VAE_IN_16, wd.data_ptr(), bd.data_ptr(), None, via_vae.data_ptr(), L.VAE_OUT_F32, N, H, W, Cin, Cout, k, 0)
    _fn("vae_conv", prec)(C.byref(va), L.cur_stream())
    ia = L.IncConv(xd.data_ptr(), L.INC_IN_16, wd.data_ptr(), bd.data_ptr(), via_inc.data_ptr(), L.INC_OUT_F32, N, H, W, Cin, Cout, k, k, 1, k // 2, k // 2,
                   0, Cout, 0)
    _fn("inc_conv", prec)(C.byref(ia), L.cur_stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(via_vae).all()) and bool((via_vae < 0).any())
    assert torch.equal(via_vae, via_inc)


def test_conv_refusals():
    L = _L()
    x, w, b = _operands("bf16", 1, 16, 4, 4, 16, 3, 3, seed=1)
    with pytest.raises(L.MapditError, match="ld_out"):
        _conv("bf16", x, w, b, 1, (1, 1), ld=24, coff=16, out=torch.zeros(1, 4, 4, 24, device=DEV))


# ---- pools ---------------------------------------------------------------------------------------------------------------------------
def _pool(prec, x, mode, in16=False, out16=False, ld=None, coff=0, fill=0.0):
    """x fp64 [N, C, H, W] -> the kernel's output buffer [N, Ho, Wo, ld]."""
    L = _L()
    N, Cc, H, W = x.shape
    Ho, Wo = ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if mode == L.INC_POOL_MAX_S2 else (H, W)
    ld = Cc if ld is None else ld
    xd = x.permute(0, 2, 3, 1).contiguous().to(DTYPES[prec] if in16 else torch.float32).to(DEV)
    out = torch.full((N, Ho, Wo, ld), fill, dtype=DTYPES[prec] if out16 else torch.float32, device=DEV)
    _fn("inc_pool", prec)(xd.data_ptr(), L.INC_IN_16 if in16 else L.INC_IN_F32, out.data_ptr(), L.INC_OUT_16 if out16 else L.INC_OUT_F32, N, H, W, Cc,
                          mode, ld, coff, L.cur_stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_pools_against_fp64(prec):
    L = _L()
    x = torch.randn(2, 32, 5, 5, generator=torch.Generator().manual_seed(41), dtype=torch.float64).float().double()
    refs = {L.INC_POOL_MAX_S2: F.max_pool2d(x, 3, 2), L.INC_POOL_AVG: F.avg_pool2d(x, 3, 1, 1, count_include_pad=False),
            L.INC_POOL_MAX_S1: F.max_pool2d(x, 3, 1, 1)}
    for mode, ref in refs.items():
        out = _pool(prec, x, mode).cpu().double()
        ref = ref.permute(0, 2, 3, 1)
        assert out.shape == ref.shape, mode
        if mode == L.INC_POOL_AVG:                                     # nine fp32 additions and a division: 10 u sum|x| / count
            tol = 10 * 2.0 ** -24 * F.avg_pool2d(x.abs(), 3, 1, 1, count_include_pad=False).permute(0, 2, 3, 1)
            assert bool(((out - ref).abs() <= tol).all())
        else:
            assert torch.equal(out, ref), mode                         # a maximum of fp32 values is one of them
    # into a channel slice, 16-bit in and out: the max pool of Mixed_6a / 7a (max commutes with the rounding: exact)
    xr = _rt(x, prec)
    out = _pool(prec, xr, L.INC_POOL_MAX_S2, in16=True, out16=True, ld=80, coff=16, fill=-3.5)
    assert torch.equal(out[..., 16:48].cpu().double(), F.max_pool2d(xr, 3, 2).permute(0, 2, 3, 1))
    assert bool((out[..., :16] == -3.5).all()) and bool((out[..., 48:] == -3.5).all())
    # global average
    gx = x.permute(0, 2, 3, 1).contiguous().float().to(DEV)
    g = torch.empty(2, 32, dtype=torch.float32, device=DEV)
    _fn("inc_global_avg", prec)(gx.data_ptr(), L.INC_IN_F32, g.data_ptr(), 2, 25, 32, L.cur_stream())
    torch.cuda.synchronize()
    assert bool(((g.cpu().double() - x.mean(dim=(2, 3))).abs() <= 26 * 2.0 ** -24 * x.abs().mean(dim=(2, 3))).all())


def test_average_pool_excludes_the_padding():
    """count_include_pad = False: a constant image stays that constant exactly, corners (4 taps) and edges (6) included.  (Dividing by
    9 everywhere, torchvision's form, would give 4/9 and 6/9 of it there.)"""
    L = _L()
    for prec in ("f16", "bf16"):
        x = torch.full((2, 32, 5, 5), 0.71875, dtype=torch.float64)
        out = _pool(prec, x, L.INC_POOL_AVG)
        assert bool((out == 0.71875).all())
        out16 = _pool(prec, x, L.INC_POOL_AVG, in16=True, out16=True)
        assert bool((out16.float() == 0.71875).all())


# ---- resize ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H, W", [(8, 8), (13, 17), (299, 299)])
def test_resize_u8_against_interpolate(H, W):
    """Against F.interpolate in fp64 followed by x / 255 * 2 - 1: 1e-6 absolute (fp32 interpolation weights on values in [0, 255],
    then scaled by 2 / 255).  299 x 299 is the identity: exact up to the final fp32 arithmetic."""
    L = _L()
    img = torch.randint(0, 256, (2, H, W, 3), generator=torch.Generator().manual_seed(H), dtype=torch.uint8)
    ref = F.interpolate(img.permute(0, 3, 1, 2).double(), size=(299, 299), mode="bilinear", align_corners=False) / 255.0 * 2.0 - 1.0
    out = torch.empty(2, 299, 299, 3, dtype=torch.float32, device=DEV)
    L.lib().inc_resize_u8(img.to(DEV).data_ptr(), out.data_ptr(), 2, H, W, 3, 299, L.cur_stream())
    torch.cuda.synchronize()
    err = float((out.cpu().double() - ref.permute(0, 2, 3, 1)).abs().max())
    print(f"resize {H} x {W} -> 299: max abs err {err:.2e}")
    assert err <= 1e-6
    # the fp32 NCHW form: the same picture handed over as [-1, 1] floats
    xf = (img.permute(0, 3, 1, 2).double() / 255.0 * 2.0 - 1.0).float().contiguous()
    out2 = torch.empty_like(out)
    L.lib().inc_resize_f32(xf.to(DEV).data_ptr(), out2.data_ptr(), 2, H, W, 3, 299, L.cur_stream())
    torch.cuda.synchronize()
    assert float((out2.cpu().double() - ref.permute(0, 2, 3, 1)).abs().max()) <= 1e-6


# ---- statistics -----------------------------------------------------------------------------------------------------------------------
def test_stats_accumulate_is_batching_independent_and_matches_numpy():
    L = _L()
    D, N = 48, 37
    x = torch.rand(N, D, generator=torch.Generator().manual_seed(51)) * 3.0        # (pool features are >= 0)
    xd = x.to(DEV)

    def run(cuts):
        s = torch.zeros(D, dtype=torch.float64, device=DEV)
        o = torch.zeros(D, D, dtype=torch.float64, device=DEV)
        i = 0
        for n in cuts:
            L.lib().inc_stats_accumulate(xd[i:i + n].contiguous().data_ptr(), n, D, s.data_ptr(), o.data_ptr(), L.cur_stream())
            i += n
        torch.cuda.synchronize()
        return s.cpu().numpy(), o.cpu().numpy()

    s1, o1 = run([37])
    s2, o2 = run([5, 32])
    assert np.array_equal(s1, s2) and np.array_equal(o1, o2)
    x64 = x.numpy().astype(np.float64)
    assert np.abs(s1 - x64.sum(0)).max() <= 1e-13 * np.abs(x64.sum(0)).min()
    want = x64.T @ x64
    assert (np.abs(o1 - want) <= 1e-13 * want).all() and np.array_equal(o1, o1.T)
