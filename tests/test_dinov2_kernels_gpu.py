"""The kernels of csrc/vit.hip one by one, through the C ABI, against the fp64 restatement of tests/dinov2_reference.py, at the
smallest shapes at which each can go wrong.

Two tolerances per kernel.
(1) Against the PLAIN fp64 restatement: max |got - ref| <= 2 x e_emul x max |ref|, e_emul the measured cost of the 16-bit operands
    alone on the very inputs of the case (E_EMUL below; measured by tests/test_dinov2_cpu.py with dinov2_reference.measure_e_emul,
    which also asserts that these constants are what it measures).  The factor 2 covers fp32 accumulation order and fp32 exp / erf.
(2) Against the restatement with the emulation ON, per element, where only fp32 arithmetic differs: terms x 2^-24 x sum |a_i b_i|
    with the term count and the absolute sum of the kernel at hand (each test derives its own).  The comparison is with the emulated
    value BEFORE its final 16-bit store (two values that close can still round to neighbouring 16-bit numbers), so a 16-bit output
    adds the store's own half step, u16 (|ref| + bound)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dinov2_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
U32 = 2.0 ** -24

# e_emul = max |ref(emulate=p) - ref(None)| / max |ref(None)| per case, as dinov2_reference.measure_e_emul(p) gives them on the CPU
E_EMUL = {
    "f16": {"prepare_32to28": 3.434e-04, "prepare_64to28": 3.363e-04, "prepare_16to28": 3.359e-04, "prepare_40x24to28": 3.270e-04,
            "prepare_256to224": 3.127e-04, "prepare_28to28": 3.689e-04, "prepare_f32_32to28": 3.434e-04, "layernorm_128": 4.375e-04,
            "layernorm_1024": 2.854e-04, "attention_2": 3.153e-04, "attention_5": 2.754e-04, "attention_63": 3.474e-04,
            "attention_64": 4.159e-04, "attention_65": 3.604e-04, "attention_256": 2.356e-04, "attention_257": 3.070e-04,
            "attention_258": 4.198e-04, "attention_513": 3.830e-04, "attention_65_big": 2.655e-04, "gelu": 1.490e-08},
    "bf16": {"prepare_32to28": 2.742e-03, "prepare_64to28": 3.337e-03, "prepare_16to28": 2.704e-03, "prepare_40x24to28": 2.606e-03,
             "prepare_256to224": 2.501e-03, "prepare_28to28": 2.951e-03, "prepare_f32_32to28": 2.742e-03, "layernorm_128": 3.715e-03,
             "layernorm_1024": 2.114e-03, "attention_2": 2.758e-03, "attention_5": 2.535e-03, "attention_63": 2.572e-03,
             "attention_64": 2.141e-03, "attention_65": 3.309e-03, "attention_256": 1.921e-03, "attention_257": 2.752e-03,
             "attention_258": 2.887e-03, "attention_513": 2.868e-03, "attention_65_big": 2.306e-03, "gelu": 1.185e-07},
}


def _L():
    import mapdit_amd
    return mapdit_amd._lib


def _fn(name, prec):
    return getattr(_L().lib(), name + ("_f16" if prec == "f16" else ""))


def _check(name, prec, got, plain, emulated, tight):
    """Both tolerances; prints each figure before it asserts."""
    got, plain, emulated = got.double().cpu(), plain.double(), emulated.double()
    e1, lim1 = float((got - plain).abs().max()), 2 * E_EMUL[prec][name] * float(plain.abs().max())
    over = (got - emulated).abs() - (tight + R.UNIT[prec] * (emulated.abs() + tight))
    print(f"{name} {prec}: max err vs fp64 {e1:.3e} (limit {lim1:.3e}); worst (err - tight bound) vs emulation {float(over.max()):.3e}")
    assert torch.isfinite(got).all()
    assert e1 <= lim1, (name, prec, e1, lim1)
    assert float(over.max()) <= 0.0, (name, prec, float(over.max()))


# ---- prepare ------------------------------------------------------------------------------------------------------------------------
def _prepare(prec, images, S):
    L = _L()
    u8 = images.dtype == torch.uint8
    N, H, W = (images.shape[0], images.shape[1], images.shape[2]) if u8 else (images.shape[0], images.shape[2], images.shape[3])
    x = images.contiguous().to(DEV)
    rows = torch.full((N * (S // 14) ** 2, L.VIT_PATCH_K), 7.0, dtype=DTYPES[prec], device=DEV)
    _fn("vit_prepare", prec)(x.data_ptr(), L.VIT_IMG_U8_NHWC if u8 else L.VIT_IMG_F32_NCHW, rows.data_ptr(), N, H, W, S, L.cur_stream())
    torch.cuda.synchronize()
    return rows


def _prepare_tight(images, S):
    """terms x 2^-24 x sum |a_i b_i|: terms = the taps of the widest output pixel + 16 (a weight's evaluation and normalisation, the
    three pointwise steps), the absolute sum = (sum |w_y| |w_x| v / 255 + mean) / std per element."""
    px = R.pixels_255(images)
    my, mx = np.abs(R.aa_matrix(px.shape[2], S)), np.abs(R.aa_matrix(px.shape[3], S))
    terms = int((my > 0).sum(1).max() * (mx > 0).sum(1).max()) + 16
    a = np.einsum("yh,nchx->ncyx", my, np.einsum("xw,nchw->nchx", mx, px)) / 255.0
    a = (a + np.array(R.MEAN)[None, :, None, None]) / np.array(R.STD)[None, :, None, None]
    N, g = a.shape[0], S // 14
    p = a.reshape(N, 3, g, 14, g, 14).transpose(0, 2, 4, 1, 3, 5).reshape(N * g * g, 588)
    out = np.zeros((N * g * g, R.PATCH_K))
    out[:, :588] = p
    return torch.from_numpy(terms * U32 * out)


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("case", ["32to28", "64to28", "16to28", "40x24to28", "256to224"])
def test_prepare_u8(case, prec):
    S = R.RESIZE_CASES[case][2]
    images = R.case_images(case)
    rows = _prepare(prec, images, S)
    assert (rows[:, 588:] == 0).all()                       # the tail of every row
    _check(f"prepare_{case}", prec, rows, R.patch_rows(images, S), R.patch_rows(images, S), _prepare_tight(images, S))


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_prepare_f32_nchw_and_agreement_with_u8(prec):
    images = R.case_images("32to28", f32=True)
    rows = _prepare(prec, images, 28)
    assert (rows[:, 588:] == 0).all()
    _check("prepare_f32_32to28", prec, rows, R.patch_rows(images, 28), R.patch_rows(images, 28), _prepare_tight(images, 28))
    # the same picture as bytes: the two inputs differ by the fp32 rounding of v / 127.5 - 1 and of (x + 1) * 127.5, 2 x 2^-24 x 255
    # each on a pixel, through weights of absolute sum <= 1.7^2, / 255 / std: below 2e-6, far under one 16-bit step -> at most one
    # step apart where a value sits on a rounding boundary
    rows_u8 = _prepare(prec, R.case_images("32to28"), 28)
    d = (rows.double() - rows_u8.double()).abs().cpu()
    step = 2 * R.UNIT[prec] * rows_u8.double().abs().cpu() + 1e-7
    assert (d <= step).all() and float((d > 0).double().mean()) < 0.01, (float(d.max()), float((d > 0).double().mean()))


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_prepare_identity_28(prec):
    """size == H == W: the taps are the identity, the values (v / 255 - mean) / std in fp32, rounded once to the operand format."""
    images = R.case_images("28to28")
    rows = _prepare(prec, images, 28)
    v = images.permute(0, 3, 1, 2).to(torch.float32)
    mean, std = torch.tensor(R.MEAN, dtype=torch.float32)[None, :, None, None], torch.tensor(R.STD, dtype=torch.float32)[None, :, None, None]
    want = ((v / 255.0 - mean) / std).reshape(2, 3, 2, 14, 2, 14).permute(0, 2, 4, 1, 3, 5).reshape(8, 588).to(DTYPES[prec])
    assert torch.equal(rows[:, :588].cpu(), want) and (rows[:, 588:] == 0).all()
    _check("prepare_28to28", prec, rows, R.patch_rows(images, 28), R.patch_rows(images, 28), _prepare_tight(images, 28))


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------
def _layernorm(prec, x, w, b, eps=1e-6, out16=True, ldx=None):
    L = _L()
    M, D = x.shape
    xd, wd, bd = x.contiguous().to(DEV), w.to(DEV), b.to(DEV)
    out = torch.empty(M, D, dtype=DTYPES[prec] if out16 else torch.float32, device=DEV)
    _fn("vit_layernorm", prec)(xd.data_ptr(), D if ldx is None else ldx, wd.data_ptr(), bd.data_ptr(), eps, out.data_ptr(),
                               L.VIT_OUT_16 if out16 else L.VIT_OUT_F32, M, D, L.cur_stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("D", [128, 1024])
def test_layernorm_outlier_rows(D, prec):
    x, w, b = R.case_layernorm(D)
    got = _layernorm(prec, x, w, b)
    ref = R.layernorm(x.double(), w, b)
    # fp32 error.  The mean and the variance are sums of D terms: d(mean) <= D u mean|x|, d(rstd) / rstd <= (D + 8) u; so
    # |dy| <= (D + 8) u (mean|x| rstd |w| + |y - b|) + 4 u (|y| + |b|) for the pointwise steps
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xd - mean) ** 2).mean(-1, keepdim=True) + 1e-6)
    tight = (D + 8) * U32 * (xd.abs().mean(-1, keepdim=True) * rstd * w.double().abs() + (ref - b.double()).abs()) + 4 * U32 * (ref.abs() + b.double().abs())
    _check(f"layernorm_{D}", prec, got, ref, ref, tight)
    got32 = _layernorm(prec, x, w, b, out16=False)          # the fp32 store (the final norm): the fp32 bound alone
    assert ((got32.double().cpu() - ref).abs() <= tight).all()
    # a row's bits do not depend on the number of rows
    alone = _layernorm(prec, x[2:3], w, b)
    many = _layernorm(prec, x.repeat(50, 1), w, b)
    assert torch.equal(alone[0], got[2]) and torch.equal(many[:6], got) and torch.equal(many[-6:], got)
    # rows ldx apart (the CLS rows of a token stream)
    wide = torch.cat([x, torch.full_like(x, 1e4)], dim=1).contiguous()
    strided = torch.empty(6, D, dtype=DTYPES[prec], device=DEV)
    L = _L()
    wd, bd, xs = w.to(DEV), b.to(DEV), wide.to(DEV)
    _fn("vit_layernorm", prec)(xs.data_ptr(), 2 * D, wd.data_ptr(), bd.data_ptr(), 1e-6, strided.data_ptr(), L.VIT_OUT_16, 6, D, L.cur_stream())
    torch.cuda.synchronize()
    assert torch.equal(strided, got)


# ---- attention ------------------------------------------------------------------------------------------------------------------------
def _attention(prec, qkv, heads=2):
    """qkv fp64 [N, T, 3 D] of operand-format values -> 16-bit [N, T, D].  The buffers are exactly N * T rows: a read or a write
    past the last row is outside the allocation."""
    L = _L()
    N, T, D3 = qkv.shape
    q = qkv.to(DTYPES[prec]).contiguous().to(DEV)
    out = torch.full((N, T, D3 // 3), 3.0, dtype=DTYPES[prec], device=DEV)
    _fn("vit_attention", prec)(q.data_ptr(), out.data_ptr(), N, T, heads, 64, L.cur_stream())
    torch.cuda.synchronize()
    return out


def _attention_tight(qkv, prec, heads=2):
    """Per output element, first order.  PV: T + 72 terms (the keys, the online rescales of the tiles, the division) of absolute sum
    A = sum_j p_j |v_j| / sum_j p_j.  The probabilities are rounded to 16 bits relative to the RUNNING maximum, the emulation's
    relative to the final one: up to 2 u16 A between them.  A score is 64 fp32 terms of absolute sum S = sum_d |q_d k_d| / 8, and an
    error ds in a score is a relative error ds in its probability, in the numerator and in the denominator: 2 x 68 u max_j S_j x A."""
    N, T, D3 = qkv.shape
    D = D3 // 3
    _, A = R.attention(qkv, heads, prec, absolute=True)
    q, k = (qkv[:, :, i * D:(i + 1) * D].abs().reshape(N, T, heads, 64).permute(0, 2, 1, 3) for i in range(2))
    S = (torch.einsum("nhqd,nhkd->nhqk", q, k) / 8.0).max(dim=-1).values               # [N, heads, T]
    S = S.permute(0, 2, 1)[:, :, :, None].expand(N, T, heads, 64).reshape(N, T, D)
    return ((T + 72) * U32 + 2 * R.UNIT[prec] + 2 * 68 * U32 * S) * A


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("T", R.ATTN_T)
def test_attention_ragged_T(T, prec):
    qkv = R.case_attention(T, prec)                          # N = 3, 2 heads
    got = _attention(prec, qkv)
    _check(f"attention_{T}", prec, got, R.attention(qkv, 2), R.attention(qkv, 2, prec), _attention_tight(qkv, prec))
    # N = 1: sample 1 alone, the same bits
    alone = _attention(prec, qkv[1:2])
    assert torch.equal(alone[0], got[1])
    # ... and with the neighbours' rows filled with 1e4: a read across the ragged edge would change a bit, not add a small error
    loud = qkv.clone()
    loud[0] = 1e4
    loud[2] = 1e4
    assert torch.equal(_attention(prec, loud)[1], alone[0])


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_attention_large_logits(prec):
    """q and k scaled by 9: logits near +-80 (exp(80) = 5.5e34 would still be finite in fp32, its sum over a row of such not far from
    the edge; exp(2 x 80) between two tiles is not) - the online maximum is what keeps every exp at or below 1."""
    qkv = R.case_attention(65, prec, scale=9.0)
    s = torch.einsum("ntd,nsd->nts", qkv[:, :, :64], qkv[:, :, 128:192]) / 8.0
    assert float(s.abs().max()) > 60.0
    got = _attention(prec, qkv)
    _check("attention_65_big", prec, got, R.attention(qkv, 2), R.attention(qkv, 2, prec), _attention_tight(qkv, prec))


def test_attention_refusals():
    L = _L()
    lib = L.lib()
    buf = torch.zeros(4096, dtype=torch.float16, device=DEV)
    for hd, word in ((32, "head_dim=32"), (72, "head_dim=72")):
        with pytest.raises(L.MapditError) as e:
            lib.vit_attention_f16(buf.data_ptr(), buf.data_ptr(), 1, 4, 2, hd, L.cur_stream())
        assert word in str(e.value) and "head_dim 64 only" in str(e.value)
    with pytest.raises(L.MapditError) as e:
        lib.vit_attention(buf.data_ptr(), buf.data_ptr(), 1, 1, 2, 64, L.cur_stream())
    assert "T=1" in str(e.value) and "T >= 2" in str(e.value)


# ---- GELU, residual, embed, linear ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_gelu_per_element(prec):
    L = _L()
    x = R.case_gelu(prec)                                    # +-0, +-10, the fp16 saturation edge, +-300, 1016 draws of 3 N(0, 1)
    xd = x.to(DTYPES[prec]).to(DEV)
    out = torch.empty_like(xd)
    _fn("vit_gelu", prec)(xd.data_ptr(), out.data_ptr(), x.numel(), L.cur_stream())
    torch.cuda.synchronize()
    ref = R.gelu(x)
    # per element: fp32 erfc and two products (8 u |g|), the 16-bit store (u16 |g|, and half a step of fp16's subnormals, 2^-25)
    tight = 8 * U32 * ref.abs() + 2.0 ** -25
    _check("gelu", prec, out, ref, ref, tight)
    got = out.double().cpu()
    assert got[0] == 0 and got[1] == 0 and got[2] == 10 and abs(got[3]) <= 2.0 ** -24
    assert got[4] == float(x[4]) and got[5] == 0 and got[6] == 300 and got[7] == 0
    inplace = xd.clone()
    _fn("vit_gelu", prec)(inplace.data_ptr(), inplace.data_ptr(), x.numel(), L.cur_stream())
    torch.cuda.synchronize()
    assert torch.equal(inplace, out)


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_residual_per_element(prec):
    L = _L()
    g = torch.Generator().manual_seed(6)
    M, D = 37, 128
    x = (300 * torch.randn(M, D, generator=g)).float()
    y = torch.randn(M, D, generator=g).float()
    gamma = (0.05 + 0.95 * torch.rand(D, generator=g)).float()
    for y16 in (False, True):
        yv = y.to(DTYPES[prec]) if y16 else y
        xd, yd, gd = x.clone().to(DEV), yv.to(DEV), gamma.to(DEV)
        _fn("vit_residual", prec)(xd.data_ptr(), yd.data_ptr(), L.VIT_OUT_16 if y16 else L.VIT_OUT_F32, gd.data_ptr(), M, D, L.cur_stream())
        torch.cuda.synchronize()
        ref = x.double() + gamma.double() * yv.double()
        assert ((xd.double().cpu() - ref).abs() <= U32 * ref.abs()).all()           # one fma: one fp32 rounding


def test_embed_exact():
    L = _L()
    g = torch.Generator().manual_seed(7)
    N, P, D = 3, 4, 128
    patch, cls, pos = torch.randn(N * P, D, generator=g), torch.randn(D, generator=g), torch.randn(P + 1, D, generator=g)
    out = torch.empty(N, P + 1, D, device=DEV)
    pd, cd, sd = patch.to(DEV), cls.to(DEV), pos.to(DEV)
    L.lib().vit_embed(pd.data_ptr(), cd.data_ptr(), sd.data_ptr(), out.data_ptr(), N, P + 1, D, L.cur_stream())
    torch.cuda.synchronize()
    want = torch.cat([cls.reshape(1, 1, D).expand(N, 1, D), patch.reshape(N, P, D)], dim=1) + pos[None]      # one fp32 addition: exact
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("M, Cin, Cout", [(5, 592, 128), (257, 128, 384), (130, 512, 80)])
def test_linear_guards(M, Cin, Cout, prec):
    """The 1 x 1 form of the implicit GEMM: the patch rows' K = 592 (a last K tile of one granule), a row count one past two tiles,
    the 64-wide tile's column guard (Cout = 80) and the 128-wide tile; fp32 and 16-bit stores; K u sum |x||w| as for the convolutions."""
    L = _L()
    g = torch.Generator().manual_seed(M + Cin)
    x = R.rnd(torch.randn(M, Cin, generator=g, dtype=torch.float64), prec)
    w = R.rnd(torch.randn(Cout, Cin, generator=g, dtype=torch.float64) / Cin ** 0.5, prec)
    b = torch.randn(Cout, generator=g).float()
    ref = x @ w.T + b.double()
    tight = 2 * Cin * U32 * (x.abs() @ w.abs().T + b.double().abs())
    xd, wd, bd = x.to(DTYPES[prec]).to(DEV), w.to(DTYPES[prec]).to(DEV), b.to(DEV)
    for out16 in (False, True):
        out = torch.empty(M, Cout, dtype=DTYPES[prec] if out16 else torch.float32, device=DEV)
        _fn("vit_linear", prec)(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), L.VIT_OUT_16 if out16 else L.VIT_OUT_F32, M, Cin, Cout,
                                L.cur_stream())
        torch.cuda.synchronize()
        err = (out.double().cpu() - ref).abs()
        assert (err <= tight + (R.UNIT[prec] * ref.abs() if out16 else 0)).all(), float(err.max())
        if M > 1:                                            # a row alone: the same bits
            one = torch.empty(1, Cout, dtype=out.dtype, device=DEV)
            _fn("vit_linear", prec)(xd[M - 1:].data_ptr(), wd.data_ptr(), bd.data_ptr(), one.data_ptr(), L.VIT_OUT_16 if out16 else L.VIT_OUT_F32, 1,
                                    Cin, Cout, L.cur_stream())
            torch.cuda.synchronize()
            assert torch.equal(one[0], out[M - 1])
