"""The REPA kernels one by one against fp64 (tests/repa_reference.py): the cosine loss with its gradient, bias + SiLU forward and
backward with the deterministic bias column sum, and the gradient-stream add behind mapdit_engine_set_hidden_grad.

Tolerances are operation-count bounds of the kernels' own order of operations (u = 2^-24; see each test), not fits to the output:
 * cosine loss: repa_reference.cos_loss_bound (row sums of 8 ceil(P / 512) sequential fmas and a six-level butterfly, two square
   roots, two divisions, the per-sample sum of ceil(T / 4) + 3 additions), doubled for second-order terms;
 * SiLU: exp(-x) is one product with log2(e) (relative error |x| u in the result) and a one-ulp exp2, so sigmoid carries at most
   (2 |x| + 7) u and silu one product more; its derivative s (1 + x (1 - s)) four operations on top of s's error, scaled by
   s (1 + |x|); a 16-bit result may then sit one rounding of the 16-bit format away from the rounded fp64 value;
 * column sum of M rows: 32 sequential additions per wave and chunk, 3 to join the waves, one per chunk, the scale: gamma_(36 + chunks)
   relative to the sum of magnitudes;
 * stream add: equality with the correctly rounded fp64 sum, bit for bit."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import repa_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = R.U32
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
U16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
TINY16 = {"bf16": 2.0 ** -133, "f16": 2.0 ** -24}           # the subnormal spacing


def lib():
    from mapdit_amd import _lib as L
    return L, L.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def fn(l, name, prec):
    return getattr(l, name + ("_f16" if prec == "f16" else ""))


# ---- cosine loss ------------------------------------------------------------------------------------------------------------------
def cos_case(Rr, T, P, kind):
    rng = np.random.default_rng(100 + Rr + P)
    z = rng.standard_normal((Rr, P))
    f = rng.standard_normal((Rr, P))
    z[0] *= 1e4
    f[1 % Rr] *= 1e4
    z[2 % Rr] *= 1e-6
    if kind == "f32":
        f[3 % Rr] *= 1e-6                                   # (fp16 holds no row of that size: the fp32 form alone)
    z[Rr - 1] = 0.0                                         # an all-zero row in z ...
    f[Rr - 2] = 0.0                                         # ... and one in f
    g = rng.standard_normal(Rr // T)
    z = z.astype(np.float32)
    f = f.astype(np.float16 if kind == "f16" else np.float32)
    return z, f, g.astype(np.float32)


@pytest.mark.parametrize("kind", ["f16", "f32"])
@pytest.mark.parametrize("shape", [(5, 5, 8), (130, 65, 768), (21, 7, 1000)])
def test_cos_loss_and_gradient_against_fp64(shape, kind):
    L, l = lib()
    Rr, T, P = shape
    z, f, g = cos_case(Rr, T, P, kind)
    scale = 0.5
    zt, ft, gt = torch.from_numpy(z).to(DEV), torch.from_numpy(f).to(DEV), torch.from_numpy(g).to(DEV)
    loss, dz = torch.empty(Rr // T, device=DEV), torch.empty(Rr, P, device=DEV)
    k = L.REPA_F_F16 if kind == "f16" else L.REPA_F_F32
    l.repa_cos_loss(zt.data_ptr(), ft.data_ptr(), k, gt.data_ptr(), scale, loss.data_ptr(), dz.data_ptr(), Rr, T, P, stream())
    torch.cuda.synchronize()
    want_l, want_dz = R.cos_loss(z, f, T, g.astype(np.float64) * scale)
    bl, bdz = R.cos_loss_bound(z, f, T, g.astype(np.float64) * scale)
    got_l, got_dz = loss.double().cpu().numpy(), dz.double().cpu().numpy()
    assert np.isfinite(got_l).all() and np.isfinite(got_dz).all()
    el, ed = np.abs(got_l - want_l), np.abs(got_dz - want_dz)
    print(f"{shape} {kind}: loss err / bound {float((el / (2 * bl + 1e-300)).max()):.3f}, dz err / bound {float((ed / (2 * bdz + 1e-300)).max()):.3f}")
    assert (el <= 2 * bl + 1e-45).all()
    assert (ed <= 2 * bdz + 1e-45).all()
    # the zero rows add nothing: the loss of the same input with those rows' partners zeroed too is the same number
    z2, f2 = z.copy(), f.copy()
    f2[Rr - 1], z2[Rr - 2] = 0, 0
    assert np.array_equal(R.cos_loss(z2, f2, T)[0], R.cos_loss(z, f, T)[0])
    assert (got_dz[Rr - 2] == 0).all()                      # f = 0: no direction to pull toward
    # gscale = NULL is scale alone, dz = NULL / loss = NULL are honoured, and two runs give the same bits
    loss2, dz2 = torch.empty_like(loss), torch.empty_like(dz)
    l.repa_cos_loss(zt.data_ptr(), ft.data_ptr(), k, None, 1.0, loss2.data_ptr(), None, Rr, T, P, stream())
    l.repa_cos_loss(zt.data_ptr(), ft.data_ptr(), k, gt.data_ptr(), scale, None, dz2.data_ptr(), Rr, T, P, stream())
    torch.cuda.synchronize()
    assert torch.equal(loss2, loss) and torch.equal(dz2, dz)


def test_cos_loss_refusals():
    L, l = lib()
    z = torch.zeros(16, 16, device=DEV)
    out = torch.zeros(16, device=DEV)
    for Rr, T, P, word in ((16, 5, 16, "samples"), (16, 4, 12, "multiple of 8"), (16, 0, 16, "samples")):
        with pytest.raises(L.MapditError, match=word):
            l.repa_cos_loss(z.data_ptr(), z.data_ptr(), L.REPA_F_F32, None, 1.0, out.data_ptr(), None, Rr, T, P, stream())
    with pytest.raises(L.MapditError, match="f_kind"):
        l.repa_cos_loss(z.data_ptr(), z.data_ptr(), 7, None, 1.0, out.data_ptr(), None, 16, 4, 16, stream())


# ---- bias + SiLU --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("C_", [16, 2048])
@pytest.mark.parametrize("M", [1, 7, 300])
def test_bias_silu_forward_backward_and_column_sum(M, C_, prec):
    L, l = lib()
    rng = np.random.default_rng(M * 31 + C_)
    acc = (3.0 * rng.standard_normal((M, C_))).astype(np.float32)
    acc.reshape(-1)[:4] = [0.0, 30.0, -30.0, -100.0]
    bias = rng.standard_normal(C_).astype(np.float32)
    dact = rng.standard_normal((M, C_)).astype(np.float32)
    alpha, bscale = 4.0, 0.25
    u16, tiny = U16[prec], TINY16[prec]

    pre = torch.from_numpy(acc).to(DEV)
    bt = torch.from_numpy(bias).to(DEV)
    act = torch.empty(M, C_, dtype=DT[prec], device=DEV)
    fn(l, "repa_bias_silu_fwd", prec)(pre.data_ptr(), bt.data_ptr(), act.data_ptr(), M, C_, stream())
    torch.cuda.synchronize()
    pre64 = acc.astype(np.float64) + bias.astype(np.float64)
    assert np.array_equal(pre.cpu().numpy(), pre64.astype(np.float32))          # one fp32 addition: the correctly rounded sum
    x = pre.double().cpu().numpy()                                              # the kernels' own pre-activation from here on
    want = R.silu(x)
    e32 = (2 * np.abs(x) + 8) * U * np.abs(want)
    err = np.abs(act.double().cpu().numpy() - want)
    assert (err <= u16 * np.abs(want) + 2 * e32 + tiny).all(), float((err / (u16 * np.abs(want) + 2 * e32 + tiny)).max())
    # the bias alone (act = NULL) writes the same pre-activation
    pre_b = torch.from_numpy(acc).to(DEV)
    fn(l, "repa_bias_silu_fwd", prec)(pre_b.data_ptr(), bt.data_ptr(), None, M, C_, stream())
    assert torch.equal(pre_b, pre)

    nparts = -(-M // L.REPA_PART_ROWS)
    dt_ = torch.from_numpy(dact).to(DEV)
    outs = []
    for _ in range(2):
        dpre16 = torch.empty(M, C_, dtype=DT[prec], device=DEV)
        db = torch.full((C_,), 3.0, device=DEV)
        part = torch.empty(nparts * C_, device=DEV)
        fn(l, "repa_bias_silu_bwd", prec)(dt_.data_ptr(), pre.data_ptr(), dpre16.data_ptr(), db.data_ptr(), part.data_ptr(), alpha, bscale, 1, M, C_,
                                          stream())
        db0 = torch.full((C_,), 3.0, device=DEV)
        fn(l, "repa_bias_silu_bwd", prec)(dt_.data_ptr(), pre.data_ptr(), None, db0.data_ptr(), part.data_ptr(), alpha, bscale, 0, M, C_, stream())
        torch.cuda.synchronize()
        outs.append((dpre16, db, db0))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))              # a fixed order, no atomics: the same bits
    dpre16, db, db0 = outs[0]
    s = R.sigmoid(x)
    want_d = alpha * dact.astype(np.float64) * R.dsilu(x)
    e32 = np.abs(alpha * dact) * s * (1 + np.abs(x)) * (2 * np.abs(x) + 13) * U
    err = np.abs(dpre16.double().cpu().numpy() - want_d)
    assert (err <= u16 * np.abs(want_d) + 2 * e32 + tiny).all(), float((err / (u16 * np.abs(want_d) + 2 * e32 + tiny)).max())
    k = 36 + nparts
    gam = k * U / (1 - k * U)
    want_b = bscale * want_d.sum(0)
    lim = bscale * (gam * np.abs(want_d).sum(0) + 2 * e32.sum(0)) + U * np.abs(want_b)
    assert (np.abs(db0.double().cpu().numpy() - want_b) <= lim + 1e-30).all()
    assert (np.abs(db.double().cpu().numpy() - (3.0 + want_b)) <= lim + U * (3.0 + np.abs(want_b)) + 1e-30).all()     # accumulate: one more addition
    # pre = NULL: the layer without activation, dpre = alpha * dact
    dlin = torch.empty(M, C_, dtype=DT[prec], device=DEV)
    fn(l, "repa_bias_silu_bwd", prec)(dt_.data_ptr(), None, dlin.data_ptr(), db0.data_ptr(), part.data_ptr(), alpha, bscale, 0, M, C_, stream())
    torch.cuda.synchronize()
    assert np.array_equal(dlin.double().cpu().numpy(), R.round16(alpha * dact.astype(np.float64), prec))


# ---- the gradient-stream add --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_stream_add_is_the_correctly_rounded_sum(prec):
    L, l = lib()
    n = 4096 + 8                                            # more than one workgroup, a last one that is part empty
    rng = np.random.default_rng(9)
    # (1) a power-of-two alpha and representable sums: small integers
    a = rng.integers(-60, 60, n).astype(np.float64)
    d = rng.integers(-30, 30, n).astype(np.float64)
    out = torch.from_numpy(a).to(DT[prec]).to(DEV)
    l_add = fn(l, "repa_stream_add", prec)
    l_add(out.data_ptr(), torch.from_numpy(d.astype(np.float32)).to(DEV).data_ptr(), 2.0, n, stream())
    torch.cuda.synchronize()
    assert np.array_equal(out.double().cpu().numpy(), a + 2.0 * d)
    # (2) anything else: the fp64 sum rounded once.  Ties and near-ties of the 16-bit grid that a rounding through fp32 gets wrong sit
    # in front: x + alpha d just above the midpoint of two neighbours by less than an fp32 ulp.
    x16 = R.round16(rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n)), prec)
    dh = (rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))).astype(np.float32)
    half = U16[prec]                                        # half a spacing at 1.0
    x16[:4] = [1.0, 1.0, -1.0, 1.0]
    dh[:4] = np.array([half * (1 + 2.0 ** -20), half, -half * (1 + 2.0 ** -20), half * (1 - 2.0 ** -20)], np.float64).astype(np.float32)
    alpha = np.float32(1.0 + 2.0 ** -12)
    dh[:4] = (dh[:4].astype(np.float64)).astype(np.float32)
    out = torch.from_numpy(x16).to(DT[prec]).to(DEV)
    assert np.array_equal(out.double().cpu().numpy(), x16)
    l_add(out.data_ptr(), torch.from_numpy(dh).to(DEV).data_ptr(), float(alpha), n, stream())
    torch.cuda.synchronize()
    want = R.round16(x16 + np.float64(alpha) * dh.astype(np.float64), prec)
    assert np.array_equal(out.double().cpu().numpy(), want)
    through_f32 = R.round16((x16 + np.float64(alpha) * dh.astype(np.float64)).astype(np.float32).astype(np.float64), prec)
    print(f"{prec}: {int((through_f32 != want).sum())} of {n} sums would differ after a rounding through fp32")
    with pytest.raises(L.MapditError, match="multiple of 8"):
        l_add(out.data_ptr(), out.data_ptr(), 1.0, 12, stream())


def test_stream_add_f32():
    L, l = lib()
    n = 1028
    rng = np.random.default_rng(10)
    a, d = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    out = torch.from_numpy(a).to(DEV)
    l.repa_stream_add_f32(out.data_ptr(), torch.from_numpy(d).to(DEV).data_ptr(), 1.5, n, stream())
    torch.cuda.synchronize()
    want = (a.astype(np.float64) + 1.5 * d.astype(np.float64)).astype(np.float32)        # one fma: the correctly rounded fp32 sum
    assert np.array_equal(out.cpu().numpy(), want)
