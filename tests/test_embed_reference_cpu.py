"""The references of tests/embed_reference.py checked on the CPU, so that tests/test_embed_kernels_gpu.py does not lean on unverified
helpers: the closed-form backward formulas against fp64 autograd (1e-12), the exactness claims the GPU file's bit-equal assertions rest
on (an fp32 evaluation equals the fp64 one bit for bit), the fp32 emulation of the Fourier argument, and the 16-bit rounding helpers.
"""
import math

import numpy as np
import pytest
import torch

import embed_reference as R
from oracle import dit_oracle as O


def close12(a, b):
    return float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


# ---- the building blocks -------------------------------------------------------------------------------------------------------------
def test_patchify_round_trip_in_fp64():
    rng = np.random.default_rng(1)
    for C_, S, p in [(4, 16, 2), (3, 12, 2), (1, 16, 4), (4, 20, 4), (4, 16, 8)]:
        x = R.grid((3, C_, S, S), rng)
        h = O.patchify(x, p)
        assert h.dtype == torch.float64 and torch.equal(O.unpatchify(h, S, p), x)
        rows = R.patch_rows(x, p)
        assert rows.shape == (3 * (S // p) ** 2, p * p * C_ + 1) and float(rows[:, -1].min()) == 1.0 == float(rows[:, -1].max())


def test_grid_is_exact_in_every_format():
    g = R.grid((4096,), np.random.default_rng(2))
    assert float(g.min()) >= -2.0 and float(g.max()) <= 2.0 and torch.equal(g * 64, (g * 64).round())
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        assert torch.equal(g.to(dt).double(), g)
    allv = torch.arange(-128, 129, dtype=torch.float64) / 64                          # every value of the generator, not a sample
    assert torch.equal(allv.bfloat16().double(), allv) and torch.equal(allv.half().double(), allv)


# ---- backward formulas against fp64 autograd -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,rows", [(1, 128, 11), (5, 384, 11), (33, 128, 1001)])
def test_cond_combine_backward_formula(n, D, rows):
    g = torch.Generator().manual_seed(n)
    temb, table = torch.randn(n, D, generator=g, dtype=torch.float64), torch.randn(rows, D, generator=g, dtype=torch.float64)
    y = torch.randint(0, min(rows, 4), (n,), generator=g)                              # duplicates
    y[0] = rows - 1
    dcs, dcd = torch.randn(n, D, generator=g, dtype=torch.float64), torch.randn(n, D, generator=g, dtype=torch.float64)
    lt, ltab = temb.clone().requires_grad_(True), table.clone().requires_grad_(True)
    c = R.cond_combine_ref(lt, ltab, y)
    assert close12(c.detach(), (temb + table[y]) * math.sqrt(0.5))
    ((O.mp_silu(c) * dcs).sum() + (c * dcd).sum()).backward()
    dtemb, dtable, terms = R.cond_combine_bwd_ref(c.detach(), dcs, dcd, y, rows)
    assert close12(dtemb, lt.grad) and close12(dtable, ltab.grad)
    assert float(terms.min()) >= 0 and bool((terms * math.sqrt(0.5) + 1e-15 >= dtemb.abs()).all())


@pytest.mark.parametrize("shape", [(3, 4, 16, 2), (16, 3, 6, 2), (2, 4, 20, 4), (2, 4, 16, 8)])
def test_final_out_backward_formula(shape):
    N, C_, S, p = shape
    P, T = p * p * C_, (S // p) ** 2
    g = torch.Generator().manual_seed(S)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    leaves = [z.requires_grad_(True) for z in (rn(N * T, 2 * P), rn(N, 8), rn(N, 8), rn(8), rn(8))]
    lin, am, asg, rm, rs = leaves
    gm, gs = R.gates_ref(am, rm), R.gates_ref(asg, rs)
    out = R.final_out_ref(lin, gm, gs, N, S, p)
    # the forward itself, restated without the oracle's helpers: out[n, chunk C + c, h p + p1, w p + p2] = lin[n T + h g + w, chunk P + (p1 p + p2) C + c] gate
    n_, ch, yy, xx = 1 % N, C_ + C_ - 1, S - 1, p - 1 if p > 1 else 0
    tok, j = (yy // p) * (S // p) + xx // p, ((yy % p) * p + xx % p) * C_ + (ch - C_)
    assert close12(out[n_, ch, yy, xx].detach(), (lin[n_ * T + tok, P + j] * gs[n_]).detach())
    dout = rn(*out.shape)
    out.backward(dout)
    r = R.final_out_bwd_ref(dout, lin.detach(), am.detach(), asg.detach(), rm.detach(), rs.detach(), gm.detach(), gs.detach(), p)
    for got, want in ((r["dlin"], lin.grad), (r["da_mean"], am.grad), (r["da_sigma"], asg.grad), (r["dref_mean"], rm.grad),
                      (r["dref_sigma"], rs.grad)):
        assert close12(got, want)
    # the quantities the error bounds are stated in dominate the results they bound
    assert bool((r["abs_mean"] * r["kap_mean"] * rm.detach().abs().max() + 1e-15 >= r["da_mean"].abs().max(1).values).all())


@pytest.mark.parametrize("n,C_,HW", [(2, 4, 64), (6, 4, 64), (10, 3, 25)])
@pytest.mark.parametrize("s", [1.5, 0.0, -0.5, 1.37])
def test_cfg_combine_backward_formula(n, C_, HW, s):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, 2 * C_, HW, generator=g, dtype=torch.float64).requires_grad_(True)
    out = R.cfg_combine_ref(x, C_, s)
    half = n // 2
    assert torch.equal(out[:half, :C_], out[half:, :C_]) and torch.equal(out[:, C_:], x[:, C_:].detach())
    dout = torch.randn(n, 2 * C_, HW, generator=g, dtype=torch.float64)
    out.backward(dout)
    din = R.cfg_combine_bwd_ref(dout, C_, s)
    assert close12(din, x.grad)
    # the adjoint identity the GPU test evaluates on device results
    assert abs(float((dout * out.detach()).sum() - (din * x.detach()).sum())) <= 1e-10 * float((dout * out.detach()).abs().sum())


# ---- exactness claims ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,S,p", [(3, 12, 2), (4, 16, 2), (8, 8, 2), (4, 20, 4), (4, 16, 8)], ids=["P13", "P17", "P33", "P65", "P257"])
def test_grid_sums_of_patch_embedding_are_exact_in_fp32(C_, S, p):
    rng = np.random.default_rng([C_, S, p])
    N, D, T = 3, 128, (S // p) ** 2
    x, w, pos = R.grid((N, C_, S, S), rng), R.grid((D, p * p * C_ + 1), rng), R.grid((T, D), rng)
    want = R.patch_embed_sum(x, w, pos, p)
    got32 = R.patch_embed_sum(x.float(), w.float(), pos.float(), p)
    assert got32.dtype == torch.float32 and torch.equal(got32.double(), want)
    # near the worst case of the claim, not a sample: 257 products (127/64)^2 (lowest bit 2^-12 set), one sign, plus 2 - a sequential fp32 sum
    acc, v = np.float32(0), np.float32(127 / 64)
    for _ in range(257):
        acc = np.float32(acc + np.float32(v * v))
    assert float(np.float32(acc + np.float32(2.0))) == 257 * 16129 / 4096 + 2
    # out_scale 0: one rounding, of the exact sum times the fp32 constant
    mp = R.patch_embed_mp(x, w, pos, p)
    one = (want.float() * np.float32(R.C5)).double()
    assert float(((one - mp) / mp.abs().clamp_min(1e-30)).abs().max()) < 2.0 ** -23


def test_cfg_combine_with_dyadic_scales_is_exact_in_fp32():
    rng = np.random.default_rng(5)
    x, dout = R.grid((6, 8, 64), rng), R.grid((6, 8, 64), rng)
    for s in (1.5, 1.0, 0.0, 4.0, -0.5):
        assert torch.equal(R.cfg_combine_ref(x.float(), 4, s).double(), R.cfg_combine_ref(x, 4, s))
        assert torch.equal(R.cfg_combine_bwd_ref(dout.float(), 4, s).double(), R.cfg_combine_bwd_ref(dout, 4, s))


def test_gate_one_half_case_is_exact_in_fp32():
    """a = 0: the gate is sigmoid(0) = 1 / (1 + 1) = 0.5 in any format, so out = 0.5 lin and dlin = grad_scale 0.5 dout are exact in fp32
    and, on grid operands with a power-of-two grad_scale, in both 16-bit formats."""
    rng = np.random.default_rng(6)
    N, C_, S, p = 2, 4, 8, 2
    lin, dout = R.grid((N * 16, 32), rng), R.grid((N, 8, S, S), rng)
    z = torch.zeros(N, 8, dtype=torch.float64)
    ref = R.grid((8,), rng)
    gate = R.gates_ref(z, ref)
    assert torch.equal(gate, torch.full((N,), 0.5, dtype=torch.float64)) and torch.equal(R.gates_ref(z.float(), ref.float()).double(), gate)
    out = R.final_out_ref(lin, gate, gate, N, S, p)
    assert torch.equal(R.final_out_ref(lin.float(), gate.float(), gate.float(), N, S, p).double(), out)
    r = R.final_out_bwd_ref(dout, lin, z, z, ref, ref, gate, gate, p)
    for gscale in (1.0, 2.0 ** -3):
        d = r["dlin"] * gscale
        assert torch.equal(d.bfloat16().double(), d) and torch.equal(d.half().double(), d)
    assert float(r["dref_mean"].abs().max()) == 0.0 == float(r["dref_sigma"].abs().max())
    # dg, the only long sum of the backward: a multiple of 2^-12 whose terms sum to less than 2^12 in magnitude - exact in fp32 in any order
    assert float(r["abs_mean"].max()) < 4096 and float(r["abs_sigma"].max()) < 4096


# ---- Fourier argument --------------------------------------------------------------------------------------------------------------------
def test_fourier_argument_emulation_matches_torch():
    g = torch.Generator().manual_seed(14)
    scale, shift = 2 * math.pi * torch.randn(256, generator=g), 2 * math.pi * torch.rand(256, generator=g)
    t = torch.arange(0, 1000)
    want = torch.outer(t.float(), scale) + shift
    got = R.fourier_arg_f32(t.numpy(), scale.numpy(), shift.numpy())
    assert got.dtype == np.float32 and np.array_equal(got, want.numpy())
    assert float(np.abs(got).max()) > 1e4                                           # the range where a fused multiply-add would show
    fused = (t.double()[:, None] * scale.double()[None, :] + shift.double()[None, :]).float().numpy()
    assert np.mean(fused != got) > 0.1                                              # ... and does: the emulation is not vacuous


# ---- 16-bit helpers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_round16_is_the_single_rounding(fmt):
    dt = R.FORMATS[fmt]["dtype"]
    g = torch.Generator().manual_seed(3)
    v32 = torch.cat([torch.randn(20000, generator=g) * 3, torch.randn(2000, generator=g) * 1e-3, torch.tensor([0.0, 1.0, -1.0, 0.5, 3.0])])
    # from fp32 torch rounds once: the helper must agree everywhere
    assert np.array_equal(R.round16(v32.double().numpy(), fmt), v32.to(dt).double().numpy())
    one, u = 1.0, float(R.ulp16(1.0, fmt))
    assert u == 2.0 ** -R.FORMATS[fmt]["mant"] and float(R.ulp16(0.99, fmt)) == u / 2 and float(R.ulp16(2.0, fmt)) == 2 * u
    assert float(R.round16(one + u / 2, fmt)) == one and float(R.round16(one + 3 * u / 2, fmt)) == one + 2 * u      # ties to even
    # a double just above a tie: through fp32 it would land ON the tie and round down
    assert float(R.round16(one + u / 2 + 2.0 ** -40, fmt)) == one + u
    worst, share = R.ulp_report(np.array([one + u, one]), np.array([one + u / 2 + 2.0 ** -40, one + 0.4 * u]), fmt)
    assert share == 0.0 and 0.4 <= worst <= 0.5
