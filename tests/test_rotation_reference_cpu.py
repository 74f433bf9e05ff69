"""The references and bounds of tests/rotation_reference.py checked on the CPU, so that tests/test_rotation_kernels_gpu.py does not lean on
unverified helpers:

(a) coef followed by modulate IS oracle.dit_oracle.modulate_rot (fp64, 1e-13), and the backward stages composed (resid_mod_bwd_rot, then
    coef_bwd) are fp64 autograd through mp_sum and modulate_rot (1e-11) - the per-stage GPU checks add up to the oracle's semantics;
    the AdaLN form likewise against autograd through mp_sum and modulate.
(b) at theta = 0 or g = 0, coef gives A = scale exactly and B = 0.
(c) for every GPU case's own operands a plain numpy float32 evaluation (float32 arithmetic, sums sequential over t, np.float32 sin / cos of
    the fp32 product g theta) lies inside every bound with ratio <= 0.5: a bound that honest fp32 arithmetic cannot meet is a wrong bound.
    A 16-bit output is held to that at the fp32 value in front of its store (the bound's fp32 part e); the stored value itself is held to
    ratio <= 1, because the store's share of the bound, half a unit in the last place, is exact and a correct rounding attains it.
"""
import numpy as np
import pytest
import torch

import embed_reference as E
import rotation_reference as R
from oracle import dit_oracle as O

FMTS = ["bf16", "f16"]
F = np.float32
HALF = 0.5


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1.0, float(np.abs(b).max())))


def to16(v32, fmt):
    """fp32 array -> the 16-bit format (round to nearest even, what the device's conversion does) -> float64."""
    return torch.from_numpy(np.ascontiguousarray(v32, dtype=np.float32)).to(E.FORMATS[fmt]["dtype"]).double().numpy()


def swap32(a):
    return R.pairswap(a)


def seqsum(terms, axis):
    """float32 sum in index order along `axis`."""
    return np.take(np.cumsum(terms, axis=axis, dtype=np.float32), -1, axis=axis)


# ---- (a) the restatements against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", R.COEF_DS)
def test_coef_then_modulate_is_the_oracle(D):
    c = R.coef_case(D)
    x = np.random.default_rng(D).standard_normal((R.COEF_N, 5, D))
    A, B = R.coef(c["theta"], c["scale"], c["g"])
    y, _ = R.modulate(x, A, B)
    want = O.modulate_rot(t64(x), t64(c["theta"]), t64(c["scale"]), c["g"]).numpy()
    assert rel(y, want) <= 1e-13


@pytest.mark.parametrize("n,T,D", [(2, 7, 8), (3, 5, 136)])
def test_backward_stages_compose_to_autograd(n, T, D):
    rng = np.random.default_rng([n, T, D])
    x_up, y_up, dxm, dxo = (rng.standard_normal((n, T, D)) for _ in range(4))
    g_up, scale, theta, g = rng.standard_normal((n, D)), rng.standard_normal((n, D)) + 1, rng.uniform(-3, 3, (n, D // 2)), 0.83
    leaves = [t64(v).requires_grad_(True) for v in (x_up, y_up, g_up, theta, scale, np.array(g))]
    xu, yu, gu, th, sc, gg = leaves
    xp = O.mp_sum(xu, gu.unsqueeze(1) * yu, 0.3)
    u = O.modulate_rot(xp, th, sc, gg)
    ca, cb = 0.7 / np.sqrt(0.58), 0.3 / np.sqrt(0.58)
    ((u * t64(dxm)).sum() + (xp * (ca * t64(dxo))).sum()).backward()
    A, B = R.coef(theta, scale, g)
    r = R.resid_mod_bwd_rot(dxo, dxm, xp.detach().numpy(), A, B, y_up, g_up, ca, cb)
    b = R.coef_bwd(r["dA"], r["dB"], theta, scale, g)
    assert rel(ca * r["dx"], xu.grad.numpy()) <= 1e-11
    assert rel(r["dy_up"], yu.grad.numpy()) <= 1e-11
    assert rel(r["dg_up"], gu.grad.numpy()) <= 1e-11
    assert rel(b["dtheta"], th.grad.numpy()) <= 1e-11
    assert rel(b["dscale"], sc.grad.numpy()) <= 1e-11
    assert rel(b["gterm"].sum(), gg.grad.numpy()) <= 1e-11
    # the parts switched off: modulate only and residual only are the same formulas with the other input at zero
    r5a = R.resid_mod_bwd_rot(None, dxm, xp.detach().numpy(), A, B, None, None, ca, cb)
    assert rel(r5a["dx"], r["dx"] - ca * dxo) <= 1e-13 and np.array_equal(r5a["dA"], r["dA"])
    r5b = R.resid_mod_bwd_rot(dxo, None, None, None, None, y_up, g_up, ca, cb)
    assert np.array_equal(r5b["dx"], ca * dxo) and "dA" not in r5b


def test_adaln_backward_is_autograd():
    n, T, D, cols = 2, 6, 256, 128
    rng = np.random.default_rng(11)
    x_up, y_up, dxm, dxo = (rng.standard_normal((n, T, D)) for _ in range(4))
    g_up, scale, shift, g = rng.standard_normal((n, D)), rng.standard_normal((n, D)), rng.standard_normal((n, D)), 0.37
    xu, yu, gu, sh, sc, gg = [t64(v).requires_grad_(True) for v in (x_up, y_up, g_up, shift, scale, np.array(g))]
    xp = O.mp_sum(xu, gu.unsqueeze(1) * yu, 0.3)
    u = O.modulate(xp, sh, sc, gg)
    ca, cb = 0.7 / np.sqrt(0.58), 0.3 / np.sqrt(0.58)
    ((u * t64(dxm)).sum() + (xp * (ca * t64(dxo))).sum()).backward()
    r = R.resid_mod_bwd_adaln(dxo, dxm, xp.detach().numpy(), shift, scale, g, y_up, g_up, ca, cb, cols)
    assert r["dgain_part"].shape == (n, D // cols)
    for got, want in ((ca * r["dx"], xu.grad), (r["dy_up"], yu.grad), (r["dg_up"], gu.grad), (r["dshift"], sh.grad), (r["dscale"], sc.grad),
                      (r["dgain_part"].sum(), gg.grad)):
        assert rel(got, want.numpy()) <= 1e-11


# ---- (b) the exact cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", R.COEF_DS)
def test_coef_is_scale_at_zero_angle(D):
    c = R.coef_case(D)
    A, B = R.coef(c["theta"], c["scale"], 0.0)
    assert np.array_equal(A, c["scale"]) and not B.any()
    A, B = R.coef(c["theta"], c["scale"], c["g"])
    assert not c["theta"][1].any() and np.array_equal(A[1], c["scale"][1]) and not B[1].any() and B[0].any()


def test_operands_are_what_the_kernels_receive():
    """Every generated operand is an fp32 value; the 16-bit ones are values of their format."""
    for fmt in FMTS:
        for name in R.RMB_CASES:
            o = R.rmb_case(name, fmt)
            for k, v in o.items():
                if isinstance(v, np.ndarray):
                    assert np.array_equal(R.f32(v), v), (name, k)
            for k in ("dxm", "y_up") + (("dxo",) if R.RMB_CASES[name]["dxo"] == "16" else ()):
                if o[k] is not None:
                    assert np.array_equal(E.round16(o[k], fmt), o[k]), (name, k)
        e = R.epilogue_case(64, fmt)
        assert np.array_equal(E.round16(e["a"], fmt), e["a"]) and np.array_equal(E.round16(e["b"], fmt), e["b"])
    assert R.CA == float(F(R.CA)) and R.RMB_GAIN == float(F(R.RMB_GAIN)) and all(g == float(F(g)) for g in R.ALL_GAINS)


# ---- (c) honest fp32 inside every bound ------------------------------------------------------------------------------------------------------
def coef_f32(theta, scale, g):
    ang = (F(g) * theta.astype(F)).astype(F)
    c, s = np.cos(ang), np.sin(ang)
    assert c.dtype == F and s.dtype == F
    sc = scale.astype(F)
    A = np.repeat(c, 2, axis=-1) * sc
    B = np.repeat(s, 2, axis=-1) * swap32(sc)
    B[..., 0::2] *= F(-1)
    return A, B, c, s


def modulate_f32(x, A, B):
    x, A, B = x.astype(F), A.astype(F), B.astype(F)
    y = x * A[:, None, :] + swap32(x) * B[:, None, :]
    assert y.dtype == F
    return y


def show(what, r):
    print("ratio", what, " ".join(f"{k} {v:.3f}" for k, v in r.items()))


@pytest.mark.parametrize("D", R.COEF_DS)
def test_fp32_coefficients_within_half_the_bound(D):
    c = R.coef_case(D)
    for g in (c["g"], 0.0):
        A, B, _, _ = coef_f32(c["theta"], c["scale"], g)
        r = R.coef_ratios(c["theta"], c["scale"], g, A, B)
        show(f"coef D={D} g={g}", r)
        assert max(r.values()) <= HALF
    a = R.coef_all_case(D)
    for s, g in enumerate(a["gains"]):
        A, B, _, _ = coef_f32(a["theta"][s], a["scale"][s], g)
        assert max(R.coef_ratios(a["theta"][s], a["scale"][s], g, A, B).values()) <= HALF


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", R.MOD_SHAPES)
def test_fp32_modulate_within_half_the_bound_and_mutants_outside(shape, fmt):
    c = R.modulate_case(*shape)
    y32 = modulate_f32(c["x"], c["A"], c["B"])
    got = to16(y32, fmt)
    r32, r = R.modulate_ratio(c, y32, None), R.modulate_ratio(c, got, fmt)
    m = R.modulate_mutant_ratios(c, got, fmt)
    show(f"modulate {shape} {fmt}", dict(y_fp32=r32, y=r, **m))
    assert r32 <= HALF and r <= 1.0
    assert min(m.values()) > 100.0                      # a swapped partner or a flipped sign: orders of magnitude outside


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("rows", R.EPI_ROWS)
def test_fp32_epilogue_modulate_within_half_the_bound(rows, fmt):
    """The RESID epilogue's xm from an fp32 xout = ca x + cb gate acc (acc: the exact product rounded to fp32)."""
    e = R.epilogue_case(rows, fmt)
    acc = (e["a"] @ e["b"].T).astype(F)
    gate = np.repeat(e["gate"].astype(F), rows, axis=0)
    xout = (F(R.CB) * gate) * acc + F(R.CA) * e["x"].astype(F)
    s = R.EPI_M // rows
    c = dict(x=xout.astype(np.float64).reshape(s, rows, R.EPI_N), A=e["A"], B=e["B"])
    y32 = modulate_f32(c["x"], c["A"], c["B"])
    got = to16(y32, fmt)
    r32, r = R.modulate_ratio(c, y32, None), R.modulate_ratio(c, got, fmt)
    show(f"epilogue rows={rows} {fmt}", dict(xm_fp32=r32, xm=r))
    assert r32 <= HALF and r <= 1.0 and min(R.modulate_mutant_ratios(c, got, fmt).values()) > 100.0


def rmb_f32(o, fmt, rot, cols, dx32):
    """resid_mod_bwd in numpy float32, the column sums sequential over t; the 16-bit outputs rounded from the fp32 values (fmt None: left
    as those fp32 values)."""
    to16 = (lambda v, f: v.astype(np.float64)) if fmt is None else globals()["to16"]
    n, T, D = o["x"].shape
    ca, cb = F(o["ca"]), F(o["cb"])
    dx = np.zeros((n, T, D), dtype=F)
    got = {}
    if o["dxo"] is not None:
        dx = ca * o["dxo"].astype(F)
    if o["dxm"] is not None:
        dm, x, sc, sh = o["dxm"].astype(F), o["x"].astype(F), o["scale"].astype(F)[:, None, :], o["shift"].astype(F)[:, None, :]
        if rot:
            dx = dx + (sc * dm + swap32(sh * dm))
            got.update(dA=seqsum(x * dm, 1), dB=seqsum(swap32(x) * dm, 1))
        else:
            g = F(o["gain"])
            den = np.sqrt((F(1) - g) * (F(1) - g) + g * g)
            k, kb, kd = (F(1) - g) / den, g / den, F(1) / den
            assert all(v.dtype == F for v in (den, k, kb, kd))
            dx = (k * sc) * dm + dx
            terms = (dm * (sh - x * sc)) * kd
            part = seqsum(terms.reshape(n, T, D // cols, cols).transpose(0, 2, 1, 3).reshape(n, D // cols, T * cols), 2)
            got.update(dscale=seqsum((k * x) * dm, 1), dshift=seqsum(kb * dm, 1), dgain_part=part)
    assert dx.dtype == F
    if dx32:
        got["dx"] = dx
    got["dx16"] = to16(dx, fmt)
    if o["y_up"] is not None:
        gu, y = o["g_up"].astype(F)[:, None, :], o["y_up"].astype(F)
        got.update(dy_up=to16((cb * gu) * dx, fmt), dg_up=seqsum((cb * y) * dx, 1))
    return got


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("rot", [1, 0], ids=["rot", "adaln"])
@pytest.mark.parametrize("name", list(R.RMB_CASES))
def test_fp32_resid_mod_bwd_within_half_the_bound(name, rot, fmt):
    c = R.RMB_CASES[name]
    o = R.rmb_case(name, fmt)
    for dx32 in sorted({c.get("dx32", True), False}):     # (without the fp32 dx: the propagated form of the dependent bounds)
        r32 = R.rmb_ratios(o, rmb_f32(o, None, rot, c["cols"], dx32), None, rot, c["cols"])
        r = R.rmb_ratios(o, rmb_f32(o, fmt, rot, c["cols"], dx32), fmt, rot, c["cols"])
        show(f"resid_mod_bwd {name} {'rot' if rot else 'adaln'} {fmt} dx32={dx32} before the 16-bit stores", r32)
        show(f"resid_mod_bwd {name} {'rot' if rot else 'adaln'} {fmt} dx32={dx32}", r)
        assert r32 and max(r32.values()) <= HALF
        assert max(r.values()) <= 1.0 and all(v <= HALF for k, v in r.items() if k not in ("dx16", "dy_up"))


@pytest.mark.parametrize("D", R.COEF_DS)
def test_fp32_coef_bwd_within_half_the_bound(D):
    c = R.coef_bwd_case(D)
    for g in (c["g"], 0.0):
        _, _, cs, sn = coef_f32(c["theta"], c["scale"], g)
        a, b, sc, th = c["dA"].astype(F), c["dB"].astype(F), c["scale"].astype(F), c["theta"].astype(F)
        a0, a1, b0, b1, s0, s1 = a[:, 0::2], a[:, 1::2], b[:, 0::2], b[:, 1::2], sc[:, 0::2], sc[:, 1::2]
        dsc = np.empty_like(a)
        dsc[:, 0::2], dsc[:, 1::2] = cs * a0 + sn * b1, cs * a1 - sn * b0
        dphi = -sn * (s0 * a0 + s1 * a1) + cs * (s0 * b1 - s1 * b0)
        assert dphi.dtype == F
        h = D // 2
        nb = -(-h // 256)
        part = seqsum(np.pad(th * dphi, ((0, 0), (0, nb * 256 - h))).reshape(-1, nb, 256), 2)
        r = R.coef_bwd_ratios(c, g, dsc, F(g) * dphi, part)
        show(f"coef_bwd D={D} g={g}", r)
        assert max(r.values()) <= HALF
        if g == 0.0:
            assert not (F(g) * dphi).any() and np.array_equal(dsc, a)


def test_scale_accumulate_reference_rounds_the_product_first():
    """At alpha = 0.3 some elements of the largest case differ between the two-rounding form and a fused multiply-add - the case can tell them
    apart; at the power-of-two alphas the product is exact and they cannot differ."""
    c = R.accumulate_case(4099)
    two = R.scale_accumulate_f32(c["out"], c["x"], R.ACC_ALPHAS[2])
    fused = (c["out"] + R.ACC_ALPHAS[2] * c["x"]).astype(F)                      # float64 arithmetic, one rounding
    assert two.dtype == F and int((two != fused).sum()) > 10
    for alpha in R.ACC_ALPHAS[:2]:
        assert np.array_equal(R.scale_accumulate_f32(c["out"], c["x"], alpha), (c["out"] + alpha * c["x"]).astype(F))
