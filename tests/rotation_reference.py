"""fp64 restatements of the rotation-modulation kernels and of the fused residual / modulate backward (csrc/pointwise.hip; the rot form of
the RESID epilogue in csrc/gemm.hip), the error bounds the GPU tests hold the kernels to, and the generators of every GPU case's
operands (fixed seeds: tests/test_rotation_reference_cpu.py and tests/test_rotation_kernels_gpu.py see the same numbers).

Every function takes float64 numpy arrays that hold exactly what the kernel receives: fp32 values, or values exact in the 16-bit format.
The references return each result together with the sum of the absolute values of the terms it is made of ("*_abs"): the bounds are
stated in those.  With u = 2^-24, first order and doubled (as in tests/test_inception_kernels_gpu.py):

  a sum of n fp32 products            2 n u sum|terms|      whatever the order
  an expression of k fp32 operations  2 k u sum|terms|
  a 16-bit store of an fp32 value     e + ulp16(|want| + e) / 2     e = the fp32 bound; two roundings, and a value that crosses a binade
  a coefficient                       2 (|g theta| + 4) u |sc|      the rounding of the fp32 product g theta reaches the angle (slope of
                                      sin, cos <= 1); 4 = sincosf within 2 ulp of a value in [-1, 1] (the device library's documented
                                      figure) and one product

Nothing here imports the library or touches a device.
"""
import math

import numpy as np

import embed_reference as R

U24 = R.U24
CA, CB = float(np.float32(0.7 / math.sqrt(0.58))), float(np.float32(0.3 / math.sqrt(0.58)))     # mp_sum(., ., 0.3) as the engine passes it


def pairswap(a):
    """a[..., j ^ 1]."""
    return np.ascontiguousarray(a.reshape(a.shape[:-1] + (-1, 2))[..., ::-1]).reshape(a.shape)


def f32(a):
    """Round to fp32, keep as float64."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ---- the bound rules -------------------------------------------------------------------------------------------------------------------
def sum_bound(n, abs_terms):
    return 2.0 * n * U24 * np.asarray(abs_terms, dtype=np.float64)


def expr_bound(k, abs_terms):
    return 2.0 * k * U24 * np.asarray(abs_terms, dtype=np.float64)


def store16_bound(want, e, fmt):
    """fmt None: the bound of the fp32 value in front of the store (what the CPU test holds an fp32 evaluation to at ratio 0.5; the half ulp
    of the store itself is no first-order estimate but the exact bound of a correct rounding, which a correct store attains)."""
    want, e = np.asarray(want, dtype=np.float64), np.asarray(e, dtype=np.float64)
    return e if fmt is None else e + R.ulp16(np.abs(want) + e, fmt) / 2


def trig_bound(theta, g):
    """|cos_f32(fl(g theta)) - cos(g theta)| and the same for sin: the coefficient rule at sc = 1."""
    return 2.0 * (np.abs(g * theta) + 4.0) * U24


# ---- 1. coefficients ---------------------------------------------------------------------------------------------------------------------
def coef(theta, scale, g):
    """theta [n, D/2], scale [n, D], g scalar -> A, B [n, D]:  A[2i] = c sc[2i], A[2i+1] = c sc[2i+1], B[2i] = -s sc[2i+1],
    B[2i+1] = s sc[2i]  with c, s = cos, sin(g theta[i])."""
    c, s = np.cos(g * theta), np.sin(g * theta)
    A = np.repeat(c, 2, axis=-1) * scale
    B = np.repeat(s, 2, axis=-1) * pairswap(scale)
    B[..., 0::2] *= -1.0
    return A, B


def coef_bound(theta, scale, g):
    """(bound of A, bound of B): 2 (|g theta| + 4) u |sc| for the sc each coefficient is made of."""
    t = np.repeat(trig_bound(theta, g), 2, axis=-1)
    return t * np.abs(scale), t * np.abs(pairswap(scale))


# ---- 2. modulate -------------------------------------------------------------------------------------------------------------------------
def modulate(x, A, B):
    """x [n, T, D], A / B [n, D] -> (y, y_abs):  y[j] = x[j] A[j] + x[j ^ 1] B[j]."""
    a, b = x * A[:, None, :], pairswap(x) * B[:, None, :]
    return a + b, np.abs(a) + np.abs(b)


MOD_OPS = 3                                              # two products and an addition (two roundings where the first product is fused)


def modulate_bound(y, y_abs, fmt):
    return store16_bound(y, expr_bound(MOD_OPS, y_abs), fmt)


# ---- 3. / 4. the fused residual / modulate backward ------------------------------------------------------------------------------------------
def resid_up(dx, y_up, g_up, cb):
    """The residual half, from a given dx [n, T, D]:  dy_up = cb g_up dx,  dg_up[n, j] = sum_t cb y_up dx."""
    dy = cb * g_up[:, None, :] * dx
    t = cb * y_up * dx
    return dict(dy_up=dy, dy_up_abs=np.abs(dy), dg_up=t.sum(1), dg_up_abs=np.abs(t).sum(1))


ROT_DX_OPS = 5                                           # ca dxo, A dm, B' dm', two additions
DY_OPS = 2                                               # cb g_up, times dx


def resid_mod_bwd_rot(dxo, dxm, x, A, B, y_up, g_up, ca, cb):
    """dx[j] = ca dxo[j] + A[j] dm[j] + B[j ^ 1] dm[j ^ 1],  dA[n, j] = sum_t x[j] dm[j],  dB[n, j] = sum_t x[j ^ 1] dm[j],  and resid_up
    of dx.  dxo, dxm, y_up may be None (that part is off)."""
    o = {}
    dx, ab = 0.0, 0.0
    if dxo is not None:
        dx = ca * dxo
        ab = np.abs(dx)
    if dxm is not None:
        ta, tb = A[:, None, :] * dxm, pairswap(B[:, None, :] * dxm)
        dx, ab = dx + ta + tb, ab + np.abs(ta) + np.abs(tb)
        pa, pb = x * dxm, pairswap(x) * dxm
        o.update(dA=pa.sum(1), dA_abs=np.abs(pa).sum(1), dB=pb.sum(1), dB_abs=np.abs(pb).sum(1))
    o.update(dx=dx, dx_abs=ab)
    if y_up is not None:
        o.update(resid_up(dx, y_up, g_up, cb))
    return o


ADALN_DX_OPS = 9     # k = (1 - g) / den carries six roundings (1 - g, two squares, their sum, the root, the quotient), k scale one, the fma one, ca dxo one


def adaln_consts(g):
    den = math.sqrt((1.0 - g) ** 2 + g ** 2)
    return (1.0 - g) / den, g / den, 1.0 / den


def resid_mod_bwd_adaln(dxo, dxm, x, shift, scale, g, y_up, g_up, ca, cb, cols_per_block):
    """The formulas above resid_mod_bwd_kernel (den detached: the mp_sum denominator is a constant for the learnable gain):
    dx = ca dxo + k scale dm,  dscale[n, j] = sum_t k x dm,  dshift[n, j] = sum_t kb dm,  gain partial of (sample n, column block c) =
    sum over t and the block's columns of dm (shift - x scale) kd,  k = (1 - g) / den, kb = g / den, kd = 1 / den.  The partials come as
    [n, D / cols_per_block]; their absolute terms are |dm| (|shift| + |x scale|) kd."""
    k, kb, kd = adaln_consts(g)
    o = {}
    dx, ab = 0.0, 0.0
    if dxo is not None:
        dx = ca * dxo
        ab = np.abs(dx)
    if dxm is not None:
        n, T, D = dxm.shape
        t = k * scale[:, None, :] * dxm
        dx, ab = dx + t, ab + np.abs(t)
        ps, ph = k * x * dxm, kb * dxm
        pg = dxm * (shift[:, None, :] - x * scale[:, None, :]) * kd
        pg_abs = np.abs(dxm) * (np.abs(shift[:, None, :]) + np.abs(x * scale[:, None, :])) * kd
        blk = lambda v: v.reshape(n, T, D // cols_per_block, cols_per_block).sum((1, 3))
        o.update(dscale=ps.sum(1), dscale_abs=np.abs(ps).sum(1), dshift=ph.sum(1), dshift_abs=np.abs(ph).sum(1), dgain_part=blk(pg),
                 dgain_part_abs=blk(pg_abs))
    o.update(dx=dx, dx_abs=ab)
    if y_up is not None:
        o.update(resid_up(dx, y_up, g_up, cb))
    return o


# ---- 5. coefficient backward -----------------------------------------------------------------------------------------------------------------
DSCALE_OPS, DPHI_OPS = 2, 8


def coef_bwd(dA, dB, theta, scale, g):
    """dsc[2i] = c dA[2i] + s dB[2i+1],  dsc[2i+1] = c dA[2i+1] - s dB[2i],
    dphi = -s (sc[2i] dA[2i] + sc[2i+1] dA[2i+1]) + c (sc[2i] dB[2i+1] - sc[2i+1] dB[2i]),  dtheta = g dphi,  dgain = sum theta dphi (returned per
    element as gterm = theta dphi: the kernel sums it per sample and block of 256 pairs).  *_abs: the absolute terms; *_trig: what an error of
    c or s is multiplied by."""
    c, s = np.cos(g * theta), np.sin(g * theta)
    a0, a1, b0, b1, s0, s1 = dA[..., 0::2], dA[..., 1::2], dB[..., 0::2], dB[..., 1::2], scale[..., 0::2], scale[..., 1::2]
    dsc, dsc_abs, dsc_trig = (np.empty_like(dA) for _ in range(3))
    dsc[..., 0::2], dsc[..., 1::2] = c * a0 + s * b1, c * a1 - s * b0
    dsc_abs[..., 0::2], dsc_abs[..., 1::2] = np.abs(c * a0) + np.abs(s * b1), np.abs(c * a1) + np.abs(s * b0)
    dsc_trig[..., 0::2], dsc_trig[..., 1::2] = np.abs(a0) + np.abs(b1), np.abs(a1) + np.abs(b0)
    pa, pb = np.abs(s0 * a0) + np.abs(s1 * a1), np.abs(s0 * b1) + np.abs(s1 * b0)
    dphi = -s * (s0 * a0 + s1 * a1) + c * (s0 * b1 - s1 * b0)
    return dict(dscale=dsc, dscale_abs=dsc_abs, dscale_trig=dsc_trig, dphi=dphi, dphi_abs=np.abs(s) * pa + np.abs(c) * pb, dphi_trig=pa + pb,
                dtheta=g * dphi, gterm=theta * dphi)


def coef_bwd_bounds(r, theta, g):
    """Bounds of dscale, dtheta (per element) and of the gain partials (per sample and block of 256 pairs, [n, ceil(D / 512)]), and the
    reference partials themselves."""
    tb = trig_bound(theta, g)
    e_dscale = expr_bound(DSCALE_OPS, r["dscale_abs"]) + np.repeat(tb, 2, axis=-1) * r["dscale_trig"]
    e_dphi = expr_bound(DPHI_OPS, r["dphi_abs"]) + tb * r["dphi_trig"]
    n, h = theta.shape
    nb = -(-h // 256)
    pad = lambda v: np.pad(v, ((0, 0), (0, nb * 256 - h))).reshape(n, nb, 256).sum(-1)
    part = pad(r["gterm"])
    e_part = sum_bound(256, pad(np.abs(r["gterm"]))) + pad(np.abs(theta) * e_dphi)
    return dict(dscale=e_dscale, dtheta=abs(g) * e_dphi, part=part, e_part=e_part)


# ---- generators: the operands of every GPU case ---------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([ord(ch) for ch in "rotation"] + [int(k) for k in key])


def _n32(rng, *shape, scale=1.0, shift=0.0):
    return f32(rng.standard_normal(shape) * scale + shift)


def q16(v, fmt):
    """Values of the 16-bit format (rounded once), as float64."""
    return R.round16(f32(v), fmt)


COEF_DS = [8, 128, 384, 1152]
COEF_N = 3
COEF_GAIN = float(np.float32(1.7))


def coef_case(D):
    """n = 3 samples; g theta spread over about +-50 (|theta| < 30 at g = 1.7); sample 1 carries a row of zero angles."""
    rng = _rng(1, D)
    theta = f32(rng.uniform(-30.0, 30.0, (COEF_N, D // 2)))
    theta[1] = 0.0
    return dict(theta=theta, scale=_n32(rng, COEF_N, D, shift=1.0), g=COEF_GAIN)


ALL_SLOTS = 5
ALL_GAINS = [float(np.float32(v)) for v in (1.7, 0.0, -0.6, 2.5, 0.9)]


def coef_all_case(D):
    """Five slots with their own angles, scales and gains (slot 1: gain 0)."""
    rng = _rng(2, D)
    return dict(theta=f32(rng.uniform(-20.0, 20.0, (ALL_SLOTS, COEF_N, D // 2))), scale=_n32(rng, ALL_SLOTS, COEF_N, D, shift=1.0), gains=ALL_GAINS)


MOD_SHAPES = [(2, 3, 8), (3, 5, 136), (2, 4, 1152)]


def modulate_case(n, T, D):
    """A and B random, not from the coefficient kernel: the four terms of a pair are independent."""
    rng = _rng(3, n, T, D)
    return dict(x=_n32(rng, n, T, D), A=_n32(rng, n, D), B=_n32(rng, n, D))


EPI_M, EPI_N, EPI_K = 512, 256, 64
EPI_ROWS = [64, 256]


def epilogue_case(rows, fmt):
    """The RESID epilogue with rot2: a [M, K], b [N, K] 16-bit, the residual input x, the gate rows and the coefficient rows."""
    rng = _rng(4, rows)
    s = EPI_M // rows
    return dict(a=q16(rng.standard_normal((EPI_M, EPI_K)), fmt), b=q16(rng.standard_normal((EPI_N, EPI_K)) * 0.2, fmt), x=_n32(rng, EPI_M, EPI_N),
                gate=_n32(rng, s, EPI_N), A=_n32(rng, s, EPI_N), B=_n32(rng, s, EPI_N))


# name: (n, T, D, what is on).  Z: the row split the kernel takes with scratch for 8 slices given; cols: columns per block (gain partials)
RMB_CASES = {
    "1_wide_ragged":    dict(n=2, T=10, D=256, dxo="f32", dxm=True, y_up=True, cols=256),
    "2_lanes32":        dict(n=3, T=19, D=384, dxo="f32", dxm=True, y_up=True, cols=128),
    "3_split8":         dict(n=2, T=64, D=128, dxo="f32", dxm=True, y_up=True, cols=128, Z=8),
    "3b_split2":        dict(n=2, T=48, D=128, dxo="f32", dxm=True, y_up=True, cols=128, Z=2),
    "4_column_range":   dict(n=2, T=12, D=128, dxo="16", dxm=True, y_up=True, cols=128, ldx=384, col0=256, dx32=False),
    "5a_modulate_only": dict(n=2, T=10, D=256, dxo=None, dxm=True, y_up=False, cols=256),
    "5b_residual_only": dict(n=2, T=10, D=256, dxo="f32", dxm=False, y_up=True, cols=256),
}
RMB_GAIN = float(np.float32(0.37))                      # the AdaLN form's gain


def rmb_case(name, fmt):
    """Operands of one resid_mod_bwd case: scale / shift are the A / B rows in the rotation form and the scale / shift rows in the AdaLN
    form (random either way).  Parts that are off come as None."""
    c = RMB_CASES[name]
    n, T, D = c["n"], c["T"], c["D"]
    rng = _rng(5, n, T, D, len(name))
    o = dict(x=_n32(rng, n, T, D), scale=_n32(rng, n, D), shift=_n32(rng, n, D), g_up=_n32(rng, n, D), ca=CA, cb=CB, gain=RMB_GAIN)
    dxo, dxm, y_up = _n32(rng, n, T, D), q16(rng.standard_normal((n, T, D)), fmt), q16(rng.standard_normal((n, T, D)), fmt)
    o["dxo"] = dxo if c["dxo"] == "f32" else q16(dxo, fmt) if c["dxo"] == "16" else None
    o["dxm"] = dxm if c["dxm"] else None
    o["y_up"] = y_up if c["y_up"] else None
    return o


def coef_bwd_case(D):
    """The forward case's angles, scales and gain with random fp32 dA / dB."""
    rng = _rng(6, D)
    c = coef_case(D)
    c.update(dA=_n32(rng, COEF_N, D), dB=_n32(rng, COEF_N, D))
    return c


ACC_NS, ACC_ALPHAS = [1, 255, 4099], [1.0, 2.0 ** -10, float(np.float32(0.3))]


def accumulate_case(n):
    rng = _rng(7, n)
    return dict(out=_n32(rng, n), x=_n32(rng, n))


def scale_accumulate_f32(out, x, alpha):
    """out + alpha x with the product rounded to fp32 before the addition, in numpy float32."""
    prod = (np.float32(alpha) * x.astype(np.float32)).astype(np.float32)
    return (out.astype(np.float32) + prod).astype(np.float32)


# ---- the checks, shared by the CPU test (on an fp32 evaluation in numpy) and the GPU test (on the kernels' results) ---------------------------
def worst(got, want, tol):
    """Worst |got - want| / tol over the elements (0 / 0 counts as 0); `got` must be finite."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), got.shape)
    assert got.shape == want.shape and np.isfinite(got).all()
    err = np.abs(got - want)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300)))) if got.size else 0.0


def coef_ratios(theta, scale, g, A, B):
    (A64, B64), (eA, eB) = coef(theta, scale, g), coef_bound(theta, scale, g)
    return dict(A=worst(A, A64, eA), B=worst(B, B64, eB))


def modulate_ratio(c, got, fmt):
    y, y_abs = modulate(c["x"], c["A"], c["B"])
    return worst(got, y, modulate_bound(y, y_abs, fmt))


def modulate_mutant_ratios(c, got, fmt):
    """`got` against the two wrong references: B[j ^ 1] in place of B[j], and -B."""
    r = {}
    for name, Bm in (("partner", pairswap(c["B"])), ("sign", -c["B"])):
        y, y_abs = modulate(c["x"], c["A"], Bm)
        r[name] = worst(got, y, modulate_bound(y, y_abs, fmt))
    return r


def rmb_ratios(o, got, fmt, rot, cols):
    """Ratios of one resid_mod_bwd call.  got: dx (fp32) and / or dx16, dy_up, dg_up, and dA / dB (rot) or dscale / dshift / dgain_part
    [n, D / cols] (AdaLN; the partials of a row-split call summed over the slices).  What depends on dx takes the call's OWN fp32 dx as its
    input where the call returns it (each bound then covers that stage's arithmetic alone), and the reference dx with its bound
    propagated where it does not."""
    if rot:
        ref = resid_mod_bwd_rot(o["dxo"], o["dxm"], o["x"], o["scale"], o["shift"], o["y_up"], o["g_up"], o["ca"], o["cb"])
    else:
        ref = resid_mod_bwd_adaln(o["dxo"], o["dxm"], o["x"], o["shift"], o["scale"], o["gain"], o["y_up"], o["g_up"], o["ca"], o["cb"], cols)
    T = o["x"].shape[1]
    e_dx = expr_bound(ROT_DX_OPS if rot else ADALN_DX_OPS, ref["dx_abs"])
    r = {}
    if got.get("dx") is not None:
        r["dx"] = worst(got["dx"], ref["dx"], e_dx)
        dx_in, e_in = np.asarray(got["dx"], dtype=np.float64), np.zeros_like(e_dx)
    else:
        dx_in, e_in = ref["dx"], e_dx
    if got.get("dx16") is not None:
        r["dx16"] = worst(got["dx16"], dx_in, store16_bound(dx_in, e_in, fmt))
    if o["dxm"] is not None:
        for name in (("dA", "dB") if rot else ("dscale", "dshift")):
            r[name] = worst(got[name], ref[name], sum_bound(T, ref[name + "_abs"]))
        if not rot:
            r["dgain_part"] = worst(got["dgain_part"], ref["dgain_part"], sum_bound(T * cols, ref["dgain_part_abs"]))
    if o["y_up"] is not None:
        up = resid_up(dx_in, o["y_up"], o["g_up"], o["cb"])
        e_dy = expr_bound(DY_OPS, up["dy_up_abs"]) + np.abs(o["cb"] * o["g_up"])[:, None, :] * e_in
        r["dy_up"] = worst(got["dy_up"], up["dy_up"], store16_bound(up["dy_up"], e_dy, fmt))
        r["dg_up"] = worst(got["dg_up"], up["dg_up"], sum_bound(T, up["dg_up_abs"]) + (np.abs(o["cb"] * o["y_up"]) * e_in).sum(1))
    return r


def coef_bwd_ratios(c, g, dscale, dtheta, part):
    """part: [n, ceil(D / 512)] unscaled gain partials."""
    ref = coef_bwd(c["dA"], c["dB"], c["theta"], c["scale"], g)
    b = coef_bwd_bounds(ref, c["theta"], g)
    return dict(dscale=worst(dscale, ref["dscale"], b["dscale"]), dtheta=worst(dtheta, ref["dtheta"], b["dtheta"]),
                dgain_part=worst(part, b["part"], b["e_part"]))
