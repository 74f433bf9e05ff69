"""fp64 reference of the fused Adam + EMA step (csrc/weights.hip: adam_ema_apply4) and of the per-step scalars FusedAdamEMA.step hands
to it, written from the definitions: torch.optim.Adam without weight decay (bias corrections folded into step_size and inv_sqrt_bc2),
the gradient scale applied to the gradient before both moments, and ema.lerp_(p_new, beta) for the two power-function EMA copies.

    gk = g gs      m' = b1 m + (1 - b1) gk      v' = b2 v + (1 - b2) gk^2
    upd = step_size m' / (sqrt(v') inv_sqrt_bc2 + eps)      p' = p - upd      e' = e + beta (p' - e)

Error scales (u = 2^-24, ma = |b1 m| + |(1 - b1) gk|, den = sqrt(v') c + eps, us = |upd| + step_size ma / den):

    m': u ma      v': u |v'|      p': u (|p'| + us)      e': u (|e| + |p'| + us)

ma is the size of the two addends of m', not of their sum: where they cancel, m' carries an absolute error of a few u ma, and the divide
hands it on to upd, p' and e' - that is the conditioning of the operation, which any fp32 evaluation shares.  tests/
test_optimizer_reference_cpu.py measures a plain fp32 evaluation (emulate32) at <= 4 of these scales per quantity; the GPU tests allow 8.

numpy and fp64 only; nothing here imports the library or touches a device.
"""
import math

import numpy as np

U24 = 2.0 ** -24                                     # unit roundoff of fp32
QUANTITIES = ("p", "m", "v", "ea", "eb")
MUTANTS = ("eps_in_sqrt", "no_bias_correction", "grad_scale_m_only", "ema_old_p")
GRAD_MAX = 1e6                                       # largest |g| of stress_state: v' <= 1e12 + 1e10, finite in fp32
HAND = 64                                            # length of the hand-picked block at the front of stress_state


def f32(x):
    """The fp32 rounding of a Python float, as a Python float (what a `float` argument of the C ABI receives)."""
    return float(np.float32(x))


# ---- the per-step scalars ------------------------------------------------------------------------------------------------------------
def gamma_of_std(std):
    """Exponent of the power-function EMA profile of relative width `std`: the positive root of
    g^3 + 7 g^2 + (16 - s^-2) g + (12 - s^-2)  (for s^-2 > 12 the constant term is negative, the product of the three roots is positive
    and their sum is -7: exactly one root is positive, so it is the largest real one).  Bisection on (0, 1/s): the cubic is
    negative at 0 and equals 6 s^-2 + 16 / s + 12 > 0 at 1 / s."""
    t = float(std) ** -2
    assert t > 12.0

    def f(g):
        return ((g + 7.0) * g + (16.0 - t)) * g + (12.0 - t)

    lo, hi = 0.0, 1.0 / float(std)
    assert f(lo) < 0.0 < f(hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if f(mid) < 0.0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def hyper64(t, lr, b1, b2, stds, grad_scale):
    """The five scalars of optimiser step t (counted from 1), fp64:
    [lr / (1 - b1^t), 1 / sqrt(1 - b2^t), beta_a(t), beta_b(t), grad_scale], beta(t) = (1 - 1/t)^(gamma + 1); no EMA copies -> betas 0.
    `lr` is the learning rate of this step, schedule factor included."""
    assert t >= 1
    betas = [(1.0 - 1.0 / t) ** (gamma_of_std(s) + 1.0) for s in stds] if len(stds) else [0.0, 0.0]
    assert len(betas) == 2
    return np.array([lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t), betas[0], betas[1], grad_scale], dtype=np.float64)


def hyper(t, lr, b1, b2, stds, grad_scale):
    """hyper64 rounded to fp32: what the kernel receives (the five `float` fields of mapdit_adam_scalars_t)."""
    return hyper64(t, lr, b1, b2, stds, grad_scale).astype(np.float32)


# ---- one step ------------------------------------------------------------------------------------------------------------------------
def _check_inputs(arrays, hy, dtypes):
    for a in arrays:
        assert a is None or (a.dtype in dtypes and a.ndim == 1)
    hy = np.asarray(hy)
    assert hy.dtype in dtypes and hy.shape == (5,)
    return hy


def step64(p, g, m, v, ea, eb, hyper, b1, b2, eps):
    """One step in fp64 on the fp32 inputs.  b1, b2, eps: Python floats that are already fp32 values; 1 - b1 and 1 - b2 are formed in fp32
    as the kernel forms them (exact there: both betas lie in [0.5, 1]).  ea / eb may be None.  Returns (out, scale): dicts over QUANTITIES
    of fp64 arrays (None for an absent copy).  fp64 arrays and scalars are taken too: a trajectory that carries its own fp64 state."""
    hy = _check_inputs((p, g, m, v, ea, eb), hyper, (np.float32, np.float64)).astype(np.float64)
    assert f32(b1) == b1 and f32(b2) == b2 and f32(eps) == eps
    step_size, c, beta_a, beta_b, gs = (float(z) for z in hy)
    omb1, omb2 = float(np.float32(1) - np.float32(b1)), float(np.float32(1) - np.float32(b2))
    p, g, m, v = (z.astype(np.float64) for z in (p, g, m, v))
    gk = g * gs
    m1 = b1 * m + omb1 * gk
    v1 = b2 * v + omb2 * gk * gk
    den = np.sqrt(v1) * c + eps
    upd = step_size * m1 / den
    p1 = p - upd
    ma = np.abs(b1 * m) + np.abs(omb1 * gk)
    us = np.abs(upd) + step_size * ma / den
    out = {"p": p1, "m": m1, "v": v1, "ea": None, "eb": None}
    scale = {"p": U24 * (np.abs(p1) + us), "m": U24 * ma, "v": U24 * np.abs(v1), "ea": None, "eb": None}
    for key, e, beta in (("ea", ea, beta_a), ("eb", eb, beta_b)):
        if e is not None:
            e = e.astype(np.float64)
            out[key] = e + beta * (p1 - e)
            scale[key] = U24 * (np.abs(e) + np.abs(p1) + us)
    return out, scale


def emulate32(p, g, m, v, ea, eb, hyper, b1, b2, eps, mutant=None):
    """The kernel's operation order in numpy fp32 (every operation rounded, no fused multiply-add); used to measure the error scales on
    the CPU.  `mutant` (one of MUTANTS) evaluates a deliberately wrong variant: the CPU test shows that stress_state tells each apart."""
    hy = _check_inputs((p, g, m, v, ea, eb), hyper, (np.float32,))
    assert mutant is None or mutant in MUTANTS
    F = np.float32
    step_size, c, beta_a, beta_b, gs = hy
    b1, b2, eps = F(b1), F(b2), F(eps)
    gk = g * gs
    m1 = b1 * m + (F(1) - b1) * gk
    gv = g if mutant == "grad_scale_m_only" else gk
    v1 = b2 * v + (F(1) - b2) * gv * gv
    if mutant == "eps_in_sqrt":
        den = np.sqrt(v1 + eps) * c
    elif mutant == "no_bias_correction":
        den = np.sqrt(v1) + eps
    else:
        den = np.sqrt(v1) * c + eps
    p1 = p - step_size * m1 / den
    out = {"p": p1, "m": m1, "v": v1, "ea": None, "eb": None}
    target = p if mutant == "ema_old_p" else p1
    for key, e, beta in (("ea", ea, beta_a), ("eb", eb, beta_b)):
        if e is not None:
            out[key] = e + beta * (target - e)
    assert all(z is None or z.dtype == np.float32 for z in out.values())
    return out


def ratios(got, want, scale):
    """Worst |got - want| / scale per quantity (0 / 0 counts as 0; an error on a zero scale is inf).  got: dict of arrays, any float type."""
    out = {}
    for k in QUANTITIES:
        if want[k] is None:
            continue
        gk = np.asarray(got[k], dtype=np.float64)
        assert gk.shape == want[k].shape and np.isfinite(gk).all(), k
        err = np.abs(gk - want[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            out[k] = float(np.max(np.where(err == 0, 0.0, err / scale[k])))
    return out


# ---- the input family ----------------------------------------------------------------------------------------------------------------
def _log_uniform(n, lo, hi, rng):
    return 10.0 ** rng.uniform(math.log10(lo), math.log10(hi), n)


def hand_block(eps=1e-8):
    """The HAND hand-picked elements at the front of stress_state -> fp32 arrays p, g, m, v.
    0..3   m = v = g = 0 (the element must not move: 0 / (0 + eps))
    4..11  g = +-1e-25, its square (1e-50) far below fp32: with v in {eps^2, 1e-12, 1, 0.25} and m in {0, +-1e-3}
    12..19 v = eps^2 exactly (sqrt(v') c is of the size of eps): g, m from 1e-9 to 1e-7
    20..23 v = 0 and g tiny but with a normal square: the whole second moment comes from this step
    24..63 m and g of opposite sign with |b1 m| ~ |(1 - b1) g gs| for gs in {1, 1/8, 1/3, 1/7} and relative offsets from 0 to 1e-2"""
    p = np.ones(HAND)
    g, m, v = np.zeros(HAND), np.zeros(HAND), np.zeros(HAND)
    p[0:4] = [0.0, 1.0, -3.5, 1e-3]
    i = 4
    for sign in (1.0, -1.0):
        for vv, mm in ((eps * eps, 0.0), (1e-12, 1e-3), (1.0, -1.0e-3), (0.25, 0.0)):
            g[i], v[i], m[i] = sign * 1e-25, vv, mm
            i += 1
    for k, (gg, mm) in enumerate(((1e-8, 0.0), (-1e-8, 1e-8), (1e-9, -1e-9), (1e-7, 1e-9), (0.0, 1e-8), (3e-8, 0.0), (-1e-7, -1e-7), (1e-9, 0.0))):
        g[12 + k], m[12 + k], v[12 + k] = gg, mm, eps * eps
    for k, gg in enumerate((1e-12, -1e-10, 1e-8, -1e-15)):
        g[20 + k], m[20 + k], v[20 + k] = gg, 0.0, 0.0
    i = 24
    for gs in (1.0, 1.0 / 8, 1.0 / 3, 1.0 / 7):
        for k, off in enumerate((0.0, 1e-7, -1e-7, 1e-6, 1e-5, -1e-4, 1e-3, 1e-2, -3e-7, 3e-6)):
            mm = (1.0 if k % 2 == 0 else -1.0) * 10.0 ** (k % 5 - 2)
            m[i], g[i], v[i] = mm, -9.0 * mm / gs * (1.0 + off), 10.0 ** (2 * (k % 4) - 4)
            i += 1
    assert i == HAND
    return tuple(z.astype(np.float32) for z in (p, g, m, v))


def stress_state(n, rng):
    """The input family of the optimiser tests -> dict of fp32 arrays p, g, m, v, ea, eb of length n >= HAND.
    p ~ N(0, 1) 10^k, k uniform in -3..2; |g| and |m| log-uniform in [1e-12, 1e6] with random signs, every 17th g and every 13th m
    exactly 0; v log-uniform in [1e-24, 1e12], every 11th exactly 0; the EMA copies within 1 % of p; hand_block() at the front.
    |g| <= GRAD_MAX keeps v' finite in fp32, so the reference alone never yields inf; the smallest non-zero |g| times a gradient scale
    >= 1/8 has a square above 1e-26, a normal fp32 number (the one underflowing square, g = 1e-25, sits beside a normal v)."""
    assert n >= HAND
    p = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)
    g = _log_uniform(n, 1e-12, GRAD_MAX, rng) * rng.choice([-1.0, 1.0], n)
    m = _log_uniform(n, 1e-12, 1e6, rng) * rng.choice([-1.0, 1.0], n)
    v = _log_uniform(n, 1e-24, 1e12, rng)
    g[::17], m[::13], v[::11] = 0.0, 0.0, 0.0
    s = dict(p=p.astype(np.float32), g=g.astype(np.float32), m=m.astype(np.float32), v=v.astype(np.float32))
    for k, z in zip("pgmv", hand_block()):
        s[k][:HAND] = z
    s["ea"] = (s["p"].astype(np.float64) * (1.0 + rng.uniform(-0.01, 0.01, n))).astype(np.float32)
    s["eb"] = (s["p"].astype(np.float64) * (1.0 + rng.uniform(-0.01, 0.01, n))).astype(np.float32)
    assert float(np.max(np.abs(s["g"]))) <= GRAD_MAX
    return s


def args_of(s):
    return s["p"], s["g"], s["m"], s["v"], s["ea"], s["eb"]
