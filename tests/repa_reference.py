"""The yardstick of the REPA kernels and of ``repa.RepaHead``: fp64 restatements, in numpy on the CPU, of the cosine loss with its
gradient, of the projector z = W3 silu(W2 silu(W1 h + b1) + b2) + b3 with its hand-written backward, and of the correctly rounded
fp64 -> 16-bit conversion.  Written with explicit formulas, not through autograd; tests/test_repa_cpu.py pins them to torch's fp64
autograd and the rounding to exact rational arithmetic.

``emulate="f16" | "bf16"`` rounds every operand the head rounds to 16 bits - the hidden state, the three weights, the two activations
and the three activation gradients (under the loss scale) - and keeps the rest fp64, so that what is left between it and the kernels
is fp32 accumulation and fp32 pointwise math; ``emulate=None`` is the exact head."""
import math

import numpy as np

EPS = 1e-12
U32 = 2.0 ** -24                # unit roundoff of fp32
_FMT = {"f16": (11, -14), "bf16": (8, -126)}                # (significand bits, minimum normal exponent)


def round16(x, fmt):
    """fp64 -> the nearest value of the 16-bit format, ties to even, subnormals included, as fp64 (no saturation: beyond the largest
    finite value the result is +-inf).  One rounding: x is scaled to an integer grid by an exact power of two and np.rint ties to even."""
    if fmt is None:
        return np.asarray(x, np.float64)
    p, emin = _FMT[fmt]
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)                                       # x = m 2^e, 0.5 <= |m| < 1
    e = np.maximum(e - 1, emin)                              # exponent of the leading bit, held at the subnormal range
    q = np.ldexp(1.0, e - (p - 1))                           # the spacing of the format at x
    out = np.rint(x / q) * q                                 # (x / q and the product are exact: q is a power of two)
    big = (2.0 - 2.0 ** (1 - p)) * 2.0 ** (15 if fmt == "f16" else 127)
    return np.where(np.abs(out) > big, np.copysign(np.inf, x), out)


def rnd(x, emulate):
    """The kernels' conversion of an operand: fp16 saturates at +-65504 (pack16s), then round16."""
    if emulate is None:
        return np.asarray(x, np.float64)
    x = np.asarray(x, np.float64)
    if emulate == "f16":
        x = np.clip(x, -65504.0, 65504.0)
    return round16(x, emulate)


def cos_loss(z, f, T, g=None):
    """z, f [R, P] -> loss [R / T] = -(1 / T) sum_t <z_t / max(|z_t|, eps), f_t / max(|f_t|, eps)> and dz [R, P] = g_n d loss[n] / d z
    (g = None: ones).  Below eps the normalisation is the constant 1 / eps, so only the first term of the derivative is left."""
    z, f = np.asarray(z, np.float64), np.asarray(f, np.float64)
    R, P = z.shape
    N = R // T
    g = np.ones(N) if g is None else np.asarray(g, np.float64)
    nzr, nfr = np.sqrt((z * z).sum(1)), np.sqrt((f * f).sum(1))
    nz, nf = np.maximum(nzr, EPS), np.maximum(nfr, EPS)
    cos = (z * f).sum(1) / nz / nf
    loss = -cos.reshape(N, T).sum(1) / T
    gr = np.repeat(g, T) / T
    kf = -gr / (nz * nf)
    kz = np.where(nzr >= EPS, gr * cos / (nz * nz), 0.0)
    return loss, kf[:, None] * f + kz[:, None] * z


def cos_loss_bound(z, f, T, g=None):
    """Operation-count bounds of the fp32 kernel's error, per element, from the kernel's own order of operations (u = 2^-24, gamma_k =
    k u / (1 - k u)).  A row sum over P terms is P / 64 (rounded up to 8-element chunks) sequential fmas in a lane and a six-level
    butterfly: gamma_(8 ceil(P / 512) + 6) relative to the sum of the terms' magnitudes.  The two norms add half of that bound and a
    square root each, the quotient two divisions; the per-sample sum adds ceil(T / 4) + 3 additions.  dz adds the reciprocal products,
    one multiplication and one fma.  Returns (loss bound [R / T], dz bound [R, P])."""
    z, f = np.asarray(z, np.float64), np.asarray(f, np.float64)
    R, P = z.shape
    N = R // T
    g = np.ones(N) if g is None else np.asarray(g, np.float64)
    k = 8 * math.ceil(P / 512) + 6

    def gam(n):
        return n * U32 / (1 - n * U32)

    nz, nf = np.maximum(np.sqrt((z * z).sum(1)), EPS), np.maximum(np.sqrt((f * f).sum(1)), EPS)
    adot = (np.abs(z) * np.abs(f)).sum(1)
    # |cos error| <= gamma_k adot / (nz nf) + |cos| (two norms: gamma_k / 2 + 2u each with the square root; two divisions; slack 2u)
    cos = (z * f).sum(1) / nz / nf
    ecos = gam(k) * adot / (nz * nf) + np.abs(cos) * (gam(k) + 8 * U32)
    eloss = (ecos.reshape(N, T).sum(1) + gam(math.ceil(T / 4) + 4) * np.abs(cos).reshape(N, T).sum(1)) / T
    gr = np.abs(np.repeat(g, T)) / T
    # kf = -g / (nz nf): the norms gamma_k + 4u, their product, the division, g x scale and / T: gamma_k + 10u;  kz = g cos / nz^2: ecos,
    # the same and the product with cos: gamma_k + 12u
    ekf = gr / (nz * nf) * (gam(k) + 10 * U32)
    ekz = gr / (nz * nz) * (ecos + np.abs(cos) * (gam(k) + 12 * U32))
    edz = ekf[:, None] * np.abs(f) + ekz[:, None] * np.abs(z) + 2 * U32 * (gr / (nz * nf))[:, None] * np.abs(f) \
        + 2 * U32 * (gr * np.abs(cos) / (nz * nz))[:, None] * np.abs(z)
    return eloss, edz


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def silu(x):
    return x * sigmoid(x)


def dsilu(x):
    s = sigmoid(x)
    return s * (1.0 + x * (1.0 - s))


def init_params(in_dim, feat_dim, hidden, seed=0):
    """The head's initial parameters as ``RepaHead`` draws them (nn.Linear's default from one seeded generator), fp64."""
    import torch
    g = torch.Generator().manual_seed(int(seed))
    out = {}
    for i, (o, k) in enumerate([(hidden, in_dim), (hidden, hidden), (feat_dim, hidden)], 1):
        bound = 1.0 / math.sqrt(k)
        out[f"w{i}"] = ((torch.rand(o, k, generator=g) * 2 - 1) * bound).double().numpy()
        out[f"b{i}"] = ((torch.rand(o, generator=g) * 2 - 1) * bound).double().numpy()
    return out


def head_loss(h, feats, p, T, g=None, emulate=None, scale=1.0):
    """h [M, D], feats [M, P], p the six parameters -> (loss [M / T], dh [M, D], parameter gradients), by hand.  ``scale``: the loss
    scale the 16-bit activation gradients are rounded under (the fp16 head's; exact powers of two leave emulate=None unchanged)."""
    h, feats = np.asarray(h, np.float64), np.asarray(feats, np.float64)
    w = [rnd(p[f"w{i}"], emulate) for i in (1, 2, 3)]
    x = rnd(h, emulate)
    pre1 = x @ w[0].T + p["b1"]
    a1 = rnd(silu(pre1), emulate)
    pre2 = a1 @ w[1].T + p["b2"]
    a2 = rnd(silu(pre2), emulate)
    z = a2 @ w[2].T + p["b3"]
    loss, dz = cos_loss(z, feats, T, g)
    grads = {}
    d3 = scale * dz
    d3r = rnd(d3, emulate)
    grads["b3"], grads["w3"] = d3.sum(0) / scale, d3r.T @ a2 / scale
    d2 = (d3r @ w[2]) * dsilu(pre2)
    d2r = rnd(d2, emulate)
    grads["b2"], grads["w2"] = d2.sum(0) / scale, d2r.T @ a1 / scale
    d1 = (d2r @ w[1]) * dsilu(pre1)
    d1r = rnd(d1, emulate)
    grads["b1"], grads["w1"] = d1.sum(0) / scale, d1r.T @ x / scale
    return loss, (d1r @ w[0]) / scale, grads


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


# ---- the case of tests/test_repa_head_gpu.py, built here so that tests/test_repa_cpu.py measures the emulation figure on its very inputs
HEAD_CASE = dict(in_dim=128, feat_dim=24, hidden=64, N=2, T=64, seed=5)


def head_case():
    c = HEAD_CASE
    rng = np.random.default_rng(77)
    h = rng.standard_normal((c["N"] * c["T"], c["in_dim"])).astype(np.float32)
    feats = rng.standard_normal((c["N"] * c["T"], c["feat_dim"])).astype(np.float16)
    g = np.array([0.25, -0.4], np.float32)
    return h, feats, g, init_params(c["in_dim"], c["feat_dim"], c["hidden"], c["seed"])


def head_scale(prec):
    c = HEAD_CASE
    return 2.0 ** math.floor(math.log2(c["N"] * c["T"] * c["feat_dim"])) if prec == "f16" else 1.0


def measure_head_emulation(prec) -> dict:
    """name -> relative (norm-wise) distance between the emulated and the exact head on HEAD_CASE: loss, dh and every gradient."""
    h, feats, g, p = head_case()
    T = HEAD_CASE["T"]
    exact = head_loss(h, feats, p, T, g)
    emul = head_loss(h, feats, p, T, g, emulate=prec, scale=head_scale(prec))
    out = {"loss": rel(emul[0], exact[0]), "dh": rel(emul[1], exact[1])}
    for k in exact[2]:
        out[k] = rel(emul[2][k], exact[2][k])
    return out
