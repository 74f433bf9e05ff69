"""fp64 reference of global gradient-norm clipping (csrc/weights.hip: grad_sqnorm_kernel, grad_clip_coef_kernel), written from the
formulas - torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2) on the gradient the optimiser uses:

    norm = |grad_scale| sqrt(sum g^2)      coef = min(max_norm / (norm + 1e-6), 1)      the step uses g grad_scale coef

The bound of the GPU tests.  The kernels square and add in fp64 from the first operation on (the product of two fp32 values is exact
there), so the sum errs by at most n 2^-53 relative (5e-10 at n = 2^22) and the fp32 word the device writes is the rounding of an almost
exact value: TOL = 2^-23 relative, one fp32 ulp, for norm and coef alike.  Nothing is measured.

emulate() evaluates the kernels' structure - a partial sum per 4,096-element workgroup, then their sum - and, by name, deliberately wrong
variants; tests/test_grad_clip_cpu.py shows that family(), the inputs of the GPU tests, tells each of them from clip64 by more than TOL.

numpy and fp64 only; nothing here imports the library or touches a device.
"""
import math

import numpy as np

import optimizer_reference as R

TOL = 2.0 ** -23
EPS = 1e-6
BLOCK = 4096
MUTANTS = ("grad_scale_ignored", "no_eps", "unclamped", "fp32_squares", "tail_block_dropped")
SIZES = (4, 4096, 4100, 3 * 4096 + 8)
POSITIONS = (0, 4095, 4096, -1)                      # -1: the last element
SCALES = (1.0, 1.0 / 8, 1.0 / 3)
N_ACCURACY = 1 << 22


def f32(x):
    return float(np.float32(x))


def sqsum64(g):
    """Sum of squares of the fp32 (or fp64) array g, in fp64."""
    g = np.asarray(g, dtype=np.float64).ravel()
    return float(np.sum(g * g))


def _coef(norm, max_norm, eps=EPS, clamp=True):
    with np.errstate(invalid="ignore", divide="ignore"):
        c = float(np.float64(max_norm) / (np.float64(norm) + np.float64(eps)))
    return 1.0 if clamp and c > 1.0 else c           # (a NaN stays a NaN: the comparison is false)


def clip64(g, grad_scale, max_norm):
    """(norm, coef) as Python floats.  grad_scale and max_norm are taken as given: pass the fp32 values the C ABI carries."""
    with np.errstate(invalid="ignore", over="ignore"):
        norm = abs(float(grad_scale)) * math.sqrt(sqsum64(g))       # (sqrt(inf) = inf, sqrt(NaN) = NaN)
    return norm, _coef(norm, max_norm)


def emulate(g, grad_scale, max_norm, mutant=None):
    """The kernels' structure in numpy: partials[b] = sum of squares of elements [4096 b, 4096 (b + 1)), their sum, the two formulas.
    `mutant` (one of MUTANTS) evaluates a deliberately wrong variant."""
    assert mutant is None or mutant in MUTANTS
    g = np.asarray(g, dtype=np.float32).ravel()
    n = g.size
    nblocks = n // BLOCK if mutant == "tail_block_dropped" else (n + BLOCK - 1) // BLOCK
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if mutant == "fp32_squares":
            partials = [np.sum(g[b * BLOCK:(b + 1) * BLOCK] * g[b * BLOCK:(b + 1) * BLOCK], dtype=np.float32) for b in range(nblocks)]
            total = float(np.sum(np.asarray(partials, dtype=np.float32), dtype=np.float32)) if partials else 0.0
        else:
            partials = [sqsum64(g[b * BLOCK:(b + 1) * BLOCK]) for b in range(nblocks)]
            total = float(np.sum(np.asarray(partials, dtype=np.float64))) if partials else 0.0
        scale = 1.0 if mutant == "grad_scale_ignored" else abs(float(grad_scale))
        norm = scale * float(np.sqrt(np.float64(total)))
    return norm, _coef(norm, max_norm, eps=0.0 if mutant == "no_eps" else EPS, clamp=mutant != "unclamped")


def rel_diff(a, b):
    """|a - b| / |b| (0 for equal values, inf where exactly one is not finite or b is 0 and a is not)."""
    if a == b or (math.isnan(a) and math.isnan(b)):
        return 0.0
    if not (math.isfinite(a) and math.isfinite(b)) or b == 0.0:
        return math.inf
    return abs(a - b) / abs(b)


def one_hot(n, i, value):
    g = np.zeros(n, dtype=np.float32)
    g[i] = value
    return g


def stress_gradient(n=N_ACCURACY, seed=7):
    """optimizer_reference.stress_state's gradient family: |g| log-uniform in [1e-12, 1e6], finite by construction."""
    return R.stress_state(n, np.random.default_rng(seed))["g"]


def family(accuracy_n=N_ACCURACY):
    """The inputs of tests/test_grad_clip_kernels_gpu.py: name -> (g, grad_scale, max_norm), grad_scale and max_norm fp32 values.
    positions: one non-zero element first / last of a block / first of the next / last of the buffer, coef < 1
    range:     one 3e19 (square above FLT_MAX) or 1e-30 (square below the smallest fp32 denormal), three gradient scales
    accuracy:  the stress gradients, clipped and measured only
    coef:      the clamp at exactly 1 from norm + 1e-6 on, max_norm = inf, and the visible 1e-6"""
    out = {}
    for n in SIZES:
        for pos in POSITIONS:
            i = n - 1 if pos < 0 else pos
            if i < n:
                out[f"position n={n} i={i}"] = (one_hot(n, i, -1.5), f32(1.0 / 3), f32(0.25))
    for value in (3e19, 1e-30):
        for gs in SCALES:
            out[f"range {value:g} gs={gs:.4f}"] = (one_hot(4100, 4097, value), f32(gs), f32(1.0))
    g = stress_gradient(accuracy_n)
    out["accuracy clipped"] = (g, f32(1.0 / 3), f32(1.0))
    out["accuracy measured"] = (g, f32(1.0 / 8), math.inf)
    half = one_hot(8, 5, 0.5)
    out["coef clamped"] = (half, 1.0, f32(0.5 + 2e-6))
    out["coef just below"] = (half, 1.0, f32(0.5))
    out["coef far above"] = (half, 1.0, f32(40.0))
    out["coef inf"] = (half, 1.0, math.inf)
    out["coef eps visible"] = (one_hot(8, 2, 2e-5), 1.0, f32(1e-5))
    return out
