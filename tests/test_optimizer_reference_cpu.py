"""tests/optimizer_reference.py checked on the CPU, so that tests/test_optimizer_kernels_gpu.py does not lean on an unverified reference:
step64 against torch.optim.Adam on fp64 tensors, hyper() against the golden fixtures and the oracle, the measurement the GPU bound is
built on (a plain fp32 evaluation stays within 4 error scales of step64 on the stress inputs; the GPU tests allow 8), and the proof that
those inputs tell wrong variants of the update apart (four mutants, each beyond 8 scales).
"""
import math

import numpy as np
import pytest
import torch

import optimizer_reference as R
from conftest import load_golden

B1, B2, EPS = R.f32(0.9), R.f32(0.99), R.f32(1e-8)      # the betas and eps as a `float` argument of the C ABI carries them
STEPS = (1, 2, 10, 1000, 100000)
SCALES = (1.0, 1.0 / 8, 1.0 / 3, 1.0 / 7)
STDS = (0.05, 0.1)


@pytest.fixture(scope="module")
def stress():
    s = R.stress_state(1 << 20, np.random.default_rng(2024))
    for z in s.values():
        z.setflags(write=False)
    return s


def test_step64_is_torch_adam_plus_lerp_in_fp64():
    """grad_scale 1, five consecutive steps from zero moments, the fp64 state carried from step to step: torch.optim.Adam on fp64 tensors
    (lr 1e-2, betas (0.9, 0.99), eps 1e-8 - the fp32 values of the three, which is what step64 is defined on) and ema.lerp_(p, beta) in
    fp64, to 1e-12 relative, every quantity after every step."""
    n = 4096
    rng = np.random.default_rng(5)
    w = torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n)))
    opt = torch.optim.Adam([w], lr=1e-2, betas=(B1, B2), eps=EPS)
    ema = [w.detach().clone(), w.detach().clone()]
    s = {k: w.detach().numpy().copy() for k in ("p", "ea", "eb")}
    s["m"], s["v"] = np.zeros(n), np.zeros(n)
    for t in range(1, 6):
        g = rng.standard_normal(n) * 10.0 ** rng.integers(-4, 1, n)
        w.grad = torch.from_numpy(g.copy())
        opt.step()
        hy = R.hyper64(t, 1e-2, B1, B2, STDS, 1.0)
        for e, beta in zip(ema, hy[2:4]):
            e.lerp_(w.detach(), float(beta))
        s, _ = R.step64(s["p"], g, s["m"], s["v"], s["ea"], s["eb"], hy, B1, B2, EPS)
        st = opt.state[w]
        for got, want in ((s["p"], w.detach()), (s["m"], st["exp_avg"]), (s["v"], st["exp_avg_sq"]), (s["ea"], ema[0]), (s["eb"], ema[1])):
            assert float(np.max(np.abs(got - want.numpy()))) <= 1e-12 * float(want.abs().max()), t
    assert int(opt.state[w]["step"]) == 5
    assert not np.array_equal(s["ea"], s["eb"]) and not np.array_equal(s["ea"], s["p"])


def test_hyper_against_fixtures_and_oracle():
    """The EMA exponents and beta(100) are in tables.npz (written by the reference's own src/ema.py); optim3.npz holds three recorded
    steps of the reference (fp32): at step 1 the update of an element is lr * sign(g) wherever |g| >> eps, which pins
    step_size (1 - b1) / (sqrt(1 - b2) inv_sqrt_bc2) = lr, and at step 2 the copies moved by beta(2) of their distance to the new weights.
    Everything else against oracle.dit_oracle and the closed forms."""
    from oracle import dit_oracle as O
    tab = load_golden("tables")
    assert np.allclose([R.gamma_of_std(s) for s in STDS], tab["ema_gamma"], rtol=1e-12, atol=0)
    assert np.allclose(R.hyper64(100, 1e-2, 0.9, 0.99, STDS, 1.0)[2:4], tab["ema_beta_t100"], rtol=1e-12, atol=0)
    for t in (1, 2, 3, 7, 100, 1000, 100000):
        for lr, gs in ((1e-2, 1.0), (3.3e-3, 1.0 / 3)):
            h = R.hyper64(t, lr, 0.9, 0.99, STDS, gs)
            want = [lr / (1 - 0.9 ** t), 1 / math.sqrt(1 - 0.99 ** t), O.ema_beta(0.05, t), O.ema_beta(0.1, t), gs]
            assert np.allclose(h, want, rtol=1e-12, atol=0), (t, h, want)
            h32 = R.hyper(t, lr, 0.9, 0.99, STDS, gs)
            assert h32.dtype == np.float32 and np.array_equal(h32, h.astype(np.float32))
    assert np.array_equal(R.hyper64(1, 1e-2, 0.9, 0.99, STDS, 1.0)[2:4], [0.0, 0.0])          # beta(1) = 0: the copies keep their value
    assert np.array_equal(R.hyper64(5, 1e-2, 0.9, 0.99, (), 1.0)[2:4], [0.0, 0.0])
    g = load_golden("optim3")
    key = "final_layer.linear.weight"                                                        # (no forced weight norm on the recorded values' scale)
    w2 = g[f"s2/w/{key}"].astype(np.float64)
    e1 = {s: g[f"s1/ema{s}/{key}"].astype(np.float64) for s in ("0.05", "0.1")}
    e2 = {s: g[f"s2/ema{s}/{key}"].astype(np.float64) for s in ("0.05", "0.1")}
    h1, h2 = R.hyper64(1, 1e-2, 0.9, 0.99, STDS, 1.0), R.hyper64(2, 1e-2, 0.9, 0.99, STDS, 1.0)
    assert np.array_equal(e1["0.05"], e1["0.1"])                                             # beta(1) = 0: both are still the initial weights
    b1, b2 = 0.9, 0.99
    assert h1[0] * (1 - b1) / (math.sqrt(1 - b2) * h1[1]) == pytest.approx(1e-2, rel=1e-12)  # |first update| = lr
    for k in ("blocks.0.gain_msa", "final_layer.mean_scale.reference"):                      # (parameters the forward does not renormalise)
        first = np.abs(g[f"s1/w/{k}"].astype(np.float64) - g[f"s1/ema0.05/{k}"].astype(np.float64))
        assert float(np.max(np.abs(first - 1e-2))) <= 1e-5 + 4 * R.U24 * float(np.max(np.abs(g[f"s1/w/{k}"])))
    for s, beta in (("0.05", h2[2]), ("0.1", h2[3])):
        want = e1[s] + beta * (w2 - e1[s])
        assert float(np.max(np.abs(e2[s] - want))) <= 4 * R.U24 * float(np.max(np.abs(want)))


def test_emulation_within_4_scales_and_reference_finite(stress):
    """THE measurement behind the GPU bound: numpy fp32 in the kernel's operation order against step64 on 2^20 stress elements, t in STEPS,
    grad_scale in SCALES.  Worst ratios measured: m' 2.60, v' 3.94, p' 2.23, e' 2.19 / 2.06 scales - asserted <= 4, so that the GPU limit
    of 8 stays twice the worst case of a plain fp32 evaluation.  The reference itself stays finite on the family."""
    worst = {}
    for t in STEPS:
        for gs in SCALES:
            hy = R.hyper(t, 1e-2, 0.9, 0.99, STDS, gs)
            want, scale = R.step64(*R.args_of(stress), hy, B1, B2, EPS)
            assert all(np.isfinite(want[k]).all() and np.isfinite(scale[k]).all() for k in R.QUANTITIES), (t, gs)
            r = R.ratios(R.emulate32(*R.args_of(stress), hy, B1, B2, EPS), want, scale)
            for k, x in r.items():
                worst[k] = max(worst.get(k, 0.0), x)
    print("ratio emulate32 / step64 on stress_state(2^20): " + ", ".join(f"{k} {x:.2f}" for k, x in worst.items()) + " (limit 4)")
    assert set(worst) == set(R.QUANTITIES)
    assert all(x <= 4.0 for x in worst.values()), worst
    assert all(x >= 1.0 for x in worst.values()), worst                                      # (the scales are not slack by an order of magnitude either)


def test_stress_state_is_the_documented_family():
    s = R.stress_state(65540, np.random.default_rng(3))
    assert all(s[k].dtype == np.float32 and s[k].shape == (65540,) for k in ("p", "g", "m", "v", "ea", "eb"))
    body = slice(R.HAND, None)
    idx = np.arange(65540)[body]
    assert np.all(s["g"][body][idx % 17 == 0] == 0) and np.all(s["m"][body][idx % 13 == 0] == 0) and np.all(s["v"][body][idx % 11 == 0] == 0)
    assert np.all(s["v"] >= 0) and float(s["v"].max()) <= 1.0001e12 and float(np.abs(s["g"]).max()) <= R.GRAD_MAX
    nz = np.abs(s["g"][body][s["g"][body] != 0])
    assert 1e-12 * 0.999 <= float(nz.min()) < 1e-11 and 1e5 < float(nz.max())
    assert float(np.max(np.abs(s["ea"] - s["p"]) - 0.0101 * np.abs(s["p"]))) <= 0
    # the hand-picked block: the all-zero elements, the underflowing squares, v = eps^2, and the cancelling pairs for every scale
    assert np.all(s["g"][:4] == 0) and np.all(s["m"][:4] == 0) and np.all(s["v"][:4] == 0)
    assert np.all(np.abs(s["g"][4:12]) == np.float32(1e-25)) and np.all(np.float32(s["g"][4:12]) ** 2 == 0) and np.all(s["v"][4:12] > 0)
    assert np.all(s["v"][12:20] == np.float32(1e-16))
    for j, gs in enumerate(SCALES):
        q = slice(24 + 10 * j, 34 + 10 * j)
        a, b = 0.9 * s["m"][q].astype(np.float64), 0.1 * s["g"][q].astype(np.float64) * gs
        assert np.all(a * b < 0) and float(np.max(np.abs(a + b) / np.abs(a))) <= 1.1e-2


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_stress_state_tells_the_mutants_apart(mutant):
    """eps inside the square root, the bias correction c dropped, grad_scale on the first moment only, the EMA lerped towards the old p:
    each is beyond 8 scales on the n = 65,536 + 4 inputs the GPU tests use (t = 10: c = 3.2 and beta > 0; grad_scale 1/3), while the
    unmutated emulation stays within 4 there - the family can tell the variants apart."""
    s = R.stress_state(65540, np.random.default_rng(3))
    hy = R.hyper(10, 1e-2, 0.9, 0.99, STDS, 1.0 / 3)
    want, scale = R.step64(*R.args_of(s), hy, B1, B2, EPS)
    clean = R.ratios(R.emulate32(*R.args_of(s), hy, B1, B2, EPS), want, scale)
    bad = R.ratios(R.emulate32(*R.args_of(s), hy, B1, B2, EPS, mutant=mutant), want, scale)
    assert max(clean.values()) <= 4.0
    hit = {"eps_in_sqrt": ("p", "ea", "eb"), "no_bias_correction": ("p", "ea", "eb"), "grad_scale_m_only": ("v", "p"), "ema_old_p": ("ea", "eb")}[mutant]
    assert all(bad[k] > 8.0 for k in hit), bad
    if mutant == "ema_old_p":
        assert bad["p"] <= 4.0 and bad["m"] <= 4.0 and bad["v"] <= 4.0
    # ... and on the hand-picked block alone (the random part is not what carries the distinction for the denominator variants)
    h = {k: z[:R.HAND] for k, z in s.items()}
    wh, sh = R.step64(*R.args_of(h), hy, B1, B2, EPS)
    badh = R.ratios(R.emulate32(*R.args_of(h), hy, B1, B2, EPS, mutant=mutant), wh, sh)
    assert max(badh[k] for k in hit) > 8.0, badh
