"""Global gradient-norm clipping, the parts that need no GPU: tests/grad_clip_reference.py against torch.nn.utils.clip_grad_norm_ in
fp64, the proof that the GPU tests' inputs tell wrong variants of the computation apart, and the harness' --max-grad-norm."""
import math

import numpy as np
import pytest
import torch

import grad_clip_reference as G


@pytest.fixture(scope="module")
def family():
    return G.family()


@pytest.mark.parametrize("gs", [1.0, 1.0 / 8, 1.0 / 3])
def test_clip64_is_torch_clip_grad_norm_in_fp64(gs):
    """One flat fp32 vector cut into "parameters" in several ways; the optimiser's gradient g * grad_scale as fp64 CPU tensors through
    torch.nn.utils.clip_grad_norm_ with max_norm below the norm, above it and inf: the returned total norm and the factor the gradients
    were multiplied by agree with clip64 to 1e-12, whatever the split."""
    rng = np.random.default_rng(17)
    n = 10007
    g = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 2, n)).astype(np.float32)
    gs = G.f32(gs)
    norm0, _ = G.clip64(g, gs, math.inf)
    assert norm0 > 1.0
    splits = ([n], [1, n - 1], [4096, 4096, n - 8192], [3, 1000, 4, 9000], [100] * 100 + [7])
    for max_norm in (G.f32(0.5 * norm0), G.f32(1e-3), G.f32(2.0 * norm0), G.f32(norm0 + 1.0), math.inf):
        want_norm, want_coef = G.clip64(g, gs, max_norm)
        assert (want_coef == 1.0) == (max_norm >= norm0 + G.EPS)
        for sizes in splits:
            assert sum(sizes) == n
            params, off = [], 0
            for k in sizes:
                p = torch.nn.Parameter(torch.zeros(k, dtype=torch.float64))
                p.grad = torch.from_numpy(g[off:off + k].astype(np.float64)) * gs
                params.append(p)
                off += k
            before = torch.cat([p.grad.clone() for p in params])
            total = float(torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2))
            after = torch.cat([p.grad for p in params])
            i = int(before.abs().argmax())
            coef = float(after[i] / before[i])
            assert abs(total - want_norm) <= 1e-12 * want_norm, (max_norm, sizes[:3], total, want_norm)
            assert abs(coef - want_coef) <= 1e-12 * want_coef, (max_norm, sizes[:3], coef, want_coef)
            assert torch.allclose(after, before * want_coef, rtol=1e-12, atol=0.0)


def test_emulate_without_a_mutant_is_clip64(family):
    """The kernels' structure (a partial sum per 4,096 elements, then their sum) agrees with the plain fp64 sum far inside the GPU bound."""
    for name, (g, gs, mx) in family.items():
        want, got = G.clip64(g, gs, mx), G.emulate(g, gs, mx)
        assert all(math.isfinite(x) for x in want), name
        assert G.rel_diff(got[0], want[0]) < 1e-12 and G.rel_diff(got[1], want[1]) < 1e-12, (name, got, want)


@pytest.mark.parametrize("mutant", G.MUTANTS)
def test_the_gpu_inputs_tell_every_mutant_apart(mutant, family):
    """On at least one case of family() - the inputs of tests/test_grad_clip_kernels_gpu.py - each wrong variant ends further from clip64
    than the GPU tolerance of 2^-23, in the norm or in the coefficient; printed: the cases that see it."""
    seen = []
    for name, (g, gs, mx) in family.items():
        want, got = G.clip64(g, gs, mx), G.emulate(g, gs, mx, mutant)
        d = max(G.rel_diff(got[0], want[0]), G.rel_diff(got[1], want[1]))
        if d > G.TOL:
            seen.append((name, d))
    print(f"{mutant}: seen by {len(seen)} of {len(family)} cases, e.g. {seen[:3]}")
    assert seen, mutant
    expected = {"grad_scale_ignored": "position", "no_eps": "coef eps visible", "unclamped": "coef far above", "fp32_squares": "range 3e+19",
                "tail_block_dropped": "position n=4100 i=4099"}[mutant]
    assert any(name.startswith(expected) for name, _ in seen), (mutant, seen)


def test_the_named_values_of_the_family(family):
    """What the issue names: the 1e-6 is visible (0.476, not 0.5), the clamp is exact from norm + 1e-6 on and not below, 3e19 and 1e-30 give
    the finite norms |value * grad_scale|, and the stress gradients are finite with a norm far above every max_norm used."""
    assert G.clip64(*family["coef eps visible"])[1] == pytest.approx(0.476, abs=5e-4)
    assert G.clip64(*family["coef clamped"])[1] == 1.0 and G.clip64(*family["coef inf"])[1] == 1.0
    assert 0.99999 < G.clip64(*family["coef just below"])[1] < 1.0
    assert np.float32(G.clip64(*family["coef just below"])[1]) != np.float32(1.0)
    for value in (3e19, 1e-30):
        for gs in G.SCALES:
            norm, _ = G.clip64(*family[f"range {value:g} gs={gs:.4f}"])
            assert norm == pytest.approx(float(np.float32(value)) * G.f32(gs), rel=1e-15) and np.isfinite(np.float32(norm)) and np.float32(norm) > 0
    g = family["accuracy clipped"][0]
    assert g.size == 1 << 22 and np.isfinite(g).all() and float(np.abs(g).max()) <= 1e6
    assert G.clip64(*family["accuracy clipped"])[1] < 1e-3 and G.clip64(*family["accuracy measured"])[1] == 1.0


def test_parser_accepts_max_grad_norm_and_defaults_to_none(tmp_path):
    from mapdit_amd import train
    base = ["--synthetic", "--results-dir", str(tmp_path)]
    assert train.build_parser().parse_args(base).max_grad_norm is None
    assert train.build_parser().parse_args(base + ["--max-grad-norm", "1.0"]).max_grad_norm == 1.0
    assert train.build_parser().parse_args(base + ["--max-grad-norm", "inf"]).max_grad_norm == math.inf


def test_sharded_weight_passes_refuse_clipping_by_name():
    """ShardedPassReducer.attach refuses an optimiser with max_grad_norm, naming both, and arms the refusal of step() for an attribute
    set later (no device is needed: the refusals come before any launch)."""
    from mapdit_amd import parallel
    from mapdit_amd._lib import MapditError

    class Opt:
        max_grad_norm = 1.0
        _clip_refused = None

    with pytest.raises(MapditError, match=r"max_grad_norm.*zero1w"):
        parallel.ShardedPassReducer.attach(object.__new__(parallel.ShardedPassReducer), Opt())
    assert "max_grad_norm" in parallel.SHARDED_CLIP_ERROR and "sharded weight passes" in parallel.SHARDED_CLIP_ERROR
