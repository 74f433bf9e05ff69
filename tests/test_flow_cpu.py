"""Rectified flow without a device: the solver plan of RectifiedFlow._schedule against the numpy restatement (tests/flow_reference.py),
the restatement against an exact solution of the flow ODE, argument errors, CLI parsing and the objective / sampler refusals."""
import numpy as np
import pytest
import torch

import flow_reference as R

DRAW_SEED, DRAW_N = 2024, 100_000          # the logit-normal draw of tests/test_flow_gpu.py (checked here to be robust to one ulp of z)


def make_flow(T=1000, shift=1.0):
    from mapdit_amd.flow import create_flow
    return create_flow(num_timesteps=T, shift=shift)


@pytest.mark.parametrize("T,shift", [(1000, 1.0), (1000, 3.0), (7, 1.0), (7, 3.0), (1, 1.0), (16384, 3.0)])
def test_time_grid(T, shift):
    f = make_flow(T, shift)
    assert f.num_timesteps == T and f.sigmas.dtype == np.float64 and f.sigmas.shape == (T,)
    np.testing.assert_allclose(f.sigmas, R.sigmas(T, shift), rtol=1e-15)
    assert f.sigmas[0] > 0 and f.sigmas[-1] == 1.0 and (np.diff(f.sigmas) > 0).all()
    assert (np.diff(f.sigmas.astype(np.float32)) > 0).all()            # the device copy still tells the grid points apart
    if shift == 1.0:
        np.testing.assert_allclose(f.sigmas, (np.arange(T) + 1) / T, rtol=1e-15)


CASES = [(1000, s, k) for s in (1.0, 3.0) for k in (2, 10, 50, 1000)] + [(7, 1.0, 20), (7, 3.0, 20)]


@pytest.mark.parametrize("T,shift,num_steps", CASES)
@pytest.mark.parametrize("order", [1, 2])
def test_schedule(T, shift, num_steps, order):
    f = make_flow(T, shift)
    plan = f._schedule(num_steps, order)
    steps, h, t, coef, kind = R.schedule(f.sigmas, shift, num_steps, order)
    assert np.array_equal(plan.steps, steps) and np.array_equal(plan.t, t) and np.array_equal(plan.kind, kind)
    np.testing.assert_allclose(plan.h, h, rtol=1e-14)
    np.testing.assert_allclose(plan.coef, coef, rtol=1e-14)
    K = len(plan.steps)
    assert K <= min(num_steps, T) and (K < num_steps) == (T == 7)       # T = 7, 20 targets: duplicates are dropped
    if T == 1000:
        assert K == num_steps
    times = f.sigmas[plan.steps]
    assert plan.steps[0] == T - 1 and (np.diff(plan.steps) < 0).all() and (np.diff(times) < 0).all()
    assert (plan.h < 0).all()
    assert plan.h[-1] == -times[-1]                                      # the last step ends at exactly 0
    np.testing.assert_allclose(plan.h.sum(), -f.sigmas[T - 1], rtol=1e-13)
    np.testing.assert_allclose(plan.h[:-1], times[1:] - times[:-1], rtol=0, atol=0)   # differences of the table values used
    commit = plan.kind == 0
    np.testing.assert_allclose(plan.coef[commit].sum(), -1.0, rtol=1e-13)            # the committing rows carry every step once
    if order == 1:
        assert len(plan.t) == K and commit.all() and (plan.coef[:, 0] == 0).all()
        assert np.array_equal(plan.t, plan.steps)
    else:
        assert len(plan.t) == 2 * K - 1
        assert plan.kind[-1] == 0 and plan.coef[-1, 0] == 0 and plan.t[-1] == plan.steps[-1]         # the final row is an Euler row
        assert (plan.kind[:-1] == np.tile([1, 0], K - 1)).all()
        assert np.array_equal(plan.t[:-1:2], plan.steps[:-1]) and np.array_equal(plan.t[1:-1:2], plan.steps[1:])
        assert (plan.coef[:-1:2, 0] == 0).all() and np.array_equal(plan.coef[1:-1:2, 0], plan.coef[1:-1:2, 1])


def test_bad_arguments_raise_value_error():
    from mapdit_amd.flow import create_flow
    f = make_flow()
    for bad in (0, -3, 2.5, "10", None, True):
        with pytest.raises(ValueError, match="num_steps"):
            f._schedule(bad, 1)
    for bad in (0, 3, 1.5, None, True):
        with pytest.raises(ValueError, match="order"):
            f._schedule(10, bad)
    for bad in (0.0, -1.0, float("inf"), float("nan"), None, "3"):
        with pytest.raises(ValueError, match="shift"):
            create_flow(shift=bad)
    for bad in (0, 16385, -1, 10.0, None):
        with pytest.raises(ValueError, match="num_timesteps"):
            create_flow(num_timesteps=bad)
    with pytest.raises(ValueError, match="shift"):
        create_flow(num_timesteps=16384, shift=1e6)                     # grid points that fp32 cannot tell apart
    with pytest.raises(TypeError):
        f.sample_loop(None, (1, 4, 8, 8), clip_denoised=True)           # the hooks and the clip are not accepted
    with pytest.raises(ValueError, match="density"):
        f.sample_timesteps(4, "cuda", density="lognormal")


EXPECTED = {1: (1.384e-1, 7.15e-2, 3.64e-2), 2: (1.84e-2, 4.22e-3, 1.01e-3)}


@pytest.mark.parametrize("order", [1, 2])
def test_restatement_converges_to_the_exact_solution(order):
    """Data N(0, c^2 I), c = 0.5: the exact velocity is a(s) x and the ODE ends at c x(1) (flow_reference.exact_velocity_coef).  Relative
    error max |got - exact| / max |exact| at K = 10 / 20 / 40, T = 1000, shift 1 - the figures of the issue, held to 1 %."""
    sig = R.sigmas(1000, 1.0)
    x1 = np.random.default_rng(0).standard_normal((2, 4, 8, 8))
    exact = R.C_DATA * x1
    errs = []
    for K in (10, 20, 40):
        out = R.sample_loop(lambda x, k: R.exact_velocity_coef(sig[k]) * x, x1, sig, 1.0, K, order)
        errs.append(float(np.abs(out - exact).max() / np.abs(exact).max()))
    print(order, [f"{e:.4e}" for e in errs], errs[0] / errs[1], errs[1] / errs[2])
    for got, want in zip(errs, EXPECTED[order]):
        assert abs(got - want) <= 0.01 * want, (got, want)
    ratios = (errs[0] / errs[1], errs[1] / errs[2])
    for got, want in zip(ratios, {1: (1.94, 1.97), 2: (4.35, 4.19)}[order]):
        assert abs(got - want) <= 0.01 * want, (got, want)


def test_package_plan_reaches_the_same_errors():
    """The same loop on the plan RectifiedFlow._schedule builds (host side only): what the device kernels are handed."""
    f = make_flow()
    x1 = np.random.default_rng(0).standard_normal((2, 4, 8, 8))
    for order in (1, 2):
        for K, want in zip((10, 20, 40), EXPECTED[order]):
            plan = f._schedule(K, order)
            x = base = x1.copy()
            hist = np.zeros_like(x1)
            for k, (c_h, c_v), pred in zip(plan.t, plan.coef, plan.kind):
                x, base, hist, _ = R.step(base, hist, R.exact_velocity_coef(f.sigmas[k]) * x, c_h, c_v, bool(pred))
            err = float(np.abs(x - R.C_DATA * x1).max() / np.abs(R.C_DATA * x1).max())
            assert abs(err - want) <= 0.01 * want, (order, K, err, want)


def test_logit_normal_seed_is_robust_to_one_ulp():
    """The device's exp may differ from numpy's in the last place; the GPU test allows at most 1 index in 10,000 to differ, each by
    exactly 1.  The seed is chosen so that numpy against itself with z moved by one ulp either way stays inside that cap."""
    z = np.random.default_rng(DRAW_SEED).standard_normal(DRAW_N)
    for T, loc, scale in ((1000, 0.0, 1.0), (7, 0.5, 1.5)):
        base = R.logit_normal_index(z, loc, scale, T)
        assert base.min() >= 0 and base.max() <= T - 1 and len(np.unique(base)) >= min(T, 900) * 0.9
        for towards in (-np.inf, np.inf):
            other = R.logit_normal_index(np.nextafter(z, towards), loc, scale, T)
            diff = np.abs(other - base)
            print(T, towards, int((diff > 0).sum()))
            assert (diff > 0).sum() * 10_000 <= DRAW_N and diff.max(initial=0) <= 1
    assert R.logit_normal_index(np.array([-700.0, 700.0, 0.0]), 0.0, 1.0, 1000).tolist() == [0, 999, 500]


def test_cpu_tensors_are_refused():
    f = make_flow()
    x, t = torch.zeros(2, 4, 8, 8), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        f.q_sample(x, t)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        f.training_losses(lambda *a, **k: x, x, t)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        f.pred_xstart_from_velocity(x, t, x)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        f.sample_timesteps(4, "cpu")
    with pytest.raises(NotImplementedError, match="no CPU path"):
        f.sample_timesteps(4, torch.device("cpu"), density="logit-normal")
    with pytest.raises(NotImplementedError, match="no CPU path"):
        f.timesteps_from_normals(torch.zeros(4, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="no CPU path"):
        f.q_sample(np.zeros((2, 4, 8, 8)), t)


def test_schedule_sampler_takes_a_flow():
    """create_named_schedule_sampler needs num_timesteps only."""
    from mapdit_amd.diffusion.timestep_sampler import LossSecondMomentResampler, UniformSampler, create_named_schedule_sampler
    f = make_flow(250)
    s = create_named_schedule_sampler("loss-second-moment", f)
    assert isinstance(s, LossSecondMomentResampler) and s.diffusion is f and s._T == 250
    assert isinstance(create_named_schedule_sampler("uniform", f), UniformSampler)


def test_train_flags_parse():
    from mapdit_amd import train
    p = train.build_parser()
    a = p.parse_args(["--results-dir", "r"])
    assert (a.objective, a.flow_shift, a.flow_timestep_density) == ("diffusion", 1.0, "uniform")
    a = p.parse_args(["--results-dir", "r", "--objective", "flow", "--flow-shift", "3", "--flow-timestep-density", "logit-normal"])
    assert (a.objective, a.flow_shift, a.flow_timestep_density) == ("flow", 3.0, "logit-normal")
    with pytest.raises(SystemExit):
        p.parse_args(["--results-dir", "r", "--objective", "velocity"])
    # refused before any device work
    with pytest.raises(ValueError, match="--objective flow"):
        train.main(["--synthetic", "--results-dir", "r", "--batch-size", "4", "--flow-shift", "3"])
    with pytest.raises(ValueError, match="--objective flow"):
        train.main(["--synthetic", "--results-dir", "r", "--batch-size", "4", "--flow-timestep-density", "logit-normal"])
    with pytest.raises(ValueError, match="shift"):
        train.main(["--synthetic", "--results-dir", "r", "--batch-size", "4", "--objective", "flow", "--flow-shift", "-1"])


def test_sampler_flags_and_objective_refusals():
    import argparse

    from mapdit_amd import sample, sample_ema, sample_fid
    from mapdit_amd import sampling as S
    from mapdit_amd.flow import RectifiedFlow
    for mod in (sample, sample_fid, sample_ema):
        a = mod.build_parser().parse_args(["--result-dir", "r", "--sampler", "flow-heun", "--num-sampling-steps", "4"])
        assert a.sampler == "flow-heun" and a.num_sampling_steps == 4
        assert mod.build_parser().parse_args(["--result-dir", "r"]).sampler == "ancestral"
    args = argparse.Namespace(sampler="flow-heun", num_sampling_steps=4, solver_order=2, solver_spacing="logsnr")
    flow, kw = S.make_diffusion(args, {"objective": "flow", "flow_shift": 3.0})
    assert isinstance(flow, RectifiedFlow) and flow.shift == 3.0 and kw == dict(sampler="flow", num_steps=4, order=2)
    args.sampler = "flow-euler"
    assert S.make_diffusion(args, {"objective": "flow"})[1] == dict(sampler="flow", num_steps=4, order=1)
    # a flow run refuses the diffusion samplers, and the message names the flag to pass
    for sampler in ("ancestral", "dpm++"):
        args.sampler = sampler
        with pytest.raises(ValueError, match="--sampler flow-euler or --sampler flow-heun"):
            S.make_diffusion(args, {"objective": "flow", "flow_shift": 1.0})
    # the reverse; a config.yaml from before the key existed counts as diffusion
    for cfg in ({"objective": "diffusion"}, {}, None):
        for sampler in ("flow-euler", "flow-heun"):
            args.sampler = sampler
            with pytest.raises(ValueError, match="--sampler ancestral or --sampler dpm\\+\\+"):
                S.make_diffusion(args, cfg)
    args.sampler = "dpm++"
    d, kw = S.make_diffusion(args, {})
    assert d.num_timesteps == 1000 and kw["sampler"] == "dpm++"
    args.sampler = "ancestral"
    d, kw = S.make_diffusion(args)
    assert d.num_timesteps == 4 and kw == {}


def test_graphed_sampler_refuses_a_mismatched_process():
    """Decided before anything touches a device: the error names both the sampler and the process."""
    from mapdit_amd import sampling as S
    from mapdit_amd.diffusion import create_diffusion

    class Eval:
        training = False
    for sampler in ("ancestral", "dpm++"):
        with pytest.raises(ValueError, match=f"(?s)flow.*{sampler.replace('+', '.')}.*RectifiedFlow"):
            S.GraphedSampler(Eval(), make_flow(), (2, 4, 8, 8), None, sampler=sampler)
    with pytest.raises(ValueError, match="(?s)flow.*SpacedDiffusion"):
        S.GraphedSampler(Eval(), create_diffusion("10"), (2, 4, 8, 8), None, sampler="flow")
    with pytest.raises(ValueError, match="(?s)flow.*SpacedDiffusion"):
        S.run_sampler(Eval(), create_diffusion("10"), torch.zeros(2, 4, 8, 8), None, None, use_graph=False, sampler="flow")
