"""Rectified flow on the GPU: the four mapdit_flow_* kernels against the fp64 restatement of tests/flow_reference.py, the logit-normal
draw, refusals and device-error reports, the loss reaching the parameter gradients, convergence to an exact solution of the flow ODE,
the captured sampler against the eager loop, launch counts, and the training / sampling scripts.

Rounding bounds (fp32 kernel against fp64 on the same fp32 sig table and fp32 plan coefficients), elementwise, U = 16 x 2^-24 - a
handful of roundings of at most 2^-24 of the term magnitudes each, and room for FMA contraction, as tests/test_dpm_solver_gpu.py:
    q_sample     |err| <= U (|(1 - s) x0| + |s eps|)                     (1 - s, two products, one sum)
    G            |err| <= U (|v| + |eps| + |x0|) 2 / per_sample          (two differences, 1 / per_sample, two products)
    loss         |err| <= sum_e |G_e| U (|v| + |eps| + |x0|)_e + (ceil(per_sample / 256) + 12) 2^-24 loss
                 (the error of each difference through d loss / d diff_e = G_e; then a lane's ceil(per_sample / 256) additions, six
                 butterfly levels, three wave totals, the square, the 1 / per_sample and its product)
    flow_step    |err| <= U (|base| + |c_h hist| + |c_v v|);   pred_xstart: U (|x_eval| + |s v|)
"""
import math
import os
import re

import numpy as np
import pytest
import torch

import flow_reference as R
from test_flow_cpu import DRAW_N, DRAW_SEED

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 16 * 2.0 ** -24


def make_flow(T=1000, shift=1.0):
    from mapdit_amd.flow import create_flow
    return create_flow(num_timesteps=T, shift=shift)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def lib():
    from mapdit_amd import _lib as L
    return L.lib()


def stream():
    from mapdit_amd import _lib as L
    return L.cur_stream()


def poll():
    lib().device_error_poll(stream())


def t_sets(N, T):
    """Timesteps that hold 0, T - 1 and values that differ per sample."""
    if N == 3:
        return [[0, T - 1, T // 3]]
    return [[0, T - 1], [T // 3, T - 2]]


SHAPES = [(3, 4, 6, 6), (2, 4, 8, 8), (2, 4, 32, 32)]          # per_sample 144 (ragged, under one block), 256, 4,096 (several passes)


@pytest.mark.parametrize("T,shift", [(1000, 1.0), (1000, 3.0), (7, 1.0), (7, 3.0)])
@pytest.mark.parametrize("shape", SHAPES)
def test_q_sample_matches_fp64(shape, T, shift):
    f = make_flow(T, shift)
    sig32 = _np(f._tables(torch.device(DEV)))
    assert np.array_equal(sig32, f.sigmas.astype(np.float32).astype(np.float64))
    g = torch.Generator().manual_seed(sum(shape) + T)
    x0, eps = (torch.randn(shape, generator=g).to(DEV) for _ in range(2))
    worst = 0.0
    for ts in t_sets(shape[0], T):
        t = torch.tensor(ts, device=DEV)
        got = f.q_sample(x0, t, eps)
        ref, mag = R.q_sample(_np(x0), _np(eps), sig32[np.array(ts)])
        err = np.abs(_np(got) - ref)
        worst = max(worst, float((err / (U * mag)).max()))
        assert (err <= U * mag).all(), worst
        assert torch.equal(f.q_sample(x0, t, eps), got)                        # two runs, the same bits
        if T - 1 in ts:                                                        # s = 1 is pure noise, exactly
            assert torch.equal(got[ts.index(T - 1)], eps[ts.index(T - 1)])
    # an odd base address takes the one-element kernel: the same values
    pad = torch.zeros(x0.numel() + 1, device=DEV)
    pad[1:] = x0.flatten()
    err = np.abs(_np(f.q_sample(pad[1:].view(shape), t, eps)) - ref)
    assert (err <= U * mag).all()
    xs = f.pred_xstart_from_velocity(got, t, eps - x0)
    assert float((xs - x0).abs().max()) < 1e-5
    poll()
    print(f"q_sample {shape} T={T} shift={shift}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_loss_and_gradient_match_fp64(shape, groups):
    N, C = shape[:2]
    per = int(np.prod(shape[1:]))
    g = torch.Generator().manual_seed(sum(shape) + groups)
    x0, eps = (torch.randn(shape, generator=g).to(DEV) for _ in range(2))
    mo = torch.randn(N, groups * C, *shape[2:], generator=g).to(DEV)
    ref_loss, ref_G = R.loss_and_grad(_np(mo[:, :C]), _np(x0), _np(eps))
    mag = np.abs(_np(mo[:, :C])) + np.abs(_np(eps)) + np.abs(_np(x0))
    outs = []
    for _ in range(2):
        G = torch.full_like(mo, float("nan"))
        loss = torch.full((N,), float("nan"), device=DEV)
        lib().flow_loss_fwd(mo.data_ptr(), x0.data_ptr(), eps.data_ptr(), loss.data_ptr(), G.data_ptr(), N, per, groups, stream())
        outs.append((loss, G))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])      # two runs, the same bits
    loss, G = outs[0]
    if groups == 2:
        assert bool((G[:, C:] == 0).all())                                                  # written, and exactly zero
    e_G = np.abs(_np(G[:, :C]) - ref_G)
    b_G = U * mag * 2 / per
    assert (e_G <= b_G).all(), float((e_G / b_G).max())
    b_loss = (np.abs(ref_G) * U * mag).reshape(N, -1).sum(axis=1) + (math.ceil(per / 256) + 12) * 2.0 ** -24 * ref_loss
    e_loss = np.abs(_np(loss) - ref_loss)
    assert (e_loss <= b_loss).all(), (e_loss / b_loss).max()
    print(f"loss {shape} groups={groups}: worst error / bound: G {float((e_G / b_G).max()):.3f}, loss {float((e_loss / b_loss).max()):.3f}")
    # through the autograd function: the same loss bits, and dout = g_loss x G through mapdit_obj_loss_bwd
    f = make_flow()
    t = torch.zeros(N, dtype=torch.int64, device=DEV)
    mo_leaf = mo.clone().requires_grad_(True)
    out = f.training_losses(lambda *a, **k: mo_leaf, x0, t, noise=eps)
    assert set(out) == {"loss", "mse"} and torch.equal(out["loss"], loss) and torch.equal(out["mse"], loss)
    w = torch.arange(1, N + 1, device=DEV, dtype=torch.float32)
    (out["loss"] * w).sum().backward()
    assert torch.equal(mo_leaf.grad, G * w.view(-1, 1, 1, 1))
    poll()


@pytest.mark.parametrize("T,shift", [(1000, 1.0), (7, 3.0)])
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_flow_step_matches_fp64(shape, groups, T, shift):
    """Predictor, corrector and Euler rows of a Heun plan, rows that differ per sample; sample written to a new tensor and over base
    (committing rows only: that is the contract); base_out given / null; pred_xstart given / null."""
    f = make_flow(T, shift)
    dev = torch.device(DEV)
    tabs = f._plan_tables(dev, 6, 2)
    tau, ctab, flags, ts, kinds = tabs
    J = len(ts)
    assert J == 2 * len(f._schedule(6, 2).steps) - 1 and J >= 5
    c32, tau_h, flag_h = ctab.cpu().numpy().astype(np.float64), tau.cpu().numpy(), flags.cpu().numpy()
    assert flag_h[J - 1] == 1 and flag_h[J - 2] == 0 and flag_h[0] == 0 and c32[J - 2, 0] != 0 and c32[0, 0] == 0     # predictor, corrector, Euler
    assert list(tau_h[::-1]) == ts and list(flag_h[::-1]) == kinds
    sig32 = _np(f._tables(dev))
    N, C = shape[:2]
    per = int(np.prod(shape[1:]))
    g = torch.Generator().manual_seed(sum(shape) + groups + T)
    base0, x_eval, hist0 = (torch.randn(shape, generator=g).to(DEV) for _ in range(3))
    mo = torch.randn(N, groups * C, *shape[2:], generator=g).to(DEV)
    v = _np(mo[:, :C])
    mixed = [J - 1, J - 2, 0] if N == 3 else [J - 2, J - 1]
    commit = [J - 2, 0, J - 4] if N == 3 else [0, J - 2]
    worst = 0.0
    for rows, aliases in ((mixed, (False,)), (commit, (False, True))):
        r = np.array(rows)
        bc = lambda a: a.reshape(-1, 1, 1, 1)
        c_h, c_v = bc(c32[r, 0]), bc(c32[r, 1])
        ref = _np(base0) + c_h * _np(hist0) + c_v * v
        mag = np.abs(_np(base0)) + np.abs(c_h * _np(hist0)) + np.abs(c_v * v)
        s = bc(sig32[tau_h[r]])
        ref_xs, mag_xs = _np(x_eval) - s * v, np.abs(_np(x_eval)) + np.abs(s * v)
        step = torch.tensor(rows, dtype=torch.int64, device=DEV)
        for alias in aliases:
            for with_extras in (True, False):
                base, hist = base0.clone(), hist0.clone()
                sample = base if alias else torch.full_like(base, float("nan"))
                base_out = torch.full_like(base, 7.0) if with_extras and not alias else None
                got, xs = f._flow_step(mo, x_eval if with_extras else None, base, hist, step, tabs, sample=sample, base_out=base_out,
                                       want_xstart=with_extras)
                torch.cuda.synchronize()
                assert got.data_ptr() == sample.data_ptr() and (alias or torch.equal(base, base0))
                err = np.abs(_np(got) - ref)
                worst = max(worst, float((err / (U * mag)).max()))
                assert (err <= U * mag).all(), (rows, alias, worst)
                for n, row in enumerate(rows):                                  # hist <- v on a predictor row, untouched otherwise
                    assert torch.equal(hist[n], mo[n, :C] if flag_h[row] else hist0[n])
                    if base_out is not None:                                    # base_out <- out on a committing row, untouched otherwise
                        assert torch.equal(base_out[n], torch.full_like(base_out[n], 7.0) if flag_h[row] else got[n])
                if with_extras:
                    e_xs = np.abs(_np(xs) - ref_xs)
                    worst = max(worst, float((e_xs / (U * mag_xs)).max()))
                    assert (e_xs <= U * mag_xs).all()
                else:
                    assert xs is None
                if not alias:                                                   # two runs, the same bits
                    again, _ = f._flow_step(mo, None, base0, hist0.clone(), step, tabs, want_xstart=False)
                    assert torch.equal(again, got)
    # an Euler plan never reads hist: a buffer of NaN stays out of the sum
    etabs = f._plan_tables(dev, 6, 1)
    step = torch.full((N,), len(etabs[3]) - 1, dtype=torch.int64, device=DEV)
    got, _ = f._flow_step(mo, None, base0, torch.full_like(base0, float("nan")), step, etabs, want_xstart=False)
    assert bool(torch.isfinite(got).all())
    poll()
    print(f"flow_step {shape} groups={groups} T={T}: worst error / bound {worst:.3f}")


# ---- the logit-normal draw ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,loc,scale", [(1000, 0.0, 1.0), (7, 0.5, 1.5)])
def test_logit_normal_draw_equals_numpy(T, loc, scale):
    """N = 100,000 (391 workgroups) and N = 1 against the numpy formula in fp64.  The device's exp may differ from numpy's in the last
    place: at most 1 index in 10,000 may differ, each by exactly 1 (tests/test_flow_cpu.py shows the seed leaves that room)."""
    f = make_flow(T)
    z = np.random.default_rng(DRAW_SEED).standard_normal(DRAW_N)
    want = R.logit_normal_index(z, loc, scale, T)
    zd = torch.from_numpy(z).to(DEV)
    got = f.timesteps_from_normals(zd, loc, scale)
    assert got.dtype == torch.int64 and got.shape == (DRAW_N,) and torch.equal(f.timesteps_from_normals(zd, loc, scale), got)
    diff = np.abs(got.cpu().numpy() - want)
    print(f"T={T}: {int((diff > 0).sum())} of {DRAW_N} indices differ from numpy")
    assert (diff > 0).sum() * 10_000 <= DRAW_N and diff.max() <= 1
    one = f.timesteps_from_normals(zd[:1], loc, scale)
    assert one.shape == (1,) and abs(int(one[0]) - int(want[0])) <= 1
    edge = f.timesteps_from_normals(torch.tensor([-1e300, 1e300, float("-inf"), float("inf")], dtype=torch.float64, device=DEV), loc, scale)
    assert edge.tolist() == [0, T - 1, 0, T - 1]
    poll()
    # through the public entry: the caller's generator decides the draw
    gen = torch.Generator(device=DEV).manual_seed(5)
    a = f.sample_timesteps(64, DEV, density="logit-normal", loc=loc, scale=scale, generator=gen)
    zz = torch.randn(64, dtype=torch.float64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    assert torch.equal(a, f.timesteps_from_normals(zz, loc, scale))
    u = f.sample_timesteps(64, DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    assert torch.equal(u, torch.randint(0, T, (64,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)))


def test_nan_draw_is_clamped_and_reported():
    from mapdit_amd import _lib as L
    f = make_flow()
    poll()                                                                      # nothing pending
    z = torch.tensor([0.0, float("nan"), 1.0], dtype=torch.float64, device=DEV)
    t = f.timesteps_from_normals(z)
    with pytest.raises(L.MapditError, match="timestep"):
        poll()
    poll()                                                                      # the record is cleared
    assert t.tolist() == [500, 0, int(R.logit_normal_index(np.array([1.0]), 0.0, 1.0, 1000)[0])]


# ---- refusals and reports -----------------------------------------------------------------------------------------------------------------
def test_out_of_range_indices_are_reported_not_faulted():
    """Every bad index is clamped by construction (MAPDIT_CHECKED_INDEX): nothing here reads out of bounds."""
    from mapdit_amd import _lib as L
    f = make_flow(250)
    dev = torch.device(DEV)
    tabs = f._plan_tables(dev, 6, 2)
    J = len(tabs[3])
    x, mo = torch.randn(3, 4, 6, 6, device=DEV), torch.randn(3, 8, 6, 6, device=DEV)
    poll()
    for bad, clamped in ((J, J - 1), (-1, 0), (1 << 40, J - 1)):
        step = torch.tensor([2, bad, 0], dtype=torch.int64, device=DEV)
        got, xs = f._flow_step(mo, x, x, torch.ones_like(x), step, tabs)
        with pytest.raises(L.MapditError, match="timestep"):
            poll()
        poll()
        want, wxs = f._flow_step(mo, x, x, torch.ones_like(x), torch.tensor([2, clamped, 0], dtype=torch.int64, device=DEV), tabs)
        assert torch.equal(got, want) and torch.equal(xs, wxs)
    for bad, clamped in ((250, 249), (-5, 0)):
        t = torch.tensor([3, bad, 0], device=DEV)
        got = f.q_sample(x, t, mo[:, :4].contiguous())
        with pytest.raises(L.MapditError, match="timestep"):
            poll()
        poll()
        assert torch.equal(got, f.q_sample(x, torch.tensor([3, clamped, 0], device=DEV), mo[:, :4].contiguous()))
    poll()


def test_argument_errors_name_what_is_wrong():
    """The host-side checks: nothing is launched."""
    from mapdit_amd import _lib as L
    f = make_flow(250)
    dev = torch.device(DEV)
    tau, ctab, flags, ts, _ = f._plan_tables(dev, 6, 2)
    sig = f._tables(dev)
    p = lambda v: None if v is None else v.data_ptr()
    x, eps, hist, out, out2 = (torch.randn(3, 4, 6, 6, device=DEV) for _ in range(5))
    mo, G = torch.randn(3, 8, 6, 6, device=DEV), torch.empty(3, 8, 6, 6, device=DEV)
    t = torch.zeros(3, dtype=torch.int64, device=DEV)
    loss = torch.empty(3, device=DEV)
    z = torch.zeros(8, dtype=torch.float64, device=DEV)
    tz = torch.zeros(8, dtype=torch.int64, device=DEV)

    def q(x0=x, noise=eps, t_=t, sig_=sig, T=250, xt=out, n=3, per=144):
        lib().flow_q_sample(p(x0), p(noise), p(t_), p(sig_), T, p(xt), n, per, stream())

    def lf(mo_=mo, x0=x, noise=eps, loss_=loss, G_=G, n=3, per=144, groups=2):
        lib().flow_loss_fwd(p(mo_), p(x0), p(noise), p(loss_), p(G_), n, per, groups, stream())

    def dr(z_=z, loc=0.0, scale=1.0, T=250, t_out=tz, n=8):
        lib().flow_draw_timesteps(p(z_), loc, scale, T, p(t_out), n, stream())

    def st(mo_=mo, x_eval=x, base=x, hist_=hist, step=t, J=len(ts), T=250, sample=out, base_out=None, xs=None, n=3, per=144, groups=2):
        lib().flow_step(p(mo_), p(x_eval), p(base), p(hist_), p(step), p(tau), p(ctab), p(flags), J, p(sig), T, p(sample), p(base_out), p(xs),
                        n, per, groups, stream())

    part = x.flatten()[8:]                                                       # a partial overlap with x
    cases = [(q, dict(x0=None), "flow_q_sample: null/empty"), (q, dict(xt=None), "flow_q_sample: null/empty"), (q, dict(n=0), "flow_q_sample: null/empty"),
             (q, dict(per=0), "flow_q_sample: null/empty"), (q, dict(T=0), "flow_q_sample: T=0"), (q, dict(T=16385), "flow_q_sample: T=16385"),
             (q, dict(xt=x), "flow_q_sample: overlapping"), (q, dict(xt=eps), "flow_q_sample: overlapping"), (q, dict(xt=part, n=2), "flow_q_sample: overlapping"),
             (lf, dict(mo_=None), "flow_loss_fwd: null/empty"), (lf, dict(G_=None), "flow_loss_fwd: null/empty"), (lf, dict(n=0), "flow_loss_fwd: null/empty"),
             (lf, dict(groups=0), "flow_loss_fwd: groups=0"), (lf, dict(groups=3), "flow_loss_fwd: groups=3"),
             (lf, dict(G_=mo), "flow_loss_fwd: overlapping"), (lf, dict(G_=x, groups=1), "flow_loss_fwd: overlapping"),
             (dr, dict(z_=None), "flow_draw_timesteps: null/empty"), (dr, dict(n=0), "flow_draw_timesteps: null/empty"),
             (dr, dict(T=0), "flow_draw_timesteps: T=0"), (dr, dict(T=20000), "flow_draw_timesteps: T=20000"),
             (dr, dict(scale=0.0), "flow_draw_timesteps: loc"), (dr, dict(scale=float("inf")), "flow_draw_timesteps: loc"),
             (dr, dict(loc=float("nan")), "flow_draw_timesteps: loc"), (dr, dict(t_out=z), "flow_draw_timesteps: overlapping"),
             (st, dict(mo_=None), "flow_step: null/empty"), (st, dict(hist_=None), "flow_step: null/empty"), (st, dict(sample=None), "flow_step: null/empty"),
             (st, dict(J=0), "flow_step: null/empty"), (st, dict(n=0), "flow_step: null/empty"),
             (st, dict(x_eval=None, xs=out2), "flow_step: pred_xstart needs x_eval"),
             (st, dict(T=0), "flow_step: T=0"), (st, dict(groups=3), "flow_step: groups=3"),
             (st, dict(hist_=x), "hist must not overlap"), (st, dict(sample=hist), "hist must not overlap"), (st, dict(base_out=hist), "hist must not overlap"),
             (st, dict(xs=hist), "hist must not overlap"), (st, dict(hist_=mo), "hist must not overlap"),
             (st, dict(xs=out), "flow_step: overlapping"), (st, dict(xs=x), "flow_step: overlapping"), (st, dict(sample=mo), "flow_step: overlapping"),
             (st, dict(sample=part, n=2), "flow_step: overlapping")]
    for fn, kw, match in cases:
        with pytest.raises(L.MapditError, match=match):
            fn(**kw)
    # what the contract allows: sample over base, base_out = base, x_eval = base; x_eval null without pred_xstart
    commit = torch.zeros(3, dtype=torch.int64, device=DEV)
    b = x.clone()
    st(base=b, x_eval=b, sample=b, step=commit, xs=out2)
    b = x.clone()
    st(base=b, x_eval=None, sample=out, base_out=b, step=commit)
    assert torch.equal(b, out)
    poll()
    # and the Python surface
    with pytest.raises(ValueError, match="channels"):
        f.training_losses(lambda *a, **k: torch.zeros(3, 12, 6, 6, device=DEV), x, t)


# ---- the loss reaches the gradients ---------------------------------------------------------------------------------------------------------
def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def test_loss_reaches_the_parameter_gradients():
    """Parameter gradients of flow.training_losses(...)["loss"].mean() on the fixture tiny_a (bf16x3, eval mode) against the same loss
    written in torch ops on the model's first C channels; 2e-4 per parameter, the tolerance tests/test_train_gpu.py holds that
    precision to.  The same loss with the target's sign flipped is more than 0.1 away: the comparison can fail.  With
    model.input_gradients the gradient also arrives at the model's input x_s (the flow helpers, like the diffusion helpers, are not
    differentiable in x_start itself)."""
    from grad_accum_worker import fixture_model, reset_grads
    m, _, (x, t, y, noise) = fixture_model("tiny_a", "bf16x3")
    assert not m.training
    f = make_flow()
    C = x.shape[1]

    def flat():
        torch.cuda.synchronize()
        return m._gflat.double().cpu().numpy()

    reset_grads(m)
    f.training_losses(m, x, t, dict(y=y), noise=noise)["loss"].mean().backward()
    got = flat()

    def torch_loss(sign):
        out = m(f.q_sample(x, t, noise), t, y=y)[:, :C].float()
        return ((out - sign * (noise - x)) ** 2).mean(dim=(1, 2, 3)).mean()

    reset_grads(m)
    torch_loss(1.0).backward()
    want = flat()
    reset_grads(m)
    torch_loss(-1.0).backward()
    flipped = flat()
    assert np.isfinite(got).all() and np.abs(want).max() > 0
    worst = 0.0
    for (k, p), o in zip(m.named_parameters(), m._poffs):
        sl = slice(o, o + p.numel())
        if float(np.linalg.norm(want[sl])) == 0.0:
            assert float(np.abs(got[sl]).max()) == 0.0, k
            continue
        e = rel_err(got[sl], want[sl])
        worst = max(worst, e)
        assert e < 2e-4, (k, e)
    away = rel_err(flipped, want)
    print(f"flow loss: worst per-parameter rel err {worst:.2e}; the sign-flipped target is {away:.2f} away")
    assert away > 0.1
    # dL/dx_s through the model
    m.input_gradients = True
    seen = []

    def wrapped(xs, tt, **kw):
        seen.append(xs.requires_grad_(True))
        return m(xs, tt, **kw)
    reset_grads(m)
    f.training_losses(wrapped, x, t, dict(y=y), noise=noise)["loss"].mean().backward()
    torch.cuda.synchronize()
    gx = seen[0].grad
    assert gx is not None and gx.shape == x.shape and bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0
    m.input_gradients = False
    reset_grads(m)


# ---- convergence on the device ----------------------------------------------------------------------------------------------------------------
def test_convergence_to_exact_solution():
    """Data N(0, c^2 I), c = 0.5 (flow_reference.exact_velocity_coef): the ODE ends at c x(1).  T = 1000, shift 1, K = 10 / 20 / 40; in
    fp64 numpy: Euler 1.384e-1, 7.15e-2, 3.64e-2 (ratios 1.94, 1.97), Heun 1.84e-2, 4.22e-3, 1.01e-3 (4.35, 4.19).  Asserted: Heun
    beats Euler at every K; each doubling shrinks the Heun error >= 3 x and the Euler error by a factor in [1.5, 2.5].  The fp32 floor
    (~1e-6) is far below every value involved."""
    f = make_flow()
    a = torch.from_numpy(R.exact_velocity_coef(f.sigmas)).float().to(DEV)
    model = lambda x, t, **kw: torch.cat([a[t].view(-1, 1, 1, 1) * x, torch.zeros_like(x)], dim=1)
    noise = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(0)).to(DEV)
    exact = R.C_DATA * _np(noise)
    err = {}
    for order in (1, 2):
        for K in (10, 20, 40):
            out = f.sample_loop(model, noise.shape, noise=noise, device=DEV, num_steps=K, order=order)
            err[order, K] = float(np.abs(_np(out) - exact).max() / np.abs(exact).max())
    print({k: f"{v:.3e}" for k, v in err.items()})
    for K in (10, 20, 40):
        assert err[2, K] < err[1, K]
        assert err[2, K] > 1e-4                                                 # far above the fp32 floor
    for lo, hi in ((10, 20), (20, 40)):
        assert err[2, lo] / err[2, hi] >= 3.0, (err[2, lo], err[2, hi])
        assert 1.5 <= err[1, lo] / err[1, hi] <= 2.5, (err[1, lo], err[1, hi])


# ---- captured loop against eager loop ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def xs2():
    """DiT-XS/2 on 16x16 latents (64 tokens), the oracle's initialisation (a fresh DiT's output layer is zero): the fixture of
    tests/test_dpm_solver_gpu.py."""
    from mapdit_amd.src.dit import DiT
    from oracle import dit_oracle as O
    cfg = O.DiTConfig(depth=6, hidden_size=256, patch_size=2, input_size=16, in_channels=4, num_heads=4, num_classes=10)
    m = DiT(**cfg.to_dict())
    m.load_state_dict(O.init_state_dict(cfg, seed=7, gains=0.3, perturb_reference=0.3))
    return m.to(DEV).eval()


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("cfg_scale", [None, 1.5])
def test_captured_sampler_is_bit_equal_to_eager(xs2, cfg_scale, order):
    from mapdit_amd import sampling as S
    f = make_flow(shift=3.0)
    g = torch.Generator().manual_seed(11)
    z = torch.randn(1, 4, 16, 16, generator=g)
    z = torch.cat([z, z] if cfg_scale else [z, torch.randn(1, 4, 16, 16, generator=g)]).to(DEV)
    y = torch.tensor([3, 10] if cfg_scale else [3, 7], device=DEV)
    kw = dict(y=y) if cfg_scale is None else dict(y=y, cfg_scale=cfg_scale)
    fn = xs2.forward if cfg_scale is None else xs2.forward_with_cfg
    z0 = z.clone()
    with torch.no_grad():
        eager = f.sample_loop(fn, z.shape, noise=z, model_kwargs=kw, device=DEV, num_steps=6, order=order)
    assert torch.equal(z, z0)                                                   # the caller's noise is not written
    assert torch.isfinite(eager).all() and not torch.equal(eager, z)
    gs = S.GraphedSampler(xs2, f, z.shape, y, cfg_scale, sampler="flow", num_steps=6, order=order)
    assert gs.num_replays == (6 if order == 1 else 11)
    first = gs.sample(z)
    assert torch.equal(first, eager)
    assert torch.equal(gs.sample(z), first)                                     # the state and the evaluation counter are reset
    assert torch.equal(S.run_sampler(xs2, f, z, y, cfg_scale, use_graph=False, sampler="flow", num_steps=6, order=order), eager)
    assert torch.equal(S.flow_sample_loop_graphed(f, xs2, z.shape, z, kw, num_steps=6, order=order), eager)
    if order == 2:
        other = S.run_sampler(xs2, f, z, y, cfg_scale, sampler="flow-euler", num_steps=6)
        assert torch.isfinite(other).all() and not torch.equal(other, eager)


def test_other_captured_samplers_still_run(xs2):
    from mapdit_amd import sampling as S
    from mapdit_amd.diffusion import create_diffusion
    z = torch.randn(2, 4, 16, 16, device=DEV)
    y = torch.tensor([3, 7], device=DEV)
    out = S.GraphedSampler(xs2, create_diffusion("4"), z.shape, y, clip_denoised=True).sample(z)
    assert out.shape == z.shape and torch.isfinite(out).all()
    out = S.GraphedSampler(xs2, create_diffusion(""), z.shape, y, sampler="dpm++", num_steps=4).sample(z)
    assert out.shape == z.shape and torch.isfinite(out).all()


# ---- launch counts --------------------------------------------------------------------------------------------------------------------------
class Counting:
    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, k):
        self._calls.append(k)
        return getattr(self._real, k)


def test_launch_counts(monkeypatch):
    """After the model an eager evaluation is exactly one mapdit_flow_step; training_losses is flow_q_sample, the model, flow_loss_fwd
    and one obj_loss_bwd in backward; the create_diffusion paths call no mapdit_flow_* entry."""
    from mapdit_amd import _lib as L
    from mapdit_amd.diffusion import create_diffusion
    f = make_flow(250)
    z, mo = torch.randn(2, 4, 8, 8, device=DEV), torch.randn(2, 8, 8, 8, device=DEV)
    f._tables(torch.device(DEV))
    real, calls = L.lib(), []
    monkeypatch.setattr(L, "lib", lambda: Counting(real, calls))

    def stub(x, t, **kw):
        calls.append("model")
        return mo
    f.sample_loop(stub, z.shape, noise=z, device=DEV, num_steps=4, order=1)
    assert calls == ["model", "flow_step"] * 4 + ["device_error_poll"]
    calls.clear()
    f.sample_loop(stub, z.shape, noise=z, device=DEV, num_steps=4, order=2)
    assert calls == ["model", "flow_step"] * 7 + ["device_error_poll"]
    calls.clear()
    leaf = mo.clone().requires_grad_(True)

    def stub_grad(x, t, **kw):
        calls.append("model")
        return leaf
    t = torch.tensor([3, 200], device=DEV)
    loss = f.training_losses(stub_grad, z, t)["loss"].mean()
    assert calls == ["flow_q_sample", "model", "flow_loss_fwd"]
    loss.backward()
    assert calls == ["flow_q_sample", "model", "flow_loss_fwd", "obj_loss_bwd"]
    calls.clear()
    d = create_diffusion("4")
    d.training_losses(stub_grad, z, torch.tensor([0, 3], device=DEV))["loss"].mean().backward()
    d.p_sample_loop(stub, z.shape, noise=z, device=DEV)
    create_diffusion("").dpm_solver_sample_loop(stub, z.shape, noise=z, device=DEV, num_steps=3)
    assert calls and not [c for c in calls if c.startswith("flow_")], calls


# ---- the harness ----------------------------------------------------------------------------------------------------------------------------
TRAIN = ["--synthetic", "--model", "DiT-XS/2", "--num-steps", "3", "--batch-size", "4", "--log-every", "1", "--ckpt-every", "3",
         "--num-classes", "10", "--num-lin-warmup", "1", "--start-decay", "2", "--precision", "bf16"]
CASES = {"plain": ["--ema-snapshot-every", "1000"],
         "flow": ["--ema-snapshot-every", "1", "--objective", "flow", "--flow-shift", "3"],
         "flow_lsm": ["--ema-snapshot-every", "1000", "--objective", "flow", "--flow-timestep-density", "logit-normal", "--grad-accum-steps", "2",
                      "--schedule-sampler", "loss-second-moment"]}


def run_train(tag, root, monkeypatch=None):
    from mapdit_amd import _lib as L
    from mapdit_amd import train
    calls = []
    if monkeypatch is not None:
        real = L.lib()
        monkeypatch.setattr(L, "lib", lambda: Counting(real, calls))
    exp = train.main(TRAIN + CASES[tag] + ["--results-dir", str(root / tag)])
    return exp, calls


@pytest.fixture(scope="module")
def flow_run(tmp_path_factory):
    return run_train("flow", tmp_path_factory.mktemp("flow_run"))[0]


def check_run(exp, tag):
    import yaml
    lines = [ln for ln in open(os.path.join(exp, "log.txt")).read().splitlines() if ln.startswith("(step=")]
    assert len(lines) == 3, lines
    for ln in lines:                                                            # today's format to the byte, finite losses
        assert re.fullmatch(r"\(step=\d{7}\) train loss: \d+\.\d{4}, train steps/sec: \d+\.\d{2}", ln), (tag, ln)
    cfg = yaml.safe_load(open(os.path.join(exp, "config.yaml")))
    assert cfg["objective"] == ("diffusion" if tag == "plain" else "flow")
    assert cfg["flow_shift"] == (3.0 if tag == "flow" else 1.0)
    return torch.load(os.path.join(exp, "checkpoints", "0000003.pt"), weights_only=True)


@pytest.mark.parametrize("tag", ["plain", "flow_lsm"])
def test_train_harness(tmp_path, monkeypatch, tag):
    exp, calls = run_train(tag, tmp_path, monkeypatch)
    ck = check_run(exp, tag)
    flow_calls = {c for c in calls if c.startswith("flow_")}
    if tag == "plain":
        assert set(ck) == {"model", "opt"}
        assert calls and not flow_calls, flow_calls                             # the default path calls no mapdit_flow_* entry
        return
    assert set(ck) == {"model", "opt", "schedule_sampler"}
    assert int(ck["schedule_sampler"]["loss_counts"].sum()) == 12               # 3 steps x 2 micro-batches x 2 samples reached the history
    assert flow_calls == {"flow_q_sample", "flow_loss_fwd"}                     # (the loss-aware sampler draws the timesteps)
    assert calls.count("flow_loss_fwd") == 6 and calls.count("obj_loss_bwd") == 6 and "loss_fwd" not in calls


def test_flow_run_and_sampler_clis(flow_run, tmp_path):
    """The run trained with --objective flow, then --sampler flow-heun through the three scripts on its directory (shapes only: a
    network trained for 3 steps denoises nothing), and the refusal of the diffusion samplers there."""
    from mapdit_amd import sample, sample_ema, sample_fid
    ck = check_run(flow_run, "flow")
    assert set(ck) == {"model", "opt"}
    base = ["--result-dir", flow_run, "--use-vae", "false", "--num-sampling-steps", "4"]
    heun = base + ["--sampler", "flow-heun"]
    path = sample_fid.main(heun + ["--num-classes", "10", "--batch-size", "4", "--num-samples", "6", "--output-file", "a.npz"])
    assert np.load(path)["arr_0"].shape == (6, 32, 32, 4)
    path = sample_fid.main(base + ["--sampler", "flow-euler", "--num-classes", "10", "--batch-size", "4", "--num-samples", "4", "--cfg-scale", "1.0",
                                   "--no-graph", "--output-file", "b.npz"])
    assert np.load(path)["arr_0"].shape == (4, 32, 32, 4)
    out = str(tmp_path / "grid.png")
    assert sample.main(heun + ["--class-label", "3", "--output-file", out]).shape == (4, 4, 32, 32)
    assert sample_ema.main(heun + ["--class-label", "0", "--output-file", out]).shape == (8 * 5, 4, 32, 32)
    for mod, extra in ((sample, ["--class-label", "3"]), (sample_ema, ["--class-label", "0"]), (sample_fid, ["--num-classes", "10"])):
        for sampler in ([], ["--sampler", "dpm++"]):
            with pytest.raises(ValueError, match="--sampler flow-euler or --sampler flow-heun"):
                mod.main(base + extra + sampler + ["--output-file", out])


def test_diffusion_run_refuses_the_flow_samplers(tmp_path):
    """The reverse case without a training run: config.yaml is read before anything else; one written before the key existed counts
    as diffusion."""
    import yaml

    from mapdit_amd import sample_fid
    cfg = dict(model="DiT-XS/2", num_classes=10, in_channels=4, input_size=32, stats_mean=[0.0] * 4, stats_std=[1.0] * 4)
    for extra in ({}, {"objective": "diffusion", "flow_shift": 1.0}):
        d = tmp_path / f"run{len(extra)}"
        d.mkdir()
        yaml.dump(dict(cfg, **extra), open(d / "config.yaml", "w"))
        with pytest.raises(ValueError, match="--sampler ancestral or --sampler dpm\\+\\+"):
            sample_fid.main(["--result-dir", str(d), "--use-vae", "false", "--sampler", "flow-heun", "--num-sampling-steps", "4"])
