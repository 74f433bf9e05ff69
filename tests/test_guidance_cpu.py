"""Host side of the sampler hooks (no GPU): an fp32 torch restatement of mapdit_obj_xstart / mapdit_obj_step_guided, in the
kernels' operation order, reproduces every kernel-tier golden of tests/golden/guidance.npz (make_golden_guidance.py) within
1e-5 - the tolerance the GPU tests hold the kernels to is reachable in fp32.  Also: the public surface (condition_mean /
condition_score on both classes), and what stays refused.

Measured here, worst case over the 1,056 compared arrays: 3.6e-7.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err

MEANS = ["EPSILON", "START_X"]
VARS = ["LEARNED_RANGE", "FIXED_SMALL", "FIXED_LARGE"]
SCHEDS = {"full": "", "s250": "250"}
SHAPES = ["a", "b"]
PSAMPLE, DDIM, DDIM_REVERSE = 0, 1, 2


def diffusion(sched, mean, var):
    from mapdit_amd.diffusion import gaussian_diffusion as gd
    from mapdit_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    return SpacedDiffusion(use_timesteps=space_timesteps(1000, sched or [1000]), betas=gd.get_named_beta_schedule("linear", 1000),
                           model_mean_type=gd.ModelMeanType[mean], model_var_type=gd.ModelVarType[var], loss_type=gd.LossType.MSE)


def denoised_fn(x0):
    return 0.8 * torch.tanh(1.5 * x0)


def make_cond_fn(target, scale=3.0):
    def cond_fn(x, t, **kw):
        return scale * (target - x) * (1 + t.float().view(-1, *([1] * (x.dim() - 1))) / 1000)
    return cond_fn


@pytest.fixture(scope="module")
def gold():
    return load_golden("guidance")


def golden_outputs(g, key):
    return dict(zip([str(k) for k in g["outputs"]], g[key]))


def kept(g, name, a):
    """The entries of a full tensor that the fixture stores: all of shape a, every b_stride-th of shape b."""
    f = np.asarray(a).reshape(-1)
    return f if name == "a" else f[::int(g["b_stride"])]


def model_out(g, name, var, device="cpu"):
    mo = torch.from_numpy(g[f"{name}/mo"]).to(device)
    return mo if var == "LEARNED_RANGE" else mo[:, :mo.shape[1] // 2].contiguous()


def case_t(g, name, tag, tcase, device="cpu"):
    t = torch.from_numpy(g[f"{name}/{tag}/t"]).to(device)
    return t if tcase == "mix" else torch.zeros_like(t)


# ---- the restatement: fp32 torch, one expression per kernel statement ------------------------------------------------------

def _rows(d, t, ndim):
    tab, otab = d._tables("cpu"), d._obj_tables("cpu")
    sh = (-1,) + (1,) * (ndim - 1)
    r = {k: tab[i][t].view(sh) for k, i in (("ra", 2), ("rm1", 3), ("minlog", 4), ("maxlog", 5), ("c1", 6), ("c2", 7))}
    r.update({k: otab[i][t].view(sh) for k, i in (("ab", 0), ("abp", 1), ("abn", 2), ("fixlog", 3))})
    return r


def restate_xstart(d, mo, x, t, mean):
    """obj_xstart_kernel."""
    c = _rows(d, t, x.dim())
    m = mo[:, :x.shape[1]]
    return m.clone() if mean == "START_X" else c["ra"] * x - c["rm1"] * m


def restate_step(d, mo, x, t, noise, mean, var, clip, mode, eta=0.0, xstart_in=None, cond_grad=None):
    """obj_step_guided_kernel -> (sample, pred_xstart, mean)."""
    c = _rows(d, t, x.dim())
    C = x.shape[1]
    if xstart_in is not None:
        xs = xstart_in
    else:
        m = mo[:, :C]
        xs = m if mean == "START_X" else c["ra"] * x - c["rm1"] * m
    if clip:
        xs = xs.clamp(-1, 1)
    nonzero = (t != 0).float().view(c["ra"].shape)
    if mode == PSAMPLE:
        if var == "LEARNED_RANGE":
            frac = (mo[:, C:] + 1) * 0.5
            lv = frac * c["maxlog"] + (1 - frac) * c["minlog"]
        else:
            lv = (c["minlog"] if var == "FIXED_SMALL" else c["fixlog"]).expand_as(x)
        mu = c["c1"] * xs + c["c2"] * x
        if cond_grad is not None:
            variance = torch.exp(lv) * nonzero if var == "FIXED_SMALL" else torch.exp(lv)      # posterior_variance[0] = 0
            mu = mu + variance * cond_grad
        out = mu if noise is None else mu + nonzero * torch.exp(0.5 * lv) * noise
        return out, xs, mu
    if cond_grad is not None:          # condition_score as the shift of x0 it amounts to (no round trip through eps)
        xs = xs + c["rm1"] * torch.sqrt(1 - c["ab"]) * cond_grad
    mu = c["c1"] * xs + c["c2"] * x
    eps = (c["ra"] * x - xs) / c["rm1"]
    if mode == DDIM_REVERSE:
        out = xs * torch.sqrt(c["abn"]) + torch.sqrt(1 - c["abn"]) * eps
    else:
        sigma = eta * torch.sqrt((1 - c["abp"]) / (1 - c["ab"])) * torch.sqrt(1 - c["ab"] / c["abp"])
        out = xs * torch.sqrt(c["abp"]) + torch.sqrt(1 - c["abp"] - sigma * sigma) * eps + nonzero * sigma * noise
    return out, xs, mu


def restated_outputs(g, name, tag, mean, var, tcase, clip):
    """Every output of the fixture's key, full tensors, through the restatement and the facade's own tables."""
    d = diffusion(SCHEDS[tag], mean, var)
    x, target = torch.from_numpy(g[f"{name}/x"]), torch.from_numpy(g[f"{name}/target"])
    psn, ddn = torch.from_numpy(g[f"{name}/ps_noise"]), torch.from_numpy(g[f"{name}/ddim_noise"])
    mo, t = model_out(g, name, var), case_t(g, name, tag, tcase)
    grad = make_cond_fn(target, float(g["cond_scale"]))(x, d._mapped_t(t))
    xin = denoised_fn(restate_xstart(d, mo, x, t, mean))
    step = lambda noise, mode, eta=0.0, xi=None, gr=None: restate_step(d, mo, x, t, noise, mean, var, clip, mode, eta, xi, gr)
    r = {}
    r["pmv_mean"], r["pmv_pred_xstart"], _ = step(None, PSAMPLE, xi=xin)
    r["ps_den_sample"] = step(psn, PSAMPLE, xi=xin)[0]
    r["ps_cond_sample"] = step(psn, PSAMPLE, gr=grad)[0]
    r["ps_both_sample"] = step(psn, PSAMPLE, xi=xin, gr=grad)[0]
    r["ddim_sample"], r["ddim_pred_xstart"], _ = step(ddn, DDIM, 0.5, xin, grad)
    r["ddimrev_sample"] = step(None, DDIM_REVERSE, 0.0, xin, grad)[0]
    r["cm_mean"] = step(None, PSAMPLE, gr=grad)[2]
    # condition_score on the unhooked p_mean_variance: its (clipped) pred_xstart comes back in as xstart_in, unclipped
    plain_xs = step(None, PSAMPLE)[1]
    _, r["cs_pred_xstart"], r["cs_mean"] = restate_step(d, None, x, t, ddn, mean, var, 0, DDIM, 0.0, plain_xs, grad)
    return r


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("tag", list(SCHEDS))
@pytest.mark.parametrize("mean", MEANS)
@pytest.mark.parametrize("var", VARS)
def test_restatement_matches_reference(gold, name, tag, mean, var):
    """1e-5 on every recorded array; measured worst 3.6e-7."""
    worst = 0.0
    for tcase in ("mix", "zero"):
        for clip in (0, 1):
            key = f"{name}/{tag}/{mean}/{var}/{tcase}/clip{clip}"
            ref = golden_outputs(gold, key)
            got = restated_outputs(gold, name, tag, mean, var, tcase, clip)
            assert sorted(got) == sorted(ref)
            for k, v in ref.items():
                e = rel_err(kept(gold, name, got[k].numpy()), v)
                worst = max(worst, e)
                assert e < 1e-5, (key, k, e)
    print(f"{name}/{tag}/{mean}/{var}: worst rel err {worst:.2e}")


def test_fixture_shapes_cover_the_block_edges(gold):
    """Shape a stays under one 256-thread block; shape b ends in a partial block and has sample boundaries inside a block, and the
    stored entries of b lie on both sides of each boundary and inside the partial block."""
    a, b = gold["a/x"], gold["b/x"]
    assert a.size == 128 and b.size == 864 and b[0].size == 288
    idx = np.arange(b.size)[::int(gold["b_stride"])]
    for edge in (288, 576):
        assert ((idx >= edge - 16) & (idx < edge)).any() and ((idx >= edge) & (idx < edge + 16)).any()
    assert (idx >= 768).any()
    for tag, T in (("full", 1000), ("s250", 250)):
        for name in SHAPES:
            t = gold[f"{name}/{tag}/t"]
            assert t[0] == 0 and t[-1] == T - 1


def test_condition_methods_are_public_on_both_classes():
    from mapdit_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    from mapdit_amd.diffusion.respace import SpacedDiffusion
    for name in ("condition_mean", "condition_score"):
        assert callable(getattr(GaussianDiffusion, name))
        assert name in SpacedDiffusion.__dict__, name          # overridden: cond_fn sees the mapped timesteps (respace.py:99-103)


def test_hooks_are_accepted_and_previous_x_stays_refused():
    """A hooked call no longer answers "not built": on a CPU tensor it gets as far as the device check.  PREVIOUS_X has no
    behaviour in the reference to match and stays refused, with the reason in the message."""
    from mapdit_amd.diffusion import create_diffusion
    from mapdit_amd.diffusion import gaussian_diffusion as gd
    from mapdit_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    x, t = torch.zeros(2, 4, 8, 8), torch.zeros(2, dtype=torch.int64)
    cond = make_cond_fn(torch.zeros_like(x))
    model = lambda xx, tt, **kw: torch.cat([xx, xx], 1)
    for kw in ({}, dict(predict_xstart=True), dict(learn_sigma=False)):
        d = create_diffusion("10", **kw)
        with pytest.raises(NotImplementedError, match="no CPU path"):
            d.p_mean_variance(model, x, t, denoised_fn=denoised_fn)
        for fn in (d.p_sample, d.ddim_sample, d.ddim_reverse_sample):
            with pytest.raises(NotImplementedError, match="no CPU path"):
                fn(model, x, t, denoised_fn=denoised_fn, cond_fn=cond)
        for fn in (d.p_sample_loop, d.ddim_sample_loop):
            with pytest.raises(NotImplementedError, match="no CPU path"):
                fn(model, x.shape, noise=x, denoised_fn=denoised_fn, cond_fn=cond, device="cpu")
        with pytest.raises(NotImplementedError, match="no CPU path"):
            d.condition_score(cond, {"pred_xstart": x}, x, t)
    d = SpacedDiffusion(use_timesteps=space_timesteps(1000, [10]), betas=gd.get_named_beta_schedule("linear", 1000),
                        model_mean_type=gd.ModelMeanType.PREVIOUS_X, model_var_type=gd.ModelVarType.LEARNED_RANGE,
                        loss_type=gd.LossType.MSE)
    with pytest.raises(NotImplementedError, match="PREVIOUS_X is not built"):
        d._supported()
    with pytest.raises(NotImplementedError, match="PREVIOUS_X"):
        d.p_sample(model, x, t, cond_fn=cond)


def test_captured_sampler_refuses_the_hooks():
    from mapdit_amd.sampling import p_sample_loop_graphed
    with pytest.raises(NotImplementedError, match="captured sampler"):
        p_sample_loop_graphed(None, None, (2, 4, 8, 8), cond_fn=lambda x, t, **kw: x)
    with pytest.raises(NotImplementedError, match="captured sampler"):
        p_sample_loop_graphed(None, None, (2, 4, 8, 8), denoised_fn=denoised_fn)
