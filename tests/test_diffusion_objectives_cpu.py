"""Host side of the diffusion objectives (no GPU): create_diffusion's switches build the reference's enums, every objective
it can produce passes _supported(), and the schedule rows the mapdit_obj_* kernels read equal the reference's rows
(tests/golden/objectives.npz) for each variance type on the full schedule and on '250'."""
import numpy as np
import pytest
import torch

from conftest import load_golden


def _diff(sched, **kw):
    from mapdit_amd.diffusion import create_diffusion
    return create_diffusion(sched, **kw)


@pytest.mark.parametrize("kw,mean,var,loss", [
    ({}, "EPSILON", "LEARNED_RANGE", "MSE"),
    (dict(use_kl=True), "EPSILON", "LEARNED_RANGE", "RESCALED_KL"),
    (dict(rescale_learned_sigmas=True), "EPSILON", "LEARNED_RANGE", "RESCALED_MSE"),
    (dict(use_kl=True, rescale_learned_sigmas=True), "EPSILON", "LEARNED_RANGE", "RESCALED_KL"),
    (dict(predict_xstart=True), "START_X", "LEARNED_RANGE", "MSE"),
    (dict(learn_sigma=False), "EPSILON", "FIXED_LARGE", "MSE"),
    (dict(learn_sigma=False, sigma_small=True), "EPSILON", "FIXED_SMALL", "MSE"),
    (dict(learn_sigma=False, sigma_small=True, predict_xstart=True, use_kl=True), "START_X", "FIXED_SMALL", "RESCALED_KL"),
])
def test_create_diffusion_switches_build_the_enums(kw, mean, var, loss):
    d = _diff("", **kw)
    assert (d.model_mean_type.name, d.model_var_type.name, d.loss_type.name) == (mean, var, loss)
    d._supported()                                   # every objective create_diffusion produces is built
    assert d._is_default() == (not kw)


def test_out_of_scope_enums_are_refused():
    from mapdit_amd.diffusion import gaussian_diffusion as gd
    from mapdit_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    for mean, var in ((gd.ModelMeanType.PREVIOUS_X, gd.ModelVarType.LEARNED_RANGE), (gd.ModelMeanType.EPSILON, gd.ModelVarType.LEARNED)):
        d = SpacedDiffusion(use_timesteps=space_timesteps(1000, [10]), betas=gd.get_named_beta_schedule("linear", 1000),
                            model_mean_type=mean, model_var_type=var, loss_type=gd.LossType.MSE)
        with pytest.raises(NotImplementedError):
            d._supported()


@pytest.mark.parametrize("tag,sched", [("full", ""), ("s250", "250")])
@pytest.mark.parametrize("var", ["LEARNED_RANGE", "FIXED_SMALL", "FIXED_LARGE"])
def test_schedule_rows_match_reference(tag, sched, var):
    g = load_golden("objectives")
    kw = {} if var == "LEARNED_RANGE" else dict(learn_sigma=False, sigma_small=var == "FIXED_SMALL")
    d = _diff(sched, **kw)
    tab = d._tables("cpu").numpy()
    otab = d._obj_tables("cpu").numpy()
    rows = dict(zip([str(k) for k in g[f"{tag}/row_names"]], g[f"{tag}/rows"]))      # fp32, as uploaded
    r = lambda k: rows[k]
    assert otab.shape == (5, d.num_timesteps)
    for i, k in enumerate(["alphas_cumprod", "alphas_cumprod_prev", "alphas_cumprod_next"]):
        np.testing.assert_array_equal(otab[i], r(k))
    np.testing.assert_array_equal(otab[4], r("log_one_minus_alphas_cumprod"))
    if var == "LEARNED_RANGE":
        np.testing.assert_array_equal(tab[4], r("logvar/LEARNED_RANGE/min"))
        np.testing.assert_array_equal(tab[5], r("logvar/LEARNED_RANGE/max"))
    elif var == "FIXED_SMALL":
        np.testing.assert_array_equal(tab[4], r("logvar/FIXED_SMALL"))
    else:
        np.testing.assert_array_equal(otab[3], r("logvar/FIXED_LARGE"))
    # the rows p_mean_variance returns as variance / log_variance for the fixed types
    t = torch.tensor([0, 1, d.num_timesteps - 1])
    np.testing.assert_array_equal(d._extract("posterior_variance", t, (3, 1)).numpy()[:, 0], r("posterior_variance")[t.numpy()])
    np.testing.assert_array_equal(d._extract("fixed_large_log_variance", t, (3, 1)).numpy()[:, 0], r("logvar/FIXED_LARGE")[t.numpy()])



def test_non_gpu_inputs_are_refused():
    """The kernels have no CPU path: a CPU tensor (or no tensor) raises NotImplementedError before any launch, for the default
    objective and the others alike (an assert would vanish under python -O and hand a host pointer to a kernel)."""
    from mapdit_amd.diffusion import create_diffusion
    x = torch.zeros(2, 4, 8, 8)
    t = torch.zeros(2, dtype=torch.int64)
    for kw in ({}, dict(use_kl=True), dict(predict_xstart=True), dict(learn_sigma=False)):
        d = create_diffusion("10", **kw)
        with pytest.raises(NotImplementedError, match="no CPU path"):
            d.training_losses(lambda xx, tt: xx, x, t)
        with pytest.raises(NotImplementedError, match="no CPU path"):
            d.q_sample(x, t)
        with pytest.raises(NotImplementedError, match="no CPU path"):
            d.calc_bpd_loop(lambda xx, tt: xx, x)
        with pytest.raises(NotImplementedError, match="no CPU path"):
            d._prior_bpd(None)
