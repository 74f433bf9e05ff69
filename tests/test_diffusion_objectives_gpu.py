"""Every objective create_diffusion() can build, and the likelihood evaluation, against the reference
(tests/golden/objectives.npz, bpd_synthetic.npz, bpd_tiny_a.npz; make_golden_objectives.py).

Tolerances.  The pointwise math is fp32 like the reference's: loss values 1e-5 relative, output gradients 1e-4, step outputs
1e-5, the synthetic calc_bpd_loop 1e-5.  The tiny_a DiT in bf16x3 precision (fp32-accurate): total / prior bpd 1e-4, the
[N, T] arrays 1e-3, training losses 1e-5, parameter gradients 1e-4 (the standard of the bf16x3 training test).  The default
f16 engine's total_bpd: F16_BPD_TOL below, at least twice the error measured on the MI355X.
"""
import numpy as np
import pytest
import torch

from conftest import golden_cfg, golden_state_dict, load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"

MEANS = ["EPSILON", "START_X"]
VARS = ["LEARNED_RANGE", "FIXED_SMALL", "FIXED_LARGE"]
LOSSES = ["MSE", "RESCALED_MSE", "KL", "RESCALED_KL"]
SCHEDS = {"full": "", "s250": "250"}
F16_BPD_TOL = 1.5e-4        # default f16 engine, tiny_a total_bpd vs the fp32 reference: measured 2.3e-5 on the MI355X


def diffusion(sched, mean, var, loss):
    from mapdit_amd.diffusion import gaussian_diffusion as gd
    from mapdit_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    return SpacedDiffusion(use_timesteps=space_timesteps(1000, sched or [1000]), betas=gd.get_named_beta_schedule("linear", 1000),
                           model_mean_type=gd.ModelMeanType[mean], model_var_type=gd.ModelVarType[var], loss_type=gd.LossType[loss])


@pytest.fixture(scope="module")
def obj():
    return load_golden("objectives")


def _d(g, k):
    return torch.from_numpy(g[k]).to(DEV)


def _model_out(g, var, name="mo"):
    mo = _d(g, name)
    return mo if var == "LEARNED_RANGE" else mo[:, :int(g["C"])].contiguous()


@pytest.mark.parametrize("tag", list(SCHEDS))
@pytest.mark.parametrize("mean", MEANS)
@pytest.mark.parametrize("var", VARS)
@pytest.mark.parametrize("loss", LOSSES)
def test_training_losses_every_objective(obj, tag, mean, var, loss):
    g = obj
    key = f"{tag}/{mean}/{var}/{loss}"
    d = diffusion(SCHEDS[tag], mean, var, loss)
    leaf = _model_out(g, var).clone().requires_grad_(True)
    x0, noise, t = _d(g, "x0"), _d(g, "noise"), _d(g, f"{tag}/t")
    r = d.training_losses(lambda xx, tt, **kw: leaf, x0, t, noise=noise)
    keys = [str(k) for k in g[key + "/keys"]]
    assert sorted(r) == keys
    vals, w = g[key + "/vals"], _d(g, key + "/w")
    for i, k in enumerate(keys):
        assert rel_err(r[k].detach().cpu().numpy(), vals[i]) < 1e-5, k
    sum((r[k] * w[i]).sum() for i, k in enumerate(keys)).backward()
    torch.cuda.synchronize()
    assert rel_err(leaf.grad.cpu().numpy(), g[key + "/grad"]) < 1e-4


@pytest.mark.parametrize("tag", list(SCHEDS))
@pytest.mark.parametrize("mean", MEANS)
@pytest.mark.parametrize("var", VARS)
def test_reverse_steps_every_objective(obj, tag, mean, var):
    """p_mean_variance, p_sample, ddim_sample (eta 0.5) and ddim_reverse_sample at mixed t (t = 0 included) and at t = 0, clip
    on and off; the random draws are the recorded ones, fed to the same step kernel the methods run."""
    from mapdit_amd.diffusion.gaussian_diffusion import _STEP_DDIM, _STEP_DDIM_REVERSE, _STEP_PSAMPLE
    g = obj
    d = diffusion(SCHEDS[tag], mean, var, "MSE")
    mo, x = _model_out(g, var, "step/mo"), _d(g, "step/x")
    N = x.shape[0]
    for tcase in ("mix", "zero"):
        t = _d(g, f"{tag}/step_t") if tcase == "mix" else torch.zeros(N, dtype=torch.int64, device=DEV)
        for clip in (0, 1):
            key = f"{tag}/{mean}/{var}/{tcase}/clip{clip}"
            ref = dict(zip([str(k) for k in g["step_outputs"]], g[key]))
            pm = d.p_mean_variance(lambda xx, tt, **kw: mo, x, t, clip_denoised=bool(clip))
            for k in ("mean", "variance", "log_variance", "pred_xstart"):
                assert pm[k].shape == x.shape
                assert rel_err(pm[k].cpu().numpy(), ref[f"pmv_{k}"]) < 1e-5, (key, k)
            s, xs = d._step_math(mo, x, t, _d(g, "step/ps_noise"), clip)
            assert rel_err(s.cpu().numpy(), ref["ps_sample"]) < 1e-5, key
            assert rel_err(xs.cpu().numpy(), ref["pmv_pred_xstart"]) < 1e-5, key
            s, _ = d._obj_step(mo, x, t, _d(g, "step/ddim_noise"), clip, _STEP_DDIM, 0.5)
            assert rel_err(s.cpu().numpy(), ref["ddim_sample"]) < 1e-5, key
            s, _ = d._obj_step(mo, x, t, None, clip, _STEP_DDIM_REVERSE)
            assert rel_err(s.cpu().numpy(), ref["ddimrev_sample"]) < 1e-5, key
            # the public methods run the same kernels (their own draws): shapes, pred_xstart and the deterministic paths
            r = d.p_sample(lambda xx, tt, **kw: mo, x, t, clip_denoised=bool(clip))
            assert rel_err(r["pred_xstart"].cpu().numpy(), ref["pmv_pred_xstart"]) < 1e-5
            r = d.ddim_reverse_sample(lambda xx, tt, **kw: mo, x, t, clip_denoised=bool(clip))
            assert rel_err(r["sample"].cpu().numpy(), ref["ddimrev_sample"]) < 1e-5
            r = d.ddim_sample(lambda xx, tt, **kw: mo, x, t, clip_denoised=bool(clip), eta=0.0)
            s0, _ = d._obj_step(mo, x, t, torch.zeros_like(x), clip, _STEP_DDIM, 0.0)
            assert rel_err(r["sample"].cpu().numpy(), s0.cpu().numpy()) < 1e-6
            s1, _ = d._obj_step(mo, x, t, None, clip, _STEP_PSAMPLE)
            assert rel_err(s1.cpu().numpy(), pm["mean"].cpu().numpy()) < 1e-6


def test_generalised_kernels_match_default_kernels(obj):
    """At EPSILON / LEARNED_RANGE / MSE the mapdit_obj_* kernels agree with mapdit_loss_fwd / mapdit_psample_step /
    mapdit_ddim_step (which the default configuration keeps running) within 1e-6."""
    from mapdit_amd import _lib as L
    g = obj
    d = diffusion("250", "EPSILON", "LEARNED_RANGE", "MSE")
    mo, x0, noise = _d(g, "mo"), _d(g, "x0"), _d(g, "noise")
    t = _d(g, "s250/t")
    N, per = x0.shape[0], x0[0].numel()
    tab, otab = d._tables(x0.device), d._obj_tables(x0.device)
    xt = d.q_sample(x0, t, noise)
    outs = {}
    for name in ("old", "new"):
        mse, vb, loss = (torch.zeros(N, device=DEV) for _ in range(3))
        G = torch.zeros_like(mo)
        if name == "old":
            L.lib().loss_fwd(mo.data_ptr(), x0.data_ptr(), xt.data_ptr(), noise.data_ptr(), t.data_ptr(), tab.data_ptr(), 250,
                             mse.data_ptr(), vb.data_ptr(), loss.data_ptr(), G.data_ptr(), N, per, L.cur_stream())
        else:
            L.lib().obj_loss_fwd(mo.data_ptr(), x0.data_ptr(), xt.data_ptr(), noise.data_ptr(), t.data_ptr(), tab.data_ptr(),
                                 otab.data_ptr(), 250, 0, 0, 0, mse.data_ptr(), vb.data_ptr(), loss.data_ptr(), G.data_ptr(), N, per,
                                 L.cur_stream())
        outs[name] = (mse, vb, loss, G)
    for a, b in zip(outs["old"], outs["new"]):
        assert rel_err(b.cpu().numpy(), a.cpu().numpy()) < 1e-6
    w = [torch.randn(N, device=DEV) for _ in range(3)]
    d_old, d_new = torch.zeros_like(mo), torch.zeros_like(mo)
    L.lib().loss_bwd(outs["old"][3].data_ptr(), *(v.data_ptr() for v in w), d_old.data_ptr(), N, per, L.cur_stream())
    L.lib().obj_loss_bwd(outs["new"][3].data_ptr(), *(v.data_ptr() for v in w), d_new.data_ptr(), N, per, 2, L.cur_stream())
    assert rel_err(d_new.cpu().numpy(), d_old.cpu().numpy()) < 1e-6
    mo, x, t = _d(g, "step/mo"), _d(g, "step/x"), _d(g, "s250/step_t")
    N, per = x.shape[0], x[0].numel()
    pn, dn = _d(g, "step/ps_noise"), _d(g, "step/ddim_noise")
    for clip in (0, 1):
        a, b = torch.zeros_like(x), torch.zeros_like(x)
        xa, xb = torch.zeros_like(x), torch.zeros_like(x)
        L.lib().psample_step(mo.data_ptr(), x.data_ptr(), pn.data_ptr(), t.data_ptr(), tab.data_ptr(), 250, clip, a.data_ptr(),
                             xa.data_ptr(), N, per, L.cur_stream())
        L.lib().obj_step(mo.data_ptr(), x.data_ptr(), pn.data_ptr(), t.data_ptr(), tab.data_ptr(), otab.data_ptr(), 250, 0, 0, clip, 0,
                         0.0, b.data_ptr(), xb.data_ptr(), N, per, L.cur_stream())
        assert rel_err(b.cpu().numpy(), a.cpu().numpy()) < 1e-6 and rel_err(xb.cpu().numpy(), xa.cpu().numpy()) < 1e-6
        dt = d._ddim_tables(x.device)
        for reverse, eta in ((0, 0.5), (1, 0.0)):
            L.lib().ddim_step(mo.data_ptr(), x.data_ptr(), dn.data_ptr(), t.data_ptr(), tab.data_ptr(), dt.data_ptr(), 250, clip, eta,
                              reverse, a.data_ptr(), xa.data_ptr(), N, per, L.cur_stream())
            L.lib().obj_step(mo.data_ptr(), x.data_ptr(), dn.data_ptr(), t.data_ptr(), tab.data_ptr(), otab.data_ptr(), 250, 0, 0, clip,
                             2 if reverse else 1, eta, b.data_ptr(), xb.data_ptr(), N, per, L.cur_stream())
            assert rel_err(b.cpu().numpy(), a.cpu().numpy()) < 1e-6 and rel_err(xb.cpu().numpy(), xa.cpu().numpy()) < 1e-6


def _inject_noise(monkeypatch, noise):
    """calc_bpd_loop draws exactly one torch.randn_like(x_start) per timestep, T-1 down to 0: hand it the recorded draws."""
    it = iter(noise)
    monkeypatch.setattr(torch, "randn_like", lambda x, **kw: next(it).to(x.device))


def bpd_model(var):
    def f(x, t, **kw):
        m = 0.3 * x + 0.001 * t.float().view(-1, 1, 1, 1)
        return torch.cat([m, torch.tanh(x)], 1) if var == "LEARNED_RANGE" else m
    return f


@pytest.mark.parametrize("mean", MEANS)
@pytest.mark.parametrize("var", VARS)
def test_calc_bpd_loop_synthetic(monkeypatch, mean, var):
    g = load_golden("bpd_synthetic")
    key = f"{mean}/{var}"
    d = diffusion("10", mean, var, "MSE")
    _inject_noise(monkeypatch, _d(g, key + "/noise"))
    r = d.calc_bpd_loop(bpd_model(var), _d(g, "x0"))
    monkeypatch.undo()
    assert sorted(r) == ["mse", "prior_bpd", "total_bpd", "vb", "xstart_mse"]
    for k, v in r.items():
        assert v.shape == g[f"{key}/{k}"].shape
        assert rel_err(v.cpu().numpy(), g[f"{key}/{k}"]) < 1e-5, k
    # the pieces on their own
    x0 = _d(g, "x0")
    assert rel_err(d._prior_bpd(x0).cpu().numpy(), g[f"{key}/prior_bpd"]) < 1e-5
    t = torch.full((x0.shape[0],), 4, device=DEV, dtype=torch.int64)
    nz = _d(g, key + "/noise")[10 - 1 - 4]
    x_t = d.q_sample(x0, t, nz)
    out = d._vb_terms_bpd(bpd_model(var), x0, x_t, t, clip_denoised=True)
    assert rel_err(out["output"].cpu().numpy(), g[f"{key}/vb"][:, 10 - 1 - 4]) < 1e-5     # columns in loop order, t = 9 first
    eps = d._predict_eps_from_xstart(x_t, t, out["pred_xstart"])
    assert rel_err(((eps - nz) ** 2).mean(dim=(1, 2, 3)).cpu().numpy(), g[f"{key}/mse"][:, 10 - 1 - 4]) < 1e-5


def test_q_helpers_match_their_definitions():
    d = diffusion("250", "EPSILON", "FIXED_LARGE", "MSE")
    g = torch.Generator().manual_seed(5)
    x0, xt = torch.randn(3, 4, 8, 8, generator=g).to(DEV), torch.randn(3, 4, 8, 8, generator=g).to(DEV)
    t = torch.tensor([0, 17, 249], device=DEV)
    f = lambda a, i: torch.tensor(np.asarray(a)[[0, 17, 249]], dtype=torch.float32, device=DEV).view(-1, 1, 1, 1)
    m, v, lv = d.q_mean_variance(x0, t)
    assert torch.allclose(m, f(d.sqrt_alphas_cumprod, t) * x0) and torch.allclose(v, f(1 - d.alphas_cumprod, t).expand_as(x0))
    assert torch.allclose(lv, f(d.log_one_minus_alphas_cumprod, t).expand_as(x0))
    pm, pv, plv = d.q_posterior_mean_variance(x0, xt, t)
    assert torch.allclose(pm, f(d.posterior_mean_coef1, t) * x0 + f(d.posterior_mean_coef2, t) * xt)
    assert torch.allclose(plv, f(d.posterior_log_variance_clipped, t).expand_as(x0))
    eps = torch.randn(3, 4, 8, 8, generator=g).to(DEV)
    xs = d._predict_xstart_from_eps(xt, t, eps)
    assert torch.allclose(d._predict_eps_from_xstart(xt, t, xs), eps, atol=1e-3)


def _tiny_model(g, precision):
    from mapdit_amd.src.dit import DiT
    cfg = golden_cfg(g)
    m = DiT(**cfg.to_dict())
    m.load_state_dict(golden_state_dict(g, cfg), strict=True)
    m = m.to(DEV)
    m.gemm_precision = precision
    return m, cfg


def _bpd_inputs(g):
    """calc_bpd_loop runs on the first two samples of the fixture."""
    nb = g["bpd/total_bpd"].shape[0]
    return _d(g, "x0")[:nb].contiguous(), dict(y=_d(g, "y")[:nb].contiguous())


def test_calc_bpd_loop_tiny_a_bf16x3(monkeypatch):
    from mapdit_amd.diffusion import create_diffusion
    g = load_golden("bpd_tiny_a")
    m, _ = _tiny_model(g, "bf16x3")
    m.eval()
    _inject_noise(monkeypatch, _d(g, "bpd/noise"))
    x0, kw = _bpd_inputs(g)
    r = create_diffusion("10").calc_bpd_loop(m.forward, x0, model_kwargs=kw)
    monkeypatch.undo()
    for k in ("total_bpd", "prior_bpd"):
        assert rel_err(r[k].cpu().numpy(), g["bpd/" + k]) < 1e-4, k
    for k in ("vb", "xstart_mse", "mse"):
        assert rel_err(r[k].cpu().numpy(), g["bpd/" + k]) < 1e-3, k


def test_calc_bpd_loop_tiny_a_default_f16(monkeypatch):
    from mapdit_amd.diffusion import create_diffusion
    g = load_golden("bpd_tiny_a")
    m, _ = _tiny_model(g, "f16")
    m.eval()
    _inject_noise(monkeypatch, _d(g, "bpd/noise"))
    x0, kw = _bpd_inputs(g)
    r = create_diffusion("10").calc_bpd_loop(m.forward, x0, model_kwargs=kw)
    monkeypatch.undo()
    e = rel_err(r["total_bpd"].cpu().numpy(), g["bpd/total_bpd"])
    print(f"f16 total_bpd rel err {e:.2e}")
    assert e < F16_BPD_TOL


@pytest.mark.parametrize("tag,kw", [("kl", dict(use_kl=True)), ("xs_rmse", dict(predict_xstart=True, rescale_learned_sigmas=True))])
def test_training_step_tiny_a_bf16x3(tag, kw):
    from conftest import sub
    from mapdit_amd.diffusion import create_diffusion
    g = load_golden("bpd_tiny_a")
    m, cfg = _tiny_model(g, "bf16x3")
    m.train()
    m.y_embedder.token_drop = lambda labels, force_drop_ids=None: labels        # the recorded label drop is in y_eff
    seen = {}

    def model_fn(xx, tt, **kw2):
        o = m(xx, tt, **kw2)
        o.retain_grad()
        seen["out"] = o
        return o
    losses = create_diffusion("", **kw).training_losses(model_fn, _d(g, "x0"), _d(g, f"{tag}/t"), dict(y=_d(g, f"{tag}/y_eff")),
                                                        noise=_d(g, "train_noise"))
    assert sorted(losses) == [str(k) for k in g[f"{tag}/keys"]]
    for k in losses:
        assert rel_err(losses[k].detach().cpu().numpy(), g[f"{tag}/{k}"]) < 1e-5, k
    losses["loss"].mean().backward()
    torch.cuda.synchronize()
    e_out = rel_err(seen["out"].grad.cpu().numpy(), g[f"{tag}/model_out_grad"])
    worst, worst_k = 0.0, ""
    for k, p in m.named_parameters():
        if float(g[f"{tag}/gradnorm/{k}"]) < 1e-12:
            continue
        e = rel_err(sub(p.grad, stride=97, limit=512), g[f"{tag}/grad/{k}"])       # the fixture's sub-sampling
        e = max(e, abs(float(p.grad.double().norm()) / float(g[f"{tag}/gradnorm/{k}"]) - 1))
        if e > worst:
            worst, worst_k = e, k
    print(f"{tag}: model-output gradient rel err {e_out:.2e}; worst parameter gradient {worst:.2e} ({worst_k})")
    assert e_out < 1e-4
    assert worst < 1e-4, (worst_k, worst)


def test_graphed_sampler_x0_prediction_equals_eager():
    """GraphedSampler on a START_X diffusion replays the generalised step kernel: one replay at t = 0 (no draw) equals the
    eager step bit for bit, and a prefix of the chain stays finite; a fixed-variance diffusion (a DiT always outputs
    learned-range channels) is refused."""
    from mapdit_amd.diffusion import create_diffusion
    from mapdit_amd.sampling import GraphedSampler
    g = load_golden("bpd_tiny_a")
    m, cfg = _tiny_model(g, "bf16")
    m.eval()
    d = create_diffusion("10", predict_xstart=True)
    z, y = _d(g, "x0"), _d(g, "y")
    s = GraphedSampler(m, d, tuple(z.shape), y)
    assert s.otab is not None
    s.img.copy_(z)
    s.t.fill_(0)
    s.graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        t0 = torch.zeros(z.shape[0], dtype=torch.int64, device=DEV)
        mo = d._wrap_model(m.forward)(z, t0, y=y)
        ref, _ = d._step_math(mo, z, t0, torch.zeros_like(z), False)
        eager = d.p_mean_variance(m.forward, z, t0, clip_denoised=False, model_kwargs=dict(y=y))["mean"]
    assert torch.equal(s.img, ref) and torch.equal(eager, ref)
    out = s.sample(z, steps=3)
    assert torch.isfinite(out).all() and int(s.t[0]) == 9 - 3
    with pytest.raises(NotImplementedError, match="FIXED_LARGE"):
        GraphedSampler(m, create_diffusion("10", learn_sigma=False), tuple(z.shape), y)
