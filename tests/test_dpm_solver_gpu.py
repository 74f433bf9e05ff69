"""DPM-Solver++ on the GPU: mapdit_dpm_step against the fp64 restatement of tests/test_dpm_solver_cpu.py, order 1 against the pinned
DDIM loop, convergence to an exact solution of the probability-flow ODE, the captured sampler against the eager loop, the hooks.

Rounding bound of one step (fp32 kernel against fp64 on the same fp32 tables), elementwise:
    |got - ref| <= 16 x 2^-24 x (|c_x x| + |c_0 D| + |c_1 hist| + |D-terms|)
about six roundings of at most 2^-24 of the term magnitudes each, and room for FMA contraction.  Over several steps the bound is
propagated through the step's own (linear, 1-Lipschitz-clamped) dependence on x and hist (``hooked_reference``)."""
import numpy as np
import pytest
import torch

from test_dpm_solver_cpu import ref_schedule, ref_step, ref_xstart

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 16 * 2.0 ** -24


def make_diffusion(respacing, mean="EPSILON", var="LEARNED_RANGE"):
    from mapdit_amd.diffusion import create_diffusion
    return create_diffusion(respacing, predict_xstart=mean == "START_X", learn_sigma=var == "LEARNED_RANGE",
                            sigma_small=var == "FIXED_SMALL")


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("shape,steps", [((3, 4, 6, 6), (11, 5, 0)), ((2, 4, 8, 8), (4, 1))])
@pytest.mark.parametrize("mean", ["EPSILON", "START_X"])
@pytest.mark.parametrize("var", ["LEARNED_RANGE", "FIXED_SMALL"])
def test_one_step_matches_fp64(shape, steps, mean, var):
    """per_sample 144 (a ragged last block, no multiple of 64) and 256; step indices that differ per sample and cover a row without
    history (K-1, and 1 under lower_order_final), rows with c_1 != 0 and the final row; clip on / off, xstart_in given / null, sample
    written to a new tensor / over x."""
    d = make_diffusion("250", mean, var)
    tabs = d._dpm_tables(torch.device(DEV), 12, 2, "logsnr", True)
    tau, ctab, taus = tabs
    K = len(taus)
    assert K == 12 and d._out_channels(4) == (8 if var == "LEARNED_RANGE" else 4)
    c32 = ctab.cpu().numpy()
    assert c32[11, 2] == 0 and c32[1, 2] == 0 and c32[5, 2] != 0 and c32[4, 2] != 0 and tuple(c32[0]) == (0, 1, 0)
    g = torch.Generator().manual_seed(sum(shape) + len(mean) + len(var))
    N, C = shape[:2]
    x = torch.randn(shape, generator=g).to(DEV)
    mo = torch.randn(N, d._out_channels(C), *shape[2:], generator=g).to(DEV)
    hist0 = (0.7 * torch.randn(shape, generator=g)).to(DEV)
    given = (0.8 * torch.randn(shape, generator=g)).to(DEV)
    step = torch.tensor(steps, dtype=torch.int64, device=DEV)
    worst = 0.0
    for clip in (False, True):
        for xin in (None, given):
            ref, D, mag = ref_step(d, _np(x), _np(mo[:, :C]), _np(hist0), np.array(steps), taus, c32, mean, clip,
                                   None if xin is None else _np(xin))
            if clip:
                assert (np.abs(D) == 1).any() and (np.abs(D) < 1).any()
            for alias in (False, True):
                xx, hist = x.clone(), hist0.clone()
                sample, xstart = d._dpm_step(mo, xx, hist, step, tabs, clip, xstart_in=xin, sample=xx if alias else None)
                torch.cuda.synchronize()
                assert (sample.data_ptr() == xx.data_ptr()) == alias and (alias or torch.equal(xx, x))
                assert torch.equal(xstart, hist)
                e_s, e_h = np.abs(_np(sample) - ref), np.abs(_np(hist) - D)
                worst = max(worst, float((e_s / (U * mag)).max()), float((e_h / (U * mag)).max()))
                assert (e_s <= U * mag).all() and (e_h <= U * mag).all(), (clip, xin is not None, alias, worst)
    print(f"{shape} {mean} {var}: worst error / bound {worst:.3f}")


def test_out_of_range_step_is_reported_not_faulted():
    from mapdit_amd import _lib as L
    d = make_diffusion("250")
    tabs = d._dpm_tables(torch.device(DEV), 12, 2, "logsnr", True)
    x, mo = torch.randn(3, 4, 6, 6, device=DEV), torch.randn(3, 8, 6, 6, device=DEV)
    L.lib().device_error_poll(L.cur_stream())                       # nothing pending
    for bad, clamped in ((12, 11), (-1, 0), (1 << 40, 11)):
        step = torch.tensor([3, bad, 0], dtype=torch.int64, device=DEV)
        hist = torch.zeros_like(x)
        sample, _ = d._dpm_step(mo, x, hist, step, tabs, False)
        with pytest.raises(L.MapditError, match="timestep"):
            L.lib().device_error_poll(L.cur_stream())
        L.lib().device_error_poll(L.cur_stream())                   # the record is cleared
        want, _ = d._dpm_step(mo, x, torch.zeros_like(x), torch.tensor([3, clamped, 0], dtype=torch.int64, device=DEV), tabs, False)
        assert torch.equal(sample, want)                            # the index was clamped, nothing was read out of bounds
    # the host-side checks: nothing is launched
    p = lambda v: None if v is None else v.data_ptr()
    tau, ctab, taus = tabs
    step, hist, out = torch.zeros(3, dtype=torch.int64, device=DEV), torch.zeros_like(x), torch.empty_like(x)

    def call(mo_=mo, x_=x, hist_=hist, K=len(taus), mean_type=0, var_type=0, xin=None, sample=out, xs=None, n=3):
        L.lib().dpm_step(p(mo_), p(x_), p(hist_), step.data_ptr(), ctab.data_ptr(), tau.data_ptr(), K, d._tables(x.device).data_ptr(), 250,
                         mean_type, var_type, 0, p(xin), p(sample), p(xs), n, 144, L.cur_stream())
    for kw, match in ((dict(x_=None), "null/empty"), (dict(hist_=None), "null/empty"), (dict(n=0), "null/empty"), (dict(K=0), "null/empty"),
                      (dict(mean_type=2), "bad objective"), (dict(var_type=3), "bad objective"), (dict(mo_=None), "model output"),
                      (dict(hist_=x), "overlapping"), (dict(sample=hist), "overlapping"), (dict(xs=out), "overlapping")):
        with pytest.raises(L.MapditError, match=match):
            call(**kw)
    call(mo_=None, xin=mo[:, :4].contiguous(), sample=x)             # model_out may be null with xstart_in; sample may alias x
    L.lib().device_error_poll(L.cur_stream())


def smooth_eps(x, t):
    """A smooth 'model': eps(x, t), the same expression for torch (fp32) and numpy (fp64) inputs."""
    lib = torch if isinstance(x, torch.Tensor) else np
    return 0.5 * lib.sin(x) + 0.1 * lib.cos(t / 1000.0).reshape(-1, 1, 1, 1)


def ddim_reference(d, noise, clip):
    """ddim_sample_loop(eta = 0) restated in fp64 (reference gaussian_diffusion.py:513-567, 638-680) on the fp64 schedule."""
    x = noise.astype(np.float64)
    tmap = np.array(d.timestep_map)
    for i in range(d.num_timesteps)[::-1]:
        t = np.full(x.shape[0], i)
        eps = smooth_eps(x, tmap[t].astype(np.float64))
        xs = d.sqrt_recip_alphas_cumprod[i] * x - d.sqrt_recipm1_alphas_cumprod[i] * eps
        if clip:
            xs = np.clip(xs, -1, 1)
        eps = (d.sqrt_recip_alphas_cumprod[i] * x - xs) / d.sqrt_recipm1_alphas_cumprod[i]
        x = xs * np.sqrt(d.alphas_cumprod_prev[i]) + np.sqrt(1 - d.alphas_cumprod_prev[i]) * eps
    return x


@pytest.mark.parametrize("clip", [False, True])
def test_order_one_is_ddim(clip):
    """dpm_solver_sample_loop(order=1, spacing="uniform", num_steps=n) visits every timestep with the DDIM eta = 0 update associated
    differently.  Yardstick: the pinned ddim_sample_loop's own deviation from the fp64 loop on the same inputs; the solver may
    deviate at most 4 x as much.  (Measured figures: DESIGN.md section 5.)"""
    d = make_diffusion("25")
    n = d.num_timesteps
    model = lambda x, t, **kw: torch.cat([smooth_eps(x, t.float()), torch.zeros_like(x)], dim=1)
    noise = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(3)).to(DEV)
    ref = ddim_reference(d, _np(noise), clip)
    ddim = d.ddim_sample_loop(model, noise.shape, noise=noise, clip_denoised=clip, eta=0.0, device=DEV)
    dpm = d.dpm_solver_sample_loop(model, noise.shape, noise=noise, clip_denoised=clip, device=DEV, num_steps=n, order=1, spacing="uniform")
    dev_ddim, dev_dpm = float(np.abs(_np(ddim) - ref).max()), float(np.abs(_np(dpm) - ref).max())
    print(f"clip {clip}: max deviation from fp64: ddim {dev_ddim:.3e}, dpm-solver++ order 1 {dev_dpm:.3e}; |ref| max {np.abs(ref).max():.3f}")
    assert np.isfinite(ref).all() and dev_ddim > 0
    assert dev_dpm <= 4 * dev_ddim, (dev_dpm, dev_ddim)


def test_convergence_to_exact_solution():
    """Data N(0, I): the exact eps predictor is eps = sigma_t x, the probability-flow ODE then leaves x unchanged, and the sampler's
    exact output is the exact denoiser at tau_0 applied to the initial noise, alpha_{tau_0} x_T.  Full 1000-step linear schedule,
    "logsnr" spacing; num_steps 20 / 40 / 80 deduplicate to 20 / 39 / 76.  Error = max |got - exact| / max |exact|; in fp64 numpy:
        order 1: 1.19e-1, 6.0e-2, 3.0e-2 (ratios 1.99, 1.99)     order 2: 1.45e-2, 3.75e-3, 9.3e-4 (ratios 3.87, 4.04)
    Asserted: order 2 beats order 1 at every K; each doubling shrinks the order-2 error >= 3 x (second order: 4, first order: 2); the
    order-1 ratio lies in [1.5, 2.5].  The fp32 floor (~1e-6) is far below every value involved."""
    d = make_diffusion("")
    sig = torch.from_numpy(np.sqrt(1.0 - d.alphas_cumprod)).float().to(DEV)
    model = lambda x, t, **kw: torch.cat([sig[t].view(-1, 1, 1, 1) * x, torch.zeros_like(x)], dim=1)
    noise = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(0)).to(DEV)
    exact = np.sqrt(d.alphas_cumprod[0]) * _np(noise)
    err = {}
    for order in (1, 2):
        for num_steps, K in ((20, 20), (40, 39), (80, 76)):
            assert len(d._dpm_schedule(num_steps, order, "logsnr")[0]) == K
            out = d.dpm_solver_sample_loop(model, noise.shape, noise=noise, clip_denoised=False, device=DEV, num_steps=num_steps,
                                           order=order, spacing="logsnr")
            err[order, K] = float(np.abs(_np(out) - exact).max() / np.abs(exact).max())
    print({k: f"{v:.3e}" for k, v in err.items()})
    for K in (20, 39, 76):
        assert err[2, K] < err[1, K]
    for a, b in ((20, 39), (39, 76)):
        assert err[2, a] / err[2, b] >= 3.0, (err[2, a], err[2, b])
        assert 1.5 <= err[1, a] / err[1, b] <= 2.5, (err[1, a], err[1, b])


@pytest.fixture(scope="module")
def xs2():
    """DiT-XS/2 on 16x16 latents (64 tokens), the oracle's initialisation (a fresh DiT's output layer is zero)."""
    from mapdit_amd.src.dit import DiT
    from oracle import dit_oracle as O
    cfg = O.DiTConfig(depth=6, hidden_size=256, patch_size=2, input_size=16, in_channels=4, num_heads=4, num_classes=10)
    m = DiT(**cfg.to_dict())
    m.load_state_dict(O.init_state_dict(cfg, seed=7, gains=0.3, perturb_reference=0.3))
    return m.to(DEV).eval()


@pytest.mark.parametrize("cfg_scale,respacing", [(None, "250"), (1.5, "")])
def test_captured_sampler_is_bit_equal_to_eager(xs2, cfg_scale, respacing):
    from mapdit_amd import sampling as S
    d = make_diffusion(respacing)
    g = torch.Generator().manual_seed(11)
    z = torch.randn(1, 4, 16, 16, generator=g)
    z = torch.cat([z, z] if cfg_scale else [z, torch.randn(1, 4, 16, 16, generator=g)]).to(DEV)
    y = torch.tensor([3, 10] if cfg_scale else [3, 7], device=DEV)
    kw = dict(y=y) if cfg_scale is None else dict(y=y, cfg_scale=cfg_scale)
    fn = xs2.forward if cfg_scale is None else xs2.forward_with_cfg
    with torch.no_grad():
        eager = d.dpm_solver_sample_loop(fn, z.shape, noise=z, clip_denoised=False, model_kwargs=kw, device=DEV, num_steps=6)
    assert torch.isfinite(eager).all() and not torch.equal(eager, z)
    gs = S.GraphedSampler(xs2, d, z.shape, y, cfg_scale, clip_denoised=False, sampler="dpm++", num_steps=6)
    assert gs.num_replays == 6
    first = gs.sample(z)
    assert torch.equal(first, eager)
    assert torch.equal(gs.sample(z), first)                      # hist and the step index are reset
    assert torch.equal(S.run_sampler(xs2, d, z, y, cfg_scale, use_graph=False, sampler="dpm++", num_steps=6), eager)
    assert torch.equal(S.dpm_solver_sample_loop_graphed(d, xs2, z.shape, z, False, kw, num_steps=6), eager)
    order1 = S.dpm_solver_sample_loop_graphed(d, xs2, z.shape, z, False, kw, num_steps=6, order=1, spacing="uniform")
    assert torch.isfinite(order1).all() and not torch.equal(order1, eager)


def test_ancestral_sampler_still_runs(xs2):
    """The default sampler is the captured p_sample step it was (clip on: without it the chain of an untrained network overflows the
    16-bit engine, in the eager loop too); its last step, which draws no noise, equals the eager kernel bit for bit."""
    from mapdit_amd import sampling as S
    d = make_diffusion("4")
    z = torch.randn(2, 4, 16, 16, device=DEV)
    y = torch.tensor([3, 7], device=DEV)
    gs = S.GraphedSampler(xs2, d, z.shape, y, clip_denoised=True)
    assert gs.dpm is None and gs.num_replays == 4
    out = gs.sample(z)
    assert out.shape == z.shape and torch.isfinite(out).all()
    gs.img.copy_(z)
    gs.t.fill_(0)
    gs.graph.replay()
    with torch.no_grad():
        t0 = torch.zeros(2, dtype=torch.int64, device=DEV)
        want = d._step_math(d._wrap_model(xs2.forward)(z, t0, y=y), z, t0, torch.zeros_like(z), True)[0]
    assert torch.equal(gs.img, want)
    out = S.p_sample_loop_graphed(d, xs2, z.shape, z, True, dict(y=y))
    assert out.shape == z.shape and torch.isfinite(out).all()
    with pytest.raises(ValueError, match="sampler"):
        S.GraphedSampler(xs2, d, z.shape, y, sampler="heun")


def denoised_fn(x0):
    return x0.clamp(-0.5, 0.5)


def hooked_reference(d, x0, mo, target, scale, sched, steps, mean, clip, den, cond):
    """The first `steps` solver steps with hooks in fp64 on the fp32 tables -> per step (sample, pred_xstart, bound on the sample, bound on
    pred_xstart).  denoised_fn = clamp(-0.5, 0.5) on the raw x0, then the clip; cond_fn = scale (target - x) through
    condition_score: x0 += sqrt_recipm1_acp sqrt(1 - acp) grad after the clip.  The bounds are the one-step bound plus the errors
    carried in by x and hist, through |c_x|, |c_0| x (d x0 / d x), |c_1|."""
    tau, c32 = sched
    K = len(tau)
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    x, hist = x0.copy(), np.zeros_like(x0)
    e_x, e_h = np.zeros_like(x0), np.zeros_like(x0)
    out = []
    for i in range(K - 1, K - 1 - steps, -1):
        t = int(tau[i])
        raw, terms = ref_xstart(d, x, mo, np.full(x.shape[0], t), mean, False)
        ra = f32(d.sqrt_recip_alphas_cumprod)[t] if mean == "EPSILON" else 0.0
        D = np.clip(raw, -0.5, 0.5) if den else raw
        if clip:
            D = np.clip(D, -1, 1)
        dD_dx = ra                                     # the clamps are 1-Lipschitz
        if cond:
            gk = f32(d.sqrt_recipm1_alphas_cumprod)[t] * np.sqrt(1.0 - f32(d.alphas_cumprod)[t])
            D = D + gk * scale * (target - x)
            terms = terms + np.abs(gk * scale * (target - x)) + gk * scale * (np.abs(target) + np.abs(x))
            dD_dx = ra + gk * scale
        e_D = U * (terms + np.abs(D)) + dD_dx * e_x
        cx, c0, c1 = c32[i].astype(np.float64)
        sample = cx * x + c0 * D + c1 * hist
        e_s = U * (np.abs(cx * x) + np.abs(c0 * D) + np.abs(c1 * hist)) + abs(cx) * e_x + abs(c0) * e_D + abs(c1) * e_h
        out.append((sample, D, e_s, e_D))
        x, hist, e_x, e_h = sample, D, e_s, e_D
    return out


@pytest.mark.parametrize("mean", ["EPSILON", "START_X"])
@pytest.mark.parametrize("hooks", ["denoised_fn", "cond_fn", "both"])
def test_hooks_match_fp64(mean, hooks):
    d = make_diffusion("250", mean)
    g = torch.Generator().manual_seed(5)
    shape = (3, 4, 6, 6)
    z, mo, target = (torch.randn(s, generator=g).to(DEV) for s in (shape, (3, 8, 6, 6), shape))
    if mean == "START_X":
        mo = 0.6 * mo                                                 # x0 predictions on both sides of the 0.5 clamp
    scale = 0.05
    den, cond = hooks != "cond_fn", hooks != "denoised_fn"
    seen = []

    def cond_fn(x, t, **kw):
        seen.append(t.clone())
        return scale * (target - x)
    tau, c64 = d._dpm_schedule(5, 2, "logsnr", True)
    rtau, rc = ref_schedule(d.alphas_cumprod, 5, 2, "logsnr", True)
    assert np.array_equal(tau, rtau)
    np.testing.assert_allclose(c64, rc, rtol=1e-13)
    sched = (tau, d._dpm_tables(torch.device(DEV), 5, 2, "logsnr", True)[1].cpu().numpy())      # the fp32 table the kernel reads
    loop = d.dpm_solver_sample_loop_progressive(lambda x, t, **kw: mo, shape, noise=z, clip_denoised=True, denoised_fn=denoised_fn if den else None,
                                                cond_fn=cond_fn if cond else None, device=DEV, num_steps=5)
    ref = hooked_reference(d, _np(z), _np(mo[:, :4]), _np(target), scale, sched, 3, mean, True, den, cond)
    worst = 0.0
    for k, (o, (r_s, r_D, b_s, b_D)) in enumerate(zip(loop, ref)):
        e_s, e_D = np.abs(_np(o["sample"]) - r_s), np.abs(_np(o["pred_xstart"]) - r_D)
        worst = max(worst, float((e_s / b_s).max()), float((e_D / b_D).max()))
        assert (e_s <= b_s).all() and (e_D <= b_D).all(), (k, worst)
        if den and not cond:
            assert np.abs(_np(o["pred_xstart"])).max() <= 0.5
    if cond:                # cond_fn sees the base schedule's timesteps, as the model does
        want = [d.timestep_map[int(tau[i])] for i in (4, 3, 2)]
        assert [int(t[0]) for t in seen[:3]] == want and all((t == t[0]).all() for t in seen)
    print(f"{mean} {hooks}: worst error / propagated bound {worst:.3f}")


def test_launch_count_and_refusals(monkeypatch):
    """After the model an unhooked step is one library launch; denoised_fn adds mapdit_obj_xstart, cond_fn mapdit_obj_step_guided (no new
    guided kernel); the loop ends with the device-error poll.  The captured entry refuses both hooks."""
    from mapdit_amd import _lib as L
    from mapdit_amd import sampling as S
    d = make_diffusion("250")
    z, mo = torch.randn(2, 4, 8, 8, device=DEV), torch.randn(2, 8, 8, 8, device=DEV)
    stub = lambda x, t, **kw: mo
    real, calls = L.lib(), []

    class Counting:
        def __getattr__(self, k):
            calls.append(k)
            return getattr(real, k)
    monkeypatch.setattr(L, "lib", lambda: Counting())
    d.dpm_solver_sample_loop(stub, z.shape, noise=z, device=DEV, num_steps=4)
    assert calls == ["dpm_step"] * 4 + ["device_error_poll"]
    calls.clear()
    d.dpm_solver_sample_loop(stub, z.shape, noise=z, device=DEV, num_steps=3, denoised_fn=denoised_fn)
    assert calls == ["obj_xstart", "dpm_step"] * 3 + ["device_error_poll"]
    calls.clear()
    d.dpm_solver_sample_loop(stub, z.shape, noise=z, device=DEV, num_steps=3, denoised_fn=denoised_fn, cond_fn=lambda x, t, **kw: -0.1 * x)
    assert calls == ["obj_xstart", "obj_step_guided", "dpm_step"] * 3 + ["device_error_poll"]
    for hook in ("denoised_fn", "cond_fn"):
        with pytest.raises(NotImplementedError, match="captured sampler"):
            S.dpm_solver_sample_loop_graphed(d, None, z.shape, z, False, dict(y=None), **{hook: denoised_fn})


def test_sampler_clis_run_dpm_solver(tmp_path):
    """--sampler dpm++ through the three scripts, captured and eager, on a network trained for 8 steps (shapes only: such a network
    denoises nothing)."""
    from mapdit_amd import sample, sample_ema, sample_fid, train
    exp = train.main(["--synthetic", "--results-dir", str(tmp_path), "--model", "DiT-XS/2", "--num-steps", "8", "--batch-size", "8",
                      "--log-every", "4", "--ckpt-every", "8", "--ema-snapshot-every", "2", "--num-classes", "10",
                      "--num-lin-warmup", "2", "--start-decay", "3", "--verbose", "0"])
    base = ["--result-dir", exp, "--use-vae", "false", "--sampler", "dpm++", "--num-sampling-steps", "3"]
    path = sample_fid.main(base + ["--num-classes", "10", "--batch-size", "4", "--num-samples", "6", "--output-file", "a.npz"])
    assert np.load(path)["arr_0"].shape == (6, 32, 32, 4)
    path = sample_fid.main(base + ["--num-classes", "10", "--batch-size", "4", "--num-samples", "4", "--cfg-scale", "1.0", "--no-graph",
                                   "--solver-order", "1", "--solver-spacing", "uniform", "--output-file", "b.npz"])
    assert np.load(path)["arr_0"].shape == (4, 32, 32, 4)
    out = str(tmp_path / "grid.png")
    assert sample.main(base + ["--class-label", "3", "--output-file", out]).shape == (4, 4, 32, 32)
    assert sample.main(base + ["--class-label", "3", "--output-file", out, "--no-graph"]).shape == (4, 4, 32, 32)
    assert sample_ema.main(base + ["--class-label", "0", "--output-file", out]).shape == (8 * 5, 4, 32, 32)
