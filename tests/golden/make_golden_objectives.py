#!/usr/bin/env python3
"""Golden vectors for the diffusion objectives and the likelihood evaluation (runs ONLY in the build container, where the
reference checkout exists; see make_golden.py).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_objectives.py

Writes three fixtures, inputs and expected outputs only (nothing of the reference is copied):
  objectives.npz      synthetic model outputs fed as leaf tensors, every (mean, variance, loss) objective on the full
                      1000-step schedule and on '250': the loss dict, the output gradient for random per-key weights, and
                      p_mean_variance / p_sample / ddim_sample / ddim_reverse_sample at mixed t (t = 0 included) and at t = 0,
                      clip on and off.
  bpd_synthetic.npz   calc_bpd_loop on '10' for each (mean, variance) pair with a fixed torch-expressible model and the
                      recorded per-timestep noise.
  bpd_tiny_a.npz      the tiny_a DiT (weights from oracle.dit_oracle.init_state_dict): calc_bpd_loop on '10' with labels
                      (the first two samples),
                      and one training forward / backward under create_diffusion('', use_kl=True) and under
                      create_diffusion('', predict_xstart=True, rescale_learned_sigmas=True).
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"
sys.path.insert(0, REF)

import warnings

import numpy as np
import torch

warnings.filterwarnings("ignore")
torch.set_num_threads(8)

from src.dit import DiT as RefDiT                        # noqa: E402  (reference)
from diffusion import create_diffusion as ref_create     # noqa: E402  (reference)
from diffusion import gaussian_diffusion as rgd          # noqa: E402  (reference)
from diffusion.respace import SpacedDiffusion as RefSpaced, space_timesteps as ref_space   # noqa: E402  (reference)

from oracle import dit_oracle as O                       # noqa: E402

MEANS = ["EPSILON", "START_X"]
VARS = ["LEARNED_RANGE", "FIXED_SMALL", "FIXED_LARGE"]
LOSSES = ["MSE", "RESCALED_MSE", "KL", "RESCALED_KL"]
SCHEDS = {"full": "", "s250": "250"}
STEP_OUTPUTS = ["pmv_mean", "pmv_variance", "pmv_log_variance", "pmv_pred_xstart", "ps_sample", "ddim_sample", "ddimrev_sample"]
STRIDE = 97            # tiny_a parameter gradients: every 97th entry of tensors above FULL_LIMIT (+ the whole-tensor norm)
FULL_LIMIT = 512


def ref_diffusion(sched, mean, var, loss):
    return RefSpaced(use_timesteps=ref_space(1000, sched or [1000]), betas=rgd.get_named_beta_schedule("linear", 1000),
                     model_mean_type=rgd.ModelMeanType[mean], model_var_type=rgd.ModelVarType[var], loss_type=rgd.LossType[loss])


def sub(a):
    f = a.detach().reshape(-1)
    return (f if f.numel() <= FULL_LIMIT else f[::STRIDE]).numpy().copy()


def synthetic_objectives():
    # loss tier: 288 elements per sample (more than one pass of the 256-thread blocks); sample 0 sits at t = 0 with x0 entries at
    # the decoder's +-0.999 edges and beyond
    N, C, S = 3, 2, 12
    g = torch.Generator().manual_seed(31)
    out = {"N": np.array(N), "C": np.array(C), "S": np.array(S), "step_outputs": np.array(STEP_OUTPUTS)}
    x0 = torch.randn(N, C, S, S, generator=g).clamp(-1.2, 1.2)
    x0[0, 0, 0, :4] = torch.tensor([-1.5, 1.5, 0.9995, -0.9995])
    x0[0, 1, 2, :4] = torch.tensor([-0.9995, 0.9995, 1.5, -1.5])
    noise = torch.randn(N, C, S, S, generator=g)
    mo2 = torch.randn(N, 2 * C, S, S, generator=g) * 0.7
    out.update(x0=x0.numpy(), noise=noise.numpy(), mo=mo2.numpy())
    # step tier (elementwise kernels): small tensors
    SN, SS = 4, 4
    xs = torch.randn(SN, C, SS, SS, generator=g)
    smo2 = torch.randn(SN, 2 * C, SS, SS, generator=g) * 0.7
    out.update({"step/x": xs.numpy(), "step/mo": smo2.numpy()})
    torch.manual_seed(101)
    out["step/ps_noise"] = torch.randn_like(xs).numpy()
    torch.manual_seed(102)
    out["step/ddim_noise"] = torch.randn_like(xs).numpy()
    for tag, sched in SCHEDS.items():
        T = 1000 if sched == "" else 250
        t = torch.tensor([0, 5, T - 1])
        out[f"{tag}/t"] = t.numpy()
        st = torch.tensor([0, 5, T // 2 + 3, T - 1])
        out[f"{tag}/step_t"] = st.numpy()
        d = ref_diffusion(sched, "EPSILON", "LEARNED_RANGE", "MSE")
        rows = {"alphas_cumprod": d.alphas_cumprod, "alphas_cumprod_prev": d.alphas_cumprod_prev,
                "alphas_cumprod_next": d.alphas_cumprod_next, "log_one_minus_alphas_cumprod": d.log_one_minus_alphas_cumprod,
                "posterior_variance": d.posterior_variance,
                # the log-variance rows p_mean_variance reads per variance type (reference gaussian_diffusion.py:286-311)
                "logvar/LEARNED_RANGE/min": d.posterior_log_variance_clipped, "logvar/LEARNED_RANGE/max": np.log(d.betas),
                "logvar/FIXED_SMALL": d.posterior_log_variance_clipped,
                "logvar/FIXED_LARGE": np.log(np.append(d.posterior_variance[1], d.betas[1:]))}
        out[f"{tag}/row_names"] = np.array(list(rows))
        out[f"{tag}/rows"] = np.stack([np.asarray(v, dtype=np.float64) for v in rows.values()]).astype(np.float32)   # as uploaded
        for mean in MEANS:
            for var in VARS:
                mo = mo2 if var == "LEARNED_RANGE" else mo2[:, :C].contiguous()
                for loss in LOSSES:
                    d = ref_diffusion(sched, mean, var, loss)
                    key = f"{tag}/{mean}/{var}/{loss}"
                    leaf = mo.clone().requires_grad_(True)
                    r = d.training_losses(lambda xx, tt, **kw: leaf, x0, t, noise=noise)
                    keys = sorted(r)
                    w = {k: torch.randn(N, generator=g) for k in keys}
                    sum((r[k] * w[k]).sum() for k in keys).backward()
                    out[key + "/keys"] = np.array(keys)
                    out[key + "/vals"] = torch.stack([r[k].detach() for k in keys]).numpy()      # [key, N] in `keys` order
                    out[key + "/w"] = torch.stack([w[k] for k in keys]).numpy()
                    out[key + "/grad"] = leaf.grad.numpy()
                # reverse-process step (the loss type does not enter)
                d = ref_diffusion(sched, mean, var, "MSE")
                smo = smo2 if var == "LEARNED_RANGE" else smo2[:, :C].contiguous()
                stub = lambda xx, tt, **kw: smo
                for tcase, tv in (("mix", st), ("zero", torch.zeros(SN, dtype=torch.long))):
                    for clip in (0, 1):
                        key = f"{tag}/{mean}/{var}/{tcase}/clip{clip}"
                        pm = d.p_mean_variance(stub, xs, tv, clip_denoised=bool(clip))
                        res = [pm[k] for k in ("mean", "variance", "log_variance", "pred_xstart")]
                        torch.manual_seed(101)                 # p_sample's draw: the same for every key (step/ps_noise)
                        r = d.p_sample(stub, xs, tv, clip_denoised=bool(clip))
                        res.append(r["sample"])
                        assert torch.equal(r["pred_xstart"], pm["pred_xstart"])
                        torch.manual_seed(102)                 # step/ddim_noise
                        res.append(d.ddim_sample(stub, xs, tv, clip_denoised=bool(clip), eta=0.5)["sample"])
                        res.append(d.ddim_reverse_sample(stub, xs, tv, clip_denoised=bool(clip))["sample"])
                        out[key] = torch.stack(res).numpy()    # STEP_OUTPUTS order
    np.savez_compressed(os.path.join(HERE, "objectives.npz"), **out)
    print("== objectives.npz written")


def bpd_model(var):
    def f(x, t, **kw):
        m = 0.3 * x + 0.001 * t.float().view(-1, 1, 1, 1)
        return torch.cat([m, torch.tanh(x)], 1) if var == "LEARNED_RANGE" else m
    return f


def record_bpd(d, model, x0, seed, model_kwargs=None):
    """calc_bpd_loop with the per-timestep noise recorded (one randn_like per step, T-1 down to 0; the model draws nothing)."""
    torch.manual_seed(seed)
    noise = torch.stack([torch.randn_like(x0) for _ in range(d.num_timesteps)])
    torch.manual_seed(seed)
    with torch.no_grad():
        r = d.calc_bpd_loop(model, x0, model_kwargs=model_kwargs)
    return noise, r


def bpd_synthetic():
    N, C, S = 3, 4, 8
    g = torch.Generator().manual_seed(41)
    x0 = (torch.rand(N, C, S, S, generator=g) * 2 - 1)
    x0[0, 0, 0, :4] = torch.tensor([-1.0, 1.0, 0.9995, -0.9995])
    out = {"x0": x0.numpy()}
    for mean in MEANS:
        for var in VARS:
            d = ref_diffusion("10", mean, var, "MSE")
            noise, r = record_bpd(d, bpd_model(var), x0, 43)
            key = f"{mean}/{var}"
            out[key + "/noise"] = noise.numpy()
            for k, v in r.items():
                out[f"{key}/{k}"] = v.numpy()
    np.savez_compressed(os.path.join(HERE, "bpd_synthetic.npz"), **out)
    print("== bpd_synthetic.npz written")


def bpd_tiny_a():
    cfg = O.DiTConfig(depth=2, hidden_size=128, patch_size=2, input_size=16, in_channels=4, num_heads=2, num_classes=10)
    wseed, n = 1, 4
    sd = O.init_state_dict(cfg, seed=wseed, gains=None, perturb_reference=0.0)
    out = {"cfg_" + k: np.array(v) for k, v in cfg.to_dict().items()}
    out.update(n=np.array(n), wseed=np.array(wseed), gains=np.array(-1.0), perturb=np.array(0.0))
    g = torch.Generator().manual_seed(51)
    x0 = (torch.rand(n, 4, 16, 16, generator=g) * 2 - 1)
    y = torch.randint(0, 10, (n,), generator=g)
    nb = 2                                                     # calc_bpd_loop on the first two samples
    t = torch.randint(0, 1000, (n,), generator=g)
    t[0] = 0
    noise = torch.randn(n, 4, 16, 16, generator=g)
    out.update(x0=x0.numpy(), y=y.numpy(), t=t.numpy(), train_noise=noise.numpy())

    def build():
        m = RefDiT(**cfg.to_dict())
        m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
        return m

    m = build().eval()
    bnoise, r = record_bpd(ref_create("10"), m.forward, x0[:nb].contiguous(), 53, model_kwargs=dict(y=y[:nb]))
    out["bpd/noise"] = bnoise.numpy()
    for k, v in r.items():
        out["bpd/" + k] = v.numpy()
    print("   tiny_a total_bpd", r["total_bpd"].numpy())

    for tag, kw in (("kl", dict(use_kl=True)), ("xs_rmse", dict(predict_xstart=True, rescale_learned_sigmas=True))):
        # x0 prediction from a random DiT at t = 0 puts the decoder NLL where the CDF difference cancels in fp32 (its gradient is
        # rounding noise there, in the reference too): that step starts at t = 1; the t = 0 terms are pinned by objectives.npz
        tt = t.clone()
        if tag == "xs_rmse":
            tt[0] = 1
        out[f"{tag}/t"] = tt.numpy()
        m = build().train()
        d = ref_create("", **kw)
        torch.manual_seed(7)
        drop = torch.rand(n) < cfg.class_dropout_prob           # the label embedder's draw is the first
        torch.manual_seed(7)
        seen = {}

        def model_fn(xx, tt, **kw2):
            o = m(xx, tt, **kw2)
            o.retain_grad()
            seen["out"] = o
            return o
        losses = d.training_losses(model_fn, x0, tt, dict(y=y), noise=noise)
        losses["loss"].mean().backward()
        out[f"{tag}/model_out_grad"] = seen["out"].grad.numpy()
        out[f"{tag}/y_eff"] = torch.where(drop, torch.full_like(y, cfg.num_classes), y).numpy()
        out[f"{tag}/keys"] = np.array(sorted(losses))
        for k, v in losses.items():
            out[f"{tag}/{k}"] = v.detach().numpy()
        for k, p in m.named_parameters():
            out[f"{tag}/grad/{k}"] = sub(p.grad)
            out[f"{tag}/gradnorm/{k}"] = np.array(p.grad.double().norm().item())
        print(f"   tiny_a {tag}: {sorted(losses)} loss {losses['loss'].detach().numpy()}")
    np.savez_compressed(os.path.join(HERE, "bpd_tiny_a.npz"), **out)
    print("== bpd_tiny_a.npz written")


if __name__ == "__main__":
    synthetic_objectives()
    bpd_synthetic()
    bpd_tiny_a()
