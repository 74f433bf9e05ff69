#!/usr/bin/env python3
"""Golden vectors for the sampler hooks, denoised_fn and cond_fn (runs ONLY in the build container, where the reference checkout
exists; see make_golden.py).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_guidance.py

Writes guidance.npz, inputs and expected outputs only (nothing of the reference is copied).  The hooks are fixed and
torch-expressible, and the tests re-create them:

    denoised_fn = lambda x0: 0.8 * tanh(1.5 * x0)
    cond_fn     = lambda x, t, **kw: 3 * (target - x) * (1 + t / 1000)        (the t factor shows an unmapped timestep)

Kernel tier: recorded model outputs fed as stubs, on two shapes - "a" [4, 2, 4, 4] (128 elements, under one 256-thread block) and
"b" [3, 2, 12, 12] (288 per sample, 864 in all: a partial last block, and sample boundaries inside a block).  Shape b's expected
outputs are stored at every B_STRIDE-th element of the flattened tensor (both sides of each sample boundary and the partial
block are among them).  For the schedules "" and "250", every (mean, variance) pair, mixed t with t = 0 and all-zero t, clip on
and off: GUIDED_OUTPUTS below.  The draws of p_sample / ddim_sample are recorded (ps_noise, ddim_noise).

Model tier: the tiny_b DiT (weights from oracle.dit_oracle.init_state_dict), create_diffusion("250"), the first three yields of
ddim_sample_loop_progressive(forward_with_cfg, clip_denoised=True, eta=0, both hooks, model_kwargs={y, cfg_scale: 1.5}) from a
recorded start: deterministic, so no draws to inject; clip on keeps the untrained net bounded.
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
SCHEDS = {"full": "", "s250": "250"}
SHAPES = {"a": (4, 2, 4, 4), "b": (3, 2, 12, 12)}
B_STRIDE = 11
COND_SCALE = 3.0
# pmv_*: p_mean_variance(denoised_fn); ps_*: p_sample with denoised_fn alone, cond_fn alone, both; ddim_* (eta 0.5) and ddimrev_*:
# both hooks (the two share their pred_xstart); cm_mean / cs_*: condition_mean / condition_score on the unhooked p_mean_variance
GUIDED_OUTPUTS = ["pmv_mean", "pmv_pred_xstart", "ps_den_sample", "ps_cond_sample", "ps_both_sample", "ddim_sample",
                  "ddim_pred_xstart", "ddimrev_sample", "cm_mean", "cs_mean", "cs_pred_xstart"]


def denoised_fn(x0):
    return 0.8 * torch.tanh(1.5 * x0)


def make_cond_fn(target):
    def cond_fn(x, t, **kw):
        return COND_SCALE * (target - x) * (1 + t.float().view(-1, *([1] * (x.dim() - 1))) / 1000)
    return cond_fn


def ref_diffusion(sched, mean, var):
    return RefSpaced(use_timesteps=ref_space(1000, sched or [1000]), betas=rgd.get_named_beta_schedule("linear", 1000),
                     model_mean_type=rgd.ModelMeanType[mean], model_var_type=rgd.ModelVarType[var], loss_type=rgd.LossType.MSE)


def keep(name, a):
    f = a.detach().reshape(-1)
    return (f if name == "a" else f[::B_STRIDE]).numpy().copy()


def kernel_tier(out):
    g = torch.Generator().manual_seed(61)
    out["outputs"] = np.array(GUIDED_OUTPUTS)
    out["b_stride"] = np.array(B_STRIDE)
    out["cond_scale"] = np.array(COND_SCALE)
    for name, shape in SHAPES.items():
        N, C = shape[:2]
        x = torch.randn(*shape, generator=g)
        mo2 = torch.randn(N, 2 * C, *shape[2:], generator=g) * 0.7
        target = torch.rand(*shape, generator=g) * 2 - 1
        torch.manual_seed(101)
        ps_noise = torch.randn_like(x)
        torch.manual_seed(102)
        ddim_noise = torch.randn_like(x)
        out.update({f"{name}/x": x.numpy(), f"{name}/mo": mo2.numpy(), f"{name}/target": target.numpy(),
                    f"{name}/ps_noise": ps_noise.numpy(), f"{name}/ddim_noise": ddim_noise.numpy()})
        cond_fn = make_cond_fn(target)
        for tag, sched in SCHEDS.items():
            T = 1000 if sched == "" else 250
            tmix = torch.tensor([0, 5, T // 2 + 3, T - 1] if N == 4 else [0, T // 2 + 3, T - 1])
            out[f"{name}/{tag}/t"] = tmix.numpy()
            for mean in MEANS:
                for var in VARS:
                    d = ref_diffusion(sched, mean, var)
                    mo = mo2 if var == "LEARNED_RANGE" else mo2[:, :C].contiguous()
                    stub = lambda xx, tt, **kw: mo
                    for tcase, tv in (("mix", tmix), ("zero", torch.zeros(N, dtype=torch.long))):
                        for clip in (0, 1):
                            kw = dict(clip_denoised=bool(clip), model_kwargs={})
                            r = {}
                            pm = d.p_mean_variance(stub, x, tv, denoised_fn=denoised_fn, **kw)
                            r["pmv_mean"], r["pmv_pred_xstart"] = pm["mean"], pm["pred_xstart"]
                            for k, hooks in (("den", dict(denoised_fn=denoised_fn)), ("cond", dict(cond_fn=cond_fn)),
                                             ("both", dict(denoised_fn=denoised_fn, cond_fn=cond_fn))):
                                torch.manual_seed(101)             # p_sample's draw: ps_noise
                                r[f"ps_{k}_sample"] = d.p_sample(stub, x, tv, **hooks, **kw)["sample"]
                            torch.manual_seed(102)                 # ddim_noise
                            o = d.ddim_sample(stub, x, tv, denoised_fn=denoised_fn, cond_fn=cond_fn, eta=0.5, **kw)
                            r["ddim_sample"], r["ddim_pred_xstart"] = o["sample"], o["pred_xstart"]
                            o2 = d.ddim_reverse_sample(stub, x, tv, denoised_fn=denoised_fn, cond_fn=cond_fn, **kw)
                            assert torch.equal(o2["pred_xstart"], o["pred_xstart"])
                            r["ddimrev_sample"] = o2["sample"]
                            plain = d.p_mean_variance(stub, x, tv, **kw)
                            r["cm_mean"] = d.condition_mean(cond_fn, plain, x, tv, model_kwargs={})
                            cs = d.condition_score(cond_fn, plain, x, tv, model_kwargs={})
                            r["cs_mean"], r["cs_pred_xstart"] = cs["mean"], cs["pred_xstart"]
                            out[f"{name}/{tag}/{mean}/{var}/{tcase}/clip{clip}"] = np.stack([keep(name, r[k]) for k in GUIDED_OUTPUTS])


def model_tier(out):
    cfg = O.DiTConfig(depth=2, hidden_size=128, patch_size=2, input_size=16, in_channels=4, num_heads=2, num_classes=10)
    wseed, gains, perturb, n = 3, 0.3, 0.5, 4
    sd = O.init_state_dict(cfg, seed=wseed, gains=gains, perturb_reference=perturb)
    out.update({"cfg_" + k: np.array(v) for k, v in cfg.to_dict().items()})
    out.update(n=np.array(n), wseed=np.array(wseed), gains=np.array(gains), perturb=np.array(perturb))
    g = torch.Generator().manual_seed(71)
    half = torch.randn(n // 2, 4, 16, 16, generator=g)
    z = torch.cat([half, half], 0)
    y = torch.randint(0, cfg.num_classes, (n // 2,), generator=g)
    yy = torch.cat([y, torch.full((n // 2,), cfg.num_classes)], 0)
    target = torch.rand(n, 4, 16, 16, generator=g) * 2 - 1
    m = RefDiT(**cfg.to_dict())
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    m.eval()
    d = ref_create("250")
    traj, xs = [], []
    for k, o in enumerate(d.ddim_sample_loop_progressive(m.forward_with_cfg, z.shape, noise=z, clip_denoised=True, eta=0.0,
                                                         denoised_fn=denoised_fn, cond_fn=make_cond_fn(target),
                                                         model_kwargs=dict(y=yy, cfg_scale=1.5), device="cpu")):
        traj.append(o["sample"])
        xs.append(o["pred_xstart"])
        if k + 1 == 3:
            break
    out.update({"model/z": z.numpy(), "model/y": yy.numpy(), "model/target": target.numpy(),
                "model/traj": torch.stack(traj).numpy(), "model/pred_xstart": torch.stack(xs).numpy()})
    print("   model tier |sample| per step", [float(t.abs().mean()) for t in traj])


if __name__ == "__main__":
    out = {}
    kernel_tier(out)
    model_tier(out)
    path = os.path.join(HERE, "guidance.npz")
    np.savez_compressed(path, **out)
    print(f"== guidance.npz written ({os.path.getsize(path) / 1e3:.0f} kB)")
