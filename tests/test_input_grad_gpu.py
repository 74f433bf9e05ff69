"""Input-latent gradients on the engine (model.input_gradients = True): the kernel through the C ABI, dL/dx of the model against the
reference's own autograd (tests/golden/input_grad.npz), the input-only backward, forward_with_cfg under autograd, the mp_pos_enc off
form, a cond_fn that differentiates through the DiT inside p_sample, and accumulation.

Limits.  dx = c5 dx0 W_eff, where x_embedder.weight.grad = Jacobian(dx0^T patches): dx carries the same dx0 error as the parameter
gradients and is held to the project's per-tensor gradient limits (bf16 GRAD_TOL 1e-2, tests/test_model_gpu.py; f16 3e-3,
tests/test_f16_gpu.py; bf16x3 2e-4, test_precise_training_gradients_match_reference).  Measured on the MI355X (dx, worst of the four fixtures):
bf16 6.0e-3, f16 7.3e-4, bf16x3 1.1e-5; forward_with_cfg 5.8e-3 (dx) / 6.3e-3 (x_embedder.weight.grad); off form 5.7e-3; the cond_fn's
energy gradient 5.5e-3; the kernel alone on exact operands 2.5e-8.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import golden_cfg, golden_state_dict, load_golden, rel_err, sub
from oracle import dit_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRAD_TOL = {"bf16": 1e-2, "f16": 3e-3, "bf16x3": 2e-4}
PRECISIONS = ["bf16", "f16", "bf16x3"]
IG = load_golden("input_grad")
FIXTURES = [str(n) for n in IG["fixtures"]]
CFG_FIXTURE, CFG_SCALE = str(IG["cfg_fixture"]), float(IG["cfg_scale"])


# ---- 1. the kernel through the C ABI -----------------------------------------------------------------------------------------------
def unpatchify(dpatch, N, C_, S, p):
    """[M, P] -> [N, C, S, S] with the forward's index rule j = (p1 p + p2) C + c (csrc/embed.hip)."""
    g = S // p
    return dpatch.reshape(N, g, g, p, p, C_).transpose(0, 5, 1, 3, 2, 4).reshape(N, C_, S, S)


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape,pad", [((4, 4, 16, 2, 128), 0), ((5, 3, 16, 2, 128), 0), ((3, 4, 32, 8, 128), 0), ((2, 4, 32, 4, 1152), 0),
                                       ((1, 4, 16, 2, 384), 8)], ids=["base", "P12_M320", "P256_M48", "P64_D1152", "N1_ldx"])
def test_kernel_against_fp64(shape, pad, f16):
    """Operands that are exact in bf16 and fp16 (integers / 64, |k| <= 128): only the fp32 accumulation differs from the fp64 product."""
    from mapdit_amd import _lib as L
    N, C_, S, p, D = shape
    M, P = N * (S // p) ** 2, p * p * C_
    rng = np.random.default_rng(list(shape))
    dx0 = rng.integers(-128, 129, size=(M, D)).astype(np.float64) / 64
    w = rng.integers(-128, 129, size=(D, P + 1)).astype(np.float64) / 64          # (the ones column, j = P, takes no gradient: random here)
    scale = 0.3713
    want = unpatchify(dx0 @ w[:, :P] * np.float64(np.float32(scale)), N, C_, S, p)
    dt = torch.float16 if f16 else torch.bfloat16
    ldx = D + pad
    a = torch.full((M, ldx), float("nan"), dtype=dt, device=DEV)
    a[:, :D] = torch.from_numpy(dx0).to(dt)
    assert torch.equal(a[:, :D].double().cpu(), torch.from_numpy(dx0))          # exact in the operand type
    wt = torch.from_numpy(w).float().to(DEV)
    out = torch.full((N, C_, S, S), float("nan"), device=DEV)
    fn = L.lib().patch_embed_bwd_x_f16 if f16 else L.lib().patch_embed_bwd_x
    fn(a.data_ptr(), ldx, wt.data_ptr(), out.data_ptr(), N, C_, S, p, D, scale, L.cur_stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isfinite(got).all()                                                # every element written, none from the padding
    e = rel_err(got, want)
    print(f"{shape} {'f16' if f16 else 'bf16'}: rel err {e:.3e}")
    assert e < 1e-5
    # what it does not handle is refused
    with pytest.raises(L.MapditError, match="multiple of 32"):
        fn(a.data_ptr(), ldx, wt.data_ptr(), out.data_ptr(), N, C_, S, p, D - 8, scale, L.cur_stream())
    with pytest.raises(L.MapditError, match="aligned"):
        fn(a.data_ptr() + 2, ldx, wt.data_ptr(), out.data_ptr(), N, C_, S, p, D, scale, L.cur_stream())


# ---- shared model plumbing ---------------------------------------------------------------------------------------------------------
def build(name, precision, train=False):
    from mapdit_amd.src.dit import DiT
    g = load_golden(name)
    cfg = golden_cfg(g)
    sd = golden_state_dict(g, cfg)
    m = DiT(**cfg.to_dict())
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).train(train)
    m.gemm_precision = precision
    m.input_gradients = True
    return m, g, cfg, sd


def inputs(g, name):
    xk, tk, yk = ("ps_z", "ps_t", "ps_y") if name == CFG_FIXTURE else ("x", "t", "y_eff")
    x, t, y = (torch.from_numpy(g[k]).to(DEV) for k in (xk, tk, yk))
    return x, t, y, torch.from_numpy(IG[f"{name}/w"]).to(DEV)


def golden_dx_err(name, dx):
    return rel_err(dx.reshape(-1)[::int(IG["stride"])].cpu().numpy(), IG[f"{name}/dx"])


@functools.lru_cache(maxsize=None)
def full_backward(name, precision):
    """Eval-mode forward on x.requires_grad_() with every parameter requiring grad, one backward of sum(out * w): (dx, parameter
    gradients) - computed once per (fixture, precision) and shared by the tests below (read-only)."""
    m, g, cfg, sd = build(name, precision)
    x, t, y, w = inputs(g, name)
    x = x.clone().requires_grad_(True)
    (m(x, t, y) * w).sum().backward()
    torch.cuda.synchronize()
    return x.grad.clone(), {k: p.grad.clone() for k, p in m.named_parameters()}


# ---- 2. the model against the reference's autograd ---------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", FIXTURES)
def test_model_dx_matches_reference(name, precision):
    dx, pgrads = full_backward(name, precision)
    e = golden_dx_err(name, dx)
    print(f"{name} {precision}: dx rel err {e:.3e} (limit {GRAD_TOL[precision]:.0e})")
    assert e < GRAD_TOL[precision]
    # the parameter gradients of the same backward are those of a backward on a detached x, bit for bit
    m, g, cfg, sd = build(name, precision)
    x, t, y, w = inputs(g, name)
    (m(x, t, y) * w).sum().backward()
    torch.cuda.synchronize()
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, pgrads[k]), k


# ---- 3. input-only backward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", FIXTURES)
def test_input_only_backward(name, precision):
    from mapdit_amd.diffusion import create_diffusion
    dx_full, _ = full_backward(name, precision)
    m, g, cfg, sd = build(name, precision)
    m.requires_grad_(False)
    x, t, y, w = inputs(g, name)
    x = x.clone().requires_grad_(True)
    (m(x, t, y) * w).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(x.grad, dx_full)                      # the same dX kernels in the same order
    assert all(p.grad is None for p in m.parameters())
    assert m._gflat is None or float(m._gflat.abs().max()) == 0.0      # the flat gradient buffer is not written
    # a later ordinary training backward is undisturbed: every gradient tensor against its golden
    m.requires_grad_(True).train()
    xt, tt, y_eff, noise = (torch.from_numpy(g[k]).to(DEV) for k in ("x", "t", "y_eff", "noise"))
    m.y_embedder.token_drop = lambda labels, force_drop_ids=None: labels      # golden labels already carry the drop
    create_diffusion(timestep_respacing="").training_losses(m, xt, tt, dict(y=y_eff), noise=noise)["loss"].mean().backward()
    torch.cuda.synchronize()
    stride = 7 if "postw/x_embedder.weight" in g else 4099
    worst = 0.0
    for k, p in m.named_parameters():
        gref = g["grad/" + k]
        if p.dim() == 0 or gref.size < 64 or np.linalg.norm(gref) < 1e-7:
            continue
        e = rel_err(sub(p.grad, stride=stride), gref)
        worst = max(worst, e)
        assert e < GRAD_TOL[precision], (k, e)
    print(f"{name} {precision}: training gradients after an input-only backward, worst rel err {worst:.3e}")


# ---- 4. forward_with_cfg under autograd ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_cfg_grads():
    g = load_golden(CFG_FIXTURE)
    cfg = golden_cfg(g)
    sd = {k: v.clone() for k, v in golden_state_dict(g, cfg).items()}
    sd["x_embedder.weight"].requires_grad_(True)
    x, t, y = (torch.from_numpy(g[k]) for k in ("ps_z", "ps_t", "ps_y"))
    x = x.clone().requires_grad_(True)
    (O.dit_forward_with_cfg(sd, cfg, x, t, y, CFG_SCALE) * torch.from_numpy(IG[f"{CFG_FIXTURE}/w"])).sum().backward()
    return x.grad.numpy(), sd["x_embedder.weight"].grad.numpy()


def test_forward_with_cfg_is_differentiable():
    m, g, cfg, sd = build(CFG_FIXTURE, "bf16")
    x, t, y, w = inputs(g, CFG_FIXTURE)
    x = x.clone().requires_grad_(True)
    out = m.forward_with_cfg(x, t, y, CFG_SCALE)
    assert out.grad_fn is not None
    (out * w).sum().backward()
    torch.cuda.synchronize()
    e = golden_dx_err(CFG_FIXTURE, x.grad)
    assert float(x.grad[x.shape[0] // 2:].abs().max()) == 0.0         # the second half of the CFG batch never reaches the network
    wg = m.x_embedder.weight.grad
    assert wg is not None and float(wg.abs().max()) > 0
    dx_o, wg_o = oracle_cfg_grads()
    ew = rel_err(wg.cpu().numpy(), wg_o)
    print(f"forward_with_cfg: dx rel err {e:.3e}, x_embedder.weight.grad vs oracle {ew:.3e} (limit {GRAD_TOL['bf16']:.0e})")
    assert e < GRAD_TOL["bf16"]
    assert ew < GRAD_TOL["bf16"]
    with torch.no_grad():                                   # under no_grad: the plain launch, the same values
        plain = m.forward_with_cfg(x, t, y, CFG_SCALE)
    assert plain.grad_fn is None and torch.equal(plain, out.detach())


# ---- 5. the mp_pos_enc off form (c5 = 1) ---------------------------------------------------------------------------------------------
def test_plain_positional_sum_off_form():
    from mapdit_amd.src.dit import DiT
    tiny = dict(depth=2, hidden_size=128, patch_size=2, input_size=16, in_channels=4, num_heads=2, num_classes=10)
    cfg = O.DiTConfig(**tiny, mp_pos_enc=False)
    sd = O.init_state_dict(cfg, seed=5, gains=0.3, perturb_reference=0.2)
    gen = torch.Generator().manual_seed(17)
    x, t, y = torch.randn(3, 4, 16, 16, generator=gen), torch.randint(0, 1000, (3,), generator=gen), torch.randint(0, 10, (3,), generator=gen)
    w = torch.randn(3, 8, 16, 16, generator=gen)
    xo = x.clone().requires_grad_(True)
    (O.dit_forward({k: v.clone() for k, v in sd.items()}, cfg, xo, t, y, train=False) * w).sum().backward()
    m = DiT(**cfg.to_dict())
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    m.gemm_precision, m.input_gradients = "bf16", True
    xg = x.to(DEV).requires_grad_(True)
    (m(xg, t.to(DEV), y.to(DEV)) * w.to(DEV)).sum().backward()
    e = rel_err(xg.grad.cpu().numpy(), xo.grad.numpy())
    print(f"mp_pos_enc=False: dx vs oracle rel err {e:.3e} (limit {GRAD_TOL['bf16']:.0e})")
    assert e < GRAD_TOL["bf16"]


# ---- 6. guidance end to end: a cond_fn that differentiates through the DiT -------------------------------------------------------------
def test_cond_fn_through_the_model_in_p_sample():
    from mapdit_amd.diffusion import create_diffusion
    m, g, cfg, sd = build(CFG_FIXTURE, "bf16")
    m.requires_grad_(False)
    x, t, y = (torch.from_numpy(g[k]).to(DEV) for k in ("x", "ps_t", "y"))
    seen = {}

    def energy_grad(fwd, xx, tt, yy):
        with torch.enable_grad():
            xg = xx.detach().requires_grad_(True)
            eps = fwd(xg, tt, yy)[:, :cfg.in_channels]
            return torch.autograd.grad(-0.5 * (eps ** 2).sum(), xg)[0]

    def cond_fn(xx, tt, y=None):
        seen["t"], seen["grad"] = tt.clone(), energy_grad(m, xx, tt, y)
        return seen["grad"]

    d = create_diffusion("250")
    with torch.no_grad():
        torch.manual_seed(23)
        r = d.p_sample(m, x, t, clip_denoised=False, cond_fn=cond_fn, model_kwargs=dict(y=y))
        # the same step with the gradient handed in: the sampler's own forward (inference runtime) is not disturbed by the saved one
        torch.manual_seed(23)
        r2 = d.p_sample(m, x, t, clip_denoised=False, cond_fn=lambda xx, tt, y=None: seen["grad"], model_kwargs=dict(y=y))
        plain = m(x, seen["t"], y)
    assert torch.isfinite(r["sample"]).all()
    assert torch.equal(r["sample"], r2["sample"])
    sd_o = {k: v.clone() for k, v in sd.items()}
    want = energy_grad(lambda a, b, c: O.dit_forward(sd_o, cfg, a, b, c, train=False), x.cpu(), seen["t"].cpu(), y.cpu())
    e = rel_err(seen["grad"].cpu().numpy(), want.numpy())
    print(f"cond_fn through the DiT: gradient vs oracle rel err {e:.3e} (limit {GRAD_TOL['bf16']:.0e})")
    assert e < GRAD_TOL["bf16"]
    assert all(p.grad is None for p in m.parameters())
    with torch.no_grad():
        assert torch.equal(m(x, seen["t"], y), plain)


# ---- 7. accumulation ---------------------------------------------------------------------------------------------------------------
def test_two_backward_passes_accumulate_into_x_grad():
    m, g, cfg, sd = build("tiny_a", "bf16")
    x, t, y, w = inputs(g, "tiny_a")
    x = x.clone().requires_grad_(True)
    (m(x, t, y) * w).sum().backward()
    once = x.grad.clone()
    (m(x, t, y) * w).sum().backward()
    assert rel_err(x.grad.cpu().numpy(), 2 * once.cpu().numpy()) < 1e-6
    # a stale forward is still refused
    from mapdit_amd import _lib as L
    a = m(x, t, y)
    m(x, t, y)
    with pytest.raises(L.MapditError, match="stale forward"):
        a.sum().backward()
