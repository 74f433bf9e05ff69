"""head_dim-72 models (DiT-XL's width) on 1,024 tokens per sample (64x64 latents at patch 2) behind the reference API.

Parity rests on the fixture xl1024_d2 (depth 2, hidden 1152, 16 heads of 72; tests/golden/make_golden_xl1024.py): eval logits, training
losses and every parameter gradient against the reference's own outputs, bf16 and fp16 engines.  The named model DiT-XL/2 (depth 28) runs
at that resolution too: finite, repeatable bit for bit, and its captured CFG denoise step replays the eager step's bits.

Limits: fp16 logits 1e-3 is BASELINE.json's north star and fixed; the others start from test_more_than_256_tokens_matches_reference's
(bf16 logits 7e-3, gradients 1.5e-2; fp16 gradients 3e-3; losses at the logit limit) and are at most twice what the engine measures on
the MI355X (DESIGN.md section 2's rule), the measured value beside each.
"""
import pytest
import torch

from conftest import golden_cfg, golden_state_dict, load_golden, rel_err, sub

pytestmark = pytest.mark.gpu
DEV = "cuda"


def build(g, precision):
    from mapdit_amd.src.dit import DiT
    cfg = golden_cfg(g)
    m = DiT(**cfg.to_dict())
    m.load_state_dict(golden_state_dict(g, cfg), strict=True)
    m = m.to(DEV).eval()
    m.gemm_precision = precision
    return m, cfg


def dev(g, *names):
    return [torch.from_numpy(g[n]).to(DEV) for n in names]


def train_step(m, x, t, y_eff, noise):
    from mapdit_amd.diffusion import create_diffusion
    m.zero_grad(set_to_none=True)
    losses = create_diffusion("").training_losses(m, x, t, dict(y=y_eff), noise=noise)
    losses["loss"].mean().backward()
    return losses


# precision, logit limit, loss limit, gradient limit (per tensor of >= 64 entries, and every tensor's norm).  Measured on the MI355X:
#   bf16: logits 2.70e-3, loss 5.33e-5, worst gradient 4.87e-3 (norm deviation 4.3e-4)
#   f16:  logits 3.66e-4 (limit: the north star's 1e-3), loss 9.07e-6, worst gradient 6.69e-4 (norm deviation 7.1e-5)
LIMITS = [("bf16", 5.4e-3, 1.07e-4, 9.7e-3), ("f16", 1e-3, 1.8e-5, 1.34e-3)]


@pytest.mark.parametrize("precision,ltol,losstol,gtol", LIMITS)
def test_xl_width_on_1024_tokens_matches_reference(precision, ltol, losstol, gtol):
    g = load_golden("xl1024_d2")
    m, cfg = build(g, precision)
    assert (cfg.input_size // cfg.patch_size) ** 2 == 1024 and cfg.hidden_size // cfg.num_heads == 72
    x, t, y, y_eff, noise = dev(g, "x", "t", "y", "y_eff", "noise")
    with torch.no_grad():
        out = m(x, t, y)                                       # inference path: raw q, k, normalised per key tile
    e = rel_err(out.cpu().numpy(), g["eval_out"])
    print(f"xl1024_d2 [{precision}]: eval logits rel err {e:.3e}")
    assert e < ltol
    m.train()
    m.y_embedder.token_drop = lambda labels, force_drop_ids=None: labels
    losses = train_step(m, x, t, y_eff, noise)
    el = rel_err(losses["loss"].detach().cpu().numpy(), g["train_loss"])
    worst, worst_norm = 0.0, 0.0
    for k, p in m.named_parameters():
        gref = g["grad/" + k]
        if p.dim() == 0 or float(g["gradnorm/" + k]) < 1e-7:
            continue
        e = rel_err(sub(p.grad, stride=4099), gref)
        en = abs(float(p.grad.double().norm()) / float(g["gradnorm/" + k]) - 1)
        worst_norm = max(worst_norm, en)
        if gref.size >= 64:
            worst = max(worst, e)
            assert e < gtol, (k, e)
        assert en < gtol, (k, en)
    print(f"xl1024_d2 [{precision}]: loss rel err {el:.3e}, worst gradient rel err {worst:.3e}, worst gradient norm deviation {worst_norm:.3e}")
    assert el < losstol
    # the same step again from the same weights (the training forward rewrites the weights by their forced normalisation, so the
    # model is rebuilt): the same bits - no atomics, no kernel reads what another workgroup of its launch writes
    first = {k: p.grad.clone() for k, p in m.named_parameters()}
    loss1 = losses["loss"].detach().clone()
    m, _ = build(g, precision)
    m.train()
    m.y_embedder.token_drop = lambda labels, force_drop_ids=None: labels
    losses = train_step(m, x, t, y_eff, noise)
    assert torch.equal(losses["loss"].detach(), loss1)
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, first[k]), k


def test_dit_xl2_at_64x64_latents_runs_trains_and_replays():
    from mapdit_amd import sampling as S
    from mapdit_amd.diffusion import create_diffusion
    from mapdit_amd.src.models import DIT_MODELS
    torch.manual_seed(0)
    m = DIT_MODELS["DiT-XL/2"](input_size=64, in_channels=4, num_classes=1000).to(DEV).eval()
    with torch.no_grad():                                      # (fresh gains are zero: the blocks would pass x through)
        for k, p in m.named_parameters():
            if p.dim() == 0:
                p.fill_(0.3)
    n = 2
    gen = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(n, 4, 64, 64, device=DEV, generator=gen)
    noise = torch.randn(n, 4, 64, 64, device=DEV, generator=gen)
    y = torch.tensor([3, 977], device=DEV)
    t = torch.tensor([40, 900], device=DEV)
    with torch.no_grad():
        out = m(x, t, y)
        assert out.shape == (n, 8, 64, 64) and torch.isfinite(out).all()
        assert torch.equal(out, m(x, t, y))
    start = {k: v.clone() for k, v in m.state_dict().items()}
    m.train()
    m.y_embedder.token_drop = lambda labels, force_drop_ids=None: labels
    losses = train_step(m, x, t, y, noise)
    assert torch.isfinite(losses["loss"]).all()
    first = {}
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        first[k] = p.grad.clone()
    assert sum(float(v.abs().sum()) for v in first.values()) > 0
    loss1 = losses["loss"].detach().clone()
    m.load_state_dict(start)                                   # (the training forward rewrote the weights by their forced normalisation)
    losses = train_step(m, x, t, y, noise)
    assert torch.equal(losses["loss"].detach(), loss1)
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, first[k]), k
    del first, start
    # a captured CFG denoise step against the eager one (the final step, t = 0, adds no noise: comparable bit for bit)
    m.zero_grad(set_to_none=True)
    m.eval()
    d = create_diffusion("250")
    z = torch.randn(2 * n, 4, 64, 64, device=DEV, generator=gen)
    yy = torch.cat([y, torch.full((n,), 1000, device=DEV)])
    gs = S.GraphedSampler(m, d, z.shape, yy, cfg_scale=1.5)
    gs.img.copy_(z)
    gs.t.fill_(0)
    gs.graph.replay()
    torch.cuda.synchronize()
    replayed = gs.img.clone()
    with torch.no_grad():
        t0 = torch.zeros(2 * n, dtype=torch.int64, device=DEV)
        mo = d._wrap_model(m.forward_with_cfg)(z, t0, y=yy, cfg_scale=1.5)
        eager = d._step_math(mo, z, t0, torch.zeros_like(z), False)[0]
    assert torch.isfinite(replayed).all()
    assert torch.equal(replayed, eager)


def test_refusals_beyond_256_tokens_keep_their_words():
    from mapdit_amd import _lib as L
    from mapdit_amd.src.dit import DiT
    kw = dict(depth=1, hidden_size=1152, patch_size=2, in_channels=4, num_heads=16, num_classes=10)

    def run(m, size):
        z = torch.zeros(2, dtype=torch.long, device=DEV)
        with torch.no_grad():
            m(torch.zeros(2, 4, size, size, device=DEV), z, z)

    m = DiT(input_size=64, **kw).to(DEV).eval()
    m.gemm_precision = "bf16x3"
    with pytest.raises(L.MapditError, match="1024 tokens per sample unsupported.*head_dim 64 or 72 in bf16 / f16 precision"):
        run(m, 64)
    m = DiT(input_size=64, cosine_attention=False, **kw).to(DEV).eval()
    with pytest.raises(L.MapditError, match="cosine attention off.*<= 256 tokens"):
        run(m, 64)
    m = DiT(input_size=36, **kw).to(DEV).eval()                # 324 tokens: above 256, not a multiple of it
    with pytest.raises(L.MapditError, match="324 tokens per sample unsupported.*a multiple of 256 up to 16384"):
        run(m, 36)
