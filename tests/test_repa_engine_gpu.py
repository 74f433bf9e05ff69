"""The hidden tap of the engine (model.hidden_tap, mapdit_engine_set_hidden_grad): the tapped value, the gradients of a loss that reads
the logits AND a block's output against autograd through the oracle's public pieces, the bit-equalities the design promises (an unused
tap, staged against unstaged, recompute against none, accumulation) and every refusal.

Model: depth 4, hidden 128, 2 heads, patch 2, 16 x 16 latents (T = 64: the MFMA attention and the fused residual / modulate backward), N =
2 and 3, bf16 and f16.  Loss = sum A * out + sum B * h_k with fixed random A, B, k in {0, depth - 2}.  The oracle forward below is
oracle.dit_oracle.dit_forward restated from its own pieces (patchify, mp_linear, mp_sum, dit_block, final_layer, ...) under the
engine's rounding plan, returning h_k as well; oracle/ is not edited.  Limits per tensor: those of tests/test_model_gpu.py for bf16
(GRAD_TOL 1e-2, SMALL_GRAD_TOL 2e-2, GAIN_TOL 8e-3 of the largest gain gradient) and of tests/test_f16_gpu.py for f16 (3e-3, 1e-2,
5e-3)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
LIMITS = {"bf16": dict(big=1e-2, small=2e-2, gain=8e-3), "f16": dict(big=3e-3, small=1e-2, gain=5e-3)}
DEPTH = 4


def oracle():
    from oracle import dit_oracle as O
    return O


def config(**kw):
    return oracle().DiTConfig(depth=DEPTH, hidden_size=128, patch_size=2, input_size=16, in_channels=4, num_heads=2, num_classes=10, **kw)


def inputs(n, seed=3):
    g = torch.Generator().manual_seed(seed + n)
    x = torch.randn(n, 4, 16, 16, generator=g)
    t = torch.randint(0, 1000, (n,), generator=g)
    y = torch.randint(0, 10, (n,), generator=g)
    drop = torch.zeros(n, dtype=torch.bool)
    drop[n - 1] = True
    A = torch.randn(n, 8, 16, 16, generator=g)
    B = torch.randn(n, 64, 128, generator=g) * 0.5
    return x, t, y, drop, A, B


def oracle_forward_with_tap(sd, cfg, x, t, y, drop, rnd, tap):
    """dit_forward(train=True) from the oracle's pieces, also returning the residual stream after block ``tap``."""
    O = oracle()
    h = O.patchify(x, cfg.patch_size)
    h = torch.cat([h, torch.ones_like(h[:, :, :1])], dim=-1)
    h = O.mp_sum(O.mp_linear(h, sd, "x_embedder.weight", True), sd["pos_embed"], O.EMBED_T)
    four = math.sqrt(2) * torch.cos(torch.outer(t.to(h.dtype), sd["t_embedder.embedding.scale"]) + sd["t_embedder.embedding.shift"])
    temb = O.mp_linear(four, sd, "t_embedder.mlp.net.0.weight", True, rnd)
    temb = O.mp_linear(O.act_fn(cfg)(temb), sd, "t_embedder.mlp.net.2.weight", True, rnd)
    yemb = O.mp_embedding(O.effective_labels(y, cfg, True, drop), sd, "y_embedder.embedding.weight", True, mp=cfg.mp_embedding)
    c = O.mp_sum(temb, yemb, O.EMBED_T)
    tapped = None
    for i in range(cfg.depth):
        h = O.dit_block(h, c, sd, i, cfg, True, rnd)
        assert isinstance(h, torch.Tensor)                  # (the shipped plans keep the residual stream fp32: no stored / full pair)
        if i == tap:
            tapped = h
    mean, sigma = O.final_layer(h, c, sd, cfg, True, rnd)
    out = torch.cat([O.unpatchify(mean, cfg.input_size, cfg.patch_size), O.unpatchify(sigma, cfg.input_size, cfg.patch_size)], dim=1)
    return out, tapped


def build(prec, sd, cfg, **attrs):
    from mapdit_amd.src.dit import DiT
    m = DiT(**cfg.to_dict())
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    m.gemm_precision = prec
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def run(m, n, tap, use_hidden=True, use_out=True, zero=True):
    """One forward + backward of sum A * out + sum B * h_tap; returns (flat gradient copy, out, tapped copy)."""
    x, t, y, drop, A, B = inputs(n)
    if zero:
        for p in m.parameters():
            p.grad = None
    m.hidden_tap = tap
    out = m(x.to(DEV), t.to(DEV), y.to(DEV), force_drop_ids=drop.to(DEV))
    h = m.tapped_hidden
    loss = 0
    if use_out:
        loss = loss + (A.to(DEV) * out).sum()
    if use_hidden and tap is not None:
        loss = loss + (B.to(DEV) * h).sum()
    loss.backward()
    torch.cuda.synchronize()
    return m._gflat.clone(), out.detach(), (h.detach().clone() if h is not None else None)


@pytest.fixture(scope="module")
def weights():
    cfg = config()
    return cfg, oracle().init_state_dict(cfg, seed=21, gains=0.3, perturb_reference=0.3)


@pytest.fixture(scope="module")
def oracle_grads(weights):
    """(prec, n, tap) -> (name -> gradient) of the oracle under that precision's rounding plan: computed once per case."""
    cache = {}

    def get(prec, n, tap):
        key = (prec, n, tap)
        if key not in cache:
            O = oracle()
            cfg, sd = weights
            x, t, y, drop, A, B = inputs(n)
            osd = {k: v.clone().requires_grad_(k not in O.BUFFER_KEYS) for k, v in sd.items()}
            out, h = oracle_forward_with_tap(osd, cfg, x, t, y, drop, O.engine_plan if prec == "bf16" else O.engine_plan_f16, tap)
            ((A * out).sum() + (B * h).sum()).backward()
            cache[key] = {k: v.grad.numpy() for k, v in osd.items() if v.requires_grad}, h.detach().numpy()
        return cache[key]
    return get


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("tap", [0, DEPTH - 2])
def test_tap_value_and_gradients_against_the_oracle(weights, oracle_grads, tap, n, prec):
    cfg, sd = weights
    m = build(prec, sd, cfg)
    _, _, h = run(m, n, tap)
    assert h.shape == (n, 64, 128) and h.dtype == torch.float32
    assert torch.equal(h.reshape(n * 64, 128), m._peek("xout", tap))            # the tap IS the saved checkpoint
    ref, href = oracle_grads(prec, n, tap)
    print(f"{prec} n={n} tap={tap}: tapped hidden rel err {rel_err(h.cpu().numpy(), href):.3e}")
    lim = LIMITS[prec]
    gain_scale = max(float(np.abs(ref[k]).max()) for k, p in m.named_parameters() if p.dim() == 0)
    worst, worst_k, worst_gain = 0.0, "", 0.0
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        if p.dim() == 0:
            dev_ = abs(float(p.grad) - float(ref[k])) / (gain_scale + 1e-30)
            worst_gain = max(worst_gain, dev_)
            assert dev_ < lim["gain"], (k, float(p.grad), float(ref[k]))
            continue
        e = rel_err(p.grad.cpu().numpy(), ref[k])
        if e > worst:
            worst, worst_k = e, k
        assert e < (lim["big"] if ref[k].size >= 64 else lim["small"]) or np.linalg.norm(ref[k]) < 1e-7, (k, e)
    print(f"{prec} n={n} tap={tap}: worst gradient rel err {worst:.3e} ({worst_k}); worst gain deviation {worst_gain:.3e}")


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_injection_moves_the_gradients_it_should(weights, prec):
    """Against a wrong injection point the oracle comparison above is the judge; this is the coarse check that the request is consumed at
    all and reaches exactly the blocks at or before the tap: blocks behind it see the logits' gradient alone."""
    cfg, sd = weights
    m = build(prec, sd, cfg, forced_weight_normalization=False)
    with_h, _, _ = run(m, 2, 1)
    without, _, _ = run(m, 2, 1, use_hidden=False)
    views = dict(zip((k for k, _ in m.named_parameters()), m._gviews))
    flat = {"a": with_h, "b": without}
    off = {k: (v.data_ptr() - m._gflat.data_ptr()) // 4 for k, v in views.items()}
    for k, v in views.items():
        a, b = (flat[s][off[k]:off[k] + v.numel()] for s in ("a", "b"))
        behind = k.startswith(("blocks.2.", "blocks.3.", "final_layer.")) and "modulation" not in k
        if behind:
            assert torch.equal(a, b), k
        elif k.startswith(("blocks.0.", "blocks.1.", "x_embedder")):
            assert not torch.equal(a, b), k


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_bit_equalities(weights, prec):
    cfg, sd = weights
    n, tap = 3, DEPTH - 2
    m = build(prec, sd, cfg, forced_weight_normalization=False)
    plain, out0, _ = run(m, n, None)
    unused, out1, _ = run(m, n, tap, use_hidden=False)
    assert torch.equal(out0, out1) and torch.equal(plain, unused)              # a tap nobody reads: today's backward, bit for bit
    inj, _, h = run(m, n, tap)
    assert not torch.equal(inj, plain)
    m._stage_hook = lambda stage: None                                         # the staged backward (what the DP reducer drives)
    staged, _, _ = run(m, n, tap)
    del m._stage_hook
    assert torch.equal(staged, inj)
    m.activation_recompute = "block"
    rec, _, h2 = run(m, n, tap)
    assert torch.equal(h2, h) and torch.equal(rec, inj)
    m.activation_recompute = "mlp"
    rec, _, _ = run(m, n, tap)
    assert torch.equal(rec, inj)


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_accumulating_backward_with_injection(weights, prec):
    cfg, sd = weights
    n = 2
    m = build(prec, sd, cfg, forced_weight_normalization=False)
    g1, _, _ = run(m, n, 0)
    g2, _, _ = run(m, n, DEPTH - 2)
    run(m, n, 0)
    both, _, _ = run(m, n, DEPTH - 2, zero=False)                              # p.grad still set: the engine's accumulate form
    assert torch.equal(both, g1 + g2)


@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_rotation_modulation_takes_the_injection(prec):
    """The rotation form runs the stand-alone pass (dx' = ca dxo + ... as in the AdaLN form): same check against the oracle."""
    O = oracle()
    cfg = config(rotation_modulation=True)
    sd = O.init_state_dict(cfg, seed=22, gains=0.3, perturb_reference=0.3)
    n, tap = 2, 1
    m = build(prec, sd, cfg)
    run(m, n, tap)
    x, t, y, drop, A, B = inputs(n)
    osd = {k: v.clone().requires_grad_(k not in O.BUFFER_KEYS) for k, v in sd.items()}
    out, h = oracle_forward_with_tap(osd, cfg, x, t, y, drop, O.engine_plan if prec == "bf16" else O.engine_plan_f16, tap)
    ((A * out).sum() + (B * h).sum()).backward()
    lim = LIMITS[prec]
    gain_scale = max(float(osd[k].grad.abs().max()) for k, p in m.named_parameters() if p.dim() == 0)
    for k, p in m.named_parameters():
        ref = osd[k].grad.numpy()
        if p.dim() == 0:
            assert abs(float(p.grad) - float(ref)) / (gain_scale + 1e-30) < lim["gain"], k
            continue
        e = rel_err(p.grad.cpu().numpy(), ref)
        assert e < (lim["big"] if ref.size >= 64 else lim["small"]) or np.linalg.norm(ref) < 1e-7, (k, e)


def test_refusals(weights):
    from mapdit_amd import _lib as L
    cfg, sd = weights
    m = build("bf16", sd, cfg)
    for bad in (DEPTH - 1, -1, DEPTH, 1.0, True):
        with pytest.raises(ValueError, match="hidden_tap"):
            m.hidden_tap = bad
    assert m.hidden_tap is None
    x, t, y, drop, A, B = (v.to(DEV) for v in inputs(2))
    # the engine itself: block out of range, a staged backward in progress, an input-only backward, an inference engine
    m(x, t, y, force_drop_ids=drop)
    rt = m._rt[True]
    dh = torch.zeros(2 * 64, 128, device=DEV)
    dout = torch.zeros(2, 8, 16, 16, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    for bad in (DEPTH - 1, -1, DEPTH):
        with pytest.raises(L.MapditError, match="hidden"):
            rt.lib.engine_set_hidden_grad(rt.handle, bad, dh.data_ptr())
    rt.lib.engine_set_hidden_grad(rt.handle, 0, dh.data_ptr())
    rt.lib.engine_set_hidden_grad(rt.handle, 0, None)                           # NULL clears
    m._attach_grads()
    rt.bind(m)
    rt.lib.engine_backward_stages(rt.handle, dout.data_ptr(), 0, 0, st)
    with pytest.raises(L.MapditError, match="hidden"):
        rt.lib.engine_set_hidden_grad(rt.handle, 0, dh.data_ptr())
    m(x, t, y, force_drop_ids=drop)                                             # (a forward ends the staged backward)
    dx = torch.zeros(2, 4, 16, 16, device=DEV)
    rt.lib.engine_set_input_grad(rt.handle, dx.data_ptr(), 1)
    with pytest.raises(L.MapditError, match="hidden"):
        rt.lib.engine_set_hidden_grad(rt.handle, 0, dh.data_ptr())
    rt.lib.engine_set_input_grad(rt.handle, None, 0)
    rt.lib.engine_set_hidden_grad(rt.handle, 0, dh.data_ptr())
    rt.lib.engine_set_input_grad(rt.handle, dx.data_ptr(), 1)                   # the other order: the backward refuses
    with pytest.raises(L.MapditError, match="hidden"):
        rt.lib.engine_backward(rt.handle, dout.data_ptr(), st)
    m(x, t, y, force_drop_ids=drop)                                             # drops both requests
    with torch.no_grad():
        m(x, t, y)
    with pytest.raises(L.MapditError, match="hidden"):
        rt_e = m._rt[False]
        rt_e.lib.engine_set_hidden_grad(rt_e.handle, 0, dh.data_ptr())
    # the facade: an input-only backward (every parameter frozen), bf16x3, the LayerNorm form
    m.hidden_tap = 1
    m.input_gradients = True
    for p in m.parameters():
        p.requires_grad_(False)
    xg = x.clone().requires_grad_(True)
    out = m(xg, t, y, force_drop_ids=drop)
    with pytest.raises(L.MapditError, match="hidden"):
        (out.sum() + m.tapped_hidden.sum()).backward()
    for p in m.parameters():
        p.requires_grad_(True)
    m.input_gradients = False
    m.gemm_precision = "bf16x3"
    with pytest.raises(ValueError, match="hidden_tap"):
        m(x, t, y, force_drop_ids=drop)
    m.hidden_tap = None
    m(x, t, y, force_drop_ids=drop)
    rt3 = m._rt[("bf16x3", True)]
    with pytest.raises(L.MapditError, match="hidden"):
        rt3.lib.engine_set_hidden_grad(rt3.handle, 0, dh.data_ptr())
    O = oracle()
    cfg_ln = config(no_layernorm=False)
    mln = build("bf16", O.init_state_dict(cfg_ln, seed=23), cfg_ln)
    mln(x, t, y, force_drop_ids=drop)
    with pytest.raises(L.MapditError, match="hidden"):
        rt_ln = mln._rt[True]
        rt_ln.lib.engine_set_hidden_grad(rt_ln.handle, 0, dh.data_ptr())
    mln.hidden_tap = 1
    with pytest.raises(ValueError, match="hidden_tap"):
        mln(x, t, y, force_drop_ids=drop)
    # a tap survives deepcopy, and an eval / no-grad forward leaves no tapped hidden state
    import copy
    m.gemm_precision, m.hidden_tap = "bf16", 2
    assert copy.deepcopy(m).hidden_tap == 2
    with torch.no_grad():
        m(x, t, y)
    assert m.tapped_hidden is None
