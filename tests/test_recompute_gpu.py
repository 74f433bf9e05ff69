"""Activation recompute on the device (DiT.activation_recompute = "mlp" / "block", mapdit_config_t.recompute).

A recomputing engine re-issues, at the start of a block's backward stage, launches the forward already made - the block's fc1 GEMM, or the
block's whole forward - from inputs it kept.  Every kernel of the step is deterministic (no atomics, fixed summation orders), so the
regenerated activations are the forward's bit for bit and every check here is torch.equal against the plain engine, not a tolerance.
The plain result of a (model, precision) pair is computed once and shared (read-only)."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err, sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
LEVELS = ["mlp", "block"]

# depth 3: the first, an interior and the last block differ (block 0's xm comes from modulate_fwd, the last block's fc2 epilogue writes xmodf)
MODELS = {
    "A": (dict(depth=3, hidden_size=128, num_heads=2, patch_size=2, input_size=16), 3),     # 64 tokens, fused QKV epilogue, one-workgroup fused backward
    "B": (dict(depth=3, hidden_size=128, num_heads=2, patch_size=2, input_size=32), 3),     # 256 tokens, streaming backward across 6 heads
    "C": (dict(depth=3, hidden_size=128, num_heads=4, patch_size=2, input_size=16), 3),     # head_dim 32: generic attention, the qkv buffer and split / merge
    "D": (dict(depth=2, hidden_size=1152, num_heads=16, patch_size=2, input_size=16), 2),   # head_dim 72, raw q / k normalised in place
    "E": (dict(depth=3, hidden_size=128, num_heads=2, patch_size=2, input_size=64), 2),     # 1,024 tokens, tiled attention kernels
}


def slot(precision):
    return True if precision == "bf16" else (precision, True)


@functools.lru_cache(maxsize=None)
def fresh_state(key, extra=()):
    """Seeded weights of model `key` (CPU state dict, read-only).  Fresh gains are zero and every block would pass x through: 0.3."""
    from mapdit_amd.src.dit import DiT
    kw, _ = MODELS[key]
    torch.manual_seed(1000 + sorted(MODELS).index(key))
    m = DiT(**kw, in_channels=4, num_classes=10, **dict(extra))
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 0:
                p.fill_(0.3)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def make(key, precision, level, extra=()):
    from mapdit_amd.src.dit import DiT
    kw, _ = MODELS[key]
    m = DiT(**kw, in_channels=4, num_classes=10, **dict(extra))
    m.load_state_dict(fresh_state(key, extra))
    m = m.to(DEV).train()
    m.gemm_precision = precision
    m.activation_recompute = level
    m.y_embedder.token_drop = lambda labels, force_drop_ids=None: labels
    return m


def reload(m, key, extra=()):
    """The training forward rewrites the weights (forced weight normalisation): every run starts from the same state dict."""
    m.load_state_dict(fresh_state(key, extra))
    for p in m.parameters():
        p.grad = None


@functools.lru_cache(maxsize=None)
def inputs(key, n=None, seed=0):
    kw, n0 = MODELS[key]
    n = n or n0
    g = torch.Generator().manual_seed(77 + seed)
    S = kw["input_size"]
    x = torch.randn(n, 4, S, S, generator=g)
    y = torch.randint(0, 10, (n,), generator=g)
    t = torch.randint(0, 1000, (n,), generator=g)
    noise = torch.randn(n, 4, S, S, generator=g)
    return tuple(v.to(DEV) for v in (x, t, y, noise))


def losses_of(m, inp):
    from mapdit_amd.diffusion import create_diffusion
    x, t, y, noise = inp
    return create_diffusion("").training_losses(m, x, t, dict(y=y), noise=noise)["loss"]


def step(m, inp):
    """One training step's forward and backward: (per-sample losses, {name: grad})."""
    for p in m.parameters():
        p.grad = None
    loss = losses_of(m, inp)
    loss.mean().backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}


def assert_same(got, want, what=""):
    loss, grads = got
    wloss, wgrads = want
    assert torch.isfinite(wloss).all() and all(torch.isfinite(g).all() for g in wgrads.values()), what
    assert any(float(g.abs().max()) > 0 for k, g in wgrads.items() if "blocks.1." in k), what     # (the blocks do take part)
    assert torch.equal(loss, wloss), what
    assert grads.keys() == wgrads.keys()
    for k in wgrads:
        assert grads[k] is not None and torch.equal(grads[k], wgrads[k]), (what, k)


@functools.lru_cache(maxsize=None)
def plain(key, precision, extra=()):
    """(losses, grads, workspace bytes) of one step on the plain engine - shared, read-only."""
    m = make(key, precision, "none", extra)
    out = step(m, inputs(key))
    return out, m._rt[slot(precision)].workspace.numel()


# ---- plain versus recompute: every model x precision x level ---------------------------------------------------------------------------
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("precision", ["bf16", "f16"])
@pytest.mark.parametrize("key", sorted(MODELS))
def test_gradients_equal_the_plain_engine(key, precision, level):
    want, ws_plain = plain(key, precision)
    m = make(key, precision, level)
    got = step(m, inputs(key))
    assert_same(got, want, (key, precision, level))
    rt = m._rt[slot(precision)]
    assert rt.recompute == level
    print(f"{key} {precision} {level}: training workspace {rt.workspace.numel()} B (plain {ws_plain} B)")
    assert rt.workspace.numel() < ws_plain


# ---- model A, bf16: the ways a backward can be driven ----------------------------------------------------------------------------------
@pytest.mark.parametrize("level", LEVELS)
def test_staged_backward(level):
    want, _ = plain("A", "bf16")                 # the UNSTAGED plain gradients
    m = make("A", "bf16", level)
    stages = []
    m._stage_hook = stages.append                # the backward then goes through mapdit_engine_backward_stages one stage at a time
    got = step(m, inputs("A"))
    assert stages == list(range(m.depth + 2))
    assert_same(got, want, level)


@functools.lru_cache(maxsize=None)
def two_batches(level):
    """A step at 4 samples, then one at 2 samples on the same runtime (max_batch stays 4)."""
    m = make("A", "bf16", level)
    a = step(m, inputs("A", 4))
    rt = m._rt[True]
    b = step(m, inputs("A", 2, seed=1))
    assert m._rt[True] is rt and rt.max_batch == 4
    return a, b


@pytest.mark.parametrize("level", LEVELS)
def test_batch_smaller_than_max_batch(level):
    for got, want in zip(two_batches(level), two_batches("none")):
        assert_same(got, want, level)


@functools.lru_cache(maxsize=None)
def two_optimiser_steps(level):
    from mapdit_amd.optim import FusedAdamEMA
    m = make("A", "bf16", level)
    opt = FusedAdamEMA(m, lr=1e-2)
    for s in range(2):
        loss = losses_of(m, inputs("A", seed=s))
        opt.zero_grad()
        loss.mean().backward()
        opt.step()
    torch.cuda.synchronize()
    return m._pflat.clone(), opt.ema[0].clone(), opt.ema[1].clone()


@pytest.mark.parametrize("level", LEVELS)
def test_two_optimiser_steps(level):
    want = two_optimiser_steps("none")
    assert torch.isfinite(want[0]).all() and not torch.equal(want[1], want[2])
    for g, w in zip(two_optimiser_steps(level), want):
        assert torch.equal(g, w)


# forced weight normalisation off, the four off forms that are engine scalars - and the forms that ride on the same block code and are
# therefore not refused: rotation modulation, weight normalisation off (another weight pass), cosine attention off (the raw-q/k
# epilogue, plain attention, the unfused backward)
VARIANTS = {
    "forced_wn_off": (("forced_weight_normalization", False),),
    "scalar_off_forms": (("mp_silu", False), ("mp_residual", False), ("mp_pos_enc", False), ("mp_embedding", False)),
    "rotation": (("rotation_modulation", True),),
    "weight_norm_off": (("weight_normalization", False),),
    "cosine_attention_off": (("cosine_attention", False),),
}


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_model_variants(variant, level):
    extra = VARIANTS[variant]
    want, ws_plain = plain("A", "bf16", extra)
    m = make("A", "bf16", level, extra)
    assert_same(step(m, inputs("A")), want, (variant, level))
    assert m._rt[True].workspace.numel() < ws_plain


@functools.lru_cache(maxsize=None)
def input_gradient(level):
    m = make("A", "bf16", level).eval()
    m.input_gradients = True
    for p in m.parameters():
        p.requires_grad_(False)
    x, t, y, noise = inputs("A", 4)
    x = x.clone().requires_grad_(True)
    out = m.forward_with_cfg(x, t, y, 1.5)
    (out * torch.cat([noise, noise], 1)).sum().backward()
    torch.cuda.synchronize()
    assert all(p.grad is None for p in m.parameters())          # input-only: no parameter gradient appears
    return x.grad.clone()


@pytest.mark.parametrize("level", LEVELS)
def test_input_only_backward(level):
    want = input_gradient("none")
    assert torch.isfinite(want).all() and float(want[:2].abs().max()) > 0
    assert torch.equal(input_gradient(level), want)


@pytest.mark.parametrize("level", LEVELS)
def test_input_gradient_beside_parameter_gradients(level):
    def run(lv):
        m = make("A", "bf16", lv)
        m.input_gradients = True
        from mapdit_amd.diffusion import create_diffusion
        x, t, y, noise = inputs("A")
        leaf = []

        def with_x(xt, tt, **kw):                # x_t = q_sample(x, t, noise) is made a leaf: dL/dx_t lands in its .grad
            leaf.append(xt.requires_grad_(True))
            return m(xt, tt, **kw)
        create_diffusion("").training_losses(with_x, x, t, dict(y=y), noise=noise)["loss"].mean().backward()
        torch.cuda.synchronize()
        assert float(leaf[0].grad.abs().max()) > 0
        return leaf[0].grad.clone(), {k: p.grad.clone() for k, p in m.named_parameters()}
    assert_same(run(level), run("none"), level)


@pytest.mark.parametrize("level", ["none"] + LEVELS)
def test_second_backward_over_the_same_forward(level):
    """The backward reads the saved forward and changes none of it: run twice (retain_graph), the accumulated gradients are exactly twice
    the single ones - on the plain engine and, with the re-run issued a second time, on the recomputing ones."""
    want, _ = plain("A", "bf16")
    m = make("A", "bf16", level)
    loss = losses_of(m, inputs("A")).mean()
    loss.backward(retain_graph=True)
    once = {k: p.grad.clone() for k, p in m.named_parameters()}
    loss.backward()
    torch.cuda.synchronize()
    for k, p in m.named_parameters():
        assert torch.equal(once[k], want[1][k]), k
        assert torch.equal(p.grad, 2 * once[k]), k


@pytest.mark.parametrize("level", LEVELS)
def test_peek(level):
    from mapdit_amd import _lib as L
    ref = make("A", "bf16", "none")
    m = make("A", "bf16", level)
    for mm in (ref, m):
        losses_of(mm, inputs("A"))               # a saved forward, no backward yet
    refused = ["hact"] if level == "mlp" else ["hact", "qn", "kn", "v", "o", "xm2"]
    for name in refused:
        with pytest.raises(L.MapditError, match="recompute"):
            m._peek(name, 1)
    kept = ["xm", "xmid", "xout"] + ([] if level == "block" else ["qn", "kn", "v", "o", "xm2"])
    for name in kept:
        for blk in range(3):
            assert torch.equal(m._peek(name, blk), ref._peek(name, blk)), (name, blk)
    for name in ("four", "temb", "c", "mod_all", "x0", "xmodf", "lin"):
        assert torch.equal(m._peek(name), ref._peek(name)), name


def test_changing_the_level_replaces_the_training_runtime_only():
    m = make("A", "bf16", "block")
    x, t, y, _ = inputs("A")
    m.eval()
    with torch.no_grad():
        out = m(x, t, y)
    m.train()
    infer = m._rt[False]
    assert infer.recompute == "none"             # an inference runtime has no level
    step(m, inputs("A"))
    small = m._rt[True]
    assert small.recompute == "block"
    m.activation_recompute = "none"
    step(m, inputs("A"))
    assert set(m._rt) == {False, True} and m._rt[False] is infer
    assert m._rt[True] is not small and m._rt[True].recompute == "none"
    assert m._rt[True].workspace.numel() > small.workspace.numel()
    reload(m, "A")
    assert_same(step(m, inputs("A")), plain("A", "bf16")[0])
    m.eval()
    reload(m, "A")
    with torch.no_grad():
        assert torch.equal(m(x, t, y), out)


# ---- refused combinations ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("what", ["bf16x3", "layernorm"])
def test_refused_combinations(what, level):
    from mapdit_amd import _lib as L
    m = make("A", "bf16x3" if what == "bf16x3" else "bf16", level, (("no_layernorm", False),) if what == "layernorm" else ())
    with pytest.raises(L.MapditError, match="recompute"):
        losses_of(m, inputs("A"))
    m.activation_recompute = "none"              # the same model trains once the level is taken back
    loss, grads = step(m, inputs("A"))
    assert torch.isfinite(loss).all()


# ---- the link to the pinned fixtures -----------------------------------------------------------------------------------------------------
def test_block_level_against_the_reference_fixture():
    """tiny_a at level "block" within the limits tests/test_model_gpu.py holds the plain engine to (equality with the plain engine already
    implies it)."""
    from test_model_gpu import GAIN_TOL, GRAD_TOL, LOSS_TOL, SMALL_GRAD_TOL, build, dev
    from mapdit_amd.diffusion import create_diffusion
    g = load_golden("tiny_a")
    m, cfg, _ = build(g, train=True)
    m.activation_recompute = "block"
    x, t, y_eff, noise = dev(g, "x", "t", "y_eff", "noise")
    m.y_embedder.token_drop = lambda labels, force_drop_ids=None: labels
    losses = create_diffusion("").training_losses(m, x, t, dict(y=y_eff), noise=noise)
    losses["loss"].mean().backward()
    torch.cuda.synchronize()
    assert m._rt[True].recompute == "block"
    for k in ("loss", "mse", "vb"):
        assert rel_err(losses[k].detach().cpu().numpy(), g["train_" + k]) < LOSS_TOL, k
    gain_scale = max(float(np.abs(g["grad/" + k]).max()) for k, p in m.named_parameters() if p.dim() == 0)
    for k, p in m.named_parameters():
        gref = g["grad/" + k]
        if p.dim() == 0:
            assert abs(float(p.grad) - float(gref.item())) / (gain_scale + 1e-30) < GAIN_TOL, k
            continue
        e = rel_err(sub(p.grad), gref)
        assert e < (GRAD_TOL if gref.size >= 64 else SMALL_GRAD_TOL) or np.linalg.norm(gref) < 1e-7, (k, e)
