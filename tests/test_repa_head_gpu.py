"""``repa.RepaHead`` on the GPU against the fp64 restatement (tests/repa_reference.py): RepaHead(128, 24, hidden=64) on 2 x 64 tokens, the
loss, d loss / d hidden and every parameter gradient, in both operand formats; accumulation, determinism and the flat buffers the fused
optimiser steps.

Tolerance: norm-wise relative distance to the EXACT fp64 head <= 2 x e_emul, e_emul the distance the restatement's own emulation of the
16-bit operand rounding (hidden state, weights, activations, activation gradients under the loss scale) keeps from the exact head on the
very inputs of this test - the rule tests/test_dinov2_* use; the factor 2 covers fp32 accumulation and fp32 pointwise math.  E_EMUL below
is measured on the CPU by repa_reference.measure_head_emulation; tests/test_repa_cpu.py asserts these constants are what it measures."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import repa_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

E_EMUL = {
    "f16": {"loss": 3.656e-04, "dh": 5.337e-04, "w1": 5.370e-04, "b1": 4.834e-04, "w2": 5.062e-04, "b2": 3.511e-04, "w3": 4.962e-04, "b3": 1.571e-04},
    "bf16": {"loss": 5.368e-03, "dh": 4.103e-03, "w1": 4.075e-03, "b1": 3.284e-03, "w2": 4.102e-03, "b2": 2.627e-03, "w3": 4.124e-03, "b3": 1.351e-03},
}


def make_head(prec):
    from mapdit_amd.repa import RepaHead
    c = R.HEAD_CASE
    return RepaHead(c["in_dim"], c["feat_dim"], hidden=c["hidden"], precision=prec, seed=c["seed"]).to(DEV)


def run(head, h, feats, g):
    c = R.HEAD_CASE
    hid = torch.from_numpy(h).to(DEV).view(c["N"], c["T"], c["in_dim"]).requires_grad_(True)
    f = torch.from_numpy(feats).to(DEV).view(c["N"], c["T"], c["feat_dim"])
    loss = head.loss(hid, f)
    (loss * torch.from_numpy(g).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return loss.detach(), hid.grad


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_head_against_fp64(prec):
    h, feats, g, p = R.head_case()
    head = make_head(prec)
    for k, v in p.items():                                   # the seeded nn.Linear-style draw is the restatement's
        assert np.array_equal(getattr(head, k).detach().cpu().numpy(), v.astype(np.float32)), k
    loss, dh = run(head, h, feats, g)
    want_loss, want_dh, want_g = R.head_loss(h, feats, p, R.HEAD_CASE["T"], g)
    got = {"loss": loss.double().cpu().numpy(), "dh": dh.double().cpu().numpy().reshape(want_dh.shape)}
    want = {"loss": want_loss, "dh": want_dh}
    for k in want_g:
        got[k], want[k] = getattr(head, k).grad.double().cpu().numpy(), want_g[k]
    assert head.effective_loss_scale() == R.head_scale(prec)
    bad = []
    for k in want:
        e, lim = R.rel(got[k], want[k]), 2 * E_EMUL[prec][k]
        print(f"{prec} {k}: rel err {e:.3e} (limit {lim:.3e})")
        if not e <= lim:
            bad.append((k, e, lim))
    assert not bad, bad


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_head_accumulates_and_repeats(prec):
    h, feats, g, _ = R.head_case()
    head = make_head(prec)
    assert head._pflat.is_cuda and all(p.data_ptr() >= head._pflat.data_ptr() for p in head.parameters())
    run(head, h, feats, g)
    g1 = head._gflat.clone()
    assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(head.parameters(), head._gviews))
    run(head, h, feats, g)                                   # p.grad still set: the accumulate forms
    assert torch.equal(head._gflat, g1 + g1)
    for p in head.parameters():
        p.grad = None
    run(head, h, feats, g)
    assert torch.equal(head._gflat, g1)                      # a fixed order everywhere: the same bits


def test_head_steps_under_the_fused_optimiser_and_refuses():
    from mapdit_amd.optim import FusedAdamEMA
    from mapdit_amd.repa import RepaHead
    h, feats, g, _ = R.head_case()
    head = make_head("f16")
    opt = FusedAdamEMA(head, lr=1e-3, ema_stds=())
    before = head._pflat.clone()
    run(head, h, feats, g)
    opt.step()
    torch.cuda.synchronize()
    assert opt.poll_overflow() == 0 and not torch.equal(head._pflat, before) and torch.isfinite(head._pflat).all()
    sd = head.state_dict()
    assert sorted(sd) == ["b1", "b2", "b3", "w1", "w2", "w3"]
    other = make_head("f16")
    other.load_state_dict(sd)
    assert torch.equal(other._pflat, head._pflat)
    c = R.HEAD_CASE
    hid = torch.zeros(c["N"], c["T"], c["in_dim"], device=DEV)
    with pytest.raises(ValueError, match="features"):
        head.loss(hid, torch.zeros(c["N"], c["T"], c["feat_dim"] + 8, device=DEV))
    with pytest.raises(ValueError, match="fp16 or fp32"):
        head.loss(hid, torch.zeros(c["N"], c["T"], c["feat_dim"], device=DEV, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="width"):
        head.loss(torch.zeros(c["N"], c["T"], 64, device=DEV), torch.zeros(c["N"], c["T"], c["feat_dim"], device=DEV))
    for bad in (dict(precision="bf16x3"), dict(hidden=60), dict(feat_dim=20)):
        kw = dict(in_dim=128, feat_dim=24, hidden=64, precision="f16")
        kw.update(bad)
        with pytest.raises(ValueError):
            RepaHead(**kw)
