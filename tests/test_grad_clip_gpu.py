"""Global gradient-norm clipping through FusedAdamEMA (optim.py: max_grad_norm, grad_norm(), clip_coef(), norm_sync), the data-parallel
reducers and the training harness, on the tiny fixture models.  The kernels themselves: tests/test_grad_clip_kernels_gpu.py; the reference
and the bound of 2^-23: tests/grad_clip_reference.py."""
import math
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import grad_clip_reference as G
from grad_accum_worker import fixture_model, mean_loss, reset_grads

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "grad_clip_worker.py")
GS = 1.0 / 3


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def gradient():
    """The flat gradient buffer of one backward of tiny_a (bf16 engine) on the host; every optimiser under test steps from it."""
    m, _, batch = fixture_model("tiny_a", "bf16")
    reset_grads(m)
    mean_loss(m, batch).backward()
    torch.cuda.synchronize()
    g = m._gflat.cpu()
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    return g


def optimizer(gradient, precision="bf16", steps=0, plant=None, **kw):
    """FusedAdamEMA over a fresh tiny_a whose flat gradient buffer holds `gradient` (with `plant` = (index, value) written over one
    element), `steps` steps taken."""
    from mapdit_amd.optim import FusedAdamEMA
    m, _, batch = fixture_model("tiny_a", precision)
    reset_grads(m)
    mean_loss(m, batch).backward()                         # creates the flat buffer and attaches p.grad to it
    torch.cuda.synchronize()
    m._gflat.copy_(gradient)
    if plant is not None:
        m._gflat[plant[0]] = plant[1]
    kw.setdefault("grad_scale", GS)
    opt = FusedAdamEMA(m, lr=1e-2, **kw)
    for _ in range(steps):
        opt.step()
    torch.cuda.synchronize()
    return m, opt


def state(m, opt):
    return {"p": m._pflat.clone(), "m": opt.exp_avg.clone(), "v": opt.exp_avg_sq.clone(), "ea": opt.ema[0].clone(), "eb": opt.ema[1].clone()}


def same_state(a, b):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in a)


def test_none_and_inf_leave_the_step_s_bits_alone(gradient):
    """Two steps.  max_grad_norm = None: bit-equal to an optimiser built without the argument, and no clip buffer exists.  max_grad_norm =
    inf: parameters, moments and EMA copies bit-equal too; grad_norm() is clip64 of the flat gradient read back and torch's fp64 CPU
    clip_grad_norm_ over [p.grad ...] (times grad_scale), to 2^-23; clip_coef() is exactly 1."""
    m0, o0 = optimizer(gradient, steps=2)
    want = state(m0, o0)
    assert not torch.equal(want["p"], want["ea"])
    m1, o1 = optimizer(gradient, steps=2, max_grad_norm=None)
    assert same_state(state(m1, o1), want) and o1._clip is None and o1.max_grad_norm is None
    with pytest.raises(RuntimeError, match="no clipped step"):
        o1.grad_norm()
    m2, o2 = optimizer(gradient, steps=2, max_grad_norm=math.inf)
    assert same_state(state(m2, o2), want)
    norm, coef = o2.grad_norm(), o2.clip_coef()
    want_norm, _ = G.clip64(m2._gflat.cpu().numpy(), G.f32(GS), math.inf)
    params = []
    for q in m2.parameters():
        w = torch.nn.Parameter(torch.zeros(q.shape, dtype=torch.float64))
        w.grad = q.grad.detach().double().cpu() * G.f32(GS)
        params.append(w)
    torch_norm = float(torch.nn.utils.clip_grad_norm_(params, math.inf, norm_type=2))
    print(f"grad_norm {norm:.9g}, clip64 {want_norm:.17g}, torch fp64 {torch_norm:.17g}")
    assert coef == 1.0 and want_norm > 0
    assert abs(norm - want_norm) <= G.TOL * want_norm and abs(norm - torch_norm) <= G.TOL * torch_norm


def test_half_the_norm_is_the_unclipped_step_at_the_scaled_gradient(gradient):
    """max_grad_norm = 0.5 x norm: clip_coef() within 2^-23 of the reference; the step (two of them) is bit-equal to an unclipped
    FusedAdamEMA whose grad_scale is fp32(grad_scale * coef) with coef as read from the device; p.grad is not rewritten."""
    gs = G.f32(GS)
    norm, _ = G.clip64(gradient.numpy(), gs, math.inf)
    mx = G.f32(0.5 * norm)
    want_norm, want_coef = G.clip64(gradient.numpy(), gs, mx)
    m, opt = optimizer(gradient, steps=2, max_grad_norm=mx)
    got_norm, got_coef = opt.grad_norm(), opt.clip_coef()
    print(f"norm {got_norm:.9g} (want {want_norm:.17g}), coef {got_coef:.9g} (want {want_coef:.17g})")
    assert 0.49 < want_coef < 0.51
    assert abs(got_norm - want_norm) <= G.TOL * want_norm and abs(got_coef - want_coef) <= G.TOL * want_coef
    assert torch.equal(bits(m._gflat.cpu()), bits(gradient))
    for q, view in zip(m.parameters(), m._gviews):
        assert q.grad.data_ptr() == view.data_ptr()
    scaled = float(np.float32(gs) * np.float32(got_coef))
    m2, o2 = optimizer(gradient, steps=2, grad_scale=scaled)
    assert same_state(state(m, opt), state(m2, o2))
    m3, o3 = optimizer(gradient, steps=2)
    assert not same_state(state(m, opt), state(m3, o3))


def test_accumulated_micro_batches_give_the_norm_of_the_averaged_gradient():
    """Two micro-batches (samples 0-1 and 2-3), the second backward accumulating, grad_scale = 1/2: grad_norm() is clip64 of the buffer
    read back (2^-23) and the norm of the averaged gradient 0.5 (g1 + g2) formed in fp64 from two fresh backwards.  Bound of the second
    comparison: the accumulated buffer differs from g1 + g2 by at most 2 * 2^-23 (|g1| + |g2|) per element (tests/grad_accum_worker.py),
    a norm moves by at most the norm of the difference, plus the 2^-23 of the read-back."""
    from mapdit_amd.optim import FusedAdamEMA
    m, _, (x, t, y, noise) = fixture_model("tiny_a", "bf16")
    halves = [tuple(v[lo:lo + 2] for v in (x, t, y, noise)) for lo in (0, 2)]
    fresh = []
    for h in halves:
        reset_grads(m)
        mean_loss(m, h).backward()
        torch.cuda.synchronize()
        fresh.append(m._gflat.double().cpu().numpy())
    reset_grads(m)
    for h in halves:
        mean_loss(m, h).backward()                         # the second one accumulates
    opt = FusedAdamEMA(m, lr=1e-2, grad_scale=0.5, max_grad_norm=math.inf)
    opt.step()
    got = opt.grad_norm()
    want, _ = G.clip64(m._gflat.cpu().numpy(), 0.5, math.inf)
    averaged = 0.5 * float(np.linalg.norm(fresh[0] + fresh[1]))
    slack = 0.5 * 2.0 * 2.0 ** -23 * float(np.linalg.norm(np.abs(fresh[0]) + np.abs(fresh[1]))) + G.TOL * averaged
    print(f"grad_norm {got:.9g}, clip64 of the buffer {want:.17g}, norm of the averaged gradient {averaged:.17g} (+- {slack:.3e})")
    assert averaged > 0 and abs(got - want) <= G.TOL * want and abs(got - averaged) <= slack
    assert abs(averaged - float(np.linalg.norm(fresh[0]))) > 10 * slack          # (the two halves are different gradients)


def test_fp16_guard_is_subsumed_by_the_norm_pass(gradient, monkeypatch):
    """f16 engine (guard on by default) with max_grad_norm: a planted inf gives a refused step - poll_overflow() == 1, parameters,
    moments and EMA copies untouched, grad_norm() inf - and a finite gradient an applied one, both without one grad_nonfinite_check
    launch (counted through wrappers on the loaded library), through grad_sqnorm instead."""
    from mapdit_amd import _lib as L
    lib = L.lib()
    calls = {"grad_nonfinite_check": 0, "grad_nonfinite_check_ranges": 0, "grad_sqnorm": 0, "grad_clip_coef": 0}
    for name in calls:
        def counting(*a, _name=name, _fn=getattr(lib, name)):
            calls[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, counting)
    m, opt = optimizer(gradient, precision="f16", plant=(gradient.numel() // 2, float("inf")), max_grad_norm=1.0)
    before = state(m, opt)
    opt.step()
    torch.cuda.synchronize()
    assert same_state(state(m, opt), before) and opt._status.tolist() == [1, 1]
    assert opt.grad_norm() == math.inf and opt.clip_coef() == 0.0
    assert opt.poll_overflow() == 1 and opt.step_count == 0
    assert calls["grad_nonfinite_check"] == 0 and calls["grad_nonfinite_check_ranges"] == 0 and calls["grad_sqnorm"] == 1 and calls["grad_clip_coef"] == 1
    m._gflat.copy_(gradient)                               # finite again: applied
    opt.step()
    torch.cuda.synchronize()
    assert not same_state(state(m, opt), before) and opt.overflow_steps() == 1 and math.isfinite(opt.grad_norm())
    assert calls["grad_nonfinite_check"] == 0 and calls["grad_nonfinite_check_ranges"] == 0 and calls["grad_sqnorm"] == 2
    # the guard alone (no clipping) still goes through the check
    m2, o2 = optimizer(gradient, precision="f16", steps=1)
    assert calls["grad_nonfinite_check"] == 1 and calls["grad_sqnorm"] == 2 and o2.overflow_steps() == 0


def test_many_shards_take_the_table_form(gradient):
    """More than 8 live ranges (12 shards): grad_sqnorm_ranges over the optimiser's cached table; the norm is clip64 over the covered
    elements and the step is bit-equal to the unclipped one at the scaled gradient on the same shards."""
    n = gradient.numel()
    per = (n // 12) // 8 * 8
    shards = [(i * per, i * per + per - 4 * (i % 3)) for i in range(12)]
    covered = np.concatenate([gradient.numpy()[lo:hi] for lo, hi in shards])
    gs = G.f32(GS)
    mx = G.f32(0.5 * G.clip64(covered, gs, math.inf)[0])
    want_norm, want_coef = G.clip64(covered, gs, mx)
    m, opt = optimizer(gradient, max_grad_norm=mx)
    opt.shards = list(shards)
    opt.step()
    norm, coef = opt.grad_norm(), opt.clip_coef()
    assert abs(norm - want_norm) <= G.TOL * want_norm and abs(coef - want_coef) <= G.TOL * want_coef
    m2, o2 = optimizer(gradient, grad_scale=float(np.float32(gs) * np.float32(coef)))
    o2.shards = list(shards)
    o2.step()
    torch.cuda.synchronize()
    assert same_state(state(m, opt), state(m2, o2))


def test_sharded_weight_passes_refuse_clipping_by_name(gradient):
    from mapdit_amd._lib import MapditError
    from mapdit_amd.parallel import ShardedPassReducer
    m, opt = optimizer(gradient, max_grad_norm=1.0)
    red = ShardedPassReducer(m, emulate=(0, 2))            # what rank 0 of 2 would do, without the collectives
    with pytest.raises(MapditError, match=r"max_grad_norm.*zero1w"):
        red.attach(opt)
    m2, o2 = optimizer(gradient)
    red2 = ShardedPassReducer(m2, emulate=(0, 2))
    red2.attach(o2)                                        # without clipping: accepted
    o2.max_grad_norm = 1.0                                 # ... set later: refused at step(), before anything is launched
    before = state(m2, o2)
    with pytest.raises(MapditError, match=r"max_grad_norm.*zero1w"):
        o2.step()
    torch.cuda.synchronize()
    assert same_state(state(m2, o2), before) and o2.step_count == 0


# ---- two ranks on one GPU over gloo -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["allreduce", "zero1"])
def test_two_ranks_clip_with_one_norm(tmp_path, mode):
    """Two ranks (gloo, one GPU), one clipped step with coef about 0.5: norm and coef bit-equal across the ranks, the flat parameters
    bit-equal across the ranks, and the norm within 2^-22 of a single-process clip64 over the summed gradients (one ulp more than the
    other bounds: under zero1 the fp64 sum is partitioned differently - per rank, then the all-reduce)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), WORKER, str(tmp_path), mode]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, MAPDIT_DIST_BACKEND="gloo"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    a, b = (torch.load(tmp_path / f"rank{i}.pt", weights_only=False) for i in range(2))
    assert torch.equal(bits(a["clip"]), bits(b["clip"])) and torch.equal(bits(a["p"]), bits(b["p"])) and torch.equal(bits(a["g"]), bits(b["g"]))
    assert a["max_norm"] == b["max_norm"] and a["grad_scale"] == 0.5
    if mode == "zero1":
        assert a["shards"] != b["shards"] and len(a["shards"]) > 1
    want_norm, want_coef = G.clip64(a["g"].numpy(), a["grad_scale"], a["max_norm"])
    print(f"{mode}: norm {a['norm']:.9g} (want {want_norm:.17g}), coef {a['coef']:.9g} (want {want_coef:.17g})")
    assert a["coef"] < 1.0 and 0.49 < want_coef < 0.51
    assert abs(a["norm"] - want_norm) <= 2.0 ** -22 * want_norm and abs(a["coef"] - want_coef) <= 2.0 ** -22 * want_coef


# ---- the harness ------------------------------------------------------------------------------------------------------------------------
def test_train_harness_logs_norm_and_coefficient_only_with_the_flag(tmp_path):
    """train.py --synthetic --max-grad-norm 1.0, three steps of DiT-XS/2: the log line carries `, grad norm: F, clip: F` behind the
    current format; without the flag the line is the current format to the byte."""
    from mapdit_amd import train
    args = ["--synthetic", "--model", "DiT-XS/2", "--num-steps", "3", "--batch-size", "4", "--log-every", "1", "--ckpt-every", "1000",
            "--ema-snapshot-every", "1000", "--num-classes", "10", "--num-lin-warmup", "1", "--start-decay", "2", "--precision", "bf16"]
    plain = r"\(step=\d{7}\) train loss: \d+\.\d{4}, train steps/sec: \d+\.\d{2}"
    for tag, extra, pattern in (("clip", ["--max-grad-norm", "1.0"], plain + r", grad norm: \d+\.\d{4}, clip: [01]\.\d{3}"), ("plain", [], plain)):
        exp = train.main(args + extra + ["--results-dir", str(tmp_path / tag)])
        lines = [ln for ln in open(os.path.join(exp, "log.txt")).read().splitlines() if ln.startswith("(step=")]
        assert len(lines) == 3, lines
        for ln in lines:
            assert re.fullmatch(pattern, ln), (tag, ln)
        if tag == "clip":
            norms = [float(ln.split("grad norm: ")[1].split(",")[0]) for ln in lines]
            coefs = [float(ln.split("clip: ")[1]) for ln in lines]
            assert all(nm > 0 for nm in norms) and all(abs(c - min(1.0 / (nm + 1e-6), 1.0)) < 2e-3 for c, nm in zip(coefs, norms)), lines
