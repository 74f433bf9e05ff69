"""Engine-native gradient accumulation (mapdit_engine_set_grad_accumulate): a backward while p.grad is set makes every gradient writer of
the bf16 / f16 engines add in place - no copy of the flat gradient buffer, no extra pass over it, also under the data-parallel reducers
(reducer.no_sync() for the micro-steps that do not end an optimiser step)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err, sub
from grad_accum_worker import (accumulate, check_accumulate_onto_zeros, check_sum_of_micro_batches, fixture_model, mean_loss,
                               micro_batches, reset_grads)
from test_model_gpu import GAIN_TOL, GRAD_TOL, NAMED_LIMITS, SMALL_GRAD_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "grad_accum_worker.py")


# ---- 1. accumulating onto zeros gives a fresh backward's bits -------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["tiny_a", "xl_d1"])
def test_accumulating_onto_zeros_gives_a_fresh_backward_s_bits(name, precision):
    m, _, batch = fixture_model(name, precision)          # eval mode: two forwards see the same weights
    check_accumulate_onto_zeros(m, batch)


# ---- 2. sum of different micro-batches -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_three_micro_batches_accumulate_to_their_sum(precision):
    m, _, batch = fixture_model("tiny_a", precision)
    worst = check_sum_of_micro_batches(m, batch)
    print(f"[{precision}] worst |acc - sum g_i| over its bound 2 * 2^-23 * sum|g_i|: {worst:.3f}")


# ---- 3. against the reference's gradients ----------------------------------------------------------------------------------------------
def _two_half_batches(m, batch):
    x, t, y, noise = batch
    assert x.shape[0] == 4
    reset_grads(m)
    for lo in (0, 2):
        (mean_loss(m, tuple(v[lo:lo + 2] for v in (x, t, y, noise))) / 2).backward()      # the second backward accumulates
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["tiny_a", "tiny_b"])
def test_two_micro_batches_match_reference_gradients_tiny(name):
    """Samples 0-1 and 2-3 as two micro-batches, each loss.mean() / 2, in training mode, against the reference's gradients of the whole
    batch by the comparison and the limits of test_model_gpu.test_training_losses_and_gradients.  (postw/* is not asserted: the second
    training forward rewrites the weights once more.)"""
    m, g, batch = fixture_model(name, "bf16", train=True)
    _two_half_batches(m, batch)
    gain_scale = max(float(np.abs(g["grad/" + k]).max()) for k, p in m.named_parameters() if p.dim() == 0)
    worst = worst_gain = 0.0
    for k, p in m.named_parameters():
        gref = g["grad/" + k]
        if p.dim() == 0:
            gain_dev = abs(float(p.grad) - float(gref)) / (gain_scale + 1e-30)
            worst_gain = max(worst_gain, gain_dev)
            assert gain_dev < GAIN_TOL, (k, float(p.grad), float(gref))
            continue
        e = rel_err(sub(p.grad), gref)
        worst = max(worst, e)
        tol = GRAD_TOL if gref.size >= 64 else SMALL_GRAD_TOL
        assert e < tol or np.linalg.norm(gref) < 1e-7, (k, e)
    print(f"{name}: worst gradient rel err {worst:.3e}; worst gain deviation {worst_gain:.3e}")


@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_two_micro_batches_match_reference_gradients_s2_n4(precision):
    """The same on DiT-S/2 (full depth, N = 4) in both engine precisions, by the comparison and the limits of
    test_model_gpu.test_named_models_match_reference."""
    from conftest import golden_cfg, golden_state_dict
    from mapdit_amd.src.models import DIT_MODELS
    lim = NAMED_LIMITS[precision]
    g = load_golden("s2_n4")
    cfg = golden_cfg(g)
    m = DIT_MODELS["DiT-S/2"](in_channels=4, input_size=32, num_classes=1000)
    m.load_state_dict(golden_state_dict(g, cfg))
    m = m.to(DEV).train()
    m.gemm_precision = precision
    m.y_embedder.token_drop = lambda labels, force_drop_ids=None: labels
    _two_half_batches(m, tuple(torch.from_numpy(g[n]).to(DEV) for n in ("x", "t", "y_eff", "noise")))
    worst = worst_e = worst_gain = 0.0
    gain_scale = max(float(g["gradnorm/" + k]) for k, p in m.named_parameters() if p.dim() == 0)
    for k, p in m.named_parameters():
        gn = float(g["gradnorm/" + k])
        if p.dim() == 0:
            gain_dev = abs(float(p.grad) - float(g["grad/" + k])) / (gain_scale + 1e-30)
            worst_gain = max(worst_gain, gain_dev)
            assert gain_dev < lim["gain"], (k, float(p.grad), float(g["grad/" + k]))
            continue
        if gn < 1e-7:
            continue
        got = float(p.grad.double().norm())
        worst = max(worst, abs(got / gn - 1))
        assert abs(got / gn - 1) < (lim["gnorm"] if p.numel() >= 64 else lim["gsmall"]), (k, got, gn)
        gref = g["grad/" + k]
        e = rel_err(sub(p.grad, stride=4099), gref)
        if gref.size >= 64:
            worst_e = max(worst_e, e)
        assert e < (lim["gtensor"] if gref.size >= 64 else lim["gsmall"]) or p.numel() < 64, (k, e)
    print(f"s2_n4 [{precision}]: worst gradient-norm deviation {worst:.3e}, worst sub-sampled gradient tensor {worst_e:.3e}, "
          f"worst gain deviation {worst_gain:.3e}")


# ---- 4. no second gradient buffer ------------------------------------------------------------------------------------------------------
def test_accumulating_backward_allocates_no_second_gradient_buffer():
    """DiT-S/2 at two samples: the flat gradient buffer (132 MB) dominates every temporary of a backward.  The accumulating forward and
    backward must not raise the allocation peak by as much as half of it (the copy the facade used to take costs all of it)."""
    from mapdit_amd.src.models import DIT_MODELS
    torch.manual_seed(41)
    m = DIT_MODELS["DiT-S/2"](in_channels=4, input_size=32, num_classes=10).to(DEV).eval()
    m.gemm_precision = "bf16"
    g = torch.Generator().manual_seed(42)
    batch = (torch.randn(2, 4, 32, 32, generator=g).to(DEV), torch.randint(0, 1000, (2,), generator=g).to(DEV),
             torch.randint(0, 10, (2,), generator=g).to(DEV), torch.randn(2, 4, 32, 32, generator=g).to(DEV))
    mean_loss(m, batch).backward()
    torch.cuda.synchronize()
    first = m._gflat.clone()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    mean_loss(m, batch).backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    gbytes = m._gflat.numel() * 4
    print(f"allocation peak of the accumulating step: +{rise / 2**20:.1f} MiB; flat gradient buffer {gbytes / 2**20:.1f} MiB")
    assert rise < gbytes // 2, (rise, gbytes)
    assert rel_err(m._gflat.cpu().numpy(), (2 * first).cpu().numpy()) < 1e-6            # and it did accumulate


# ---- 5. staged backward with accumulation ----------------------------------------------------------------------------------------------
def test_staged_backward_accumulates_after_a_no_sync_micro_step(monkeypatch):
    from mapdit_amd.parallel import OverlappedGradReducer
    m, _, batch = fixture_model("tiny_a", "bf16")
    mb = micro_batches(batch)[:2]
    want = accumulate(m, mb)                                # the same two backwards without a reducer
    m2, _, _ = fixture_model("tiny_a", "bf16")
    monkeypatch.setenv("MAPDIT_FORCE_STAGED_BACKWARD", "1")
    red = OverlappedGradReducer(m2, force_collective=False)
    inner, seen = m2._stage_hook, []
    assert inner is not None
    m2._stage_hook = lambda s: (seen.append(s), inner(s))
    reset_grads(m2)
    with red.no_sync():
        assert m2._stage_hook is None
        mean_loss(m2, mb[0]).backward()
    assert seen == [] and m2._stage_hook is not None
    mean_loss(m2, mb[1]).backward()                         # staged: the hook runs after every stage, the engine accumulates through them
    red.finish()
    torch.cuda.synchronize()
    assert seen == list(range(m2.depth + 2))
    assert torch.equal(m2._gflat, want)


# ---- 6. activation recompute -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_accumulation_under_block_recompute_is_bit_equal(precision):
    m, _, batch = fixture_model("tiny_a", precision)
    want = accumulate(m, micro_batches(batch))
    m2, _, _ = fixture_model("tiny_a", precision)
    m2.activation_recompute = "block"
    got = accumulate(m2, micro_batches(batch))
    assert float(want.abs().max()) > 0 and torch.equal(got, want)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_bf16x3_engine_refuses_and_the_facade_keeps_its_copy_path():
    from mapdit_amd._lib import MapditError
    m, _, batch = fixture_model("tiny_a", "bf16x3")
    mean_loss(m, batch).backward()
    g1 = m._gflat.clone()
    rt = m._rt[("bf16x3", True)]
    with pytest.raises(MapditError, match="accumulate"):
        rt.lib.engine_set_grad_accumulate(rt.handle, 1)
    mean_loss(m, batch).backward()                          # accumulates by the copy-and-add path
    torch.cuda.synchronize()
    assert rel_err(m._gflat.cpu().numpy(), (2 * g1).cpu().numpy()) < 1e-6


def test_refused_between_stages_and_dropped_by_a_forward():
    from mapdit_amd import _lib as L
    m, _, batch = fixture_model("tiny_a", "bf16")
    g1 = accumulate(m, [batch])                             # a fresh backward
    rt = m._rt[True]
    x, t, y, _ = batch
    out = m(x, t, y)                                        # a saved forward (gradients are enabled)
    dout = torch.full_like(out, 1e-3)
    with torch.cuda.device(x.device):
        rt.lib.engine_backward_stages(rt.handle, dout.data_ptr(), 0, 0, L.cur_stream())
        with pytest.raises(L.MapditError, match="accumulate"):
            rt.lib.engine_set_grad_accumulate(rt.handle, 1)
        rt.lib.engine_backward_stages(rt.handle, dout.data_ptr(), 1, m.depth + 1, L.cur_stream())
        rt.lib.engine_set_grad_accumulate(rt.handle, 1)     # accepted between backwards ...
    reset_grads(m)
    mean_loss(m, batch).backward()                          # ... and dropped by this forward: a fresh backward overwrites
    torch.cuda.synchronize()
    assert torch.equal(m._gflat, g1)


def test_sharded_weight_passes_refuse_accumulation_by_name():
    from mapdit_amd._lib import MapditError
    from mapdit_amd.parallel import ShardedPassReducer
    m, _, batch = fixture_model("tiny_a", "bf16", train=True)
    red = ShardedPassReducer(m, emulate=(0, 2))             # what rank 0 of 2 would do, without the collectives
    with pytest.raises(MapditError, match="sharded weight passes"):
        red.no_sync()
    reset_grads(m)
    mean_loss(m, batch).backward()
    loss = mean_loss(m, batch)
    with pytest.raises(MapditError, match="sharded weight passes"):
        loss.backward()


# ---- 8. the other weight-gradient paths, one child process each ------------------------------------------------------------------------
def test_grouped_and_side_stream_weight_gradient_paths_accumulate():
    """MAPDIT_DW_GROUP=2 (the grouped launch with its grouped Jacobians) and MAPDIT_SIDE_JAC=1 (the Jacobians on the side stream) are
    read once per process: checks 1 and 2 in a child each, the second only after the first has exited cleanly."""
    for env in (dict(MAPDIT_DW_GROUP="2"), dict(MAPDIT_SIDE_JAC="1")):
        r = subprocess.run([sys.executable, WORKER, "paths"], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
        print(r.stdout[-1500:])
        assert r.returncode == 0, (env, r.stdout[-2000:], r.stderr[-3000:])


# ---- 9. two ranks on one GPU over gloo -------------------------------------------------------------------------------------------------
def _run_dp(out, world, mode, k):
    out.mkdir()
    env = dict(os.environ, MAPDIT_DIST_BACKEND="gloo")
    if world == 1:
        cmd = [sys.executable, WORKER, "dp", str(out), mode, str(k)]
        env.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    else:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
               "--master-port", str(port), WORKER, "dp", str(out), mode, str(k)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return [torch.load(out / f"rank{i}.pt", weights_only=False) for i in range(world)]


@pytest.fixture(scope="module")
def single_process_four_micro_batches(tmp_path_factory):
    return _run_dp(tmp_path_factory.mktemp("accum_dp") / "single", 1, "allreduce", 4)[0]


@pytest.mark.parametrize("mode", ["allreduce", "zero1"])
def test_two_ranks_accumulate_two_micro_steps_each(tmp_path, mode, single_process_four_micro_batches):
    """Two ranks (gloo, one GPU), K = 2 micro-steps per rank on tiny_a (one sample each), one optimiser step: replicas bit-identical, and
    equal to ONE process accumulating the same four micro-batches within the bound of
    test_train_gpu.test_two_rank_data_parallel_matches_single_process for one step of the bf16 engine (2e-5: the summation order differs)."""
    r = _run_dp(tmp_path / mode, 2, mode, 2)
    for k in ("p", "g", "m"):
        assert torch.equal(r[0][k], r[1][k]), f"{mode}: replicas differ in {k}"
    single = single_process_four_micro_batches
    assert not torch.equal(single["p"], torch.zeros_like(single["p"])) and float(single["g"].abs().max()) > 0
    for k in ("g", "p", "m"):
        e = rel_err(r[0][k].numpy(), single[k].numpy())
        print(f"{mode}: two ranks x 2 micro-steps vs one process x 4, {k}: {e:.2e}")
        assert e < 2e-5, (k, e)


# ---- the harness ----------------------------------------------------------------------------------------------------------------------
def test_train_harness_takes_optimiser_steps_over_micro_batches(tmp_path):
    """train.py --grad-accum-steps 2: two optimiser steps of two micro-batches each; steps, the checkpoint and the log count optimiser
    steps, config.yaml records K, and the run is reproducible bit for bit."""
    import yaml
    from mapdit_amd import train
    args = ["--synthetic", "--model", "DiT-XS/2", "--num-steps", "2", "--batch-size", "8", "--grad-accum-steps", "2", "--log-every", "1",
            "--ckpt-every", "2", "--ema-snapshot-every", "2", "--num-classes", "10", "--num-lin-warmup", "1", "--start-decay", "2",
            "--precision", "bf16"]
    runs = []
    for tag in ("a", "b"):
        exp = train.main(args + ["--results-dir", str(tmp_path / tag)])
        assert yaml.safe_load(open(os.path.join(exp, "config.yaml")))["grad_accum_steps"] == 2
        log = open(os.path.join(exp, "log.txt")).read()
        assert "(step=0000001) train loss:" in log and "(step=0000002) train loss:" in log and "step=0000003" not in log
        ck = torch.load(os.path.join(exp, "checkpoints", "0000002.pt"), weights_only=True)
        assert all(torch.isfinite(v).all() for v in ck["model"].values())
        runs.append((log.split("training for")[1].split("steps/sec")[0], ck["model"]["blocks.0.attn.qkv_proj.weight"]))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
