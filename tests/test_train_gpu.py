"""Training-step and sampling-loop level tests on the MI355X: the fused Adam + EMA step against three reference
optimiser steps (fixture optim3), the hipGraph-captured sampler, and the train.py-shaped harness."""
import os

import numpy as np
import pytest
import torch

from conftest import golden_cfg, load_golden, rel_err, sub

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("precision,wtol,ltol", [("bf16", 5e-3, 2e-2), ("f16", 1e-3, 2e-3), ("bf16x3", 2e-4, 1e-4)])
def test_three_optimizer_steps_match_reference(precision, wtol, ltol):
    """forward + backward + Adam(lr 1e-2, betas (0.9, 0.99)) + 2 power-EMA copies, three steps, vs the reference's
    weights after each step.  bf16 gradients feed Adam's sign-like early updates, so weights are compared at 5e-3
    (the update itself is ~1e-2 per element) and EMA copies likewise; in bf16x3 precision (fp32-accurate forward and
    backward) the three-step trajectory follows the reference's to 2e-4."""
    from oracle import dit_oracle as O
    from mapdit_amd.diffusion import create_diffusion
    from mapdit_amd.optim import FusedAdamEMA
    from mapdit_amd.src.dit import DiT
    g = load_golden("optim3")
    cfg = golden_cfg(g)
    sd = O.init_state_dict(cfg, seed=5, gains=0.2, perturb_reference=0.3)
    m = DiT(**cfg.to_dict())
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    m.gemm_precision = precision
    m.y_embedder.token_drop = lambda labels, force_drop_ids=None: labels
    opt = FusedAdamEMA(m, lr=1e-2, betas=(0.9, 0.99), ema_stds=(0.05, 0.1))
    diff = create_diffusion("")
    keys = [k[len("s1/w/"):] for k in g if k.startswith("s1/w/")]
    params = dict(m.named_parameters())
    for step in (1, 2, 3):
        x, y, t, noise, drop = (torch.from_numpy(g[f"s{step}/{n}"]).to(DEV) for n in ("x", "y", "t", "noise", "drop"))
        y_eff = torch.where(drop, torch.full_like(y, cfg.num_classes), y)
        loss = diff.training_losses(m, x, t, dict(y=y_eff), noise=noise)["loss"].mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        assert abs(loss.item() - float(g[f"s{step}/loss"])) < ltol * abs(float(g[f"s{step}/loss"]))
        worst = 0.0
        for k in keys:
            e = rel_err(sub(params[k].detach()), g[f"s{step}/w/{k}"])
            worst = max(worst, e)
            assert e < wtol, (step, k, e)
            for std in (0.05, 0.1):
                ema = opt.ema_state_dict(std)[k]
                assert rel_err(sub(ema), g[f"s{step}/ema{std}/{k}"]) < wtol, (step, k, std)
        print(f"{precision} step {step}: worst weight rel err {worst:.2e}")


@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_graphed_sampler_matches_eager_step(precision):
    from oracle import dit_oracle as O
    from mapdit_amd.diffusion import create_diffusion
    from mapdit_amd.sampling import GraphedSampler
    from mapdit_amd.src.dit import DiT
    cfg = O.DiTConfig(depth=2, hidden_size=128, patch_size=2, input_size=16, in_channels=4, num_heads=2, num_classes=10)
    m = DiT(**cfg.to_dict())
    m.load_state_dict(O.init_state_dict(cfg, seed=9, gains=0.3, perturb_reference=0.3))
    m = m.to(DEV).eval()
    m.gemm_precision = precision
    d = create_diffusion("250")
    n = 4
    g = torch.Generator().manual_seed(3)
    z = torch.randn(n, 4, 16, 16, generator=g)
    z = torch.cat([z, z], 0).to(DEV)
    y = torch.cat([torch.randint(0, 10, (n,), generator=g), torch.full((n,), 10)]).to(DEV)
    s = GraphedSampler(m, d, z.shape, y, cfg_scale=1.5)
    # the final step (t = 0) adds no noise: one graph replay must equal the eager step exactly
    s.img.copy_(z)
    s.t.fill_(0)
    s.graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        t0 = torch.zeros(2 * n, dtype=torch.int64, device=DEV)
        mo = d._wrap_model(m.forward_with_cfg)(z, t0, y=y, cfg_scale=1.5)
        ref, _ = d._step_math(mo, z, t0, torch.zeros_like(z), False)
    assert torch.equal(s.img, ref)
    assert int(s.t[0]) == -1
    # a short prefix of the chain from t = 249 stays finite and the step counter runs down on the device
    out = s.sample(z, steps=3)
    assert torch.isfinite(out).all() and int(s.t[0]) == 249 - 3


def test_train_harness_synthetic(tmp_path):
    from mapdit_amd import train
    exp = train.main(["--synthetic", "--results-dir", str(tmp_path), "--model", "DiT-XS/2", "--num-steps", "4", "--batch-size", "8",
                      "--log-every", "2", "--ckpt-every", "4", "--ema-snapshot-every", "4", "--num-classes", "10",
                      "--num-lin-warmup", "2", "--start-decay", "3"])     # the defaults (steps//150, steps//10) are 0 here
    assert os.path.basename(exp) == "000-DiT-XS-2"
    assert os.path.exists(os.path.join(exp, "config.yaml"))
    ck = torch.load(os.path.join(exp, "checkpoints", "0000004.pt"), weights_only=True)
    assert "blocks.0.attn.qkv_proj.weight" in ck["model"]
    snap = torch.load(os.path.join(exp, "ema", "0.050_0000004.pt"), weights_only=True)
    assert snap["std"] == 0.05 and snap["t"] == 4 and snap["state_dict"]["x_embedder.weight"].dtype == torch.float16
    log = open(os.path.join(exp, "log.txt")).read()
    assert "(step=0000004) train loss:" in log and "train steps/sec:" in log
    with pytest.raises(NotImplementedError):
        train.main(["--synthetic", "--results-dir", str(tmp_path), "--no-use-no-layernorm", "--use-rotation-modulation", "--num-steps", "2"])
    # the fp32-accurate engine through the same harness
    exp2 = train.main(["--synthetic", "--results-dir", str(tmp_path), "--model", "DiT-XS/2", "--num-steps", "2", "--batch-size", "8",
                       "--log-every", "1", "--ckpt-every", "2", "--ema-snapshot-every", "2", "--num-classes", "10",
                       "--num-lin-warmup", "1", "--start-decay", "2", "--precision", "bf16x3"])
    assert "(step=0000002) train loss:" in open(os.path.join(exp2, "log.txt")).read()


@pytest.mark.parametrize("precision", ["bf16", "f16", "bf16x3"])
def test_staged_backward_equals_monolithic(monkeypatch, precision):
    """The data-parallel path runs backward stage by stage (hooking the all-reduce in between); with one rank the
    gradients must be bit-identical to the single-call backward, and the stage slices must tile the flat buffer."""
    from oracle import dit_oracle as O
    from mapdit_amd.diffusion import create_diffusion
    from mapdit_amd.parallel import OverlappedGradReducer, stage_slices
    from mapdit_amd.src.dit import DiT
    g = load_golden("tiny_b")
    cfg = golden_cfg(g)
    sd = O.init_state_dict(cfg, seed=3, gains=0.3, perturb_reference=0.5)
    x, t, y, noise = (torch.from_numpy(g[n]).to(DEV) for n in ("x", "t", "y_eff", "noise"))
    grads = []
    for staged in (False, True):
        m = DiT(**cfg.to_dict())
        m.load_state_dict(sd)
        m = m.to(DEV).eval()                  # eval: weights are not rewritten, both runs see identical weights
        m.gemm_precision = precision
        seen = []
        if staged:
            monkeypatch.setenv("MAPDIT_FORCE_STAGED_BACKWARD", "1")
            r = OverlappedGradReducer(m)
            inner = m._stage_hook
            m._stage_hook = lambda s: (seen.append(s), inner(s))
        create_diffusion("").training_losses(m, x, t, dict(y=y), noise=noise)["loss"].mean().backward()
        if staged:
            r.finish()
            assert seen == list(range(cfg.depth + 2))
            sl = sorted(stage_slices(m))
            assert sl[0][0] == 0 and sl[-1][1] == m._pflat.numel() and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
        torch.cuda.synchronize()
        grads.append(m._gflat.clone())
    assert torch.equal(grads[1], grads[0])         # no atomics anywhere in the step: bit-identical


@pytest.mark.parametrize("precision", ["bf16", "f16", "bf16x3"])
def test_training_is_bit_reproducible(precision):
    """Same seeds -> same bits: five optimiser steps (label drops, repeated labels in the batch, split-K weight gradients, scalar
    gain reductions, fused Adam/EMA) run twice give identical losses and identical weights.  Nothing in the step uses atomics."""
    from mapdit_amd.diffusion import create_diffusion
    from mapdit_amd.optim import FusedAdamEMA
    from mapdit_amd.src.models import DIT_MODELS

    def run():
        torch.manual_seed(11)
        m = DIT_MODELS["DiT-XS/2"](in_channels=4, input_size=32, num_classes=5).to(DEV).train()   # 5 classes: rows shared by samples
        m.gemm_precision = precision
        opt = FusedAdamEMA(m, lr=1e-2, betas=(0.9, 0.99), ema_stds=(0.05, 0.1))
        diff = create_diffusion("")
        g = torch.Generator(device=DEV).manual_seed(12)
        losses = []
        for _ in range(5):
            x = torch.randn(24, 4, 32, 32, device=DEV, generator=g)
            y = torch.randint(0, 5, (24,), device=DEV, generator=g)
            t = torch.randint(0, 1000, (24,), device=DEV, generator=g)
            loss = diff.training_losses(m, x, t, dict(y=y))["loss"].mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        return torch.stack(losses), m._pflat.clone(), m._gflat.clone()

    a, b = run(), run()
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[1], b[1])


def test_bench_two_ranks_on_one_gpu():
    """The N > 1 path of bench.py end to end (rendezvous, per-rank data seeds, staged backward with one all-reduce per stage,
    fused optimiser with the 1/world gradient scale, max-over-ranks timing, rank-0 JSON) with two ranks sharing this box's one
    GPU.  The collective runs on gloo here (RCCL needs one GPU per rank); everything else is the code the 8-GPU run executes."""
    import json
    import socket
    import subprocess
    import sys
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MAPDIT_DIST_BACKEND="gloo", MAPDIT_FORCE_DEVICE="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--global-batch", "32", "--model", "DiT-S/2", "--full"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                 # exactly one JSON line, from rank 0
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["global_batch"] == 32 and d["config"]["parallelism"] == "dp2"
    assert d["config"]["per_gpu_batch"] == 16 and d["metric"].endswith("@32") and d["ms_per_step_median"] > 0
    assert d["parity"] is not None and d["parity"]["logits_rel"] < 3e-2
    assert d["value"] > 0 and d["steps"] == 2 and "cpu_baseline" not in d
    assert d["config"]["final_loss"] == d["config"]["final_loss"]          # not NaN


def _run_dp(tmp_path, tag, world, mode, precision, steps=3, rccl=False):
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / tag
    out.mkdir()
    env = dict(os.environ, MAPDIT_DIST_BACKEND="gloo")
    if rccl:                                               # one GPU per rank, RCCL: the product's multi-GPU path
        env.update(MAPDIT_DIST_BACKEND="nccl", MAPDIT_DP_DEVICE_PER_RANK="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    worker = os.path.join(root, "tests", "dp_worker.py")
    if world == 1:
        cmd = [sys.executable, worker, str(out), mode, precision, str(steps)]
        env.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    else:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr",
               "127.0.0.1", "--master-port", str(port), worker, str(out), mode, precision, str(steps)]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return [torch.load(out / f"rank{i}.pt", weights_only=False) for i in range(world)]


@pytest.mark.parametrize("mode", ["allreduce", "zero1", "zero1w"])
def test_two_rank_overflow_is_refused_on_every_rank(tmp_path, monkeypatch, mode):
    """fp16 engine, two data-parallel ranks: the SECOND rank's loss is blown up in the second of three steps, its gradients overflow.
    The non-finite guard looks at the REDUCED gradients (all-reduce: inf / NaN reaches every rank with the sum; ZeRO-1: each rank checks
    its own parts and the verdict word is all-reduced), so both ranks must refuse that step: replicas stay bit-identical and finite,
    one refused step on each, and the run equals a two-step run without the bad step on those weights up to the data it skipped."""
    monkeypatch.setenv("MAPDIT_TEST_OVERFLOW", "1:1")
    r = _run_dp(tmp_path, "ovf", 2, mode, "f16")
    for k in ("p", "m", "v", "e0", "e1"):
        assert torch.equal(r[0][k], r[1][k]), f"replicas differ in {k} after a refused step"
        assert torch.isfinite(r[0][k]).all(), k
    assert r[0]["refused"] == 1 and r[1]["refused"] == 1
    monkeypatch.delenv("MAPDIT_TEST_OVERFLOW")
    clean = _run_dp(tmp_path, "clean", 2, mode, "f16")
    assert clean[0]["refused"] == 0 and not torch.equal(clean[0]["p"], r[0]["p"])


@pytest.mark.parametrize("precision", ["bf16", "f16", "bf16x3"])
def test_two_rank_data_parallel_matches_single_process(tmp_path, precision):
    """Two data-parallel ranks (different halves of a fixed global batch each; gloo collectives, both ranks on this box's one
    GPU) against ONE process on the whole batch, three optimiser steps, for both gradient exchanges:

    * the overlapped per-stage all-reduce relies on every stage's gradient slice being FINAL when its all-reduce is issued and
      on no later stage writing into it: a write-after-reduce or a wrong slice shows up here as a gradient / weight mismatch
      (a one-rank group cannot see it: its all-reduce is an identity);
    * replicas must hold the same bits after the run (forced weight normalisation is a function of the weights alone);
    * ZeRO-1 (reduce-scatter, sharded Adam + EMA, all-gather) must produce the bits of the replicated optimiser.

    Reduced gradients / weights vs the single process: summation order differs (mean of two half-batch means), so 2e-5 on the
    fp32-accurate engine; the bf16 engine computes each sample independently of its batch, same bound on gradients of 1e-4."""
    ar = _run_dp(tmp_path, "ar", 2, "allreduce", precision)
    z1 = _run_dp(tmp_path, "z1", 2, "zero1", precision)
    for k in ("p", "g", "m", "v", "e0", "e1"):
        assert torch.equal(ar[0][k], ar[1][k]), f"allreduce replicas differ in {k}"
        assert torch.equal(z1[0][k], z1[1][k]), f"zero1 replicas differ in {k}"
    # the sharded optimiser is the replicated one, bit for bit (same reduced gradients: gloo's all-reduce on both paths)
    for k in ("p", "m", "v", "e0", "e1"):
        if not torch.equal(z1[0][k], ar[0][k]):
            d = (z1[0][k] - ar[0][k]).abs()
            idx = torch.nonzero(d > 0).flatten()
            raise AssertionError(f"zero1 != replicated optimiser in {k}: {idx.numel()} of {d.numel()} elements differ, max abs {d.max():.3e}, "
                                 f"first at {idx[:5].tolist()} last at {idx[-5:].tolist()}; grads equal: {torch.equal(z1[0]['g'], ar[0]['g'])}; "
                                 f"shards {z1[0]['shards']}")
    assert z1[0]["shards"] != z1[1]["shards"] and len(z1[0]["shards"]) == 6 + 2        # DiT-XS: 6 blocks + final + embedders
    # against ONE process on the whole batch.  After the first step only the summation order differs (identical weights in).
    # Over several steps the bf16 engine amplifies that 1e-7 through bf16 re-rounding of the re-normalised weights (a flipped
    # rounding is a 2^-9 change: DESIGN.md section 2), so its multi-step comparison is loose; the fp32-accurate engine stays tight.
    single1 = _run_dp(tmp_path, "w1s1", 1, "allreduce", precision, steps=1)[0]
    ar1 = _run_dp(tmp_path, "ars1", 2, "allreduce", precision, steps=1)[0]
    for k in ("g", "p", "m", "e0"):
        e = rel_err(ar1[k].numpy(), single1[k].numpy())
        print(f"{precision}: 2-rank all-reduce vs single process after 1 step, {k}: {e:.2e}")
        # f16: a rank's mean loss over 8 samples hands the backward twice the gradient the single process' mean over 16 does - a power
        # of two, exact except where fp16 activation gradients go subnormal: the loss-scale invariance bound of test_f16_gpu.py (2e-4)
        assert e < (2e-4 if precision == "f16" else 2e-5), (k, e)
    single3 = _run_dp(tmp_path, "w1s3", 1, "allreduce", precision)[0]
    tol = 2e-5 if precision == "bf16x3" else 2e-2
    for k in ("g", "p", "m", "e0"):
        e = rel_err(ar[0][k].numpy(), single3[k].numpy())
        print(f"{precision}: 2-rank all-reduce vs single process after 3 steps, {k}: {e:.2e}")
        assert e < tol, (k, e)


def test_block_fences_order_the_forward_behind_the_host_s_gathers():
    """mapdit_engine_set_block_fences (round 5: under sharded weight passes the host all-gathers the weight images block by block and the
    forward waits for block i's gather just before block i).  Mechanics on one GPU: a side stream REWRITES block 1's fc1 image late - after
    a delay - and records that block's event; the fenced forward must see the rewritten image (it waited), must equal the forward that
    ran after a full synchronise, and the fences are one-shot (the next forward does not wait for anything)."""
    import ctypes as C
    import time
    from oracle import dit_oracle as O
    from mapdit_amd import _lib as Lib
    from mapdit_amd.src.dit import DiT
    cfg = O.DiTConfig(depth=3, hidden_size=128, patch_size=2, input_size=16, in_channels=4, num_heads=2, num_classes=10)
    m = DiT(**cfg.to_dict())
    m.load_state_dict(O.init_state_dict(cfg, seed=3, gains=0.3))
    m = m.to(DEV).train()
    m.gemm_precision = "bf16"
    m.y_embedder.token_drop = lambda labels, force_drop_ids=None: labels
    g = torch.Generator().manual_seed(1)
    x, t, y = torch.randn(4, 4, 16, 16, generator=g).to(DEV), torch.randint(0, 1000, (4,), generator=g).to(DEV), torch.randint(0, 10, (4,), generator=g).to(DEV)
    m(x, t, y)                                              # builds the training runtime (and normalises the masters once)
    rt = m._rt[True]
    img, img3, rows, cols, sh = C.c_void_p(), C.c_void_p(), C.c_int(), C.c_int(), C.c_int()
    pidx = Lib.NUM_GLOBAL + 1 * Lib.NUM_BLOCK + Lib.B_FC1
    rt.lib.engine_weight_image(rt.handle, pidx, C.byref(img), C.byref(img3), C.byref(rows), C.byref(cols), C.byref(sh))
    off = img.value - rt.workspace.data_ptr()
    view = rt.workspace[off:off + rows.value * cols.value * 2].view(torch.bfloat16)
    assert sh.value == 0 and rows.value == 512 and cols.value == 128

    def plain_forward():
        with torch.cuda.device(DEV):
            rt.lib.engine_prepare_weights(rt.handle, 0, Lib.cur_stream())       # (no rewrite: the same images every time)
            out = torch.empty(4, 8, 16, 16, device=DEV)
            rt.lib.engine_forward(rt.handle, x.data_ptr(), t.data_ptr(), y.data_ptr(), 4, 0, out.data_ptr(), Lib.cur_stream())
        torch.cuda.synchronize()
        return out

    base = plain_forward()

    def forward_with_late_rewrite(fenced):
        # the weight pass of this forward re-images everything first (hook-free: call it here, then run the network only)
        with torch.cuda.device(DEV):
            rt.lib.engine_prepare_weights(rt.handle, 0, Lib.cur_stream())
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        evs = [torch.cuda.Event() for _ in range(3)]
        with torch.cuda.stream(side):
            evs[0].record(side)
            torch.cuda._sleep(200_000_000)                   # ~0.1 s: far longer than the whole tiny forward
            view.mul_(2.0)                                   # "the gather of block 1 lands"
            evs[1].record(side)
            evs[2].record(side)
        if fenced:
            handles = (C.c_void_p * 3)(*[e.cuda_event for e in evs])
            rt.lib.engine_set_block_fences(rt.handle, handles, 3)
        else:
            torch.cuda.synchronize()
        out = torch.empty(4, 8, 16, 16, device=DEV)
        with torch.cuda.device(DEV):
            rt.lib.engine_forward(rt.handle, x.data_ptr(), t.data_ptr(), y.data_ptr(), 4, 0, out.data_ptr(), Lib.cur_stream())
        torch.cuda.synchronize()
        return out

    late = forward_with_late_rewrite(fenced=True)
    ref = forward_with_late_rewrite(fenced=False)
    assert torch.equal(late, ref) and not torch.equal(late, base), "the fenced forward must have waited for block 1's image"
    t0 = time.time()
    again = plain_forward()                                  # one-shot: nothing left to wait for, and the images are the plain ones again
    assert torch.equal(again, base) and time.time() - t0 < 5.0


def test_rccl_calls_of_the_sharded_pass_path_run_with_one_rank():
    """What a one-GPU box CAN run of parallel.ShardedPassReducer's RCCL path (tools/rccl_api_probe.py, own process): the grouped in-place
    reduce_scatter_tensor of a stage, the grouped all_gather_into_tensor on byte views with a side stream turning its completion into an
    event, the asynchronous all_to_all_single of the 16-bit exchange and the MAX all-reduce of the verdict words - through RCCL and torch's
    coalescing manager with world size 1 (identities).  More than one rank has never run: no multi-GPU node was available to any round."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_PORT="29611", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "rccl_api_probe.py")], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rccl api probe ok" in r.stdout, r.stderr[-2000:]


def test_side_stream_jacobians_give_the_same_bits(tmp_path, monkeypatch):
    """MAPDIT_SIDE_JAC=1 (round 5, opt-in: measured slower): the weight-norm Jacobians on the engine's side stream
    (48-register kernel, ping-pong slab buffers, event hand-over, join at the end of every backward call) must be an ordering change
    only - the same gradients, weights and optimiser state bit for bit after three steps, single process and staged (two-rank) backward."""
    base = _run_dp(tmp_path, "base", 1, "allreduce", "bf16")[0]
    base2 = _run_dp(tmp_path, "base2", 2, "allreduce", "f16")
    monkeypatch.setenv("MAPDIT_SIDE_JAC", "1")
    side = _run_dp(tmp_path, "side", 1, "allreduce", "bf16")[0]
    side2 = _run_dp(tmp_path, "side2", 2, "allreduce", "f16")
    for k in ("p", "g", "m", "v", "e0", "e1"):
        assert torch.equal(base[k], side[k]), k
        assert torch.equal(base2[0][k], side2[0][k]) and torch.equal(side2[0][k], side2[1][k]), k


@pytest.mark.parametrize("width", ["xl", "b"])
@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_grouped_weight_gradient_launch_equals_single_launches(tmp_path, precision, width):
    """Round 5: at DiT-XL's width and 64 samples the fc2 / fc1 / QKV weight gradients of a block run as ONE launch without a K cut (250 tiles
    against 180 + 180 + 210 workgroups: engine.hip dw_group_split).  Same products, another summation order (one slab instead of two or three):
    every gradient equals the launch-each run (MAPDIT_DW_GROUP=0) to fp32 rounding, the grouped weights' gradients are NOT the same bits (the
    grouped path did run), everything else is.  width "b": DiT-B's width at 32 samples, where the cost model groups all four gradients of a block
    (99 + 9 tiles x 2 slabs of the 256^2 kernel against four launches of the 128^2 kernel)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for mode in ("1", "0"):
        out = tmp_path / f"g{mode}.pt"
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "dw_group_worker.py"), str(out), precision, width], cwd=root,
                           env=dict(os.environ, MAPDIT_DW_GROUP=mode), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        res[mode] = torch.load(out, weights_only=False)
    assert res["1"]["loss"] == res["0"]["loss"]
    differ = 0
    for k, g1 in res["1"]["grads"].items():
        g0 = res["0"]["grads"][k]
        names = ("mlp.net.0.weight", "mlp.net.2.weight", "qkv_proj.weight") + (("out_proj.weight",) if width == "b" else ())
        grouped = any(s in k for s in names) and k.startswith("blocks.")
        if grouped:
            differ += int(not torch.equal(g0, g1))
            assert rel_err(g1.numpy(), g0.numpy()) < 2e-6, k
        else:
            assert torch.equal(g0, g1), k
    assert differ >= (4 if width == "xl" else 6), "the grouped launch did not run (same bits everywhere)"


@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_two_rank_sharded_weight_passes(tmp_path, precision):
    """--grad-comm zero1w / zero1w-bf16 (round 5): two ranks (gloo collectives, both on this box's GPU), the rows of every block linear
    split between them - each rank rewrites / images, differentiates (Jacobian), steps (Adam + EMA) ITS rows only; raw weight gradients are
    exchanged per stage, 16-bit images all-gathered before the next forward.  After gather_state the replicas hold the same bits, and the run
    equals the replicated all-reduce run up to the order of Jacobian and rank sum (a linear map: fp32 rounding only) - resp., for the 16-bit
    exchange, up to one bf16 rounding of each rank's raw gradient."""
    ar = _run_dp(tmp_path, "ar", 2, "allreduce", precision, steps=1)
    for mode, tol in (("zero1w", 2e-5), ("zero1w-bf16", 2e-3)):
        zw = _run_dp(tmp_path, mode, 2, mode, precision, steps=1)
        for k in ("p", "m", "v", "e0", "e1"):
            assert torch.equal(zw[0][k], zw[1][k]), f"{mode}: replicas differ in {k} after gather_state"
            assert torch.isfinite(zw[0][k]).all(), k
            e = rel_err(zw[0][k].numpy(), ar[0][k].numpy())
            print(f"{precision} {mode} vs all-reduce after 1 step, {k}: {e:.2e}")
            assert e < tol, (mode, k, e)
        assert zw[0]["shards"] != zw[1]["shards"]
    # three steps: the sharded run keeps training like the replicated one (bf16 re-rounding of re-normalised weights amplifies 1e-7: loose)
    ar3 = _run_dp(tmp_path, "ar3", 2, "allreduce", precision)
    zw3 = _run_dp(tmp_path, "zw3", 2, "zero1w", precision)
    for k in ("p", "m", "e0"):
        assert torch.equal(zw3[0][k], zw3[1][k])
        e = rel_err(zw3[0][k].numpy(), ar3[0][k].numpy())
        print(f"{precision} zero1w vs all-reduce after 3 steps, {k}: {e:.2e}")
        assert e < 2e-2, (k, e)
    assert abs(zw3[0]["loss"] - zw3[1]["loss"]) < 1.0 and zw3[0]["refused"] == 0


def test_two_rank_runs_with_the_grouped_weight_gradient_launch(tmp_path, monkeypatch):
    """Two ranks of 32 samples each on a two-block model of DiT-B's width: at that shape every block's four weight gradients leave in ONE grouped
    launch inside the block's backward stage (engine.hip dw_group_split), so the per-stage all-reduce / reduce-scatter of the reducers must still see
    final gradient slices: replicas bit-identical, the three exchanges agree (all-reduce == ZeRO-1 bit for bit, sharded weight passes to fp32
    rounding), and the two-rank step equals the launch-each run (MAPDIT_DW_GROUP=0) to summation order."""
    monkeypatch.setenv("MAPDIT_TEST_DIT_KW", '{"depth": 2, "hidden_size": 768, "num_heads": 12}')
    monkeypatch.setenv("MAPDIT_TEST_BATCH", "64")
    ar = _run_dp(tmp_path, "ar", 2, "allreduce", "f16", steps=1)
    z1 = _run_dp(tmp_path, "z1", 2, "zero1", "f16", steps=1)
    zw = _run_dp(tmp_path, "zw", 2, "zero1w", "f16", steps=1)
    for k in ("p", "m", "v", "e0", "e1"):
        assert torch.equal(ar[0][k], ar[1][k]) and torch.equal(zw[0][k], zw[1][k]), k
        assert torch.equal(z1[0][k], ar[0][k]), k
        assert rel_err(zw[0][k].numpy(), ar[0][k].numpy()) < 2e-5, k
    monkeypatch.setenv("MAPDIT_DW_GROUP", "0")
    each = _run_dp(tmp_path, "each", 2, "allreduce", "f16", steps=1)
    assert not torch.equal(each[0]["g"], ar[0]["g"]), "the grouped launch did not run at this shape"
    for k in ("g", "p", "m"):
        assert rel_err(each[0][k].numpy(), ar[0][k].numpy()) < 2e-5, k


def test_two_rank_sharded_weight_passes_with_off_forms(tmp_path, monkeypatch):
    """The README off forms that touch the weight passes and the block's structure (weight normalisation off: MAPDIT_WN_PLAIN in the sharded
    imaging and Jacobian jobs; plain attention; the LayerNorm form) under --grad-comm zero1w, two ranks: replicas bit-identical after gather_state
    and equal to the replicated all-reduce run of the same network up to fp32 rounding."""
    monkeypatch.setenv("MAPDIT_TEST_MODEL_KW", '{"weight_normalization": false, "cosine_attention": false, "no_layernorm": false}')
    ar = _run_dp(tmp_path, "ar", 2, "allreduce", "f16", steps=1)
    zw = _run_dp(tmp_path, "zw", 2, "zero1w", "f16", steps=1)
    for k in ("p", "m", "v", "e0", "e1"):
        assert torch.equal(zw[0][k], zw[1][k]) and torch.isfinite(zw[0][k]).all(), k
        assert rel_err(zw[0][k].numpy(), ar[0][k].numpy()) < 2e-5, k
    monkeypatch.delenv("MAPDIT_TEST_MODEL_KW")
    on = _run_dp(tmp_path, "on", 2, "allreduce", "f16", steps=1)
    assert not torch.equal(on[0]["p"], ar[0]["p"])            # (the flags reached the workers: another network)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: RCCL with more than one rank")
def test_two_gpu_rccl_data_parallel(tmp_path):
    """The same two-rank run with ONE GPU PER RANK and RCCL collectives (the in-place all_gather_into_tensor /
    reduce_scatter_tensor forms of parallel.py, which a one-GPU box can only exercise with one rank): replicas bit-identical, ZeRO-1
    equal to the replicated optimiser, gathered EMA / optimiser state verified by the owners' checksums (parallel._verify_gather),
    and the result equal to the single process on the whole batch."""
    ar = _run_dp(tmp_path, "ar", 2, "allreduce", "bf16", rccl=True)
    z1 = _run_dp(tmp_path, "z1", 2, "zero1", "bf16", rccl=True)
    for k in ("p", "g", "m", "v", "e0", "e1"):
        assert torch.equal(ar[0][k], ar[1][k]), f"allreduce replicas differ in {k}"
        assert torch.equal(z1[0][k], z1[1][k]), f"zero1 replicas differ in {k}"
    for k in ("p", "m", "v", "e0", "e1"):      # (RCCL's ring all-reduce and reduce-scatter may add in different orders: not bit for bit)
        assert rel_err(z1[0][k].numpy(), ar[0][k].numpy()) < 1e-5, k
    single1 = _run_dp(tmp_path, "w1s1", 1, "allreduce", "bf16", steps=1)[0]
    ar1 = _run_dp(tmp_path, "ars1", 2, "allreduce", "bf16", steps=1, rccl=True)[0]
    for k in ("g", "p", "m", "e0"):
        assert rel_err(ar1[k].numpy(), single1[k].numpy()) < 2e-5, k


def test_ema_class_matches_fused_optimizer(tmp_path):
    """The reference-style loop (torch.optim.Adam + EMA helper, train.py:57,94-105) on this engine gives the same weights and
    the same EMA copies as the fused optimiser kernel, and the helper's snapshots are the reference's files."""
    from oracle import dit_oracle as O
    from mapdit_amd.diffusion import create_diffusion
    from mapdit_amd.optim import FusedAdamEMA
    from mapdit_amd.src.dit import DiT
    from mapdit_amd.src.ema import EMA, calculate_posthoc_ema
    cfg = O.DiTConfig(depth=1, hidden_size=128, patch_size=4, input_size=32, in_channels=4, num_heads=2, num_classes=10)
    sd = O.init_state_dict(cfg, seed=5, gains=0.2, perturb_reference=0.3)
    diff = create_diffusion("")
    g = torch.Generator().manual_seed(0)
    batches = [(torch.randn(4, 4, 32, 32, generator=g).to(DEV), torch.randint(0, 10, (4,), generator=g).to(DEV),
                torch.randint(0, 1000, (4,), generator=g).to(DEV), torch.randn(4, 4, 32, 32, generator=g).to(DEV)) for _ in range(3)]
    models = []
    for fused in (True, False):
        m = DiT(**cfg.to_dict())
        m.load_state_dict(sd)
        m = m.to(DEV).train()
        m.gemm_precision = "f16"        # explicit: the default engine (both loops run the same engine; only the optimiser differs)
        m.y_embedder.token_drop = lambda labels, force_drop_ids=None: labels
        if fused:
            opt = FusedAdamEMA(m, lr=1e-2, betas=(0.9, 0.99), ema_stds=(0.05, 0.1))
            ema = None
        else:
            opt = torch.optim.Adam(m.parameters(), lr=1e-2, betas=(0.9, 0.99))
            ema = EMA(m, str(tmp_path), stds=[0.05, 0.1])
        for step, (x, y, t, noise) in enumerate(batches, start=1):
            loss = diff.training_losses(m, x, t, dict(y=y), noise=noise)["loss"].mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
            if ema is not None:
                m.mark_weights_changed()
                ema.update(step, m)
        models.append((m, opt, ema))
    (mf, of, _), (mt, _, ema) = models
    for (k, a), (_, b) in zip(mf.named_parameters(), mt.named_parameters()):
        # same gradients in the first step; torch.optim.Adam and the fused kernel round the bias corrections differently (fp32),
        # and from the second step on the bf16 engine turns that 1e-7 into flipped bf16 roundings (measured up to 3.3e-4 on the
        # label table after three steps)
        assert rel_err(sub(a.detach()), sub(b.detach())) < 1e-3, (k, rel_err(sub(a.detach()), sub(b.detach())))
    for std in (0.05, 0.1):
        fused_sd, helper_sd = of.ema_state_dict(std), ema.state_dict(std)
        for k in fused_sd:
            assert rel_err(sub(fused_sd[k]), sub(helper_sd[k])) < 1e-3, (std, k)
    ema.save_snapshot(3)
    snap = torch.load(os.path.join(str(tmp_path), "ema", "0.050_0000003.pt"), weights_only=True)
    assert snap["std"] == 0.05 and snap["t"] == 3 and snap["state_dict"]["x_embedder.weight"].dtype == torch.float16
    back = calculate_posthoc_ema(0.05, os.path.join(str(tmp_path), "ema"), verbose=False)
    assert torch.equal(back["x_embedder.weight"], snap["state_dict"]["x_embedder.weight"])


def test_overlapped_reducer_through_rccl_single_rank():
    """The data-parallel step with a REAL RCCL process group (one rank: every all-reduce is an identity, but it runs RCCL's
    kernels on RCCL's stream against the engine's raw-stream kernels): staged backward -> per-stage async all-reduce of the
    gradient slice -> finish() -> fused optimiser.  Gradients and updated weights must be the bits of the plain single-GPU
    step."""
    import torch.distributed as dist
    from oracle import dit_oracle as O
    from mapdit_amd.diffusion import create_diffusion
    from mapdit_amd.optim import FusedAdamEMA
    from mapdit_amd.parallel import OverlappedGradReducer
    from mapdit_amd.src.dit import DiT
    g = load_golden("tiny_b")
    cfg = golden_cfg(g)
    sd = O.init_state_dict(cfg, seed=3, gains=0.3, perturb_reference=0.5)
    x, t, y, noise = (torch.from_numpy(g[n]).to(DEV) for n in ("x", "t", "y_eff", "noise"))
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29541", rank=0, world_size=1)
    try:
        outs = []
        for through_rccl in (False, True):
            m = DiT(**cfg.to_dict())
            m.load_state_dict(sd)
            m = m.to(DEV).train()
            m.gemm_precision = "f16"    # explicit: the default engine incl. its non-finite guard on the reduced gradients
            m.y_embedder.token_drop = lambda labels, force_drop_ids=None: labels
            r = OverlappedGradReducer(m, force_collective=through_rccl)
            opt = FusedAdamEMA(m, lr=1e-2, grad_scale=r.grad_scale)
            for _ in range(2):
                loss = create_diffusion("").training_losses(m, x, t, dict(y=y), noise=noise)["loss"].mean()
                opt.zero_grad()
                loss.backward()
                r.finish()
                opt.step()
            torch.cuda.synchronize()
            outs.append((m._gflat.clone(), m._pflat.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    finally:
        if created:
            dist.destroy_process_group()
