"""Gradient accumulation, the parts that need no GPU: the harness' --grad-accum-steps, no_sync() of the data-parallel reducers, and the
premise of the GPU comparison against the reference's gradients (two half-batches, each mean / 2, add up to the whole batch's gradient)."""
import pytest
import torch

from conftest import golden_cfg, golden_state_dict, load_golden, rel_err, sub


def test_parser_accepts_grad_accum_steps_and_ragged_splits_are_rejected_early(monkeypatch, tmp_path):
    from mapdit_amd import parallel, train
    base = ["--synthetic", "--results-dir", str(tmp_path)]
    assert train.build_parser().parse_args(base).grad_accum_steps == 1
    assert train.build_parser().parse_args(base + ["--grad-accum-steps", "8"]).grad_accum_steps == 8
    assert train.micro_batch(256, 1, 8) == 32 and train.micro_batch(256, 8, 4) == 8 and train.micro_batch(24, 1, 1) == 24

    def no_device_work(*a, **k):
        raise AssertionError("the split must be checked before the process group / the device is touched")

    monkeypatch.setattr(parallel, "init_from_env", no_device_work)
    monkeypatch.setattr(torch.cuda, "set_device", no_device_work)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(ValueError, match="grad-accum-steps 4 does not divide the per-rank batch 6"):
        train.main(base + ["--batch-size", "6", "--grad-accum-steps", "4"])
    with pytest.raises(ValueError, match="grad-accum-steps"):
        train.main(base + ["--batch-size", "8", "--grad-accum-steps", "0"])
    monkeypatch.setenv("WORLD_SIZE", "2")                   # 16 over two ranks = 8 per rank: 3 micro-batches do not divide it
    with pytest.raises(ValueError, match="per-rank batch 8"):
        train.main(base + ["--batch-size", "16", "--grad-accum-steps", "3"])
    with pytest.raises(NotImplementedError, match="zero1w"):
        train.main(base + ["--batch-size", "16", "--grad-accum-steps", "2", "--grad-comm", "zero1w"])
    assert not list(tmp_path.iterdir())                     # nothing was set up


class _StubModel:
    """What the reducers read of a model: a flat buffer whose stages (final layer | block 0 | embedders) own one slice each."""
    depth = 1

    def __init__(self):
        sizes = [("final_layer.linear.weight", 64), ("blocks.0.attn.qkv_proj.weight", 96), ("x_embedder.weight", 32)]
        self._pflat = torch.zeros(sum(n for _, n in sizes))
        self._gflat = torch.arange(self._pflat.numel(), dtype=torch.float32)
        self._poffs, self._named, off = [], [], 0
        for name, n in sizes:
            self._poffs.append(off)
            self._named.append((name, self._pflat[off:off + n]))
            off += n

    def named_parameters(self):
        return list(self._named)


class _Work:
    def wait(self):
        return True


@pytest.mark.parametrize("kind", ["allreduce", "zero1"])
def test_no_sync_suppresses_the_stage_hook_and_restores_it(monkeypatch, kind):
    from mapdit_amd import parallel
    calls = []
    monkeypatch.setattr(parallel, "_all_reduce_sum", lambda t, group: (calls.append(t.numel()), _Work())[1])
    m = _StubModel()
    red = (parallel.OverlappedGradReducer if kind == "allreduce" else parallel.Zero1Reducer)(m, force_collective=True)
    hook = m._stage_hook
    assert hook is not None and hook == red._on_stage and red.grad_scale == 1.0
    with red.no_sync() as inside:
        assert inside is red and m._stage_hook is None      # the facade runs the unstaged backward
        for stage in range(m.depth + 2):
            red._on_stage(stage)                            # and a stage hook called anyway exchanges nothing
        red.finish()
        with red.no_sync():                                 # nests
            assert m._stage_hook is None
        assert m._stage_hook is None and not red._sync
    assert calls == [] and red.works == []
    assert m._stage_hook == hook and red._sync
    for stage in range(m.depth + 2):
        m._stage_hook(stage)
    assert calls == [64, 96, 32]                            # outside: every stage's slice, as before
    red.finish()
    with pytest.raises(RuntimeError, match="boom"):         # restored when the body raises, too
        with red.no_sync():
            raise RuntimeError("boom")
    assert m._stage_hook == hook and red._sync


def test_no_sync_of_the_plain_reducer_and_refusal_of_the_sharded_one(monkeypatch):
    from mapdit_amd import parallel
    from mapdit_amd._lib import MapditError
    calls = []
    monkeypatch.setattr(parallel.dist, "all_reduce", lambda t, **kw: (calls.append(t.numel()), _Work())[1])
    red = parallel.GradReducer(n_buckets=2)
    red.world = 2                                           # (as if two ranks: a one-rank reducer never exchanges)
    flat = torch.ones(4096)
    with red.no_sync():
        red.reduce(flat)
    assert calls == []
    red.reduce(flat)
    assert sum(calls) == 4096 and red.grad_scale == 0.5
    sharded = parallel.ShardedPassReducer(_StubModel())
    with pytest.raises(MapditError, match="gradient accumulation is not supported together with sharded weight passes"):
        sharded.no_sync()


def test_oracle_two_half_batches_add_up_to_the_fixture_s_gradients():
    """Premise of the GPU comparison against grad/* (it holds without the feature): the model couples no two samples, so the gradients
    of samples 0-1 and 2-3, each loss.mean() / 2, add up to the whole batch's gradient - here with the CPU oracle on tiny_a, against the
    oracle's own whole-batch gradient to fp32 rounding and against the fixture at the limit tests/test_oracle_golden.py holds the oracle to."""
    from oracle import dit_oracle as O
    from oracle.diffusion_oracle import DiffusionOracle
    g = load_golden("tiny_a")
    cfg = golden_cfg(g)
    sd = golden_state_dict(g, cfg)
    x, y, t = torch.from_numpy(g["x"]), torch.from_numpy(g["y"]), torch.from_numpy(g["t"])
    noise, drop = torch.from_numpy(g["noise"]), torch.from_numpy(g["drop"])
    d = DiffusionOracle("")

    def grads(lo, hi, scale):
        leaf = {k: v.clone().requires_grad_(k not in O.BUFFER_KEYS) for k, v in sd.items()}      # (fresh weights: the training forward rewrites them)
        loss = d.training_losses(lambda xx, tt, **kw: O.dit_forward(leaf, cfg, xx, tt, kw["y"], train=True, drop=drop[lo:hi]),
                                 x[lo:hi], t[lo:hi], dict(y=y[lo:hi]), noise=noise[lo:hi])["loss"].mean() * scale
        loss.backward()
        return {k: v.grad for k, v in leaf.items() if k not in O.BUFFER_KEYS}

    assert x.shape[0] == 4
    a, b, whole = grads(0, 2, 0.5), grads(2, 4, 0.5), grads(0, 4, 1.0)
    for k in whole:
        both = a[k] + b[k]
        if float(whole[k].norm()) > 1e-7:
            assert rel_err(both.numpy(), whole[k].numpy()) < 1e-5, k
        assert rel_err(sub(both), g["grad/" + k]) < 1e-3 or float(whole[k].norm()) < 1e-7, k
