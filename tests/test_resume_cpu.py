"""Host logic of train.py --resume and --step-rng (no device work), and the statistics of the step draws' numpy restatement."""
import math
import os

import numpy as np
import pytest
import torch
import yaml

import step_rng_reference as S


def config_of(argv):
    """What a fresh run of `argv` writes into config.yaml."""
    from mapdit_amd import train
    return yaml.safe_load(yaml.dump(vars(train.build_parser().parse_args(argv))))


def merged(old_argv, new_argv):
    from mapdit_amd import train
    args = train.build_parser().parse_args(new_argv)
    return train.merge_resume_args(args, train.explicit_args(new_argv), config_of(old_argv))


OLD = ["--synthetic", "--results-dir", "/r", "--model", "DiT-S/2", "--num-steps", "3000", "--batch-size", "64", "--step-rng", "counter", "--seed", "5",
       "--log-every", "50"]


def test_parser_knows_the_flags():
    from mapdit_amd import train
    p = train.build_parser()
    a = p.parse_args(["--synthetic"])
    assert a.step_rng == "torch" and a.resume is None and a.results_dir is None
    assert p.parse_args(["--step-rng", "counter", "--resume", "x"]).step_rng == "counter"
    with pytest.raises(SystemExit):
        p.parse_args(["--step-rng", "philox"])
    assert config_of(OLD)["step_rng"] == "counter"
    assert train.explicit_args(["--resume", "x", "--num-steps", "5"]) == {"resume": "x", "num_steps": 5}


def test_resume_takes_the_runs_arguments_and_the_free_ones_from_the_command_line():
    a = merged(OLD, ["--resume", "x"])
    assert (a.model, a.num_steps, a.batch_size, a.step_rng, a.seed, a.log_every, a.synthetic) == ("DiT-S/2", 3000, 64, "counter", 5, 50, True)
    assert a.resume == "x"
    a = merged(OLD, ["--resume", "x", "--num-steps", "9000", "--log-every", "10", "--ckpt-every", "500", "--ema-snapshot-every", "7", "--verbose", "2",
                     "--num-workers", "0", "--grad-comm", "zero1"])
    assert (a.num_steps, a.log_every, a.ckpt_every, a.ema_snapshot_every, a.verbose, a.num_workers, a.grad_comm) == (9000, 10, 500, 7, 2, 0, "zero1")
    assert merged(OLD, ["--resume", "x", "--model", "DiT-S/2", "--seed", "5"]).model == "DiT-S/2"        # the run's own value may be repeated


@pytest.mark.parametrize("flag,value", [("--model", "DiT-B/2"), ("--seed", "6"), ("--batch-size", "128"), ("--step-rng", "torch"), ("--lr", "0.02"),
                                        ("--precision", "bf16"), ("--objective", "flow"), ("--grad-accum-steps", "2"), ("--num-lin-warmup", "7")])
def test_resume_refuses_another_value_of_a_run_defining_argument(flag, value):
    with pytest.raises(ValueError, match=flag + " "):
        merged(OLD, ["--resume", "x", flag, value])


def test_resume_refuses_a_run_on_the_torch_generators():
    old = [a for a in OLD if a not in ("--step-rng", "counter")]
    with pytest.raises(ValueError, match="--step-rng counter"):
        merged(old, ["--resume", "x"])


def test_derived_schedules_follow_the_original_num_steps():
    from mapdit_amd.optim import create_lr_lambda
    a = merged(OLD, ["--resume", "x", "--num-steps", "9000"])
    assert (a.num_lin_warmup, a.start_decay, a.ema_snapshot_every) == (3000 // 150, 3000 // 10, 3000 // 250)
    fresh, cont = create_lr_lambda(3000 // 150, 3000 // 10), create_lr_lambda(a.num_lin_warmup, a.start_decay)
    assert all(fresh(s) == cont(s) for s in (0, 5, 19, 20, 299, 300, 2999, 8999))
    given = merged(OLD + ["--num-lin-warmup", "40", "--start-decay", "1000"], ["--resume", "x", "--num-steps", "9000"])
    assert (given.num_lin_warmup, given.start_decay) == (40, 1000)


def test_an_experiment_directory_resolves_to_its_latest_checkpoint(tmp_path):
    from mapdit_amd import train
    ck = tmp_path / "000-DiT-XS-2" / "checkpoints"
    os.makedirs(ck)
    with pytest.raises(ValueError, match="no checkpoints"):
        train.resolve_checkpoint(str(ck.parent))
    for n in (50000, 100000, 9000000, 10000000):
        (ck / f"{n:07d}.pt").write_bytes(b"")
    (ck / "0000003.pt.a").write_bytes(b"")
    assert train.resolve_checkpoint(str(ck.parent)) == str(ck / "10000000.pt")            # by number, not by name
    assert train.resolve_checkpoint(str(ck / "0050000.pt")) == str(ck / "0050000.pt")
    with pytest.raises(ValueError, match="neither"):
        train.resolve_checkpoint(str(tmp_path / "nothing"))


def test_resume_fails_before_any_device_work(tmp_path, monkeypatch):
    """As train.main's other early checks: on a machine without a GPU these raise their own errors, not torch's."""
    from mapdit_amd import train
    from mapdit_amd._lib import MapditError
    exp = tmp_path / "000-DiT-S-2"
    os.makedirs(exp / "checkpoints")
    with open(exp / "config.yaml", "w") as f:
        yaml.dump(config_of(OLD), f)
    ckpt = str(exp / "checkpoints" / "0000100.pt")
    torch.save({"model": {}, "opt": {}}, ckpt)                                            # a reference checkpoint's keys
    with pytest.raises(ValueError, match="no 'ema' key"):
        train.main(["--resume", ckpt])
    with pytest.raises(ValueError, match="no 'ema' key"):
        train.main(["--resume", str(exp)])
    torch.save({"model": {}, "opt": {}, "ema": {}}, ckpt)
    with pytest.raises(ValueError, match="no 'train_state' key"):
        train.main(["--resume", ckpt])
    torch.save({"model": {}, "opt": {}, "ema": {}, "train_state": {"train_steps": 100}}, ckpt)
    with pytest.raises(ValueError, match="--num-steps 99 lies below the checkpoint's step 100"):
        train.main(["--resume", ckpt, "--num-steps", "99"])
    with pytest.raises(ValueError, match="--model"):
        train.main(["--resume", ckpt, "--model", "DiT-B/2"])
    with pytest.raises(MapditError, match="--resume"):
        train.main(["--resume", ckpt, "--grad-comm", "zero1w"])
    with pytest.raises(MapditError, match="--resume"):
        train.main(["--resume", ckpt, "--grad-comm", "zero1w-bf16"])
    with pytest.raises(ValueError, match="--results-dir is required"):
        train.main(["--synthetic"])


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 1.0])
def test_drop_threshold(p):
    from mapdit_amd.step_rng import drop_threshold
    want = math.ceil(float(np.float32(p)) * 2.0 ** 24)
    assert drop_threshold(p) == want == S.drop_threshold(p)
    # the truth table of torch.rand(fp32) < p for a 24-bit uniform k 2^-24: k < thr exactly where k 2^-24 < float32(p)
    for k in {0, max(want - 1, 0), min(want, (1 << 24) - 1), (1 << 24) - 1}:
        assert (k < want) == bool(np.float32(k * 2.0 ** -24) < np.float32(p)), (p, k)


def test_drop_threshold_refuses_a_probability_outside_the_unit_interval():
    from mapdit_amd.step_rng import drop_threshold
    for p in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            drop_threshold(p)


@pytest.mark.parametrize("world,K", [(1, 1), (2, 2), (4, 1), (8, 4)])
def test_micro_batches_tile_the_global_batch(world, K):
    """first_slot(lo, k, micro) over every rank and micro-batch: each slot of the global batch exactly once, in order."""
    from mapdit_amd import parallel
    from mapdit_amd.step_rng import first_slot
    from mapdit_amd.train import micro_batch
    B = 256
    micro = micro_batch(B, world, K)
    slots = []
    for rank in range(world):
        lo, hi = parallel.shard_batch(B, rank, world)
        assert hi - lo == K * micro
        for k in range(K):
            f = first_slot(lo, k, micro)
            assert f == lo + k * micro
            slots += list(range(f, f + micro))
    assert slots == list(range(B))


def test_step_rng_has_no_cpu_path():
    from mapdit_amd.step_rng import StepRNG
    with pytest.raises(NotImplementedError):
        StepRNG(0, torch.device("cpu"))


def test_statistics_of_the_restatement():
    """1,000 slots x 64 steps of the numpy reference: the formulas themselves (the GPU test holds the kernel to them bit for bit)."""
    draws = [S.scalars(0x0123456789ABCDEF, step, 0, 1000, 1000, 10, 0.1) for step in range(64)]
    t, drop, u, y = (np.concatenate([d[k] for d in draws]) for k in ("t", "drop", "u", "y_syn"))
    n = t.size
    assert set(t.tolist()) == set(range(1000))
    assert abs(t.mean() - 499.5) <= 4 * math.sqrt((1000 ** 2 - 1) / 12 / n)
    assert abs(drop.mean() - 0.1) <= 4 * math.sqrt(0.1 * 0.9 / n)
    assert abs(u.mean() - 0.5) <= 4 * math.sqrt(1 / 12 / n) and 0 <= u.min() and u.max() < 1
    assert set(y.tolist()) == set(range(10))
    z = np.concatenate([d["z"] for d in draws])
    assert abs(z.mean()) <= 4 / math.sqrt(n) and abs(z.var() - 1) <= 4 * math.sqrt(2 / n)
    assert (S.scalars(1, 0, 0, 64, drop_prob=0.0)["drop"] == 0).all() and (S.scalars(1, 0, 0, 64, drop_prob=1.0)["drop"] == 1).all()
