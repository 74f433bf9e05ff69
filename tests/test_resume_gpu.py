"""train.py --step-rng counter and --resume on the MI355X: a step is a function of (seed, step), and a run stopped at a checkpoint and
resumed ends with the bits of the run that was never stopped."""
import os

import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
# (--num-lin-warmup / --start-decay are given: derived from 4 or 6 steps they would be 0)
BASE = ["--model", "DiT-XS/2", "--num-classes", "10", "--batch-size", "8", "--step-rng", "counter", "--num-lin-warmup", "2", "--start-decay", "3"]


def same(a, b, where="ckpt"):
    """Equality of two checkpoint trees, tensor for tensor (torch.equal), with the place of the first difference."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (where, list(a), list(b) if isinstance(b, dict) else b)
        for k in a:
            same(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), where
        for i, (u, v) in enumerate(zip(a, b)):
            same(u, v, f"{where}[{i}]")
    elif isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b), where
    else:
        assert type(a) is type(b) and a == b, (where, a, b)


def load(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def train_main(argv):
    from mapdit_amd import train
    return train.main(argv)


def test_a_step_is_a_function_of_seed_and_step(tmp_path):
    run = ["--synthetic", "--precision", "bf16", "--num-steps", "4", "--ckpt-every", "4", "--log-every", "2"] + BASE
    exps = [train_main(run + ["--results-dir", str(tmp_path / name), "--grad-accum-steps", k]) for name, k in (("a", "1"), ("b", "1"), ("k2", "2"))]
    a, b, k2 = (load(os.path.join(e, "checkpoints", "0000004.pt")) for e in exps)
    assert set(a) == {"model", "opt", "ema", "train_state"} and a["train_state"]["step_rng"] == "counter"
    same(a, b)                                           # the same run twice: model, moments, EMA copies, train_state
    assert set(k2) == set(a) and all(torch.isfinite(v).all() for v in k2["model"].values())
    assert yaml.safe_load(open(os.path.join(exps[0], "config.yaml")))["step_rng"] == "counter"
    # K = 1 against K = 2: the DRAWS are the same (the weights are not compared: the gradients are summed in another order)
    from mapdit_amd.step_rng import StepRNG, first_slot
    from mapdit_amd.train import micro_batch
    r, kw = StepRNG(0, DEV), dict(per=4 * 32 * 32, T=1000, num_classes=10, drop_prob=0.1)
    whole = r.draw(2, 0, 8, **kw)
    micro = micro_batch(8, 1, 2)
    halves = [r.draw(2, first_slot(0, k, micro), micro, **kw) for k in range(2)]
    for name in vars(whole):
        assert torch.equal(torch.cat([getattr(h, name) for h in halves]), getattr(whole, name)), name


@pytest.fixture(scope="module")
def latent_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("latents64")
    g = torch.Generator().manual_seed(0)
    torch.save(torch.randn(64, 4, 32, 32, generator=g), root / "posterior_means.pt")
    torch.save(torch.rand(64, 4, 32, 32, generator=g) * 0.3, root / "posterior_stds.pt")
    torch.save(torch.randint(0, 10, (64,), generator=g), root / "labels.pt")
    torch.save({"mean": torch.randn(4, generator=g) * 0.1, "std": torch.rand(4, generator=g) + 0.5}, root / "stats.pt")
    return str(root)


def run_a(results, extra):
    """Run A of the acceptance test: 6 steps, checkpoints at 3 and 6, log lines at 2, 4, 6 - the checkpoint at 3 falls between two polls
    of the fp16 guard."""
    return train_main(BASE + ["--num-steps", "6", "--ckpt-every", "3", "--log-every", "2", "--ema-snapshot-every", "3", "--results-dir", str(results)] + extra)


VARIANTS = {"bf16": ["--synthetic", "--precision", "bf16"],
            "f16": ["--synthetic", "--precision", "f16"],
            "loss-second-moment": ["--synthetic", "--precision", "bf16", "--schedule-sampler", "loss-second-moment"],
            "device-loader": ["--precision", "bf16", "--data-loader", "device"]}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_a_resumed_run_ends_with_the_bits_of_the_unstopped_run(tmp_path, latent_dir, variant):
    extra = VARIANTS[variant] + (["--data-path", latent_dir] if variant == "device-loader" else [])
    exp = run_a(tmp_path / "res", extra)
    final = os.path.join(exp, "checkpoints", "0000006.pt")
    snaps = [os.path.join(exp, "ema", f"{std:.3f}_0000006.pt") for std in (0.05, 0.1)]
    a, a_snaps = load(final), [load(s) for s in snaps]
    for f in [final] + snaps:                            # A's step-6 files are moved aside: B has to write its own
        os.rename(f, f + ".a")
    config = open(os.path.join(exp, "config.yaml"), "rb").read()
    old_lines = open(os.path.join(exp, "log.txt")).read().splitlines()
    log_lines = len(old_lines)
    assert train_main(["--resume", os.path.join(exp, "checkpoints", "0000003.pt")]) == exp
    b = load(final)
    assert set(b) >= {"model", "opt", "ema", "train_state"} and ("schedule_sampler" in b) == (variant == "loss-second-moment")
    same(a, b)
    for sa, s in zip(a_snaps, snaps):
        same(sa, load(s), "snapshot")
    assert os.listdir(tmp_path / "res") == [os.path.basename(exp)]                # no new experiment directory
    assert open(os.path.join(exp, "config.yaml"), "rb").read() == config
    lines = open(os.path.join(exp, "log.txt")).read().splitlines()
    assert len(lines) > log_lines and lines[:log_lines] == old_lines and any("resuming from" in ln for ln in lines[log_lines:])
    steps = [ln for ln in lines[log_lines:] if ln.startswith("(step=")]
    assert [ln[:14] for ln in steps] == ["(step=0000004)", "(step=0000006)"]
    # the window of the first log line straddles the checkpoint (steps 3 and 4): the restored accumulators give A's averages
    loss = lambda ln: ln.split("train loss: ")[1].split(",")[0]
    assert [loss(ln) for ln in steps] == [loss(ln) for ln in old_lines if ln.startswith(("(step=0000004)", "(step=0000006)"))]
    if variant == "bf16":                                # an experiment directory resolves to its latest checkpoint: nothing left to do
        os.rename(final, final + ".b")
        assert train_main(["--resume", exp, "--num-steps", "3"]) == exp
        assert not os.path.exists(final)


def test_resume_refusals(tmp_path):
    from mapdit_amd._lib import MapditError
    exp = train_main(BASE + ["--synthetic", "--precision", "bf16", "--num-steps", "3", "--ckpt-every", "3", "--log-every", "3", "--results-dir", str(tmp_path)])
    ckpt = os.path.join(exp, "checkpoints", "0000003.pt")
    with pytest.raises(ValueError, match="--model"):
        train_main(["--resume", ckpt, "--model", "DiT-S/2"])
    with pytest.raises(ValueError, match="--seed"):
        train_main(["--resume", ckpt, "--seed", "1"])
    with pytest.raises(MapditError, match="--resume"):
        train_main(["--resume", ckpt, "--grad-comm", "zero1w"])
    with pytest.raises(ValueError, match="below the checkpoint's step 3"):
        train_main(["--resume", ckpt, "--num-steps", "2"])
    full = load(ckpt)
    torch.save({"model": full["model"], "opt": full["opt"]}, ckpt)               # what the reference writes
    with pytest.raises(ValueError, match="no 'ema' key"):
        train_main(["--resume", ckpt])
    with pytest.raises(ValueError, match="--results-dir"):
        train_main(BASE + ["--synthetic"])
    assert os.listdir(tmp_path) == [os.path.basename(exp)]


def test_the_default_run_writes_the_references_checkpoint_and_is_not_continued(tmp_path):
    args = ["--model", "DiT-XS/2", "--num-classes", "10", "--batch-size", "8", "--num-lin-warmup", "2", "--start-decay", "3", "--synthetic",
            "--precision", "bf16", "--ckpt-every", "2", "--log-every", "2"]
    exp = train_main(args + ["--num-steps", "2", "--results-dir", str(tmp_path)])
    assert set(load(os.path.join(exp, "checkpoints", "0000002.pt"))) == {"model", "opt"}
    with pytest.raises(ValueError, match="--step-rng counter"):
        train_main(["--resume", exp, "--num-steps", "4"])
