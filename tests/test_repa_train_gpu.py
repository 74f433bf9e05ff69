"""train.py --repa-features end to end on the MI355X: the synthetic run in both precisions with and without gradient accumulation, a
--step-rng counter run stopped and resumed, a --data-path run on a features file, and the sampler CLI on the result."""
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
BASE = ["--model", "DiT-XS/2", "--num-classes", "10", "--batch-size", "8", "--num-lin-warmup", "2", "--start-decay", "3", "--log-every", "1"]
REPA = ["--repa-features", "synthetic:24", "--repa-hidden", "64"]


def load(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def train_main(argv):
    from mapdit_amd import train
    return train.main(argv)


def same(a, b, where="ckpt"):
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


@pytest.mark.parametrize("accum", ["1", "2"])
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_synthetic_run_trains_the_projector(tmp_path, prec, accum):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import repa_reference as R
    exp = train_main(["--synthetic", "--results-dir", str(tmp_path), "--num-steps", "3", "--ckpt-every", "3", "--ema-snapshot-every", "3",
                      "--precision", prec, "--grad-accum-steps", accum] + BASE + REPA)
    lines = [ln for ln in open(os.path.join(exp, "log.txt")).read().splitlines() if ln.startswith("(step=")]
    assert len(lines) == 3
    for ln in lines:
        assert ", repa: " in ln and np.isfinite(float(ln.split(", repa: ")[1])) and np.isfinite(float(ln.split("train loss: ")[1].split(",")[0])), ln
        assert -1.0 <= float(ln.split(", repa: ")[1]) <= 1.0                     # a mean of negative cosines
    cfg = yaml.safe_load(open(os.path.join(exp, "config.yaml")))
    assert cfg["repa_features"] == "synthetic:24" and cfg["repa_coeff"] == 0.5 and cfg["repa_hidden"] == 64 and cfg["repa_lr"] == 1e-4
    ck = load(os.path.join(exp, "checkpoints", "0000003.pt"))
    assert set(ck) == {"model", "opt", "repa_head", "repa_opt"}
    init = R.init_params(256, 24, 64, seed=0)
    for k, v in ck["repa_head"].items():
        assert v.shape == init[k].shape and torch.isfinite(v).all()
        assert not np.array_equal(v.numpy(), init[k].astype(np.float32)), k     # three Adam steps moved every tensor
    assert not any(k.startswith(("repa", "w1")) for k in ck["model"])           # the head is no part of the model's state dict ...
    snap = load(os.path.join(exp, "ema", "0.050_0000003.pt"))
    assert set(snap["state_dict"]) == set(ck["model"])                          # ... nor of the EMA snapshots


def test_resumed_counter_run_ends_with_the_bits_of_the_unstopped_run(tmp_path):
    run = ["--synthetic", "--precision", "f16", "--step-rng", "counter", "--num-steps", "4", "--ckpt-every", "2", "--ema-snapshot-every", "2",
           "--results-dir", str(tmp_path / "res")] + BASE + REPA
    exp = train_main(run)
    final = os.path.join(exp, "checkpoints", "0000004.pt")
    a = load(final)
    assert set(a) == {"model", "opt", "ema", "train_state", "repa_head", "repa_opt"}
    os.rename(final, final + ".a")
    assert train_main(["--resume", os.path.join(exp, "checkpoints", "0000002.pt")]) == exp
    same(a, load(final))
    # a checkpoint without the head cannot continue a run that trains one
    half = load(os.path.join(exp, "checkpoints", "0000002.pt"))
    del half["repa_head"]
    torch.save(half, os.path.join(exp, "checkpoints", "0000002.pt"))
    with pytest.raises(ValueError, match="repa_head"):
        train_main(["--resume", os.path.join(exp, "checkpoints", "0000002.pt")])


@pytest.fixture(scope="module")
def data_run(tmp_path_factory):
    """An 8-sample data set in the reference's four files, a features .npy beside it, and a two-step run over both."""
    root = tmp_path_factory.mktemp("repa_data")
    g = torch.Generator().manual_seed(0)
    torch.save(torch.randn(8, 4, 32, 32, generator=g), root / "posterior_means.pt")
    torch.save(torch.rand(8, 4, 32, 32, generator=g) * 0.3, root / "posterior_stds.pt")
    torch.save(torch.randint(0, 10, (8,), generator=g), root / "labels.pt")
    torch.save({"mean": torch.randn(4, generator=g) * 0.1, "std": torch.rand(4, generator=g) + 0.5}, root / "stats.pt")
    feats = str(root / "repa_features.npy")
    np.save(feats, torch.randn(8, 256, 24, generator=g).half().numpy())
    exp = train_main(["--data-path", str(root), "--results-dir", str(root / "res"), "--num-steps", "2", "--ckpt-every", "2", "--ema-snapshot-every", "2",
                      "--num-workers", "0", "--precision", "f16", "--repa-features", feats, "--repa-hidden", "64", "--repa-depth", "2"] + BASE)
    return str(root), feats, exp


def test_data_path_run_reads_the_features_file(data_run):
    root, feats, exp = data_run
    lines = [ln for ln in open(os.path.join(exp, "log.txt")).read().splitlines() if ln.startswith("(step=")]
    assert len(lines) == 2 and all(", repa: " in ln for ln in lines)
    assert "hidden state after 2 blocks, 256 x 24 features" in open(os.path.join(exp, "log.txt")).read()
    ck = load(os.path.join(exp, "checkpoints", "0000002.pt"))
    assert ck["repa_head"]["w3"].shape == (24, 64) and ck["repa_head"]["w1"].shape == (64, 256)
    from mapdit_amd.train import RepaLatentDataset
    ds = RepaLatentDataset(root, feats)
    x, y, f = ds[5]
    assert f.dtype == torch.float16 and np.array_equal(f.numpy(), np.load(feats)[5]) and int(y) == int(ds.labels[5])
    bad = os.path.join(root, "short.npy")
    np.save(bad, np.zeros((7, 256, 24), np.float16))
    with pytest.raises(ValueError, match="--repa-features.*7 rows"):
        train_main(["--data-path", root, "--results-dir", os.path.join(root, "res2"), "--num-steps", "1", "--repa-features", bad] + BASE)


def test_sampler_loads_the_run_unchanged(data_run, tmp_path):
    from mapdit_amd import sample
    _, _, exp = data_run
    out = str(tmp_path / "grid.png")
    s = sample.main(["--result-dir", exp, "--use-vae", "false", "--num-sampling-steps", "2", "--class-label", "3", "--output-file", out, "--seed", "1"])
    assert s.shape == (4, 4, 32, 32) and torch.isfinite(s).all()                 # the EMA snapshot
    c = sample.main(["--result-dir", exp, "--use-vae", "false", "--num-sampling-steps", "2", "--class-label", "3", "--output-file", out, "--seed", "1",
                     "--ckpt", "0000002"])
    assert c.shape == (4, 4, 32, 32) and torch.isfinite(c).all()                 # the checkpoint, with its two extra keys
