"""CPU-side checks of REPA: the fp64 restatements (tests/repa_reference.py) against torch's fp64 autograd and exact rational rounding, the
emulation figures tests/test_repa_head_gpu.py is held to, every train.py refusal of --repa-features, the features-file validation, the
``dinov2 tokens`` argument handling and its reuse of encode_data's flip flags, and the facade's hidden_tap checks."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import repa_reference as R  # noqa: E402


# ---- the restatements ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 5, 8), (14, 7, 16), (130, 65, 24)])
def test_cos_loss_restatement_equals_torch_autograd(shape):
    Rr, T, P = shape
    rng = np.random.default_rng(Rr)
    z, f, g = rng.standard_normal((Rr, P)), rng.standard_normal((Rr, P)), rng.standard_normal(Rr // T)
    z[0] *= 1e4
    z[1] *= 1e-6
    z[Rr - 1] = 0.0
    f[Rr - 2] = 0.0
    zt = torch.tensor(z, requires_grad=True)
    F = torch.nn.functional
    cos = (F.normalize(zt, dim=1, eps=R.EPS) * F.normalize(torch.tensor(f), dim=1, eps=R.EPS)).sum(1)
    loss = -cos.view(Rr // T, T).mean(1)
    (loss * torch.tensor(g)).sum().backward()
    got_l, got_dz = R.cos_loss(z, f, T, g)
    assert np.allclose(got_l, loss.detach().numpy(), rtol=1e-13, atol=1e-15)
    scale = np.abs(zt.grad.numpy()).max(1, keepdims=True) + 1e-300
    assert (np.abs(got_dz - zt.grad.numpy()) / scale).max() < 1e-12
    assert np.isfinite(got_dz).all() and (got_dz[Rr - 2] == 0).all()
    # the zero rows add nothing to the loss
    keep = np.ones(Rr, bool)
    keep[[Rr - 1, Rr - 2]] = False
    cos_rows = -(F.normalize(torch.tensor(z), dim=1) * F.normalize(torch.tensor(f), dim=1)).sum(1).numpy()
    assert np.allclose(got_l.sum() * T, cos_rows[keep].sum(), rtol=1e-12)
    bl, bdz = R.cos_loss_bound(z, f, T, g)
    assert (bl > 0).all() and (bl < 1e-4).all() and np.isfinite(bdz).all() and (bdz >= 0).all()


def test_projector_restatement_equals_torch_autograd():
    h, feats, g, p = R.head_case()
    T = R.HEAD_CASE["T"]
    tp = {k: torch.tensor(v, requires_grad=True) for k, v in p.items()}
    ht = torch.tensor(h.astype(np.float64), requires_grad=True)
    F = torch.nn.functional
    z = F.linear(F.silu(F.linear(F.silu(F.linear(ht, tp["w1"], tp["b1"])), tp["w2"], tp["b2"])), tp["w3"], tp["b3"])
    cos = (F.normalize(z, dim=1, eps=R.EPS) * F.normalize(torch.tensor(feats.astype(np.float64)), dim=1, eps=R.EPS)).sum(1)
    loss = -cos.view(-1, T).mean(1)
    (loss * torch.tensor(g.astype(np.float64))).sum().backward()
    got_l, got_dh, got_g = R.head_loss(h, feats, p, T, g)
    assert R.rel(got_l, loss.detach().numpy()) < 1e-13 and R.rel(got_dh, ht.grad.numpy()) < 1e-12
    for k in p:
        assert R.rel(got_g[k], tp[k].grad.numpy()) < 1e-12, k
    # a power-of-two loss scale changes nothing in exact arithmetic
    scaled = R.head_loss(h, feats, p, T, g, scale=2.0 ** 13)
    assert R.rel(scaled[1], got_dh) < 1e-15


def _exact_round(x, p, emin):
    """Round-to-nearest-even of the rational x to p significand bits with minimum normal exponent emin, in exact arithmetic."""
    if x == 0:
        return 0.0
    fx = Fraction(x)
    e = max(int(np.floor(np.log2(abs(float(fx))))), emin)
    while Fraction(2) ** (e + 1) <= abs(fx):
        e += 1
    while e > emin and Fraction(2) ** e > abs(fx):
        e -= 1
    q = Fraction(2) ** (e - (p - 1))
    n = fx / q
    lo = n.numerator // n.denominator
    r = n - lo
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and lo % 2 == 1):
        lo += 1
    return float(lo * q)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_round16_is_the_correctly_rounded_conversion(fmt):
    p, emin = {"f16": (11, -14), "bf16": (8, -126)}[fmt]
    dt = {"f16": torch.float16, "bf16": torch.bfloat16}[fmt]
    g = torch.Generator().manual_seed(1)
    x = torch.randn(20000, generator=g) * torch.exp(torch.empty(20000).uniform_(-20, 10, generator=g))
    assert np.array_equal(R.round16(x.double().numpy(), fmt), x.to(dt).double().numpy())          # fp32 inputs: torch's own conversion
    half = 2.0 ** -p                                                                             # half a spacing at 1
    ties = np.array([1 + half, 1 + 3 * half, 1 + half + 2.0 ** -40, 1 + half - 2.0 ** -40, -(1 + half + 2.0 ** -40), 2.0 ** (emin - p + 1) * 0.5,
                     2.0 ** (emin - p + 1) * 1.5, 2.0 ** (emin - p + 1) * 0.5000001, 0.0, 2.0 ** emin * (1 + half)])
    rng = np.random.default_rng(2)
    vals = np.concatenate([ties, rng.standard_normal(300) * np.exp(rng.uniform(-12, 9, 300))])
    want = np.array([_exact_round(Fraction(float(v)), p, emin) for v in vals])
    assert np.array_equal(R.round16(vals, fmt), want)
    # a sum just above a tie: a rounding through fp32 lands on the tie and goes to even, the single rounding goes up
    v = 1 + half + 2.0 ** -40
    assert R.round16(np.array([v]), fmt)[0] == 1 + 2 * half
    assert torch.tensor([v], dtype=torch.float64).float().to(dt).double().item() == 1.0


def test_head_emulation_figures_are_what_the_gpu_test_is_held_to():
    import test_repa_head_gpu as H
    for prec in ("f16", "bf16"):
        measured = R.measure_head_emulation(prec)
        assert set(measured) == set(H.E_EMUL[prec])
        for k, v in measured.items():
            print(f"{prec} {k}: e_emul {v:.3e}")
            assert abs(v - H.E_EMUL[prec][k]) <= 2e-3 * H.E_EMUL[prec][k], (prec, k, v)


# ---- train.py ------------------------------------------------------------------------------------------------------------------------
SYN = ["--synthetic", "--model", "DiT-XS/2", "--batch-size", "8", "--num-steps", "2"]


@pytest.mark.parametrize("extra, flag", [
    (["--repa-features", "synthetic:24", "--data-loader", "device", "--data-path", "/nowhere"], "--data-loader device"),
    (["--repa-features", "synthetic:24", "--precision", "bf16x3"], "--precision bf16x3"),
    (["--repa-features", "synthetic:24", "--no-use-no-layernorm"], "--no-use-no-layernorm"),
    (["--repa-features", "synthetic:20"], "--repa-features synthetic:20"),
    (["--repa-features", "synthetic:x"], "--repa-features synthetic:x"),
    (["--repa-features", "feats.npy"], "--repa-features feats.npy"),
    (["--repa-features", "synthetic:24", "--repa-hidden", "100"], "--repa-hidden"),
    (["--repa-features", "synthetic:24", "--repa-coeff", "-1"], "--repa-coeff"),
    (["--repa-features", "synthetic:24", "--repa-lr", "0"], "--repa-lr"),
    (["--repa-features", "synthetic:24", "--repa-depth", "0"], "--repa-depth"),
])
def test_train_refusals_come_before_any_device_work(tmp_path, monkeypatch, extra, flag):
    from mapdit_amd import train
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: pytest.fail("device work before the refusal"))
    argv = [a for a in SYN if a != "--synthetic" or "--data-path" not in extra] + ["--results-dir", str(tmp_path)] + extra
    with pytest.raises(ValueError) as e:
        train.main(argv)
    assert flag in str(e.value), str(e.value)
    assert os.listdir(tmp_path) == []                          # no experiment directory either


def test_train_refuses_a_world_size_above_one(tmp_path, monkeypatch):
    from mapdit_amd import train
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: pytest.fail("device work before the refusal"))
    with pytest.raises(ValueError, match="--repa-features.*world size of 2"):
        train.main(SYN + ["--results-dir", str(tmp_path), "--repa-features", "synthetic:24"])


def test_synthetic_features_need_synthetic_data(tmp_path):
    from mapdit_amd import train
    with pytest.raises(ValueError, match="--repa-features synthetic:24 draws"):
        train.main(["--data-path", "/nowhere", "--results-dir", str(tmp_path), "--repa-features", "synthetic:24"])


def test_defaults_and_parser():
    from mapdit_amd import train
    a = train.build_parser().parse_args(SYN + ["--results-dir", "x"])
    assert a.repa_features is None and a.repa_coeff == 0.5 and a.repa_depth is None and a.repa_hidden == 2048 and a.repa_lr == 1e-4
    assert train.check_repa_args(a, 8) is None                 # without the flag nothing is looked at
    a = train.build_parser().parse_args(SYN + ["--results-dir", "x", "--repa-features", "synthetic:768"])
    assert train.check_repa_args(a, 1) == ("synthetic", 768)
    assert train.parse_repa_features("dir/feats.npy") == ("file", "dir/feats.npy")


def test_features_file_validation(tmp_path):
    from mapdit_amd.train import check_repa_features_file as check
    good = str(tmp_path / "good.npy")
    np.save(good, np.zeros((8, 64, 24), np.float16))
    assert check(good, 8, 64) == 24
    cases = {"rows": (np.zeros((7, 64, 24), np.float16), "7 rows"), "tokens": (np.zeros((8, 16, 24), np.float16), "16 tokens per sample"),
             "dtype": (np.zeros((8, 64, 24), np.float32), "dtype float32"), "ndim": (np.zeros((8, 64 * 24), np.float16), "shape (8, 1536)"),
             "width": (np.zeros((8, 64, 20), np.float16), "feature width 20")}
    for name, (arr, word) in cases.items():
        path = str(tmp_path / (name + ".npy"))
        np.save(path, arr)
        with pytest.raises(ValueError) as e:
            check(path, 8, 64)
        assert "--repa-features" in str(e.value) and word in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="--repa-features.*no such file"):
        check(str(tmp_path / "missing.npy"), 8, 64)
    junk = tmp_path / "junk.npy"
    junk.write_bytes(b"not an array")
    with pytest.raises(ValueError, match="--repa-features.*not a .npy"):
        check(str(junk), 8, 64)


# ---- dinov2 tokens -------------------------------------------------------------------------------------------------------------------
def test_tokens_arguments_and_flip_flags(tmp_path):
    from mapdit_amd import dinov2 as D
    from mapdit_amd.encode_data import flip_flags
    a = D.build_parser().parse_args(["tokens", "--images", "i.npy", "--dinov2-weights", "w.pt", "--grid", "16", "--output", "o.npy"])
    assert a.cmd == "tokens" and a.grid == 16 and a.flip_seed is None and a.batch_size == 64 and a.precision == "f16"
    with pytest.raises(SystemExit):
        D.build_parser().parse_args(["tokens", "--images", "i.npy", "--output", "o.npy"])          # --grid is required
    imgs = str(tmp_path / "i.npy")
    np.save(imgs, np.zeros((3, 28, 28, 3), np.uint8))
    base = ["tokens", "--images", imgs, "--dinov2-weights", str(tmp_path / "w.pt")]
    with pytest.raises(ValueError, match="--grid 0"):
        D.main(base + ["--grid", "0", "--output", str(tmp_path / "o.npy")])
    with pytest.raises(ValueError, match="--output.*one .npy"):
        D.main(base + ["--grid", "2", "--output", str(tmp_path / "o.npz")])
    with pytest.raises(ValueError, match="--batch-size"):
        D.main(base + ["--grid", "2", "--output", str(tmp_path / "o.npy"), "--batch-size", "0"])
    with pytest.raises(ValueError, match="--dinov2-weights"):
        D.main(["tokens", "--images", imgs, "--grid", "2", "--output", str(tmp_path / "o.npy")])
    bad = str(tmp_path / "bad.npy")
    np.save(bad, np.zeros((3, 28, 28, 3), np.float32))
    with pytest.raises(ValueError, match="uint8"):                                               # a bad array ends the run before the weights are read
        D.main(["tokens", "--images", bad, "--dinov2-weights", str(tmp_path / "w.pt"), "--grid", "2", "--output", str(tmp_path / "o.npy")])
    assert not os.path.exists(tmp_path / "o.npy")
    # the flags are encode_data's, not a second draw
    assert not D.tokens_flip_flags(9, None).any() and D.tokens_flip_flags(9, None).shape == (9,)
    for seed in (0, 3, 12345):
        assert np.array_equal(D.tokens_flip_flags(50, seed), flip_flags(50, seed).numpy().astype(bool))


# ---- the facade ------------------------------------------------------------------------------------------------------------------------
def test_hidden_tap_attribute():
    from mapdit_amd.src.dit import DiT
    m = DiT(depth=4, hidden_size=128, patch_size=2, input_size=16, in_channels=4, num_heads=2, num_classes=10)
    assert m.hidden_tap is None and m.tapped_hidden is None
    for ok in (0, 2, None):
        m.hidden_tap = ok
        assert m.hidden_tap == ok
    for bad in (3, -1, 4, 1.5, "1", True):
        with pytest.raises(ValueError, match="hidden_tap"):
            m.hidden_tap = bad
    m.hidden_tap = 1
    m.gemm_precision = "bf16x3"
    with pytest.raises(ValueError, match="hidden_tap.*bf16x3"):
        m._check_hidden_tap()
    ln = DiT(depth=4, hidden_size=128, patch_size=2, input_size=16, in_channels=4, num_heads=2, num_classes=10, no_layernorm=False)
    ln.hidden_tap = 1
    with pytest.raises(ValueError, match="hidden_tap.*LayerNorm"):
        ln._check_hidden_tap()
    import copy
    m.gemm_precision = "f16"
    assert copy.deepcopy(m).hidden_tap == 1
