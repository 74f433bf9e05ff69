"""Host side of the native FID (map-dit_amd/fid.py): the Fréchet distance against scipy's sqrtm form, the key and shape checks of the
weight loader, the BatchNorm fold, the statistics file, the sampler's flag pair - and the yardstick itself
(tests/inception_reference.py).  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inception_reference as R  # noqa: E402


def _fid():
    import mapdit_amd.fid as FID
    return FID


@pytest.fixture(scope="module")
def sd():
    return R.init_state_dict(seed=3)


def _gauss(rng, n, d, shift=0.0):
    a = rng.standard_normal((d, d)) / np.sqrt(d) + np.eye(d)
    x = rng.standard_normal((n, d)) @ a + shift
    return x.mean(0), np.cov(x, rowvar=False)


# ---- frechet_distance ---------------------------------------------------------------------------------------------------------------
def test_frechet_distance_equals_the_sqrtm_formula():
    """D = 64, covariances of 512 samples: well conditioned, both sides fp64 -> 1e-8 relative.  scipy's side must be real here."""
    import scipy.linalg
    FID = _fid()
    rng = np.random.default_rng(0)
    mu1, s1 = _gauss(rng, 512, 64)
    mu2, s2 = _gauss(rng, 512, 64, shift=0.3)
    root = scipy.linalg.sqrtm(s1 @ s2)
    assert not np.iscomplexobj(root) or np.abs(root.imag).max() == 0.0
    want = float(((mu1 - mu2) ** 2).sum() + np.trace(s1) + np.trace(s2) - 2 * np.trace(root.real))
    got = FID.frechet_distance(mu1, s1, mu2, s2)
    print(f"frechet {got:.12f} vs sqrtm {want:.12f}: rel {abs(got - want) / want:.2e}")
    assert want > 1.0 and abs(got - want) <= 1e-8 * want
    assert abs(FID.frechet_distance(mu2, s2, mu1, s1) - want) <= 1e-8 * want         # symmetric in its arguments


def test_frechet_distance_of_identical_inputs_is_zero():
    FID = _fid()
    mu, s = _gauss(np.random.default_rng(1), 512, 64)
    assert abs(FID.frechet_distance(mu, s, mu, s)) <= 1e-9 * np.trace(s)


def test_frechet_distance_rank_deficient():
    """N < D: both covariances singular (rank 15 of 64), eigenvalues that rounding made negative are clamped."""
    FID = _fid()
    rng = np.random.default_rng(2)
    mu1, s1 = _gauss(rng, 16, 64)
    mu2, s2 = _gauss(rng, 16, 64, shift=0.1)
    assert np.linalg.matrix_rank(s1) == 15
    d = FID.frechet_distance(mu1, s1, mu2, s2)
    assert np.isfinite(d) and d >= 0.0
    # identical singular inputs: each of the D - 15 zero eigenvalues of S^(1/2) S S^(1/2) comes back as +- D eps lambda_max(S)^2 at the
    # worst, and the square root turns that into sqrt(D eps) lambda_max(S) - the floor of any sqrt-of-eigenvalues form, sqrtm included
    floor = 64 * np.sqrt(64 * np.finfo(np.float64).eps) * np.linalg.eigvalsh(s1)[-1]
    assert abs(FID.frechet_distance(mu1, s1, mu1, s1)) <= floor < 1e-3
    with pytest.raises(ValueError, match="shapes"):
        FID.frechet_distance(mu1, s1, mu2[:32], s2[:32, :32])


# ---- the weight loader --------------------------------------------------------------------------------------------------------------
def test_key_set_and_plan_agree(sd):
    FID = _fid()
    import mapdit_amd
    L = mapdit_amd._lib
    units, shapes = FID.conv_units(), FID.inception_shapes()
    assert len(units) == L.INC_NUM_CONV == 94 and len(shapes) == 94 * 5
    core = {k: v for k, v in sd.items() if not k.startswith(("fc.", "AuxLogits.")) and not k.endswith("num_batches_tracked")}
    assert set(core) == set(shapes) and all(tuple(core[k].shape) == tuple(s) for k, s in shapes.items())
    # the published parameter count of the feature network's convolutions and BatchNorms (Inception-v3 without fc and AuxLogits)
    assert sum(v.numel() for k, v in core.items() if k.endswith(("conv.weight", "bn.weight", "bn.bias"))) == 21_785_568
    lib, v = L.lib(), [ctypes.c_int() for _ in range(5)]
    for i, (name, cin, cout, (kh, kw), stride, _) in enumerate(units):
        lib.inc_layer_shape(i, *[ctypes.byref(x) for x in v])
        assert [x.value for x in v] == [cin, cout, kh, kw, stride], (i, name)
    with pytest.raises(L.MapditError, match="index"):
        lib.inc_layer_shape(94, *[ctypes.byref(x) for x in v])


def test_state_dict_checks(sd):
    FID = _fid()
    net = FID.InceptionFeatures.from_state_dict(sd, "cpu")             # complete (fc.*, AuxLogits.*, num_batches_tracked ignored): packs
    assert len(net.packed) == 2 * 94 and net.precision == "f16" and net.max_batch == 32
    assert net.packed[0].shape == (32, 3, 3, 3) and net.packed[0].dtype == torch.float16 and net.packed[1].dtype == torch.float32
    k7 = [u[0] for u in FID.conv_units()].index("Mixed_6b.branch7x7_2")
    assert net.packed[2 * k7].shape == (128, 1, 7, 128)                # [Cout][kh][kw][Cin]
    assert FID.InceptionFeatures.from_state_dict(sd, "cpu", precision="bf16").packed[0].dtype == torch.bfloat16

    missing = {k: v for k, v in sd.items() if k != "Mixed_6c.branch7x7dbl_3.bn.running_var"}
    with pytest.raises(KeyError, match="missing key 'Mixed_6c.branch7x7dbl_3.bn.running_var'"):
        FID.fold_state_dict(missing)
    with pytest.raises(KeyError, match="unexpected key 'Mixed_8a.conv.weight'"):
        FID.fold_state_dict(dict(sd, **{"Mixed_8a.conv.weight": torch.zeros(1)}))
    bad = dict(sd)
    bad["Mixed_7a.branch7x7x3_2.conv.weight"] = sd["Mixed_7a.branch7x7x3_2.conv.weight"].transpose(2, 3)      # 7 x 1 where 1 x 7 belongs
    with pytest.raises(ValueError, match=r"'Mixed_7a.branch7x7x3_2.conv.weight' has shape \(192, 192, 7, 1\), expected \(192, 192, 1, 7\)"):
        FID.fold_state_dict(bad)
    # a missing bn.weight counts as ones
    name = "Mixed_5b.branch5x5_2"
    no_gamma = {k: v for k, v in sd.items() if k != f"{name}.bn.weight"}
    ones = dict(sd, **{f"{name}.bn.weight": torch.ones(64, dtype=torch.float64)})
    a, b = FID.fold_state_dict(no_gamma)[name], FID.fold_state_dict(ones)[name]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], FID.fold_state_dict(sd)[name][0])
    with pytest.raises(ValueError, match="precision"):
        FID.InceptionFeatures.from_state_dict(sd, "cpu", precision="fp8")


def test_bn_fold_equals_conv_then_bn(sd):
    """The folded fp64 convolution against convolution + eval BatchNorm (torch.nn.functional), on a 7 x 1 unit: 1e-12."""
    import torch.nn.functional as F
    FID = _fid()
    name = "Mixed_6b.branch7x7_3"
    w, b = FID.fold_state_dict(sd)[name]
    x = torch.randn(2, 128, 9, 9, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    got = F.conv2d(x, w, b, 1, (3, 0))
    want = F.batch_norm(F.conv2d(x, sd[f"{name}.conv.weight"], None, 1, (3, 0)), sd[f"{name}.bn.running_mean"], sd[f"{name}.bn.running_var"],
                        sd[f"{name}.bn.weight"], sd[f"{name}.bn.bias"], False, 0.0, 1e-3)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"fold: max rel err {err:.2e}")
    assert err <= 1e-12


def test_reference_features_are_alive(sd):
    """The yardstick's own health: finite O(1) features, no channel identically 0 over the test images, the two images apart."""
    img = torch.randint(0, 256, (2, 64, 64, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    f = R.features(sd, img)
    assert f.shape == (2, 2048) and f.dtype == torch.float64 and bool(torch.isfinite(f).all())
    assert int((f == 0).all(0).sum()) == 0 and 0.05 < float(f.abs().mean()) < 20.0
    assert float((f[0] - f[1]).norm() / f[0].norm()) > 0.02
    x = R.prepare(img)
    assert x.shape == (2, 3, 299, 299) and float(x.min()) >= -1.0 and float(x.max()) <= 1.0


# ---- the statistics file -----------------------------------------------------------------------------------------------------------
def test_stats_file_round_trip_and_foreign_files(tmp_path):
    FID = _fid()
    mu, s = _gauss(np.random.default_rng(3), 100, 12)
    p = tmp_path / "ref.npz"
    FID.save_stats(p, mu, s)
    assert sorted(os.listdir(tmp_path)) == ["ref.npz"]
    mu2, s2 = FID.load_stats(p)
    assert mu2.dtype == np.float64 and np.array_equal(mu, mu2) and np.array_equal(s, s2)
    assert FID.FeatureStats.load(p)[0].shape == (12,)
    # another evaluator's file: float32 arrays and keys of its own (ADM's reference batches carry arr_0, mu_s, sigma_s beside these)
    q = tmp_path / "VIRTUAL_ref.npz"
    np.savez(q, arr_0=np.zeros((2, 4, 4, 3), np.uint8), mu=mu.astype(np.float32), sigma=s.astype(np.float32), mu_s=mu, sigma_s=s)
    mu3, s3 = FID.load_stats(q)
    assert mu3.dtype == np.float64 and np.array_equal(mu3, mu.astype(np.float32).astype(np.float64)) and s3.shape == (12, 12)
    np.savez(tmp_path / "no.npz", mu=mu)
    with pytest.raises(KeyError, match="sigma"):
        FID.load_stats(tmp_path / "no.npz")
    np.savez(tmp_path / "bad.npz", mu=mu, sigma=s[:5])
    with pytest.raises(ValueError, match="sigma"):
        FID.load_stats(tmp_path / "bad.npz")


def test_cpu_tensors_are_refused(sd):
    FID = _fid()
    net = FID.InceptionFeatures.from_state_dict(sd, "cpu")
    with pytest.raises(NotImplementedError):
        net.features(torch.zeros(1, 32, 32, 3, dtype=torch.uint8))
    with pytest.raises(NotImplementedError):
        FID.FeatureStats(8, "cpu")


def test_workspace_query(sd):
    FID = _fid()
    import mapdit_amd
    L = mapdit_amd._lib
    net = FID.InceptionFeatures.from_state_dict(sd, "cpu")
    one, many = net.workspace_bytes(1), net.workspace_bytes(32)
    e = 147 * 147 * 64                                                  # the largest activation: Conv2d_2b_3x3's output
    assert one >= 4 * 2 * e + 4 * 299 * 299 * 3 + 4 * 8 * 8 * 2048 and one < 4 * 2 * e + 4 * 299 * 299 * 3 + 4 * 8 * 8 * 2048 + 6 * 256
    assert 31 * one < many <= 32 * one
    lib = L.lib()
    assert lib.inc_workspace_bytes(ctypes.byref(L.IncConfig(image_size=74)), 1) == 0 and b"image_size" in lib.last_error()
    assert lib.inc_workspace_bytes(ctypes.byref(L.IncConfig(image_size=75)), 1) > 0          # a 1 x 1 final map
    assert lib.inc_workspace_bytes(ctypes.byref(L.IncConfig(image_size=299)), 0) == 0


# ---- the sampler's flag pair -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags, exc, match", [
    (["--fid-ref", "ref.npz"], ValueError, "go together"),
    (["--inception-weights", "w.pt"], ValueError, "go together"),
    (["--fid-ref", "nowhere_ref.npz", "--inception-weights", "w.pt"], FileNotFoundError, "nowhere_ref.npz"),
])
def test_sample_fid_refuses_half_of_the_flag_pair_before_any_model_is_built(tmp_path, flags, exc, match):
    from mapdit_amd import sample_fid
    with pytest.raises(exc, match=match):                     # before config.yaml of the (equally missing) run directory is read
        sample_fid.main(["--result-dir", str(tmp_path / "no_such_run")] + flags)


def test_sample_fid_fid_flags_need_pixels(tmp_path):
    from mapdit_amd import sample_fid
    ref, w = tmp_path / "ref.npz", tmp_path / "w.pt"
    np.savez(ref, mu=np.zeros(2048), sigma=np.eye(2048))
    w.write_bytes(b"")
    with pytest.raises(ValueError, match="pixels"):
        sample_fid.main(["--result-dir", str(tmp_path / "no_such_run"), "--use-vae", "false", "--fid-ref", str(ref), "--inception-weights", str(w)])
    args = sample_fid.build_parser().parse_args(["--result-dir", "x"])
    assert args.fid_ref is None and args.inception_weights is None and sample_fid.check_fid_flags(args) is False
