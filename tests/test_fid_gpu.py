"""The native FID end to end on the GPU (map-dit_amd/fid.py -> mapdit_inc_features, mapdit_inc_stats_accumulate) against the fp64
restatement (tests/inception_reference.py) on random weights, in both operand formats, and through sample_fid.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inception_reference as R  # noqa: E402
import vae_reference as VR  # noqa: E402
from conftest import rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

# Relative L2 error of the [2, 2048] features of two 64 x 64 noise images against the fp64 restatement, as measured on an MI355X
# (DESIGN.md section 5): operand rounding through the 47 layers of the longest path.  The kernels are deterministic; the asserted
# bound is 3 x the recorded value, a margin for another seed or image size only.
RECORDED = {"f16": 5.3e-3, "bf16": 3.4e-2}
BOUND = {k: 3 * v for k, v in RECORDED.items()}


def _net(sd, precision="f16", **kw):
    from mapdit_amd.fid import InceptionFeatures
    return InceptionFeatures.from_state_dict(sd, DEV, precision=precision, **kw)


@pytest.fixture(scope="module")
def sd():
    return R.init_state_dict(seed=3)


@pytest.fixture(scope="module")
def two(sd):
    img = torch.randint(0, 256, (2, 64, 64, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    return img, R.features(sd, img)


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_full_network_against_the_restatement(sd, two, precision):
    img, ref = two
    net = _net(sd, precision)
    out = net.features(img.to(DEV))
    assert out.shape == (2, 2048) and out.dtype == torch.float32 and out.is_cuda
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out, net.features(img.to(DEV)))
    e = rel_err(out.cpu().numpy(), ref.numpy())
    e_emul = rel_err(R.features(sd, img, operand_dtype=torch.float16 if precision == "f16" else torch.bfloat16).numpy(), ref.numpy())
    print(f"inception features {precision}: rel err {e:.3e} (recorded {RECORDED[precision]:.1e}, bound {BOUND[precision]:.1e}); "
          f"fp64 emulation of the operand rounding {e_emul:.3e}")
    assert e <= BOUND[precision]
    # the same pictures handed over as [-1, 1] floats take the other resize entry and land on the same features up to fp32 rounding
    xf = (img.permute(0, 3, 1, 2).float() / 255.0 * 2.0 - 1.0).to(DEV)
    assert rel_err(net.features(xf).cpu().numpy(), ref.numpy()) <= BOUND[precision]


def test_an_image_alone_equals_the_image_in_a_batch(sd, two):
    img = torch.cat([two[0], torch.randint(0, 256, (1, 64, 64, 3), generator=torch.Generator().manual_seed(6), dtype=torch.uint8)]).to(DEV)
    whole = _net(sd).features(img)
    chunked = _net(sd, max_batch=2).features(img)                            # 2 + 1
    assert torch.equal(whole, chunked)
    assert torch.equal(_net(sd, max_batch=1).features(img[1:2])[0], whole[1])


def test_refusals(sd):
    net = _net(sd)
    with pytest.raises(NotImplementedError):
        net.features(torch.zeros(1, 32, 32, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="expected"):
        net.features(torch.zeros(1, 32, 32, 4, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="8 x 8"):
        net.features(torch.zeros(1, 7, 32, 3, dtype=torch.uint8, device=DEV))
    from mapdit_amd.fid import FeatureStats
    with pytest.raises(ValueError, match="expected"):
        FeatureStats(2048, DEV).update(torch.zeros(2, 48, device=DEV))
    with pytest.raises(ValueError, match="two"):
        FeatureStats(8, DEV).update(torch.zeros(1, 8, device=DEV)).mean_cov()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sets(sd):
    """Two sets of 96 noise images of 32 x 32 with different means, and the restatement's fp64 features of both (computed once)."""
    g = torch.Generator().manual_seed(7)
    a = torch.randint(0, 256, (96, 32, 32, 3), generator=g, dtype=torch.uint8)
    b = torch.randint(96, 256, (96, 32, 32, 3), generator=g, dtype=torch.uint8)
    fa = torch.cat([R.features(sd, a[i:i + 32]) for i in range(0, 96, 32)])
    fb = torch.cat([R.features(sd, b[i:i + 32]) for i in range(0, 96, 32)])
    return a, b, fa.numpy(), fb.numpy()


def test_fid_end_to_end_equals_the_fid_of_the_reference_features(sd, sets):
    """Tolerance.  Let X_i = X0_i + d_i be the two feature matrices [n, D] with |d_i|_F <= eps |X0_i|_F (eps: the asserted feature
    bound above), A_i the centred X0_i, a_i = |A_i|_F.  Sigma_i = A_i^T A_i / (n - 1), so
      |delta tr Sigma_i|              <= (2 a_i |d_i| + |d_i|^2) / (n - 1)                     (centring does not lengthen d_i)
      |delta tr (Sigma_1 Sigma_2)^1/2| <= (|d_1| a_2 + a_1 |d_2| + |d_1| |d_2|) / (n - 1)
    because tr (Sigma_1 Sigma_2)^1/2 is the nuclear norm of A_1 A_2^T / (n - 1), the nuclear norm is 1-Lipschitz in itself and
    |P Q^T|_* <= |P|_F |Q|_F; and each mean moves by at most |d_i| / sqrt(n), so with m = (|d_1| + |d_2|) / sqrt(n)
      |delta |mu_1 - mu_2|^2|         <= 2 |mu_1 - mu_2| m + m^2.
    The sum of the four is the tolerance; nothing in it comes from the code under test."""
    from mapdit_amd.fid import FeatureStats, frechet_distance
    a, b, fa, fb = sets
    n = 96
    want = frechet_distance(fa.mean(0), np.cov(fa, rowvar=False), fb.mean(0), np.cov(fb, rowvar=False))
    net = _net(sd, "f16")
    stats = []
    for imgs in (a, b):
        st = FeatureStats(2048, DEV)
        for i in range(0, n, 32):
            st.update(net.features(imgs[i:i + 32].to(DEV)))
        assert st.n == n
        stats.append(st.mean_cov())
    got = frechet_distance(*stats[0], *stats[1])
    eps = BOUND["f16"]
    d1, d2 = eps * np.linalg.norm(fa), eps * np.linalg.norm(fb)
    a1, a2 = np.linalg.norm(fa - fa.mean(0)), np.linalg.norm(fb - fb.mean(0))
    m, dmu = (d1 + d2) / np.sqrt(n), np.linalg.norm(fa.mean(0) - fb.mean(0))
    tol = (2 * a1 * d1 + d1 ** 2 + 2 * a2 * d2 + d2 ** 2 + 2 * (d1 * a2 + a1 * d2 + d1 * d2)) / (n - 1) + 2 * dmu * m + m ** 2
    print(f"fid {got:.6f} vs reference features {want:.6f}: diff {abs(got - want):.3e}, tolerance {tol:.3e}")
    assert want > 0 and abs(got - want) <= tol

    # the first set against itself in another batching: features in chunks of 7, statistics in updates of 40 + 56
    st = FeatureStats(2048, DEV)
    f = _net(sd, "f16", max_batch=7).features(a.to(DEV))
    st.update(f[:40]).update(f[40:])
    mu, sigma = st.mean_cov()
    assert np.array_equal(mu, stats[0][0]) and np.array_equal(sigma, stats[0][1])


# ---- sample_fid.py --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    """A small run directory, made the way tests/test_vae_gpu.py makes its own."""
    from mapdit_amd import train
    root = tmp_path_factory.mktemp("fid_results")
    return train.main(["--synthetic", "--results-dir", str(root), "--model", "DiT-XS/2", "--num-steps", "8", "--batch-size", "8",
                       "--log-every", "4", "--ckpt-every", "8", "--ema-snapshot-every", "2", "--num-classes", "10",
                       "--num-lin-warmup", "2", "--start-decay", "3", "--verbose", "0"])


@pytest.fixture(scope="module")
def inc_file(sd, tmp_path_factory):
    """The random Inception weights as a torch file, fp32, with the keys a loader must ignore (fc.*, AuxLogits.*, num_batches_tracked)."""
    path = str(tmp_path_factory.mktemp("inception_weights") / "inception.pt")
    torch.save({k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}, path)
    return path


def test_command_line_stats_and_compare(sd, inc_file, tmp_path, capsys):
    """``python -m mapdit_amd.fid stats`` and ``compare``: statistics of an image array, a file against itself, an array against a file."""
    from mapdit_amd import fid as FID
    g = torch.Generator().manual_seed(9)
    a = torch.randint(0, 256, (8, 16, 16, 3), generator=g, dtype=torch.uint8).numpy()
    b = torch.randint(64, 256, (8, 24, 16, 3), generator=g, dtype=torch.uint8).numpy()
    np.savez(tmp_path / "a.npz", arr_0=a)
    np.save(tmp_path / "b.npy", b)
    ref = str(tmp_path / "a_stats.npz")
    assert FID.main(["stats", "--images", str(tmp_path / "a.npz"), "--inception-weights", inc_file, "--output", ref, "--batch-size", "3"]) == ref
    mu, sigma = FID.load_stats(ref)
    st = FID.FeatureStats(2048, DEV).update(_net({k: v.float() for k, v in sd.items() if v.is_floating_point()}).features(torch.from_numpy(a).to(DEV)))
    assert np.array_equal(mu, st.mean_cov()[0]) and np.array_equal(sigma, st.mean_cov()[1])      # fp32 file, batches of 3: the same bits
    capsys.readouterr()
    same = FID.main(["compare", ref, ref])
    assert f"fid: {same:.6f}" in capsys.readouterr().out.splitlines()
    # rank 7 of 2048: the floor of the sqrt-of-eigenvalues form (tests/test_fid_cpu.py), D sqrt(D eps) lambda_max
    assert abs(same) <= 2048 * np.sqrt(2048 * np.finfo(np.float64).eps) * np.linalg.eigvalsh(sigma)[-1]
    other = FID.main(["compare", str(tmp_path / "b.npy"), ref, "--inception-weights", inc_file])
    assert np.isfinite(other) and other > 10 * abs(same) and other > 0
    with pytest.raises(ValueError, match="--inception-weights"):
        FID.main(["compare", str(tmp_path / "b.npy"), ref])
    with pytest.raises(ValueError, match="uint8"):
        np.save(tmp_path / "f.npy", a.astype(np.float32))
        FID.main(["stats", "--images", str(tmp_path / "f.npy"), "--inception-weights", inc_file, "--output", str(tmp_path / "f.npz")])


def test_sample_fid_writes_the_fid(sd, inc_file, run_dir, tmp_path, monkeypatch, capsys):
    from mapdit_amd import sample_fid
    from mapdit_amd.fid import FeatureStats, frechet_distance, load_stats, save_stats
    vae_w, inc_w, ref = str(tmp_path / "tiny_vae.safetensors"), inc_file, str(tmp_path / "ref.npz")
    VR.write_safetensors(VR.init_state_dict(VR.TINY, seed=2, generation="old"), vae_w)
    rng = np.random.default_rng(8)
    save_stats(ref, 0.5 + 0.1 * rng.standard_normal(2048), np.eye(2048) * 0.05)
    base = ["--result-dir", run_dir, "--num-classes", "10", "--num-sampling-steps", "2", "--batch-size", "4", "--num-samples", "6"]
    value = sample_fid.main(base + ["--vae-weights", vae_w, "--fid-ref", ref, "--inception-weights", inc_w, "--output-file", "px.npz"])
    assert isinstance(value, float) and np.isfinite(value) and value > 0 and f"fid: {value:.6f}" in capsys.readouterr().out
    npz = os.path.join(run_dir, "fid_samples", "px.npz")
    rec = json.load(open(npz + ".fid.json"))
    assert rec == {"fid": value, "n": 6, "ref": ref, "precision": "f16", "samples": npz}
    # the number is the FID of the stored array: the same bytes through the same network in one batch
    arr = np.load(npz)["arr_0"]
    assert arr.shape == (6, 128, 128, 3) and arr.dtype == np.uint8
    net = _net({k: v.float() for k, v in sd.items() if v.is_floating_point()})
    st = FeatureStats(2048, DEV).update(net.features(torch.from_numpy(arr).to(DEV)))
    assert frechet_distance(*st.mean_cov(), *load_stats(ref)) == value
    # the same pixels without the flags: the array does not change
    plain = sample_fid.main(base + ["--vae-weights", vae_w, "--output-file", "px_plain.npz"])
    assert np.array_equal(np.load(plain)["arr_0"], arr) and not os.path.exists(plain + ".fid.json")
    # the default invocation neither needs nor touches the new module: byte-identical output with mapdit_amd.fid unimportable
    lat = sample_fid.main(base + ["--use-vae", "false", "--output-file", "lat_a.npz"])
    import mapdit_amd
    monkeypatch.setitem(sys.modules, "mapdit_amd.fid", None)
    monkeypatch.delattr(mapdit_amd, "fid", raising=False)
    with pytest.raises(ImportError):
        import mapdit_amd.fid  # noqa: F401
    lat_b = sample_fid.main(base + ["--use-vae", "false", "--output-file", "lat_b.npz"])
    assert open(lat, "rb").read() == open(lat_b, "rb").read()
    with pytest.raises(ValueError, match="pixels"):
        sample_fid.main(base + ["--use-vae", "false", "--fid-ref", ref, "--inception-weights", inc_w])
