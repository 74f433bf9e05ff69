"""The pairwise-Gram kernel of csrc/manifold.hip and map-dit_amd/metrics.py on the GPU against the fp64 restatement
(tests/metrics_reference.py): exact integer cases (every dot product and distance an integer in fp32, full of ties), the numerics
fixture, the polynomial kernel sums and KID, the refusals, and ``fid features`` / ``compare --metrics`` end to end.

Measured on an MI355X (every test prints its figures):
  radii at D = 2048: max |fp32 - fp64| 8.2e-4 (333 rows) and 6.6e-4 (200 rows), 0.51 and 0.47 of the band
    4 x 3.5e-7 x (n_i + n_j) of the worst row (1.42e-3 .. 1.76e-3 over the rows); no pair at D = 256 or D = 2048 lies inside the band of a radius other than its own;
  polynomial kernel sum at D = 256, 200 x 333: library rel err 1.3e-10, numpy fp32 Gram 1.1e-10 (bound 4 x: 4.3e-10);
  KID, 5 subsets of 64: mean, library |err| 2.0e-9, numpy fp32 Gram 1.8e-9 (bound 4 x: 7.3e-9); std, library |err| 3.7e-11, numpy
    fp32 Gram's worst subset 4.3e-9 (bound 4 x: 1.7e-8)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inception_reference as IR  # noqa: E402
import metrics_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNKS = (1, 2, 5)
EPS = 4 * 3.5e-7          # the fp32 MFMA chain's error figure at K = 4096, x 4 for the norm rounding and the final fma


def _M():
    import mapdit_amd.metrics as M
    return M


def _dev(x):
    return torch.from_numpy(np.array(x, np.float32)).to(DEV)


def _ints(seed, n, D=36):
    return np.random.default_rng(seed).integers(0, 8, (n, D)).astype(np.float32)


@pytest.fixture(scope="module")
def exact():
    """Q (200) and R (333), integers in [0, 7], D = 36, with the restatement's distances and radii (computed once, never changed)."""
    q, r = _ints(1, 200), _ints(2, 333)
    d = R.sqdist(q, r)
    out = dict(q=q, r=r, d=d, rad_q=R.knn_radii(q, 3), rad_r=R.knn_radii(r, 3))
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- exact cases --------------------------------------------------------------------------------------------------------------------
def test_exact_radii_equal_the_restatement_for_every_slicing(exact):
    M = _M()
    for name, rad in (("q", exact["rad_q"]), ("r", exact["rad_r"])):
        x = _dev(exact[name])
        got = [M.knn_radii(x, 3, chunks=c) for c in CHUNKS + (0,)]
        assert got[0].dtype == torch.float32 and got[0].is_cuda and got[0].shape == (len(rad),)
        assert np.array_equal(got[0].cpu().numpy().astype(np.float64), rad)
        assert all(torch.equal(got[0], g) for g in got[1:])
    for k in (1, 8):
        assert np.array_equal(M.knn_radii(_dev(exact["r"]), k, chunks=2).cpu().numpy().astype(np.float64), R.knn_radii(exact["r"], k))
    assert len(np.unique(exact["rad_r"])) < len(exact["rad_r"]) // 2      # integers: the radii are full of ties


def test_exact_counts_in_both_modes(exact):
    M = _M()
    q, r = _dev(exact["q"]), _dev(exact["r"])
    rad_q, rad_r = _dev(exact["rad_q"]), _dev(exact["rad_r"])
    want_ref, want_query = R.count_ref_radius(None, None, exact["rad_r"], exact["d"]), R.count_query_radius(None, None, exact["rad_q"], exact["d"])
    assert int((exact["d"] == exact["rad_r"][None, :]).sum()) >= 10        # pairs exactly on a radius: <= must count them
    for mode, rad, want in (("ref", rad_r, want_ref), ("query", rad_q, want_query)):
        got = [M.ball_count(q, r, rad, mode, chunks=c) for c in CHUNKS + (0,)]
        assert got[0].dtype == torch.int64 and np.array_equal(got[0].cpu().numpy(), want), mode
        assert all(torch.equal(got[0], g) for g in got[1:])
    # the transposed problem: 333 queries against 200 references
    want_t = R.count_ref_radius(None, None, exact["rad_q"], exact["d"].T)
    assert np.array_equal(M.ball_count(r, q, rad_q, "ref", chunks=2).cpu().numpy(), want_t)
    assert not np.array_equal(want_ref, want_query)


def test_exact_poly_kernel_sum(exact):
    M = _M()
    q, r = _dev(exact["q"]), _dev(exact["r"])
    want = R.poly_kernel_sum(exact["q"], exact["r"], 1 / 64, 1.0, 3)
    got = [M.poly_kernel_sum(q, r, 1 / 64, 1.0, 3, chunks=c) for c in CHUNKS + (0,)]
    assert got[0].dtype == torch.float64 and got[0].is_cuda and float(got[0]) == want
    assert all(torch.equal(got[0], g) for g in got[1:])
    assert float(M.poly_kernel_sum(r, q, 1 / 64, 1.0, 3)) == want
    for deg in (1, 2, 4):
        assert float(M.poly_kernel_sum(q, r, 1 / 64, 1.0, deg, chunks=2)) == R.poly_kernel_sum(exact["q"], exact["r"], 1 / 64, 1.0, deg)
    want_off = R.poly_kernel_sum(exact["r"], exact["r"], 1 / 64, 1.0, 3, skip_diag=True)
    assert [float(M.poly_kernel_sum(r, r, 1 / 64, 1.0, 3, True, chunks=c)) for c in CHUNKS] == [want_off] * 3
    assert float(M.poly_kernel_sum(r, r, 1 / 64, 1.0, 3)) == R.poly_kernel_sum(exact["r"], exact["r"], 1 / 64, 1.0, 3) != want_off


def test_self_exclusion_across_a_tile_edge():
    """N = 130: rows 128 and 129 lie in the second tile; the diagonal crosses the tile edge."""
    M = _M()
    x = _ints(3, 130)
    xd = _dev(x)
    rad = R.knn_radii(x, 3)
    for c in (1, 2):
        assert np.array_equal(M.knn_radii(xd, 3, chunks=c).cpu().numpy().astype(np.float64), rad)
    d = R.sqdist(x, x)
    with_self = M.ball_count(xd, xd, _dev(rad), "ref", chunks=2).cpu().numpy()
    no_self = M.ball_count(xd, xd, _dev(rad), "ref", exclude_self=True, chunks=2).cpu().numpy()
    assert np.array_equal(with_self, R.count_ref_radius(None, None, rad, d))
    assert np.array_equal(no_self, with_self - 1)                          # d2(q, q) = 0 <= rad[q]: the self hit, and nothing else, is gone
    off = d + np.where(np.eye(130, dtype=bool), np.inf, 0.0)
    assert np.array_equal(no_self, R.count_ref_radius(None, None, rad, off))
    q_self = M.ball_count(xd, xd, _dev(rad), "query", exclude_self=True).cpu().numpy()
    assert np.array_equal(q_self, R.count_query_radius(None, None, rad, off)) and q_self.min() >= 3


def test_nine_rows_k8_and_duplicate_rows():
    M = _M()
    x = _ints(4, 9)
    assert np.array_equal(M.knn_radii(_dev(x), 8).cpu().numpy().astype(np.float64), R.knn_radii(x, 8))
    y = _ints(5, 140)
    y[131] = y[7]                                                          # the same row at another index: a neighbour at distance 0
    got = M.knn_radii(_dev(y), 1, chunks=2).cpu().numpy().astype(np.float64)
    assert got[7] == 0.0 and got[131] == 0.0 and np.array_equal(got, R.knn_radii(y, 1)) and (got > 0).sum() >= 130


def test_row_sqnorm_is_the_fp64_sum_rounded_once():
    import mapdit_amd._lib as L
    x = np.random.default_rng(6).standard_normal((37, 2052)).astype(np.float32)
    xd, out = _dev(x), torch.empty(37, dtype=torch.float32, device=DEV)
    L.lib().row_sqnorm(xd.data_ptr(), 37, 2052, out.data_ptr(), L.cur_stream())
    want = (x.astype(np.float64) ** 2).sum(1)
    got = out.cpu().numpy()
    assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(want.astype(np.float32)) * 0.5000001)


# ---- numerics -----------------------------------------------------------------------------------------------------------------------
def test_numerics_d256_counts_and_metrics_equal_the_restatement():
    """real = set B (333), fake = set A (200).  The fp64 reference shows that no compared pair lies within the fp32 band of its
    radius, so counts and all four metrics must equal the restatement exactly."""
    M = _M()
    fake, real = R.clusters(0, 256)
    r_real, r_fake = R.knn_radii(real, 3), R.knn_radii(fake, 3)
    amb = (R.ambiguous_pairs(fake, real, r_real, "ref", EPS), R.ambiguous_pairs(real, fake, r_fake, "ref", EPS),
           R.ambiguous_pairs(real, fake, r_real, "query", EPS))
    print(f"ambiguous pairs at D = 256 (fake->real, real->fake, coverage): {amb}")
    assert amb == (0, 0, 0)
    want = R.precision_recall(real, fake, 3)
    assert round(want["precision"], 3) == 0.955 and round(want["recall"], 3) == 0.300
    fd, rd = _dev(fake), _dev(real)
    d = R.sqdist(fake, real)
    g_real, g_fake = M.knn_radii(rd, 3), M.knn_radii(fd, 3)
    assert np.array_equal(M.ball_count(fd, rd, g_real, "ref").cpu().numpy(), R.count_ref_radius(None, None, r_real, d))
    assert np.array_equal(M.ball_count(rd, fd, g_fake, "ref").cpu().numpy(), R.count_ref_radius(None, None, r_fake, d.T))
    assert np.array_equal(M.ball_count(rd, fd, g_real, "query").cpu().numpy(), R.count_query_radius(None, None, r_real, d.T))
    got = M.precision_recall(rd, fd, 3)
    print(f"D = 256: {got}")
    assert got == want and got == M.precision_recall(rd, fd, 3, chunks=2)


def test_numerics_d2048_radii_within_the_band():
    M = _M()
    fake, real = R.clusters(0, 2048)
    worst = 0.0
    for x in (real, fake):
        d = R.sqdist(x, x)
        np.fill_diagonal(d, np.inf)
        kth = np.argsort(d, axis=1, kind="stable")[:, 2]
        want = d[np.arange(len(x)), kth]
        n = (x.astype(np.float64) ** 2).sum(1)
        band = EPS * (n + n[kth])
        assert R.ambiguous_pairs(x, x, want, "ref", EPS) == len(x)          # only each row's own k-th neighbour sits on its radius
        got = M.knn_radii(_dev(x), 3).cpu().numpy().astype(np.float64)
        err = np.abs(got - want)
        worst = max(worst, float((err / band).max()))
        print(f"D = 2048, {len(x)} rows: radii mean {want.mean():.1f}, max |err| {err.max():.3e}, band {band.min():.3e}, worst err / band {(err / band).max():.3f}")
        assert np.all(err <= band)
    assert worst > 0.0


def _fp32_gram_sum(a, b, gamma, skip_diag=False):
    """The kernel's arithmetic with numpy's fp32 Gram: polynomial and sum in fp64."""
    k = (gamma * (a @ b.T).astype(np.float64) + 1.0) ** 3
    return float(k.sum() - (np.trace(k) if skip_diag else 0.0))


def test_poly_kernel_sum_d256_within_four_times_the_fp32_gram_error():
    M = _M()
    a, b = R.clusters(0, 256)
    want = R.poly_kernel_sum(a, b, 1 / 256, 1.0, 3)
    e_np = abs(_fp32_gram_sum(a, b, 1 / 256) - want) / want
    got = float(M.poly_kernel_sum(_dev(a), _dev(b), 1 / 256, 1.0, 3))
    e = abs(got - want) / want
    print(f"poly kernel sum D = 256: library rel err {e:.3e}, numpy fp32 Gram rel err {e_np:.3e}, bound {4 * e_np:.3e}")
    assert e <= 4 * e_np
    assert got == float(M.poly_kernel_sum(_dev(a), _dev(b), 1 / 256, 1.0, 3, chunks=2))


def test_kid_matches_the_restatement_on_the_same_subsets():
    M = _M()
    fake, real = R.clusters(0, 256)
    pairs = M.kid_subsets(len(real), len(fake), 5, 64, seed=0)
    want = np.array([R.mmd2_unbiased(real[i], fake[j]) for i, j in pairs])             # what R.kid takes the mean and std of
    want_mean, want_std = float(want.mean()), float(want.std())
    est_np = []
    for i, j in pairs:
        x, y = real[i], fake[j]
        est_np.append(M.mmd2_unbiased(_fp32_gram_sum(x, x, 1 / 256, True), _fp32_gram_sum(y, y, 1 / 256, True), _fp32_gram_sum(x, y, 1 / 256), 64))
    e_np = abs(float(np.mean(est_np)) - want_mean)
    e_np_worst = float(np.abs(np.array(est_np) - want).max())
    mean, std = M.kid(_dev(real), _dev(fake), 5, 64, seed=0)
    print(f"kid: {mean:.9f} +- {std:.3e} (restatement {want_mean:.9f} +- {want_std:.3e}); |err| {abs(mean - want_mean):.3e}, "
          f"numpy fp32 Gram |err| {e_np:.3e}, bound {4 * e_np:.3e}")
    assert want_mean > 0 and abs(mean - want_mean) <= 4 * e_np
    # the std of the estimates moves by no more than the largest change of one estimate (|std(a) - std(b)| <= std(a - b) <= max |a - b|):
    # its bound is the mean's rule applied to the worst subset, 4 x the numpy fp32 Gram's largest per-subset error
    print(f"kid std: |err| {abs(std - want_std):.3e}, numpy fp32 Gram worst subset |err| {e_np_worst:.3e}, bound {4 * e_np_worst:.3e}")
    assert abs(std - want_std) <= 4 * e_np_worst
    assert (mean, std) == M.kid(_dev(real), _dev(fake), 5, 64, seed=0, chunks=2)
    with pytest.raises(ValueError, match="subset_size"):
        M.kid(_dev(real), _dev(fake), 5, 201)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    import mapdit_amd._lib as L
    M = _M()
    lib = L.lib()
    x = _dev(_ints(7, 40))
    with pytest.raises(ValueError, match="D=30"):
        M.knn_radii(torch.zeros(40, 30, device=DEV))
    with pytest.raises(L.MapditError, match="k=8"):
        M.knn_radii(x[:8].clone(), 8)
    with pytest.raises(NotImplementedError):
        M.knn_radii(x.cpu())
    with pytest.raises(ValueError, match="fp32"):
        M.knn_radii(x.double())
    # a short workspace, straight at the C entry points: the outputs keep their fill
    radii = torch.full((40,), -7.0, device=DEV)
    count = torch.full((40,), -7, dtype=torch.int32, device=DEV)
    out = torch.full((), -7.0, dtype=torch.float64, device=DEV)
    need = lib.knn_radii_workspace_bytes(40, 36, 2)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    s = L.cur_stream()
    with pytest.raises(L.MapditError, match="workspace"):
        lib.knn_radii(x.data_ptr(), 40, 36, 3, radii.data_ptr(), 2, ws.data_ptr(), need - 1, s)
    with pytest.raises(L.MapditError, match="workspace"):
        lib.ball_count(x.data_ptr(), 40, x.data_ptr(), 40, 36, radii.data_ptr(), 0, 0, count.data_ptr(), 1, ws.data_ptr(), 64, s)
    with pytest.raises(L.MapditError, match="workspace"):
        lib.poly_kernel_sum(x.data_ptr(), 40, x.data_ptr(), 40, 36, 1.0, 1.0, 3, 0, out.data_ptr(), 0, ws.data_ptr(), 8, s)
    with pytest.raises(L.MapditError, match="k=40"):
        lib.knn_radii(x.data_ptr(), 40, 36, 40, radii.data_ptr(), 2, ws.data_ptr(), need, s)
    torch.cuda.synchronize()
    assert bool((radii == -7.0).all()) and bool((count == -7).all()) and float(out) == -7.0
    lib.knn_radii(x.data_ptr(), 40, 36, 3, radii.data_ptr(), 2, ws.data_ptr(), need, s)          # the exact size is enough
    assert bool((radii >= 0).all())


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_features_then_compare_with_metrics(tmp_path, capsys):
    """``fid features`` on two image sets through the random-weight Inception network, then ``compare --metrics fid,pr,kid`` on the two
    files: the printed values are metrics.* called directly on the stored features."""
    from mapdit_amd import fid as FID
    M = _M()
    sd = IR.init_state_dict(seed=3)
    inc = str(tmp_path / "inception.pt")
    torch.save({k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}, inc)
    g = torch.Generator().manual_seed(11)
    a = torch.randint(0, 256, (24, 64, 64, 3), generator=g, dtype=torch.uint8).numpy()
    b = torch.randint(0, 256, (20, 64, 64, 3), generator=g, dtype=torch.uint8).numpy()
    files = []
    for name, arr in (("a", a), ("b", b)):
        np.savez(tmp_path / f"{name}.npz", arr_0=arr)
        files.append(str(tmp_path / f"{name}_feats.npz"))
        assert FID.main(["features", "--images", str(tmp_path / f"{name}.npz"), "--inception-weights", inc, "--output", files[-1], "--batch-size", "16"]) == files[-1]
    fa, fb = FID.load_features(files[0]), FID.load_features(files[1])
    assert fa.shape == (24, 2048) and fb.shape == (20, 2048) and fa.dtype == np.float32
    mu, sigma = FID.load_stats(files[0])
    assert np.allclose(mu, fa.astype(np.float64).mean(0), rtol=0, atol=1e-9 * np.abs(mu).max() + 1e-12) and sigma.shape == (2048, 2048)
    capsys.readouterr()
    fid_only = FID.main(["compare", files[0], files[1]])
    assert capsys.readouterr().out == f"fid: {fid_only:.6f}\n"
    values = FID.main(["compare", files[0], files[1], "--metrics", "fid,pr,kid", "--kid-subsets", "3", "--kid-subset-size", "16"])
    lines = capsys.readouterr().out.splitlines()
    assert lines == [f"{k}: {v:.6f}" for k, v in values.items()]
    assert list(values) == ["fid", "precision", "recall", "density", "coverage", "kid", "kid_std"] and values["fid"] == fid_only
    want = M.precision_recall(_dev(fa), _dev(fb), 3)
    want["kid"], want["kid_std"] = M.kid(_dev(fa), _dev(fb), 3, 16, seed=0)
    assert {k: values[k] for k in want} == want
    ref = R.precision_recall(fa, fb, 3)
    print(f"end to end: {values}; restatement {ref}")
    assert all(0.0 <= values[k] <= 1.0 for k in ("precision", "recall", "coverage")) and np.isfinite(values["kid"])
    # an image array on one side, the weights given: the same features, the same values
    mixed = FID.main(["compare", files[0], str(tmp_path / "b.npz"), "--metrics", "pr", "--inception-weights", inc, "--batch-size", "16"])
    assert mixed == {k: values[k] for k in ("precision", "recall", "density", "coverage")}


def test_sample_fid_adds_the_metrics_to_its_record(tmp_path, capsys):
    """``sample_fid.py --metrics fid,pr,kid`` against a features file: the values in ``.fid.json`` and on the output are metrics.* of
    the stored array's features against the reference's, the FID line stays what it is without the flag."""
    import json
    import vae_reference as VR
    from mapdit_amd import fid as FID
    from mapdit_amd import sample_fid, train
    M = _M()
    run_dir = train.main(["--synthetic", "--results-dir", str(tmp_path / "results"), "--model", "DiT-XS/2", "--num-steps", "8", "--batch-size", "8",
                          "--log-every", "4", "--ckpt-every", "8", "--ema-snapshot-every", "2", "--num-classes", "10",
                          "--num-lin-warmup", "2", "--start-decay", "3", "--verbose", "0"])
    sd = IR.init_state_dict(seed=3)
    inc, vae_w, ref = str(tmp_path / "inception.pt"), str(tmp_path / "tiny_vae.safetensors"), str(tmp_path / "ref_feats.npz")
    torch.save({k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}, inc)
    VR.write_safetensors(VR.init_state_dict(VR.TINY, seed=2, generation="old"), vae_w)
    net = FID.InceptionFeatures.from_file(inc, DEV)
    imgs = torch.randint(0, 256, (10, 32, 32, 3), generator=torch.Generator().manual_seed(12), dtype=torch.uint8)
    ref_feat = net.features(imgs.to(DEV))
    FID.save_features(ref, ref_feat.cpu().numpy(), *FID.FeatureStats(2048, DEV).update(ref_feat).mean_cov())
    base = ["--result-dir", run_dir, "--num-classes", "10", "--num-sampling-steps", "2", "--batch-size", "4", "--num-samples", "6",
            "--vae-weights", vae_w, "--fid-ref", ref, "--inception-weights", inc]
    plain = sample_fid.main(base + ["--output-file", "plain.npz"])
    assert capsys.readouterr().out.splitlines()[-1] == f"fid: {plain:.6f}"
    value = sample_fid.main(base + ["--output-file", "m.npz", "--metrics", "fid,pr,kid", "--kid-subsets", "2", "--kid-subset-size", "4"])
    lines = capsys.readouterr().out.splitlines()
    npz = os.path.join(run_dir, "fid_samples", "m.npz")
    rec = json.load(open(npz + ".fid.json"))
    assert value == plain == rec["fid"] and rec["n"] == 6
    feat = net.features(torch.from_numpy(np.load(npz)["arr_0"]).to(DEV))
    want = M.precision_recall(ref_feat, feat, 3)
    want["kid"], want["kid_std"] = M.kid(ref_feat, feat, 2, 4, seed=0)
    assert rec["metrics"] == want and list(rec["metrics"]) == list(want)
    assert rec["precision"] == "f16" and set(rec) == {"fid", "n", "ref", "precision", "samples", "metrics"}      # the operand format stays
    assert lines[-7:] == [f"fid: {value:.6f}"] + [f"{k}: {v:.6f}" for k, v in want.items()]
    assert set(json.load(open(os.path.join(run_dir, "fid_samples", "plain.npz.fid.json")))) == {"fid", "n", "ref", "precision", "samples"}
