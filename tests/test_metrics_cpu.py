"""Host side of the metrics beside the FID (map-dit_amd/metrics.py, the ``features`` subcommand and ``--metrics`` of fid.py and
sample_fid.py): the ABI of csrc/manifold.hip, the yardstick's own properties (tests/metrics_reference.py), the KID subset draws and
estimator, the command-line refusals and the features file.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_reference as R  # noqa: E402

NEW = ["mapdit_row_sqnorm", "mapdit_knn_radii", "mapdit_knn_radii_workspace_bytes", "mapdit_ball_count", "mapdit_ball_count_workspace_bytes",
       "mapdit_poly_kernel_sum", "mapdit_poly_kernel_sum_workspace_bytes"]


def _lib():
    import mapdit_amd
    return mapdit_amd._lib


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_manifold_functions():
    L = _lib()
    if not os.path.exists(L.LIB_PATH):
        L.build()
    cdll = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in L.ABI.functions, f"{name} is not declared in mapdit.h"
        assert hasattr(cdll, name), f"{name} is not exported by libmapdit_hip.so"
    assert L.BALL_REF_RADIUS == 0 and L.BALL_QUERY_RADIUS == 1
    assert L.ABI.functions["mapdit_poly_kernel_sum_workspace_bytes"][0] == "size_t"
    assert cdll.mapdit_abi_version() == 5                                  # functions were only added


def test_workspace_queries_and_host_refusals():
    """Host logic only: the sizes follow the documented layout and every refusal comes with its message before any launch."""
    L = _lib()
    lib = L.lib()
    up = lambda n: (4 * n + 255) // 256 * 256                              # noqa: E731
    assert lib.knn_radii_workspace_bytes(200, 36, 5) == up(200) + 5 * 200 * 8 * 4
    assert lib.ball_count_workspace_bytes(200, 333, 36, 2) == up(200) + up(333) + 2 * 200 * 4
    assert lib.poly_kernel_sum_workspace_bytes(200, 333, 36, 0) == 2 * 3 * 4 * 8 == lib.poly_kernel_sum_workspace_bytes(200, 333, 36, 5)
    # chunks = 0: two workgroups per CU of 256 where the reference tiles allow it, never more slices than tiles
    assert lib.knn_radii_workspace_bytes(10_000, 2048, 0) == up(10_000) + 7 * 10_000 * 32        # 79 query tiles: ceil(512 / 79) = 7
    assert lib.knn_radii_workspace_bytes(130, 36, 0) == up(130) + 2 * 130 * 32                    # 2 tiles
    for call, word in ((lambda: lib.knn_radii_workspace_bytes(200, 30, 0), b"D=30"), (lambda: lib.knn_radii_workspace_bytes(200, 65540, 0), b"D=65540"),
                       (lambda: lib.ball_count_workspace_bytes((1 << 30) + 1, 10, 64, 0), b"rows"),
                       (lambda: lib.poly_kernel_sum_workspace_bytes(10, 0, 64, 0), b"rows"),
                       (lambda: lib.knn_radii_workspace_bytes(200, 64, 70000), b"chunks")):
        assert call() == 0 and word in lib.last_error(), lib.last_error()
    # entry points refuse on the host: null pointers, k, degree, self without Q == R (no device pointer is touched before the checks)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf) // 256 * 256 + 256                           # any aligned non-null value: refused before it is read
    for call, word in ((lambda: lib.knn_radii(None, 9, 36, 3, p, 0, p, 1 << 20, None), "null"),
                       (lambda: lib.knn_radii(p + 4, 9, 36, 3, p, 0, p, 1 << 20, None), "aligned"),
                       (lambda: lib.knn_radii(p, 9, 36, 9, p, 0, p, 1 << 20, None), "k=9"),
                       (lambda: lib.knn_radii(p, 9, 36, 0, p, 0, p, 1 << 20, None), "k=0"),
                       (lambda: lib.knn_radii(p, 8, 36, 8, p, 0, p, 1 << 20, None), "k=8"),
                       (lambda: lib.knn_radii(p, 9, 36, 3, p, 0, p, 16, None), "workspace"),
                       (lambda: lib.ball_count(p, 9, p + 256, 9, 36, p, 0, 1, p, 0, p, 1 << 20, None), "self"),
                       (lambda: lib.ball_count(p, 9, p, 9, 36, p, 2, 0, p, 0, p, 1 << 20, None), "mode"),
                       (lambda: lib.poly_kernel_sum(p, 9, p, 9, 36, 1.0, 1.0, 5, 0, p, 0, p, 1 << 20, None), "degree"),
                       (lambda: lib.poly_kernel_sum(p, 9, p + 256, 9, 36, 1.0, 1.0, 3, 1, p, 0, p, 1 << 20, None), "skip_diag"),
                       (lambda: lib.row_sqnorm(p, 9, 34, p, None), "D=34")):
        with pytest.raises(L.MapditError, match=word):
            call()


def test_cpu_tensors_are_refused():
    import mapdit_amd.metrics as M
    x = torch.zeros(16, 8)
    for call in (lambda: M.knn_radii(x), lambda: M.precision_recall(x, x), lambda: M.kid(x, x, 2, 4), lambda: M.ball_count(x, x, torch.zeros(16)),
                 lambda: M.poly_kernel_sum(x, x, 1.0)):
        with pytest.raises(NotImplementedError):
            call()


# ---- the yardstick's own properties -------------------------------------------------------------------------------------------------
def test_reference_identical_sets_score_one_and_far_clusters_zero():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 12))
    same = R.precision_recall(x, x.copy(), 3)
    assert same["precision"] == same["recall"] == same["coverage"] == 1.0 and same["density"] >= 1.0
    far = R.precision_recall(x, x + 100.0, 3)
    assert far == {"precision": 0.0, "recall": 0.0, "density": 0.0, "coverage": 0.0}


def test_reference_radii_ties_and_duplicates():
    x = np.array([[0.0, 0.0], [0.0, 0.0], [3.0, 4.0], [6.0, 8.0]])        # rows 0 and 1 identical: a neighbour at distance 0, not the row itself
    assert R.knn_radii(x, 1).tolist() == [0.0, 0.0, 25.0, 25.0]
    assert R.knn_radii(x, 2).tolist() == [25.0, 25.0, 25.0, 100.0]
    assert R.count_ref_radius(x, x, [0.0, 0.0, 25.0, 0.0]).tolist() == [3, 3, 1, 2]          # <=: a tie is inside
    assert R.count_query_radius(x, x, [25.0, 0.0, 24.9, 100.0]).tolist() == [3, 2, 1, 4]
    assert R.ambiguous_pairs(x, x, [25.0, 25.0, 25.0, 100.0], "ref") > 0


def test_reference_numerics_fixture_is_the_stated_one():
    """The fixture of the GPU numerics cases: D = 256, seed 0, real = set B (333 rows), fake = set A (200 rows)."""
    a, b = R.clusters(0, 256)
    assert a.shape == (200, 256) and b.shape == (333, 256) and a.dtype == np.float32 and float(a.min()) == 0.0
    pr = R.precision_recall(b, a, 3)
    assert round(pr["precision"], 3) == 0.955 and round(pr["recall"], 3) == 0.300


# ---- KID ----------------------------------------------------------------------------------------------------------------------------
def test_kid_subsets_are_a_function_of_the_seed_only():
    import mapdit_amd.metrics as M
    a, b = M.kid_subsets(50, 70, 4, 20, seed=5), M.kid_subsets(50, 70, 4, 20, seed=5)
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
    rng = np.random.RandomState(5)
    for ir, jf in a:                                                       # per subset: real first, then fake, from one stream
        assert np.array_equal(ir, rng.choice(50, 20, replace=False)) and np.array_equal(jf, rng.choice(70, 20, replace=False))
        assert len(set(ir.tolist())) == 20 and ir.max() < 50 and jf.max() < 70
    assert not np.array_equal(a[0][0], M.kid_subsets(50, 70, 4, 20, seed=6)[0][0])
    for bad in ((50, 70, 4, 51), (70, 50, 4, 51), (50, 70, 0, 20), (50, 70, 4, 1)):
        with pytest.raises(ValueError):
            M.kid_subsets(*bad)


def test_mmd2_assembles_from_three_sums():
    import mapdit_amd.metrics as M
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal((12, 8)), rng.standard_normal((12, 8)) + 0.5
    sums = (R.poly_kernel_sum(x, x, 1 / 8, 1.0, 3, True), R.poly_kernel_sum(y, y, 1 / 8, 1.0, 3, True), R.poly_kernel_sum(x, y, 1 / 8, 1.0, 3))
    want = R.mmd2_unbiased(x, y)                                           # the double loop of the definition
    assert want > 0 and abs(M.mmd2_unbiased(*sums, 12) - want) <= 1e-12 * abs(want) + 1e-13
    assert M.mmd2_unbiased(6.0, 12.0, 18.0, 3) == 6 / 6 + 12 / 6 - 2 * 18 / 9


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def _stats_file(path, d=2048):
    np.savez(path, mu=np.zeros(d), sigma=np.eye(d))
    return str(path)


def test_parse_metrics():
    import mapdit_amd.fid as FID
    assert FID.parse_metrics(None) == ("fid",) == FID.parse_metrics("fid")
    assert FID.parse_metrics("kid, pr,fid") == ("fid", "pr", "kid") and FID.parse_metrics("pr") == ("pr",)
    for bad in ("is", "fid,sfid", ","):
        with pytest.raises(ValueError, match="--metrics"):
            FID.parse_metrics(bad)
    args = FID.build_parser().parse_args(["compare", "a", "b"])
    assert args.metrics is None and args.kid_subsets == 100 and args.kid_subset_size == 1000


def test_compare_refuses_statistics_only_files_for_pr_and_kid(tmp_path, monkeypatch):
    import mapdit_amd.fid as FID
    monkeypatch.setattr(FID.InceptionFeatures, "from_file", lambda *a, **k: pytest.fail("the network was built"))
    st = _stats_file(tmp_path / "ref.npz")
    feats = str(tmp_path / "feats.npz")
    FID.save_features(feats, np.zeros((4, 2048), np.float32), np.zeros(2048), np.eye(2048))
    for metrics in ("pr", "kid", "fid,pr,kid"):
        for a, b in ((st, feats), (feats, st)):
            with pytest.raises(ValueError, match=r"statistics only.*fid features"):
                FID.main(["compare", a, b, "--metrics", metrics, "--inception-weights", "w.pt"])
    imgs = str(tmp_path / "imgs.npz")
    np.savez(imgs, arr_0=np.zeros((2, 8, 8, 3), np.uint8))
    with pytest.raises(ValueError, match="--inception-weights"):         # an image array without the weights
        FID.main(["compare", feats, imgs, "--metrics", "pr"])
    with pytest.raises(ValueError, match="--metrics"):
        FID.main(["compare", feats, feats, "--metrics", "precision"])


def test_default_compare_output_is_todays_line(tmp_path, capsys):
    """Without --metrics (and with --metrics fid) two statistics files print the one line `fid: <value>` and need no GPU."""
    import mapdit_amd.fid as FID
    a = str(tmp_path / "a.npz")
    FID.save_stats(a, np.zeros(6), np.eye(6))
    b = str(tmp_path / "b.npz")
    FID.save_features(b, np.zeros((3, 6), np.float32), np.ones(6), np.eye(6))
    for extra in ([], ["--metrics", "fid"]):
        assert FID.main(["compare", a, b] + extra) == pytest.approx(6.0)
        assert capsys.readouterr().out == "fid: 6.000000\n"


def test_features_file_round_trips_through_load_stats(tmp_path):
    import mapdit_amd.fid as FID
    rng = np.random.default_rng(2)
    feat = rng.standard_normal((10, 2048)).astype(np.float32)
    mu, sigma = feat.mean(0, dtype=np.float64), np.cov(feat.astype(np.float64), rowvar=False)
    p = tmp_path / "feats.npz"
    FID.save_features(p, feat, mu, sigma)
    assert sorted(os.listdir(tmp_path)) == ["feats.npz"]
    mu2, sigma2 = FID.load_stats(p)
    assert np.array_equal(mu, mu2) and np.array_equal(sigma, sigma2) and FID._is_stats(p) and FID.has_features(p)
    assert FID.features_rows(p) == 10 and FID.features_rows(tmp_path / "none.npy") is None      # (the header alone is read)
    got = FID.load_features(p)
    assert got.dtype == np.float32 and np.array_equal(got, feat)
    st = _stats_file(tmp_path / "st.npz")
    assert not FID.has_features(st) and FID.features_rows(st) is None
    with pytest.raises(KeyError, match="fid features"):
        FID.load_features(st)


@pytest.mark.parametrize("flags, match", [
    (["--metrics", "pr"], "needs --fid-ref"),
    (["--metrics", "fid,kid"], "needs --fid-ref"),
    (["--metrics", "fid"], "needs --fid-ref"),
    (["--metrics", "nonsense", "--fid-ref", "REF", "--inception-weights", "W"], "comma-separated"),
    (["--metrics", "pr", "--fid-ref", "REF", "--inception-weights", "W"], "pool_3"),
    (["--metrics", "fid,pr,kid", "--fid-ref", "REF", "--inception-weights", "W"], "fid features"),
])
def test_sample_fid_refuses_metrics_before_any_model_is_built(tmp_path, flags, match):
    from mapdit_amd import sample_fid
    ref, w = _stats_file(tmp_path / "ref.npz"), tmp_path / "w.pt"
    w.write_bytes(b"")
    flags = [ref if f == "REF" else str(w) if f == "W" else f for f in flags]
    with pytest.raises(ValueError, match=match):                          # before config.yaml of the (missing) run directory is read
        sample_fid.main(["--result-dir", str(tmp_path / "no_such_run")] + flags)


def test_sample_fid_accepts_a_features_reference(tmp_path):
    import mapdit_amd.fid as FID
    from mapdit_amd import sample_fid
    ref, w = str(tmp_path / "feats.npz"), tmp_path / "w.pt"
    FID.save_features(ref, np.zeros((4, 2048), np.float32), np.zeros(2048), np.eye(2048))
    w.write_bytes(b"")
    flags = ["--result-dir", "x", "--metrics", "fid,pr,kid", "--fid-ref", ref, "--inception-weights", str(w)]
    args = sample_fid.build_parser().parse_args(flags + ["--kid-subset-size", "4", "--num-samples", "6"])
    assert sample_fid.check_fid_flags(args) is True
    # a KID subset larger than either set is refused here, not after the sampling: 1000 (the default) of 4 reference rows, 5 of 4
    # rows, 4 of 3 samples
    for more in ([], ["--kid-subset-size", "5", "--num-samples", "6"], ["--kid-subset-size", "4", "--num-samples", "3"]):
        with pytest.raises(ValueError, match="--kid-subset-size"):
            sample_fid.check_fid_flags(sample_fid.build_parser().parse_args(flags + more))
    assert sample_fid.check_fid_flags(sample_fid.build_parser().parse_args(flags[:2] + ["--metrics", "pr"] + flags[4:])) is True
    plain = sample_fid.build_parser().parse_args(["--result-dir", "x"])
    assert plain.metrics is None and sample_fid.check_fid_flags(plain) is False
