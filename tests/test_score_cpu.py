"""Host side of the Inception Score (``isc``) and the spatial FID (``fid_s``): the metric names, the statistics file with ``mu_s`` /
``sigma_s``, the classifier head, the host finish of the score against ADM's formula, the command-line refusals and the ABI.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_reference as SR  # noqa: E402

NEW = ["mapdit_softmax_score", "mapdit_softmax_score_workspace_bytes", "mapdit_inc_spatial_shape", "mapdit_inc_features_tap",
       "mapdit_inc_features_tap_f16"]


def _lib():
    import mapdit_amd
    return mapdit_amd._lib


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_new_functions():
    L = _lib()
    if not os.path.exists(L.LIB_PATH):
        L.build()
    cdll = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in L.EXPORTS and name in L.ABI.functions, f"{name} is not declared in mapdit.h"
        assert hasattr(cdll, name), f"{name} is not exported by libmapdit_hip.so"
    assert L.ABI.functions["mapdit_softmax_score_workspace_bytes"][0] == "size_t" and L.INC_SPATIAL_CHANNELS == 7
    assert cdll.mapdit_abi_version() == 5                                  # functions were only added


def test_spatial_shape_and_workspace_are_host_queries():
    L = _lib()
    lib = L.lib()
    v = [ctypes.c_int() for _ in range(3)]
    for size, want in ((299, [17, 17, 7]), (75, [3, 3, 7])):
        cfg = L.IncConfig(image_size=size)
        lib.inc_spatial_shape(ctypes.byref(cfg), *[ctypes.byref(x) for x in v])
        assert [x.value for x in v] == want
    with pytest.raises(L.MapditError, match="image_size"):
        lib.inc_spatial_shape(ctypes.byref(L.IncConfig(image_size=40)), *[ctypes.byref(x) for x in v])
    # softmax_score: (m, s, u) per (class tile, sample), lse and p log p per sample, two partials per (sample tile, class) - each
    # rounded up to 256 bytes; the slicing does not enter
    up = lambda n: (n + 255) // 256 * 256                                  # noqa: E731
    want = up(8 * 130 * 24) + 2 * up(130 * 8) + up(2 * 1008 * 16)
    assert lib.softmax_score_workspace_bytes(130, 1008, 2048, 0) == want == lib.softmax_score_workspace_bytes(130, 1008, 2048, 3)
    for call, word in ((lambda: lib.softmax_score_workspace_bytes(130, 1008, 30, 0), b"D=30"),
                       (lambda: lib.softmax_score_workspace_bytes(130, 1008, 65540, 0), b"D=65540"),
                       (lambda: lib.softmax_score_workspace_bytes(0, 1008, 64, 0), b"rows"),
                       (lambda: lib.softmax_score_workspace_bytes(130, (1 << 30) + 1, 64, 0), b"rows"),
                       (lambda: lib.softmax_score_workspace_bytes(130, 1008, 64, 70000), b"chunks")):
        assert call() == 0 and word in lib.last_error(), lib.last_error()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf) // 256 * 256 + 256                           # any aligned non-null value: refused before it is read
    for call, word in ((lambda: lib.softmax_score(None, 9, p, 5, 36, None, p, p, 0, p, 1 << 20, None), "null"),
                       (lambda: lib.softmax_score(p, 9, p + 4, 5, 36, None, p, p, 0, p, 1 << 20, None), "aligned"),
                       (lambda: lib.softmax_score(p, 9, p, 5, 36, p + 2, p, p, 0, p, 1 << 20, None), "bias"),
                       (lambda: lib.softmax_score(p, 9, p, 5, 36, None, p + 4, p, 0, p, 1 << 20, None), "ent or marg"),
                       (lambda: lib.softmax_score(p, 9, p, 5, 36, None, p, None, 0, p, 1 << 20, None), "ent or marg"),
                       (lambda: lib.softmax_score(p, 9, p, 5, 34, None, p, p, 0, p, 1 << 20, None), "D=34"),
                       (lambda: lib.softmax_score(p, 9, p, 5, 36, None, p, p, 0, p, 16, None), "workspace")):
        with pytest.raises(L.MapditError, match=word):
            call()


# ---- names and flags ----------------------------------------------------------------------------------------------------------------
def test_parse_metrics_knows_the_new_names(capsys):
    import mapdit_amd.fid as FID
    import mapdit_amd.metrics as M
    assert M.METRICS == ("fid", "fid_s", "isc", "pr", "kid")
    assert FID.parse_metrics("isc, fid_s,kid") == ("fid_s", "isc", "kid")
    assert FID.parse_metrics(None) == ("fid",)
    with pytest.raises(ValueError, match=r"--metrics.*comma-separated.*fid_s, isc"):
        FID.parse_metrics("fid,inception")
    from mapdit_amd import sample_fid
    for parser, argv in ((FID.build_parser(), ["compare", "--help"]), (sample_fid.build_parser(), ["--help"])):
        with pytest.raises(SystemExit):
            parser.parse_args(argv)
        text = " ".join(capsys.readouterr().out.split())
        assert "fid_s" in text and "isc" in text and "comma-separated" in text
    args = FID.build_parser().parse_args(["stats", "--images", "a", "--output", "o", "--spatial"])
    assert args.spatial is True
    assert FID.build_parser().parse_args(["features", "--images", "a", "--output", "o"]).spatial is False


# ---- the statistics file ------------------------------------------------------------------------------------------------------------
def test_spatial_statistics_round_trip_and_adm_layout(tmp_path):
    import mapdit_amd.fid as FID
    rng = np.random.default_rng(3)
    mu, mu_s = rng.standard_normal(6), rng.standard_normal(5)
    sigma, sigma_s = np.cov(rng.standard_normal((9, 6)), rowvar=False), np.cov(rng.standard_normal((9, 5)), rowvar=False)
    p = tmp_path / "ref.npz"
    FID.save_stats(p, mu, sigma, mu_s=mu_s, sigma_s=sigma_s)
    assert sorted(os.listdir(tmp_path)) == ["ref.npz"] and FID.has_spatial(p)
    got = FID.load_stats(p, spatial=True)
    assert len(got) == 4 and all(np.array_equal(a, b) and a.dtype == np.float64 for a, b in zip(got, (mu, sigma, mu_s, sigma_s)))
    two = FID.load_stats(p)                                                # the default call: today's pair
    assert len(two) == 2 and np.array_equal(two[0], mu) and np.array_equal(two[1], sigma)
    # the default write: exactly today's keys
    q = tmp_path / "plain.npz"
    FID.save_stats(q, mu, sigma)
    with np.load(q) as z:
        assert sorted(z.files) == ["mu", "sigma"]
    assert not FID.has_spatial(q)
    with pytest.raises(KeyError, match=r"mu_s.*stats --spatial"):
        FID.load_stats(q, spatial=True)
    with pytest.raises(ValueError, match="go together"):
        FID.save_stats(tmp_path / "half.npz", mu, sigma, mu_s=mu_s)
    # an ADM-style reference batch: float32 arrays, the images first
    adm = tmp_path / "VIRTUAL_ref.npz"
    np.savez(adm, arr_0=np.zeros((2, 4, 4, 3), np.uint8), mu=mu.astype(np.float32), sigma=sigma.astype(np.float32),
             mu_s=mu_s.astype(np.float32), sigma_s=sigma_s.astype(np.float32))
    got = FID.load_stats(adm, spatial=True)
    assert all(a.dtype == np.float64 and np.array_equal(a, b.astype(np.float32)) for a, b in zip(got, (mu, sigma, mu_s, sigma_s)))
    bad = tmp_path / "bad.npz"
    np.savez(bad, mu=mu, sigma=sigma, mu_s=mu_s, sigma_s=sigma)
    with pytest.raises(ValueError, match="mu_s of shape"):
        FID.load_stats(bad, spatial=True)
    # a features file carries them too, and still loads as before
    f = tmp_path / "feats.npz"
    FID.save_features(f, np.zeros((3, 6), np.float32), mu, sigma, mu_s, sigma_s)
    assert FID.has_spatial(f) and FID.features_rows(f) == 3 and np.array_equal(FID.load_stats(f, spatial=True)[3], sigma_s)


# ---- the classifier head ------------------------------------------------------------------------------------------------------------
def test_classifier_head():
    import mapdit_amd.fid as FID
    g = torch.Generator().manual_seed(4)
    w, b = torch.randn(1008, 2048, generator=g, dtype=torch.float64), torch.randn(1008, generator=g, dtype=torch.float64)
    sd = {"fc.weight": w, "fc.bias": b, "Conv2d_1a_3x3.conv.weight": torch.zeros(32, 3, 3, 3)}
    hw, hb = FID.classifier_head(sd)
    assert hw.dtype == hb.dtype == torch.float32 and hw.is_contiguous() and tuple(hw.shape) == (1008, 2048) and tuple(hb.shape) == (1008,)
    assert torch.equal(hw, w.float()) and torch.equal(hb, b.float())
    with pytest.raises(KeyError, match="fc.weight"):
        FID.classifier_head({"fc.bias": b})
    with pytest.raises(KeyError, match="fc.bias"):
        FID.classifier_head({"fc.weight": w})
    with pytest.raises(ValueError, match=r"fc.weight.*\(1000, 2048\)"):
        FID.classifier_head({"fc.weight": w[:1000], "fc.bias": b})
    with pytest.raises(ValueError, match="fc.bias"):
        FID.classifier_head({"fc.weight": w, "fc.bias": b[:1000]})
    # the feature network's fold still ignores the head
    assert all(not k.startswith("fc.") for k in FID.inception_shapes())


# ---- the host finish ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, split, zero_class", [(23, 10, False), (40, 10, True), (7, 5000, True)])
def test_inception_score_from_sums_is_adms_formula(n, split, zero_class):
    """Random probabilities; ent and marg summed in fp64 by numpy, the score against ADM's compute_inception_score written out
    (tests/score_reference.py): 1e-12 relative.  A short last split; a class nobody has any mass on adds 0, not NaN."""
    import mapdit_amd.metrics as M
    rng = np.random.default_rng(n)
    logits = 3.0 * rng.standard_normal((n, 12))
    if zero_class:
        logits[:, 5] = -np.inf
    m = logits.max(axis=1, keepdims=True)
    logp = logits - (m + np.log(np.exp(logits - m).sum(axis=1, keepdims=True)))
    p = np.exp(logp)
    got = []
    for i in range(0, n, split):
        pp, lp = p[i:i + split], logp[i:i + split]
        ent = float(np.where(pp > 0, pp * np.where(pp > 0, lp, 0.0), 0.0).sum())
        marg = pp.sum(axis=0)
        assert not zero_class or marg[5] == 0.0
        got.append(M.inception_score_from_sums(ent, marg, len(pp)))
    want = [SR.split_score(logp[i:i + split]) for i in range(0, n, split)]
    assert len(got) == -(-n // split) and all(np.isfinite(got))
    assert all(abs(g - w) <= 1e-12 * w for g, w in zip(got, want)), (got, want)
    assert all(1.0 <= g <= 12.0 for g in got)                              # between one class and all of them


def test_inception_score_needs_cuda_tensors():
    import mapdit_amd.metrics as M
    x, w = torch.zeros(16, 8), torch.zeros(5, 8)
    for call in (lambda: M.inception_score(x, w), lambda: M.softmax_score(x, w)):
        with pytest.raises(NotImplementedError):
            call()


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def test_compare_refusals_for_fid_s_and_isc(tmp_path, monkeypatch):
    import mapdit_amd.fid as FID
    monkeypatch.setattr(FID.InceptionFeatures, "from_file", lambda *a, **k: pytest.fail("the network was built"))
    monkeypatch.setattr(FID, "load_head", lambda *a, **k: pytest.fail("the weights were read"))
    st, st_s, feats = str(tmp_path / "st.npz"), str(tmp_path / "st_s.npz"), str(tmp_path / "feats.npz")
    FID.save_stats(st, np.zeros(2048), np.eye(2048))
    FID.save_stats(st_s, np.zeros(6), np.eye(6), np.zeros(5), np.eye(5))
    FID.save_features(feats, np.zeros((4, 2048), np.float32), np.zeros(2048), np.eye(2048))
    # fid_s: a statistics file without mu_s, and a features file alone, name the command that writes them
    for a, b in ((st, st_s), (st_s, st), (st_s, feats)):
        with pytest.raises(ValueError, match=r"mu_s.*fid stats --spatial"):
            FID.main(["compare", a, b, "--metrics", "fid,fid_s", "--inception-weights", "w.pt"])
    # isc: the samples' pool_3 and the head
    with pytest.raises(ValueError, match=r"statistics only.*fid features"):
        FID.main(["compare", feats, st, "--metrics", "isc", "--inception-weights", "w.pt"])
    with pytest.raises(ValueError, match="--inception-weights"):
        FID.main(["compare", st, feats, "--metrics", "isc"])
    imgs = str(tmp_path / "imgs.npz")
    np.savez(imgs, arr_0=np.zeros((2, 8, 8, 3), np.uint8))
    with pytest.raises(ValueError, match="--inception-weights"):
        FID.main(["compare", imgs, st_s, "--metrics", "fid_s"])


def test_compare_fid_s_of_two_statistics_files_needs_no_gpu(tmp_path, capsys):
    import mapdit_amd.fid as FID
    a, b = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    FID.save_stats(a, np.zeros(6), np.eye(6), np.zeros(5), np.eye(5))
    FID.save_stats(b, np.ones(6), np.eye(6), 2 * np.ones(5), np.eye(5))
    values = FID.main(["compare", a, b, "--metrics", "fid,fid_s"])
    assert values == {"fid": pytest.approx(6.0), "fid_s": pytest.approx(20.0)}
    assert capsys.readouterr().out == "fid: 6.000000\nfid_s: 20.000000\n"


@pytest.mark.parametrize("flags, match", [
    (["--metrics", "fid_s"], "needs --fid-ref"),
    (["--metrics", "isc"], "needs --fid-ref"),
    (["--metrics", "fid,fid_s", "--fid-ref", "REF", "--inception-weights", "W"], r"mu_s.*fid stats --spatial"),
    (["--metrics", "fid_s,isc,pr", "--fid-ref", "REF_S", "--inception-weights", "W"], "pool_3"),
    (["--metrics", "fid_s,sfid", "--fid-ref", "REF_S", "--inception-weights", "W"], "comma-separated"),
])
def test_sample_fid_refuses_before_any_model_is_built(tmp_path, monkeypatch, flags, match):
    import mapdit_amd.fid as FID
    from mapdit_amd import sample_fid
    monkeypatch.setattr(FID.InceptionFeatures, "from_file", lambda *a, **k: pytest.fail("the network was built"))
    ref, ref_s, w = str(tmp_path / "ref.npz"), str(tmp_path / "ref_s.npz"), tmp_path / "w.pt"
    FID.save_stats(ref, np.zeros(2048), np.eye(2048))
    FID.save_stats(ref_s, np.zeros(6), np.eye(6), np.zeros(5), np.eye(5))
    w.write_bytes(b"")
    flags = [{"REF": ref, "REF_S": ref_s, "W": str(w)}.get(f, f) for f in flags]
    with pytest.raises(ValueError, match=match):                          # before config.yaml of the (missing) run directory is read
        sample_fid.main(["--result-dir", str(tmp_path / "no_such_run")] + flags)


def test_sample_fid_checks_the_head_and_the_spatial_dimension_before_any_model(tmp_path, monkeypatch):
    """fid_s and isc need no reference features; statistics of another spatial dimension and a weight file without the classifier
    head are refused by check_fid_flags - before config.yaml is read, a model built or a sample drawn."""
    import mapdit_amd.fid as FID
    from mapdit_amd import sample_fid
    monkeypatch.setattr(FID.InceptionFeatures, "from_file", lambda *a, **k: pytest.fail("the network was built"))
    assert FID.spatial_dim() == 2023 and FID.spatial_dim(75) == 63
    small, ref_s, w, headless = str(tmp_path / "small.npz"), str(tmp_path / "ref_s.npz"), str(tmp_path / "w.pt"), str(tmp_path / "headless.pt")
    FID.save_stats(small, np.zeros(2048), np.eye(2048), np.zeros(5), np.eye(5))
    FID.save_stats(ref_s, np.zeros(2048), np.eye(2048), np.zeros(2023), np.eye(2023))
    torch.save({"fc.weight": torch.zeros(1008, 2048), "fc.bias": torch.zeros(1008)}, w)
    torch.save({"fc.bias": torch.zeros(1008)}, headless)
    run = ["--result-dir", str(tmp_path / "no_such_run")]
    parse = lambda *flags: sample_fid.build_parser().parse_args(run + list(flags))      # noqa: E731
    args = parse("--metrics", "fid,fid_s,isc", "--fid-ref", ref_s, "--inception-weights", w)
    assert sample_fid.check_fid_flags(args) is True and "fc.weight" in args.inception_sd
    with pytest.raises(ValueError, match=r"spatial statistics of shape \(5,\).*2023"):
        sample_fid.main(run + ["--metrics", "fid_s", "--fid-ref", small, "--inception-weights", w])
    with pytest.raises(KeyError, match="fc.weight"):
        sample_fid.main(run + ["--metrics", "isc", "--fid-ref", ref_s, "--inception-weights", headless])
    # a file that is called .npz and is no archive: the same refusal as a file without the keys
    junk = tmp_path / "junk.npz"
    junk.write_bytes(b"not a zip")
    assert FID.has_spatial(junk) is False
