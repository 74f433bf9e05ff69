"""The Inception Score and the spatial FID on the GPU: ``mapdit_softmax_score`` (csrc/manifold.hip) against the numpy fp64
restatement, ``metrics.inception_score`` end to end, the spatial tap of ``mapdit_inc_features_tap`` (csrc/inception.hip) against the
fp64 restatement of the same tap, sFID from the tap, and the command lines (tests/score_reference.py holds the restatements)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inception_reference as R  # noqa: E402
import score_reference as SR  # noqa: E402
import vae_reference as VR  # noqa: E402
from conftest import rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- mapdit_softmax_score -----------------------------------------------------------------------------------------------------------
def _integer_case(N, C, D, seed):
    """Integer-valued fp32 data whose every partial dot product stays far below 2^24: the fp32 logits are exact, and the device
    differs from numpy fp64 by the fp64 summation order alone.  x in {0..3}; w in {-2..2} for short rows, in {-1, 0, 1} with one entry
    in 64 set for D = 2048 (|logit| <= 3 * 2048 either way)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 4, (N, D)).astype(np.float32)
    if D >= 1024:
        w = (rng.integers(0, 64, (C, D)) == 0) * rng.choice([-1.0, 1.0], (C, D))
    else:
        w = rng.integers(-2, 3, (C, D))
    bias = (rng.integers(-8, 9, C) / 4.0).astype(np.float32)             # quarters: exact in fp32 and in the fp64 sum
    return x, w.astype(np.float32), bias


def _device_sums(x, w, bias, chunks):
    import mapdit_amd.metrics as M
    ent, marg = M.softmax_score(torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV), None if bias is None else torch.from_numpy(bias).to(DEV),
                                chunks=chunks)
    return ent.cpu(), marg.cpu()


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("N, C, D", [(1, 5, 4), (130, 130, 36), (257, 1008, 2048)])
def test_softmax_score_on_integer_data(N, C, D, with_bias):
    """(130, 130, 36): two query tiles with a short last one, a K tail of 4 after a full 32, the short reference tile in both roles."""
    x, w, bias = _integer_case(N, C, D, seed=N + C)
    bias = bias if with_bias else None
    ent_ref, marg_ref, _ = SR.softmax_sums(x, w, bias)
    runs = [_device_sums(x, w, bias, chunks) for chunks in (0, 1, 3)]
    for ent, marg in runs[1:]:                                             # no output depends on the slicing, bit for bit
        assert torch.equal(ent, runs[0][0]) and torch.equal(marg, runs[0][1])
    ent, marg = float(runs[0][0]), runs[0][1].numpy()
    e_ent = abs(ent - ent_ref) / abs(ent_ref) if ent_ref != 0 else abs(ent)
    e_marg = float(np.max(np.abs(marg - marg_ref) / marg_ref))
    print(f"softmax_score ({N}, {C}, {D}) bias={with_bias}: ent {ent:.15e} (rel {e_ent:.2e}), marg rel {e_marg:.2e}; bound 1e-11")
    assert marg.shape == (C,) and np.isfinite(ent) and np.all(np.isfinite(marg))
    assert e_ent <= 1e-11 and e_marg <= 1e-11
    assert abs(marg.sum() - N) <= 1e-11 * N


def test_softmax_score_logit_gap_of_200():
    """Row 0 puts class 0 a logit of 200 above the rest: exp(-200) on the small side.  Everything stays finite, the other classes get
    next to nothing from that row.  (Rows 1 and 2 keep logits within +-3, so the entropy sum the 1e-11 is relative to is O(1):
    u / s - lse cancels to about |lse| ulps absolutely, which is nothing to a sum of that size and everything to one that is 0.)"""
    rng = np.random.default_rng(11)
    x = rng.integers(0, 2, (3, 4)).astype(np.float32)
    w = rng.integers(-1, 2, (5, 4)).astype(np.float32)
    x[0] = [10, 0, 0, 0]
    x[1:, 0] = 0
    w[0] = [20, 0, 0, 0]
    w[1:, 0] = 0
    ent_ref, marg_ref, logp = SR.softmax_sums(x, w)
    assert logp[0, 0] == 0.0 and np.all(logp[0, 1:] == -200.0)
    ent, marg = _device_sums(x, w, None, 0)
    ent, marg = float(ent), marg.numpy()
    assert np.isfinite(ent) and np.all(np.isfinite(marg)) and np.all(marg >= 0)
    assert abs(ent - ent_ref) <= 1e-11 * abs(ent_ref) and np.all(np.abs(marg - marg_ref) <= 1e-11 * marg_ref)
    one = _device_sums(x[:1], w, None, 0)                                 # the row alone: one class has it all
    assert abs(float(one[0])) <= 1e-80 and float(one[1][0]) == 1.0 and np.all(one[1][1:].numpy() <= 1e-80)


def _gaussian(N, seed, C=1008, D=2048):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, D, generator=g).abs() * 0.4).numpy().astype(np.float32)
    w = (torch.randn(C, D, generator=g) * 0.03).numpy().astype(np.float32)
    return x, w


def test_softmax_score_on_gaussian_data():
    """Tolerance: score_reference.log_is_bound, from the reference's numbers alone."""
    import mapdit_amd.metrics as M
    x, w = _gaussian(130, seed=21)
    ent_ref, marg_ref, logp = SR.softmax_sums(x, w)
    bound, eps, T = SR.log_is_bound(x, w, logp)
    want = SR.split_score(logp)
    ent, marg = _device_sums(x, w, None, 0)
    got = M.inception_score_from_sums(float(ent), marg.numpy(), 130)
    err = abs(np.log(got) - np.log(want))
    print(f"softmax_score gaussian (130, 1008, 2048): IS {got:.12f} vs fp64 {want:.12f}: |log IS - log IS_64| = {err:.3e}, bound {bound:.3e} "
          f"(eps {eps:.3e}, T {T:.3f})")
    assert want > 1.0 and err <= bound


def test_inception_score_end_to_end():
    """23 samples in splits of 10: 10 + 10 + 3.  Per split |log IS_i - log IS_i,64| <= B_i (log_is_bound on the split's rows), so
    |IS_i - IS_i,64| <= IS_i,64 (e^{B_i} - 1) =: t_i.  The mean moves by at most max t_i, and so does the standard deviation (the
    standard deviation of a vector is 1-Lipschitz in its largest component change)."""
    import mapdit_amd.metrics as M
    x, w = _gaussian(23, seed=22)
    mean_ref, std_ref, scores = SR.inception_score(x, w, None, 10)
    assert len(scores) == 3
    logp = SR.softmax_sums(x, w)[2]
    tol = max(s * np.expm1(SR.log_is_bound(x[i:i + 10], w, logp[i:i + 10])[0]) for s, i in zip(scores, range(0, 23, 10)))
    xd, wd = torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV)
    mean, std = M.inception_score(xd, wd, split_size=10)
    print(f"inception_score: {mean:.10f} +- {std:.10f} vs fp64 {mean_ref:.10f} +- {std_ref:.10f}; tolerance {tol:.3e}")
    assert abs(mean - mean_ref) <= tol and abs(std - std_ref) <= tol
    assert (mean, std) == M.inception_score(xd, wd, split_size=10, chunks=2)
    one, zero = M.inception_score(xd, wd, split_size=5000)                # one split: no spread
    assert zero == 0.0 and abs(np.log(one) - np.log(SR.inception_score(x, w, None, 5000)[0])) <= SR.log_is_bound(x, w, logp)[0]
    # with the head's bias: the same bound on the biased reference (the bias is added exactly, in fp64)
    b = torch.linspace(-2, 2, 1008)
    mean_b, std_b, scores_b = SR.inception_score(x, w, b.numpy(), 10)
    logp_b = SR.softmax_sums(x, w, b.numpy())[2]
    tol_b = max(s * np.expm1(SR.log_is_bound(x[i:i + 10], w, logp_b[i:i + 10])[0]) for s, i in zip(scores_b, range(0, 23, 10)))
    biased = M.inception_score(xd, wd, b.to(DEV), split_size=10)
    assert abs(biased[0] - mean_b) <= tol_b and abs(biased[1] - std_b) <= tol_b
    with pytest.raises(NotImplementedError):
        M.inception_score(torch.from_numpy(x), wd)
    with pytest.raises(NotImplementedError):
        M.inception_score(xd, torch.from_numpy(w))
    with pytest.raises(ValueError, match="dimensions"):
        M.inception_score(xd[:, :64].contiguous(), wd)


# ---- the spatial tap ----------------------------------------------------------------------------------------------------------------
# Relative L2 error of the tap [2, hs * ws * 7] against the fp64 restatement.  EMULATION: the restatement's own error when it rounds
# every convolution's operands to the 16-bit format (score_reference.spatial(operand_dtype=...)), computed on the CPU; the asserted
# bound is 3 x that.  RECORDED: what the kernels gave on an MI355X.
EMULATION = {(299, "f16"): 6.68e-3, (299, "bf16"): 5.02e-2, (75, "f16"): 3.17e-3, (75, "bf16"): 2.76e-2}
BOUND = {k: 3 * v for k, v in EMULATION.items()}
RECORDED = {(299, "f16"): 6.57e-3, (299, "bf16"): 5.05e-2, (75, "f16"): 2.88e-3, (75, "bf16"): 2.45e-2}


def _net(sd, precision="f16", image_size=299, **kw):
    from mapdit_amd.fid import InceptionFeatures, fold_state_dict
    return InceptionFeatures(fold_state_dict(sd), DEV, precision, image_size=image_size, **kw)


@pytest.fixture(scope="module")
def sd():
    return R.init_state_dict(seed=3)


@pytest.fixture(scope="module")
def two(sd):
    """The two 64 x 64 noise images of tests/test_fid_gpu.py and the fp64 restatement of the tap at both sizes (computed once)."""
    img = torch.randint(0, 256, (2, 64, 64, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    return img, {299: SR.spatial(sd, img, 299), 75: SR.spatial(sd, img, 75)}


@pytest.mark.parametrize("precision", ["f16", "bf16"])
@pytest.mark.parametrize("size, dim", [(299, 2023), (75, 63)])
def test_spatial_tap_against_the_restatement(sd, two, size, dim, precision):
    img, ref = two
    net = _net(sd, precision, size)
    assert net.spatial_dim == dim and tuple(ref[size].shape) == (2, dim)
    plain = net.features(img.to(DEV))
    feat, spat = net.features(img.to(DEV), spatial=True)
    assert torch.equal(feat, plain)                                        # pool_3 does not know about the tap
    assert spat.shape == (2, dim) and spat.dtype == torch.float32 and spat.is_cuda and bool(torch.isfinite(spat).all())
    e = rel_err(spat.cpu().numpy(), ref[size].numpy())
    print(f"spatial tap {size} {precision}: rel err {e:.3e} (fp64 emulation of the operand rounding {EMULATION[size, precision]:.2e}, "
          f"bound {BOUND[size, precision]:.2e}, recorded {RECORDED[size, precision]})")
    assert e <= BOUND[size, precision]
    # the library's two entry points: the tap with a null destination is mapdit_inc_features, bit for bit
    import mapdit_amd._lib as L
    lib = L.lib()
    x = img.to(DEV).contiguous()
    out = [torch.zeros(2, 2048, device=DEV) for _ in range(2)]
    fn, tap = (lib.inc_features_f16, lib.inc_features_tap_f16) if precision == "f16" else (lib.inc_features, lib.inc_features_tap)
    head = (ctypes.byref(net._cfg), net._table, x.data_ptr(), L.INC_IMG_U8_NHWC, 2, 64, 64)
    fn(*head, out[0].data_ptr(), net._ws.data_ptr(), net._ws.numel(), L.cur_stream())
    tap(*head, out[1].data_ptr(), None, net._ws.data_ptr(), net._ws.numel(), L.cur_stream())
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], plain)


def test_spatial_tap_of_an_image_alone_equals_the_image_in_a_batch(sd, two):
    img = torch.cat([two[0], torch.randint(0, 256, (1, 64, 64, 3), generator=torch.Generator().manual_seed(6), dtype=torch.uint8)]).to(DEV)
    whole = _net(sd).features(img, spatial=True)
    chunked = _net(sd, max_batch=2).features(img, spatial=True)            # 2 + 1
    assert torch.equal(whole[0], chunked[0]) and torch.equal(whole[1], chunked[1])
    alone = _net(sd, max_batch=1).features(img[1:2], spatial=True)
    assert torch.equal(alone[1][0], whole[1][1]) and torch.equal(alone[0][0], whole[0][1])
    empty = _net(sd).features(img[:0], spatial=True)
    assert tuple(empty[0].shape) == (0, 2048) and tuple(empty[1].shape) == (0, 2023)


def test_sfid_end_to_end_from_the_tap(sd):
    """Two sets of 12 images: FeatureStats(D = 2023) on the tap, then frechet_distance, against the same distance from numpy's fp64
    mean / cov of the device's own tap features - the accumulation and the plumbing at a D that is no multiple of 4 or of 64."""
    from mapdit_amd.fid import FeatureStats, frechet_distance
    g = torch.Generator().manual_seed(7)
    a = torch.randint(0, 256, (12, 32, 32, 3), generator=g, dtype=torch.uint8)
    b = torch.randint(96, 256, (12, 32, 32, 3), generator=g, dtype=torch.uint8)
    net = _net(sd)
    stats, taps = [], []
    for imgs in (a, b):
        st = FeatureStats(net.spatial_dim, DEV)
        parts = [net.features(imgs[i:j].to(DEV), spatial=True)[1] for i, j in ((0, 5), (5, 12))]
        for p in parts:
            st.update(p)
        assert st.n == 12
        stats.append(st.mean_cov())
        taps.append(torch.cat(parts).cpu().numpy().astype(np.float64))
    got = frechet_distance(*stats[0], *stats[1])
    want = frechet_distance(taps[0].mean(0), np.cov(taps[0], rowvar=False), taps[1].mean(0), np.cov(taps[1], rowvar=False))
    print(f"sFID {got:.12f} vs numpy mean / cov of the same features {want:.12f}: rel diff {abs(got - want) / want:.3e}, bound 1e-9")
    assert want > 0 and abs(got - want) <= 1e-9 * want
    for (mu, sigma), f in zip(stats, taps):
        assert np.allclose(mu, f.mean(0), rtol=1e-12, atol=1e-14)


# ---- the command lines --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inc_file(sd, tmp_path_factory):
    """The random Inception weights as a torch file, fp32, with a random classifier head."""
    path = str(tmp_path_factory.mktemp("inception_weights") / "inception.pt")
    g = torch.Generator().manual_seed(12)
    full = {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}
    full["fc.weight"], full["fc.bias"] = torch.randn(1008, 2048, generator=g) * 0.03, torch.randn(1008, generator=g)
    torch.save(full, path)
    return path


def test_command_line_spatial_stats_and_compare(sd, inc_file, tmp_path, capsys):
    from mapdit_amd import fid as FID
    from mapdit_amd import metrics as M
    g = torch.Generator().manual_seed(9)
    a = torch.randint(0, 256, (8, 16, 16, 3), generator=g, dtype=torch.uint8).numpy()
    b = torch.randint(64, 256, (8, 24, 16, 3), generator=g, dtype=torch.uint8).numpy()
    np.savez(tmp_path / "a.npz", arr_0=a)
    np.save(tmp_path / "b.npy", b)
    ref, plain = str(tmp_path / "a_stats.npz"), str(tmp_path / "a_plain.npz")
    assert FID.main(["stats", "--images", str(tmp_path / "a.npz"), "--inception-weights", inc_file, "--output", ref, "--batch-size", "3", "--spatial"]) == ref
    with np.load(ref) as z:
        assert sorted(z.files) == ["mu", "mu_s", "sigma", "sigma_s"] and z["mu_s"].shape == (2023,) and z["sigma_s"].shape == (2023, 2023)
    FID.main(["stats", "--images", str(tmp_path / "a.npz"), "--inception-weights", inc_file, "--output", plain, "--batch-size", "3"])
    with np.load(plain) as z:                                              # without the flag: today's keys, today's bits
        assert sorted(z.files) == ["mu", "sigma"]
    assert all(np.array_equal(x, y) for x, y in zip(FID.load_stats(plain), FID.load_stats(ref)))
    # the Python calls on the same images
    net = FID.InceptionFeatures.from_file(inc_file, DEV)
    head = FID.load_head(inc_file)
    fa, sa, ssa = FID.features_of_images(a, net, 3, spatial=True)
    fb, sb, ssb = FID.features_of_images(b, net, 64, spatial=True)
    mu_s, sigma_s = FID.load_stats(ref, spatial=True)[2:]
    assert np.array_equal(mu_s, ssa.mean_cov()[0]) and np.array_equal(sigma_s, ssa.mean_cov()[1])
    want = {"fid": FID.frechet_distance(*sa.mean_cov(), *sb.mean_cov()), "fid_s": FID.frechet_distance(*ssa.mean_cov(), *ssb.mean_cov())}
    want["isc"], want["isc_std"] = M.inception_score(fb, head[0].to(DEV))
    capsys.readouterr()
    values = FID.main(["compare", ref, str(tmp_path / "b.npy"), "--metrics", "fid,fid_s,isc", "--inception-weights", inc_file])
    assert values == want and 1.0 < values["isc"] < 1008.0 and values["fid_s"] > 0
    assert capsys.readouterr().out.splitlines() == [f"fid: {want['fid']:.6f}", f"fid_s: {want['fid_s']:.6f}",
                                                    f"isc: {want['isc']:.6f} ± {want['isc_std']:.6f}"]
    # a features file with --spatial carries everything compare needs: the same numbers without the network
    feats = str(tmp_path / "b_feats.npz")
    FID.main(["features", "--images", str(tmp_path / "b.npy"), "--inception-weights", inc_file, "--output", feats, "--spatial"])
    assert FID.main(["compare", ref, feats, "--metrics", "fid,fid_s,isc", "--inception-weights", inc_file]) == want


@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    """A small run directory, made the way tests/test_fid_gpu.py makes its own."""
    from mapdit_amd import train
    root = tmp_path_factory.mktemp("score_results")
    return train.main(["--synthetic", "--results-dir", str(root), "--model", "DiT-XS/2", "--num-steps", "8", "--batch-size", "8",
                       "--log-every", "4", "--ckpt-every", "8", "--ema-snapshot-every", "2", "--num-classes", "10",
                       "--num-lin-warmup", "2", "--start-decay", "3", "--verbose", "0"])


def test_sample_fid_writes_fid_s_and_isc(sd, inc_file, run_dir, tmp_path, capsys):
    from mapdit_amd import fid as FID
    from mapdit_amd import metrics as M
    from mapdit_amd import sample_fid
    vae_w, ref = str(tmp_path / "tiny_vae.safetensors"), str(tmp_path / "ref.npz")
    VR.write_safetensors(VR.init_state_dict(VR.TINY, seed=2, generation="old"), vae_w)
    rng = np.random.default_rng(8)
    FID.save_stats(ref, 0.5 + 0.1 * rng.standard_normal(2048), np.eye(2048) * 0.05, 0.3 + 0.1 * rng.standard_normal(2023), np.eye(2023) * 0.05)
    base = ["--result-dir", run_dir, "--num-classes", "10", "--num-sampling-steps", "2", "--batch-size", "4", "--num-samples", "6",
            "--vae-weights", vae_w, "--fid-ref", ref, "--inception-weights", inc_file, "--metrics", "fid,fid_s,isc"]
    value = sample_fid.main(base + ["--output-file", "sc.npz"])
    out = capsys.readouterr().out.splitlines()
    npz = os.path.join(run_dir, "fid_samples", "sc.npz")
    rec = json.load(open(npz + ".fid.json"))
    assert rec["fid"] == value and rec["n"] == 6 and sorted(rec["metrics"]) == ["fid_s", "isc", "isc_std"]
    m = rec["metrics"]
    assert out[-3:] == [f"fid: {value:.6f}", f"fid_s: {m['fid_s']:.6f}", f"isc: {m['isc']:.6f} ± {m['isc_std']:.6f}"]
    # the numbers are those of the stored array: the same bytes through the same network in the same batches of 4
    arr = np.load(npz)["arr_0"]
    net = FID.InceptionFeatures.from_file(inc_file, DEV)
    feat, st, st_s = FID.features_of_images(arr, net, 4, spatial=True)
    assert FID.frechet_distance(*st.mean_cov(), *FID.load_stats(ref)) == value
    assert FID.frechet_distance(*st_s.mean_cov(), *FID.load_stats(ref, spatial=True)[2:]) == m["fid_s"]
    assert M.inception_score(feat, FID.load_head(inc_file)[0].to(DEV)) == (m["isc"], m["isc_std"])
    # the counter generator's path scores the assembled bytes through the same pass (fid_record; its parts need the full VAE's 8 x
    # upscaling, which the tiny one does not have): the same array gives the same record
    other = str(tmp_path / "again.npz")
    args = sample_fid.build_parser().parse_args(base + ["--output-file", "again.npz", "--sample-rng", "counter"])
    assert sample_fid.fid_record(args, other, arr, DEV) == value
    rec_c = json.load(open(other + ".fid.json"))
    assert rec_c == {**rec, "samples": other}
