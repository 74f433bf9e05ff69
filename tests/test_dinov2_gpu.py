"""FD-DINOv2 end to end on the GPU: ``mapdit_vit_features`` through ``dinov2.DinoV2Features`` against the fp64 restatement
(tests/dinov2_reference.py) on random weights in both operand formats, batching, the two input kinds, the statistics and the
distance, the command line and sample_fid.py.

Tolerance of the walk: max |feat - ref| <= 2 x e_emul x max |ref| against the PLAIN fp64 network, e_emul the measured cost of the
16-bit operands alone on the very weights and images of the case (E_EMUL below; tests/test_dinov2_cpu.py measures them with
dinov2_reference.measure_e_emul and asserts these constants are what it measures); the factor 2 covers fp32 accumulation order and
fp32 exp / erfc."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dinov2_reference as R  # noqa: E402
import vae_reference as VR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

# dim 128, 2 heads, depth 2, mlp 512, LayerScale gamma in [0.05, 1]: image_size 28 (T = 5, N = 3) and 224 (T = 257, N = 2)
E_EMUL = {"f16": {"walk28": 7.893e-04, "walk224": 6.624e-04}, "bf16": {"walk28": 1.058e-02, "walk224": 5.922e-03}}


def _D():
    from mapdit_amd import dinov2
    return dinov2


@pytest.fixture(scope="module")
def walks():
    """case -> (state dict, uint8 images, image_size, the fp64 features): computed once."""
    out = {}
    for name in R.WALK_CASES:
        sd, images, size = R.case_walk(name)
        out[name] = (sd, images, size, R.vit_forward(sd, images, size))
    return out


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("case", list(R.WALK_CASES))
def test_whole_walk_against_fp64(walks, case, prec):
    sd, images, size, ref = walks[case]
    net = _D().DinoV2Features.from_state_dict(sd, DEV, prec, image_size=size)
    feat = net.features(images.to(DEV))
    assert feat.shape == ref.shape and feat.dtype == torch.float32 and torch.isfinite(feat).all()
    err, lim = float((feat.double().cpu() - ref).abs().max()), 2 * E_EMUL[prec][case] * float(ref.abs().max())
    print(f"{case} {prec}: max err {err:.3e} (limit {lim:.3e}, max |ref| {float(ref.abs().max()):.3f})")
    assert err <= lim, (case, prec, err, lim)


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_batching_changes_no_bit(walks, prec):
    D = _D()
    for case in R.WALK_CASES:
        sd, images, size, _ = walks[case]
        x = images.to(DEV)
        whole = D.DinoV2Features.from_state_dict(sd, DEV, prec, image_size=size).features(x)
        alone = D.DinoV2Features.from_state_dict(sd, DEV, prec, image_size=size).features(x[1:2])
        assert torch.equal(alone[0], whole[1])                 # an image alone = the image in a batch
        chunked = D.DinoV2Features.from_state_dict(sd, DEV, prec, max_batch=2 if len(x) > 2 else 1, image_size=size).features(x)
        assert torch.equal(chunked, whole)                     # max_batch chunking


def test_uint8_and_fp32_inputs_agree(walks):
    """The same picture as bytes and as fp32 [N, 3, H, W] in [-1, 1]: the inputs differ by the fp32 rounding of v / 127.5 - 1 and of
    the map back, a few 2^-24 of a pixel value - five orders below a 16-bit step of a patch row, so a patch value changes (by one
    step) only where it sat on a rounding boundary.  That is a small part of what e_emul counts (EVERY patch value, activation and
    weight moved by up to half a step), so the two feature sets are held to e_emul x max |feat| of each other."""
    sd, images, size, ref = walks["walk28"]
    net = _D().DinoV2Features.from_state_dict(sd, DEV, "f16", image_size=size)
    a = net.features(images.to(DEV))
    b = net.features((images.permute(0, 3, 1, 2).double() / 127.5 - 1.0).float().to(DEV))
    d = float((a - b).abs().max())
    print(f"uint8 vs fp32 input: max difference {d:.3e}")
    assert d <= E_EMUL["f16"]["walk28"] * float(ref.abs().max())
    with pytest.raises(ValueError, match="expected uint8"):
        net.features(images.permute(0, 3, 1, 2).contiguous().to(DEV))
    with pytest.raises(NotImplementedError, match="GPU only"):
        net.features(images)


@pytest.fixture(scope="module")
def dino_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("dinov2_weights") / "dinov2_tiny.pt")
    torch.save(R.make_state_dict(128, 2, 512, seed=11), path)
    return path


def test_command_line_stats_features_compare(dino_file, tmp_path, capsys):
    D = _D()
    from mapdit_amd import fid as FID
    g = torch.Generator().manual_seed(9)
    # more images than dimensions (128): with fewer the covariance is singular and the square roots of its zero eigenvalues, not the
    # features, set the floor of a set's distance to itself (tests/test_fid_cpu.py, test_frechet_distance_rank_deficient)
    a = torch.randint(0, 256, (160, 16, 16, 3), generator=g, dtype=torch.uint8).numpy()
    b = torch.randint(64, 256, (150, 20, 12, 3), generator=g, dtype=torch.uint8).numpy()
    np.savez(tmp_path / "a.npz", arr_0=a)
    np.save(tmp_path / "b.npy", b)
    ref, fb = str(tmp_path / "a_stats.npz"), str(tmp_path / "b_feats.npz")
    assert D.main(["stats", "--images", str(tmp_path / "a.npz"), "--dinov2-weights", dino_file, "--output", ref, "--batch-size", "48"]) == ref
    assert D.main(["features", "--images", str(tmp_path / "b.npy"), "--dinov2-weights", dino_file, "--output", fb]) == fb
    mu, sigma = D.load_stats(ref)
    assert mu.shape == (128,) and sigma.shape == (128, 128)
    capsys.readouterr()
    same = D.main(["compare", ref, ref])                       # a set with itself: 0 within 1e-8 of the trace
    assert f"fd_dinov2: {same:.6f}" in capsys.readouterr().out.splitlines()
    assert abs(same) <= 1e-8 * np.trace(sigma)
    # two different sets: the distance of the numpy statistics of the same features
    net = D.DinoV2Features.from_file(dino_file, DEV)
    fa, fbn = net.features(torch.from_numpy(a).to(DEV)).double().cpu().numpy(), D.load_features(fb).astype(np.float64)
    assert np.array_equal(net.features(torch.from_numpy(b).to(DEV)).cpu().numpy(), D.load_features(fb))       # batches of 64 or one: the same bits
    want = FID.frechet_distance(fa.mean(0), np.cov(fa, rowvar=False), fbn.mean(0), np.cov(fbn, rowvar=False))
    got = D.main(["compare", ref, fb])
    also = D.main(["compare", str(tmp_path / "a.npz"), str(tmp_path / "b.npy"), "--dinov2-weights", dino_file])
    print(f"fd_dinov2 of two sets: {got:.9f} (numpy statistics: {want:.9f})")
    # the device's fp64 sums and numpy's differ in the last bits of a covariance entry; an eigenvalue at the rounding floor carries that
    # into its square root: D sqrt(D eps) lambda_max, the floor tests/test_fid_cpu.py derives for the sqrt-of-eigenvalues form
    floor = 128 * np.sqrt(128 * np.finfo(np.float64).eps) * max(np.linalg.eigvalsh(sigma)[-1], np.linalg.eigvalsh(np.cov(fbn, rowvar=False))[-1])
    assert got > 0 and abs(got - want) <= floor and also == got
    # precision / recall and KID take the same rows (D = 128 is a multiple of 4)
    from mapdit_amd import metrics
    pr = metrics.precision_recall(torch.from_numpy(fa).float().to(DEV), torch.from_numpy(D.load_features(fb)).to(DEV), k=3)
    assert set(pr) >= {"precision", "recall"}


def test_sample_fid_prints_fd_dinov2_one_process_and_two_shards(dino_file, tmp_path_factory, tmp_path, capsys):
    from mapdit_amd import sample_fid, train
    D = _D()
    run_dir = train.main(["--synthetic", "--results-dir", str(tmp_path_factory.mktemp("dino_results")), "--model", "DiT-XS/2", "--num-steps", "8",
                          "--batch-size", "8", "--log-every", "4", "--ckpt-every", "8", "--ema-snapshot-every", "2", "--num-classes", "10",
                          "--num-lin-warmup", "2", "--start-decay", "3", "--verbose", "0"])
    vae_w, ref = str(tmp_path / "tiny_vae.safetensors"), str(tmp_path / "dref.npz")
    # four levels: 8 x the latent size, the pixels a --sample-rng counter part is checked to have (VR.TINY has three)
    VR.write_safetensors(VR.init_state_dict(dict(block_out_channels=(64, 64, 64, 128), layers_per_block=1, latent_channels=4, out_channels=3), seed=2,
                                            generation="old"), vae_w)
    rng = np.random.default_rng(8)
    D.save_stats(ref, 0.2 * rng.standard_normal(128), np.eye(128) * 0.05)
    base = ["--result-dir", run_dir, "--num-classes", "10", "--num-sampling-steps", "2", "--batch-size", "4", "--num-samples", "6", "--vae-weights", vae_w,
            "--sample-rng", "counter", "--dinov2-ref", ref, "--dinov2-weights", dino_file]
    capsys.readouterr()
    path = sample_fid.main(base + ["--output-file", "one.npz"])
    said = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("fd_dinov2:")]
    rec = json.load(open(path + ".fd_dinov2.json"))
    assert len(said) == 1 and said[0] == f"fd_dinov2: {rec['fd_dinov2']:.6f}" and np.isfinite(rec["fd_dinov2"]) and rec["fd_dinov2"] > 0
    assert rec == {"fd_dinov2": rec["fd_dinov2"], "n": 6, "ref": ref, "precision": "f16", "samples": path}
    assert path.endswith("one.npz") and not os.path.exists(path + ".fid.json")
    # the number is that of the stored array
    arr = np.load(path)["arr_0"]
    assert arr.shape == (6, 256, 256, 3)
    st = D.stats_of_images(arr, D.DinoV2Features.from_file(dino_file, DEV), 6)
    assert D.fd_dinov2(*st.mean_cov(), *D.load_stats(ref)) == rec["fd_dinov2"]
    # two shards: the first leaves parts and no number, the second assembles the same bytes and the same value
    got = sample_fid.main(base + ["--output-file", "two.npz", "--shard", "0/2"])
    assert got == sample_fid.parts_dir(run_dir, "two.npz") and "fd_dinov2:" not in capsys.readouterr().out
    path2 = sample_fid.main(base + ["--output-file", "two.npz", "--shard", "1/2"])
    said2 = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("fd_dinov2:")]
    assert np.load(path2)["arr_0"].tobytes() == arr.tobytes() and said2 == said
    assert json.load(open(path2 + ".fd_dinov2.json"))["fd_dinov2"] == rec["fd_dinov2"] and not os.path.exists(path2 + ".fid.json")
    # the manifest knows nothing of the flags: the same run without them finds every part and writes the same file
    manifest = open(os.path.join(sample_fid.parts_dir(run_dir, "one.npz"), "manifest.json")).read()
    assert "dinov2" not in manifest
