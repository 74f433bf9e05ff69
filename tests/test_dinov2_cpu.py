"""CPU-side checks of FD-DINOv2: the fp64 restatement (tests/dinov2_reference.py) pinned to torch.nn.functional - the thing EDM2
calls - the position-table interpolation, the loader's refusals, sample_fid's flag refusals, the file keys and ``compare`` on two
statistics files; and the measurement of e_emul, the tolerance unit of the GPU tests."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dinov2_reference as R  # noqa: E402


def _D():
    from mapdit_amd import dinov2
    return dinov2


# ---- the restatement against torch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h, w, s", [(32, 32, 28), (64, 64, 28), (16, 16, 28), (40, 24, 28), (256, 256, 224)])
def test_resize_equals_torch_antialiased_bicubic(h, w, s):
    g = torch.Generator().manual_seed(h + w)
    x = torch.rand(2, 3, h, w, generator=g, dtype=torch.float64) * 255
    want = F.interpolate(x, size=(s, s), mode="bicubic", antialias=True, align_corners=False)
    got = R.resize_aa(x.numpy(), s)
    assert float(np.abs(got - want.numpy()).max()) <= 1e-10
    # no clamping: a 0 / 255 edge overshoots both ends of the byte range, as torch's does
    edge = torch.zeros(1, 1, h, w, dtype=torch.float64)
    edge[..., w // 2:] = 255.0
    got = R.resize_aa(edge.numpy(), s)
    want = F.interpolate(edge, size=(s, s), mode="bicubic", antialias=True, align_corners=False)
    assert float(got.min()) < -0.4 and float(got.max()) > 255.4 and float(np.abs(got - want.numpy()).max()) <= 1e-10


def test_block_pieces_equal_torch_in_fp64():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(7, 128, generator=g, dtype=torch.float64) * 3
    x[:, 5] = 300
    w, b = torch.rand(128, generator=g, dtype=torch.float64), torch.randn(128, generator=g, dtype=torch.float64)
    assert float((R.layernorm(x, w, b, 1e-6) - F.layer_norm(x, (128,), w, b, 1e-6)).abs().max()) <= 1e-12
    assert float((R.gelu(x) - F.gelu(x)).abs().max()) <= 1e-12 * 300
    assert float((R.gelu(x[:, :5]) - F.gelu(x[:, :5])).abs().max()) <= 1e-12
    N, T, H = 2, 13, 2
    qkv = torch.randn(N, T, 3 * 64 * H, generator=g, dtype=torch.float64)
    q, k, v = (qkv[:, :, i * 128:(i + 1) * 128].reshape(N, T, H, 64).transpose(1, 2) for i in range(3))
    want = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(N, T, 128)
    assert float((R.attention(qkv, H) - want).abs().max()) <= 1e-12
    patch, cls, pos = torch.randn(N * 4, 128, generator=g), torch.randn(128, generator=g), torch.randn(5, 128, generator=g)
    tok = R.embed(patch.double(), cls, pos, N)
    assert tok.shape == (N, 5, 128) and torch.equal(tok[1, 0], (cls.double() + pos[0].double())) and torch.equal(tok[1, 3], patch[6].double() + pos[3].double())


def test_patch_rows_layout():
    """Row (n, gy, gx), column (c, py, px): what a [D, 3, 14, 14] convolution with stride 14 multiplies."""
    images = R.case_images("28to28")
    rows = R.patch_rows(images, 28)
    assert rows.shape == (8, 592) and float(rows[:, 588:].abs().max()) == 0
    x = images.permute(0, 3, 1, 2).double() / 255
    x = (x - torch.tensor(R.MEAN, dtype=torch.float64)[None, :, None, None]) / torch.tensor(R.STD, dtype=torch.float64)[None, :, None, None]
    w = torch.randn(16, 3, 14, 14, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    want = F.conv2d(x, w, stride=14).permute(0, 2, 3, 1).reshape(8, 16)
    assert float((rows[:, :588] @ w.reshape(16, 588).T - want).abs().max()) <= 1e-11


# ---- the position table ---------------------------------------------------------------------------------------------------------------
def test_position_table_interpolation():
    D = _D()
    sd = R.make_state_dict(128, 1, 512)
    small = D.interpolate_pos_embed(sd["pos_embed"], 16)
    assert small.shape == (257, 128) and small.dtype == torch.float32 and torch.equal(small[0], sd["pos_embed"][0, 0])
    same = D.interpolate_pos_embed(sd["pos_embed"], 37)
    assert torch.equal(same, sd["pos_embed"][0])                              # 37 -> 37: the table as it is
    # the explicit restatement (scale FACTOR (g + 0.1) / 37 places the samples): fp32 interpolation against fp64
    for g in (16, 2):
        assert float((D.interpolate_pos_embed(sd["pos_embed"], g).double() - R.interpolate_pos(sd["pos_embed"], g)).abs().max()) <= 2e-5
    # the offset is what it says: without it the samples sit elsewhere
    assert float((D.interpolate_pos_embed(sd["pos_embed"], 16, 0.0) - small).abs().max()) > 1e-4


# ---- the loader's refusals ------------------------------------------------------------------------------------------------------------
def test_state_dict_checks():
    D = _D()
    sd = R.make_state_dict(128, 2, 512)
    out, dims = D.check_state_dict(sd)
    assert dims == (128, 2, 512, 37) and "mask_token" not in out and D.feature_dim(sd) == 128
    assert D.check_state_dict({"backbone." + k: v for k, v in sd.items()})[1] == dims
    assert D.check_state_dict(R.make_state_dict(384, 1, 1536))[1] == (384, 1, 1536, 37)          # ViT-S shapes load too
    bad = dict(sd)
    del bad["blocks.1.ls2.gamma"]
    with pytest.raises(KeyError, match=r"missing key 'blocks\.1\.ls2\.gamma'"):
        D.check_state_dict(bad)
    with pytest.raises(KeyError, match=r"unexpected key 'blocks\.0\.attn\.q_norm\.weight'"):
        D.check_state_dict({**sd, "blocks.0.attn.q_norm.weight": torch.zeros(64)})
    with pytest.raises(KeyError, match=r"'norm\.weight' is given twice"):
        D.check_state_dict({**sd, "backbone.norm.weight": sd["norm.weight"]})
    with pytest.raises(NotImplementedError, match=r"register_tokens.*register variants"):
        D.check_state_dict({**sd, "register_tokens": torch.zeros(1, 4, 128)})
    swiglu = {k: v for k, v in sd.items() if ".mlp.fc1." not in k}
    swiglu["blocks.0.mlp.w12.weight"] = torch.zeros(1024, 128)
    with pytest.raises(NotImplementedError, match=r"mlp\.w12.*SwiGLU"):
        D.check_state_dict(swiglu)
    with pytest.raises(ValueError, match=r"'blocks\.0\.attn\.qkv\.weight' has shape \(384, 64\), expected \(384, 128\)"):
        D.check_state_dict({**sd, "blocks.0.attn.qkv.weight": torch.zeros(384, 64)})
    with pytest.raises(ValueError, match="head dimension"):
        D.check_state_dict(R.make_state_dict(96, 1, 384))
    with pytest.raises(NotImplementedError, match="GPU only"):
        D.DinoV2Features.from_state_dict(sd, "cpu")
    with pytest.raises(KeyError, match="missing key"):                        # a bad file is named before the device is
        D.DinoV2Features.from_state_dict(bad, "cpu")


def test_library_refusals_name_their_cause():
    """mapdit_vit_workspace_bytes is a host query: every refusal of the configuration, with its message."""
    import ctypes
    import mapdit_amd
    L = mapdit_amd._lib
    lib = L.lib()
    ok = dict(image_size=224, patch=14, dim=1024, depth=24, heads=16, mlp_dim=4096, ln_eps=1e-6)

    def need(n=1, **kw):
        return lib.vit_workspace_bytes(ctypes.byref(L.VitConfig(**{**ok, **kw})), n)

    one, many = need(1), need(32)
    M = 257
    assert one >= 256 * 592 * 2 + M * 1024 * (4 + 4 + 2 + 2 + 6) + M * 4096 * 2 and one < 2 * (256 * 592 * 2 + M * 1024 * 18 + M * 4096 * 2)
    assert 31 * one < many <= 32 * one
    for kw, n, word in ((dict(heads=32), 1, "head_dim 64"), (dict(dim=1032, heads=16), 1, "64 * heads"), (dict(mlp_dim=4100), 1, "multiples of 16"),
                        (dict(image_size=225), 1, "multiple of the patch"), (dict(patch=16, image_size=224), 1, "patch=16"), ({}, 0, "N=0"),
                        (dict(depth=0), 1, "depth")):
        assert need(n, **kw) == 0 and word.encode() in lib.last_error(), (kw, lib.last_error())
    assert need(1, dim=384, heads=6, mlp_dim=1536, depth=12) > 0 and need(1, image_size=518) > 0            # ViT-S; T = 1,370


# ---- sample_fid's flags, the file keys, compare ----------------------------------------------------------------------------------------
def _files(tmp_path, dim_ref=128, dim_net=128):
    D = _D()
    ref, w = str(tmp_path / "dref.npz"), str(tmp_path / "dino.pt")
    D.save_stats(ref, np.zeros(dim_ref), np.eye(dim_ref))
    torch.save(R.make_state_dict(dim_net, 1, 4 * dim_net), w)
    return ref, w


@pytest.mark.parametrize("flags, exc, match", [
    (["--dinov2-ref", "ref.npz"], ValueError, "go together"),
    (["--dinov2-weights", "w.pt"], ValueError, "go together"),
    (["--dinov2-ref", "nowhere_ref.npz", "--dinov2-weights", "w.pt"], FileNotFoundError, "nowhere_ref.npz"),
])
def test_sample_fid_refuses_half_of_the_dinov2_pair_before_any_model_is_built(tmp_path, flags, exc, match):
    from mapdit_amd import sample_fid
    with pytest.raises(exc, match=match):                     # before config.yaml of the (equally missing) run directory is read
        sample_fid.main(["--result-dir", str(tmp_path / "no_such_run")] + flags)


def test_sample_fid_dinov2_flags_need_pixels_and_matching_dimensions(tmp_path):
    from mapdit_amd import sample_fid
    ref, w = _files(tmp_path)
    with pytest.raises(ValueError, match="pixels"):
        sample_fid.main(["--result-dir", str(tmp_path / "no_such_run"), "--use-vae", "false", "--dinov2-ref", ref, "--dinov2-weights", w])
    ref192, _ = _files(tmp_path / ".", dim_ref=192)
    with pytest.raises(ValueError, match="statistics of 192 dimensions.*dim 128"):
        sample_fid.main(["--result-dir", str(tmp_path / "no_such_run"), "--dinov2-ref", ref192, "--dinov2-weights", w])
    args = sample_fid.build_parser().parse_args(["--result-dir", "x"])
    assert args.dinov2_ref is None and args.dinov2_weights is None and args.dinov2_precision == "f16" and sample_fid.check_dinov2_flags(args) is False
    from mapdit_amd import metrics
    assert "fd_dinov2" not in metrics.METRICS                  # flags of its own, not a name of --metrics


def test_file_keys_round_trip_beside_fid_keys(tmp_path):
    D = _D()
    from mapdit_amd import fid as FID
    rng = np.random.default_rng(1)
    path = str(tmp_path / "both.npz")
    FID.save_stats(path, rng.standard_normal(2048), np.eye(2048))
    mu, a = rng.standard_normal(64), rng.standard_normal((64, 64))
    D.save_stats(path, mu, a @ a.T, keep=True)                 # the FID keys stay: the two sets never collide
    with np.load(path) as z:
        assert sorted(z.files) == ["mu", "mu_dinov2", "sigma", "sigma_dinov2"]
    got = D.load_stats(path)
    assert np.array_equal(got[0], mu) and np.array_equal(got[1], a @ a.T) and FID.load_stats(path)[0].shape == (2048,)
    feats = rng.standard_normal((9, 64)).astype(np.float32)
    fpath = str(tmp_path / "feats.npz")
    D.save_features(fpath, feats, mu, a @ a.T)
    assert np.array_equal(D.load_features(fpath), feats) and np.array_equal(D.load_stats(fpath)[0], mu)
    with pytest.raises(KeyError, match="no 'mu_dinov2'"):
        only_fid = str(tmp_path / "fid_only.npz")
        FID.save_stats(only_fid, np.zeros(4), np.eye(4))
        D.load_stats(only_fid)
    with pytest.raises(KeyError, match="no 'dinov2_features'"):
        D.load_features(path)


def test_compare_two_statistics_files_needs_no_gpu_and_no_weights(tmp_path, capsys):
    D = _D()
    from mapdit_amd import fid as FID
    rng = np.random.default_rng(2)
    pairs = []
    for name in ("a", "b"):
        x = rng.standard_normal((200, 48)) * (1.0 + 0.2 * (name == "b")) + 0.3 * (name == "b")
        pairs.append((x.mean(0), np.cov(x, rowvar=False)))
        D.save_stats(str(tmp_path / f"{name}.npz"), *pairs[-1])
    value = D.main(["compare", str(tmp_path / "a.npz"), str(tmp_path / "b.npz")])
    assert value == FID.frechet_distance(*pairs[0], *pairs[1]) and value > 0
    assert f"fd_dinov2: {value:.6f}" in capsys.readouterr().out.splitlines()
    np.save(tmp_path / "imgs.npy", np.zeros((2, 16, 16, 3), np.uint8))
    with pytest.raises(ValueError, match="--dinov2-weights"):
        D.main(["compare", str(tmp_path / "imgs.npy"), str(tmp_path / "a.npz")])


# ---- the tolerance unit of the GPU tests -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_e_emul_constants_of_the_gpu_tests_are_what_is_measured(prec):
    """e_emul = max |ref(emulate=p) - ref(None)| / max |ref(None)| on the inputs of every GPU case: the named constants in the two GPU
    test files are these measurements (to the three digits they are written with)."""
    import test_dinov2_gpu as G
    import test_dinov2_kernels_gpu as K
    measured = R.measure_e_emul(prec)
    written = {**K.E_EMUL[prec], **G.E_EMUL[prec]}
    assert sorted(written) == sorted(measured)
    for k, v in measured.items():
        print(f"e_emul {prec} {k}: {v:.3e}")
        assert abs(written[k] - v) <= 2e-3 * v, (k, written[k], v)
        assert v < (0.02 if prec == "bf16" else 0.002)         # a few units of the format at the most
