"""``mapdit_vit_tokens`` through ``dinov2.DinoV2Features.tokens``: every token after the final LayerNorm against the fp64 restatement
(tests/dinov2_reference.py: its pieces, recomposed here with the final LayerNorm on every row) on random weights (dim 128, depth 2), at
grid 2 (T = 5) and grid 16 (T = 257), in both operand formats.  Limits: the walk's - max |tokens - ref| <= 2 x e_emul x max |ref| with
the E_EMUL of tests/test_dinov2_gpu.py's cases, which these are (walk28: 28 pixels, N = 3; walk224: 224 pixels, N = 2).  Row 0 is the
CLS token with the bits of ``features``; an image alone and in a batch gives the same bits; the ``tokens`` subcommand writes the fp16
file train.py --repa-features reads."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dinov2_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
E_EMUL = {"f16": {"walk28": 7.893e-04, "walk224": 6.624e-04}, "bf16": {"walk28": 1.058e-02, "walk224": 5.922e-03}}      # tests/test_dinov2_gpu.py


def _D():
    from mapdit_amd import dinov2
    return dinov2


def vit_tokens(sd, images, image_size):
    """dinov2_reference.vit_forward with the final LayerNorm on every row: fp64 [N, T, D]."""
    D = sd["cls_token"].shape[-1]
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    rows = R.patch_rows(images, image_size)
    N = rows.shape[0] // (image_size // R.PATCH) ** 2
    wp = torch.zeros(D, R.PATCH_K, dtype=torch.float64)
    wp[:, :3 * R.PATCH * R.PATCH] = sd["patch_embed.proj.weight"].double().reshape(D, -1)
    pos = R.interpolate_pos(sd["pos_embed"], image_size // R.PATCH).float().double()
    x = R.embed(R.linear(rows, wp, sd["patch_embed.proj.bias"]), sd["cls_token"].reshape(D), pos, N)
    for i in range(depth):
        p = f"blocks.{i}."
        h = R.layernorm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"])
        a = R.attention(R.linear(h, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"]), D // 64)
        x = x + sd[p + "ls1.gamma"].double() * R.linear(a, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
        h = R.layernorm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"])
        f = R.gelu(R.linear(h, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"]))
        x = x + sd[p + "ls2.gamma"].double() * R.linear(f, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
    return R.layernorm(x, sd["norm.weight"], sd["norm.bias"])


@pytest.fixture(scope="module")
def walks():
    out = {}
    for name in R.WALK_CASES:
        sd, images, size = R.case_walk(name)
        ref = vit_tokens(sd, images, size)
        assert torch.allclose(ref[:, 0], R.vit_forward(sd, images, size), rtol=0, atol=1e-12)      # the recomposition is the reference's walk
        out[name] = (sd, images, size, ref)
    return out


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("case", list(R.WALK_CASES))
def test_tokens_against_fp64_and_cls_row_bits(walks, case, prec):
    sd, images, size, ref = walks[case]
    net = _D().DinoV2Features.from_state_dict(sd, DEV, prec, image_size=size)
    x = images.to(DEV)
    tok = net.tokens(x)
    g = size // 14
    assert tok.shape == (len(images), 1 + g * g, 128) and tok.dtype == torch.float32 and torch.isfinite(tok).all()
    err, lim = float((tok.double().cpu() - ref).abs().max()), 2 * E_EMUL[prec][case] * float(ref.abs().max())
    print(f"{case} {prec}: max err over all rows {err:.3e} (limit {lim:.3e})")
    assert err <= lim, (case, prec, err, lim)
    assert torch.equal(tok[:, 0], net.features(x))                               # row 0: the CLS feature, bit for bit
    alone = _D().DinoV2Features.from_state_dict(sd, DEV, prec, image_size=size).tokens(x[1:2])
    assert torch.equal(alone[0], tok[1])                                         # an image alone = the image in a batch
    chunked = _D().DinoV2Features.from_state_dict(sd, DEV, prec, max_batch=1, image_size=size).tokens(x)
    assert torch.equal(chunked, tok)
    t16 = net.tokens(x, out16=True)                                              # the 16-bit output: the same values, rounded once
    assert t16.dtype == (torch.float16 if prec == "f16" else torch.bfloat16)
    assert torch.equal(t16, tok.to(t16.dtype))


def test_patch_rows_follow_the_grid_order(walks):
    """Rows 1 + p are the patches in row-major grid order: an image whose top-left patch alone differs moves row 1 most."""
    sd, images, size, _ = walks["walk28"]
    net = _D().DinoV2Features.from_state_dict(sd, DEV, "f16", image_size=size)
    a = torch.full((1, 28, 28, 3), 128, dtype=torch.uint8)
    b = a.clone()
    b[0, :14, 14:] = 250                                                         # the patch at (gy, gx) = (0, 1): row 1 + 1
    d = (net.tokens(a.to(DEV)) - net.tokens(b.to(DEV))).abs().sum(-1)[0]
    assert int(d.argmax()) == 2, d


def test_tokens_command_line(walks, tmp_path):
    D = _D()
    from mapdit_amd.encode_data import flip_flags
    sd, images, size, _ = walks["walk28"]
    wfile, ifile, out = str(tmp_path / "w.pt"), str(tmp_path / "imgs.npy"), str(tmp_path / "repa_features.npy")
    torch.save(sd, wfile)
    imgs = torch.cat([images, images.flip(0)]).numpy()                           # 6 images, batches of 4
    np.save(ifile, imgs)
    assert D.main(["tokens", "--images", ifile, "--dinov2-weights", wfile, "--grid", "2", "--output", out, "--batch-size", "4"]) == out
    got = np.load(out, mmap_mode="r")
    assert got.dtype == np.float16 and got.shape == (6, 4, 128)
    net = D.DinoV2Features.from_state_dict(sd, DEV, "f16", image_size=28)
    want = net.tokens(torch.from_numpy(imgs).to(DEV))[:, 1:].half().cpu().numpy()
    assert np.array_equal(np.asarray(got), want)
    D.main(["tokens", "--images", ifile, "--dinov2-weights", wfile, "--grid", "2", "--output", out, "--flip-seed", "2"])
    flips = flip_flags(6, 2).numpy().astype(bool)
    assert flips.tolist() == [False, True, False, True, False, False]          # (seed 2: a mixed draw)
    mirrored = imgs.copy()
    mirrored[flips] = mirrored[flips][:, :, ::-1]
    want = net.tokens(torch.from_numpy(mirrored).to(DEV))[:, 1:].half().cpu().numpy()
    assert np.array_equal(np.load(out), want)
