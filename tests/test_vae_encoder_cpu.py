"""Host side of the native VAE encoder (map-dit_amd/vae.py, map-dit_amd/encode_data.py, mapdit_vae_encode_workspace_bytes): key set,
config inference, the weight table against the header's enums, refusals - and the yardstick itself
(tests/vae_encoder_reference.py).  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_encoder_reference as E  # noqa: E402
import vae_reference as R  # noqa: E402

A = "encoder.mid_block.attentions.0."


def _vae():
    import mapdit_amd.vae as V
    return V


@pytest.fixture(scope="module")
def sd_default():
    return E.init_encoder_state_dict(R.DEFAULT, seed=1)


@pytest.fixture(scope="module")
def sd_tiny():
    return E.init_encoder_state_dict(R.TINY, seed=2)


def test_key_set_of_the_default_config(sd_default):
    V = _vae()
    shapes = V.encoder_shapes()                                              # defaults = stabilityai/sd-vae-ft-mse
    assert set(shapes) == set(sd_default)
    assert all(tuple(sd_default[k].shape) == tuple(s) for k, s in shapes.items())
    assert shapes["encoder.conv_out.weight"] == (8, 512, 3, 3) and shapes["quant_conv.weight"] == (8, 8, 1, 1)
    assert shapes["encoder.conv_in.weight"] == (128, 3, 3, 3)
    for name in ("encoder.conv_in", "encoder.down_blocks.0.resnets.1.norm1", "encoder.down_blocks.3.resnets.0.conv2",
                 "encoder.down_blocks.2.downsamplers.0.conv", "encoder.mid_block.resnets.0.conv1", "encoder.mid_block.resnets.1.norm2",
                 A + "group_norm", A + "to_q", A + "to_k", A + "to_v", A + "to_out.0", "encoder.conv_norm_out", "encoder.conv_out", "quant_conv"):
        assert name + ".weight" in shapes and name + ".bias" in shapes, name
    # conv_shortcut exactly where the width changes: blocks 1 and 2; the last block has no downsampler; two resnets per block
    assert "encoder.down_blocks.1.resnets.0.conv_shortcut.weight" in shapes and "encoder.down_blocks.2.resnets.0.conv_shortcut.weight" in shapes
    assert "encoder.down_blocks.3.resnets.0.conv_shortcut.weight" not in shapes and "encoder.down_blocks.0.resnets.0.conv_shortcut.weight" not in shapes
    assert "encoder.down_blocks.3.downsamplers.0.conv.weight" not in shapes and "encoder.down_blocks.0.resnets.2.norm1.weight" not in shapes
    # 2 (conv_in) + 10 resnets x 8 + 2 shortcuts x 2 + 3 downsamplers x 2 + 10 (attention) + 6 (conv_norm_out, conv_out, quant_conv)
    assert len(shapes) == 2 + 80 + 4 + 6 + 10 + 6
    assert sum(v.numel() for v in sd_default.values()) == 34_163_664          # the published 34.16 M of sd-vae-ft-mse's encoder side


def test_config_inference_from_a_state_dict_alone(sd_default, sd_tiny):
    V = _vae()
    assert V.infer_encoder_config(sd_default) == dict(block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=4, out_channels=3)
    assert V.infer_encoder_config(sd_tiny) == dict(block_out_channels=(64, 64, 128), layers_per_block=1, latent_channels=4, out_channels=3)
    e = V.VAEEncoder.from_state_dict(sd_tiny, "cpu")
    assert e.cfg["block_out_channels"] == (64, 64, 128) and e.scale == 4 and e.precision == "f16" and e.max_batch == 16
    assert (e._cfg.num_blocks, e._cfg.ch0, e._cfg.ch1, e._cfg.ch2, e._cfg.ch3, e._cfg.layers_per_block) == (3, 64, 64, 128, 0, 1)
    assert (e._cfg.latent_channels, e._cfg.out_channels) == (4, 3)
    # one file with both halves serves both classes; each ignores the other's keys
    both = dict(sd_tiny, **R.init_state_dict(R.TINY, seed=2))
    e2, d2 = V.VAEEncoder.from_state_dict(both, "cpu"), V.VAEDecoder.from_state_dict(both, "cpu")
    assert e2.packed.keys() == e.packed.keys() and all(torch.equal(e2.packed[k], e.packed[k]) for k in e.packed)
    assert all(k.startswith(("decoder.", "post_quant_conv.")) for k in d2.packed) and all(k.startswith(("encoder.", "quant_conv.")) for k in e2.packed)


def test_slot_table_follows_the_header_enums(sd_tiny):
    import mapdit_amd
    L = mapdit_amd._lib
    V = _vae()
    e = V.VAEEncoder.from_state_dict(sd_tiny, "cpu", precision="bf16")
    names = e.slot_names()
    assert L.VAE_E_NUM_GLOBAL == 14 and L.VAE_NUM_DOWN == 2 and (L.VAE_D_W, L.VAE_D_B) == (0, 1)
    assert len(names) == L.VAE_E_NUM_GLOBAL + (3 * 1 + 2) * L.VAE_NUM_RESNET + 2 * L.VAE_NUM_DOWN
    want = {"CONV_IN_W": "encoder.conv_in.weight", "CONV_IN_B": "encoder.conv_in.bias", "ATTN_GN_G": A + "group_norm.weight",
            "ATTN_GN_B": A + "group_norm.bias", "ATTN_QKV_W": A + "qkv.weight", "ATTN_QKV_B": A + "qkv.bias", "ATTN_OUT_W": A + "to_out.0.weight",
            "ATTN_OUT_B": A + "to_out.0.bias", "NORM_OUT_G": "encoder.conv_norm_out.weight", "NORM_OUT_B": "encoder.conv_norm_out.bias",
            "CONV_OUT_W": "encoder.conv_out.weight", "CONV_OUT_B": "encoder.conv_out.bias", "QUANT_W": "quant_conv.weight", "QUANT_B": "quant_conv.bias"}
    assert sorted(getattr(L, "VAE_E_" + k) for k in want) == list(range(14))
    for k, v in want.items():
        assert names[getattr(L, "VAE_E_" + k)] == v, k
    order = ["encoder.down_blocks.0.resnets.0", "encoder.down_blocks.1.resnets.0", "encoder.down_blocks.2.resnets.0",
             "encoder.mid_block.resnets.0", "encoder.mid_block.resnets.1"]
    for i, r in enumerate(order):
        base = L.VAE_E_NUM_GLOBAL + i * L.VAE_NUM_RESNET
        assert names[base + L.VAE_R_N1_G] == r + ".norm1.weight" and names[base + L.VAE_R_C2_B] == r + ".conv2.bias", r
        assert names[base + L.VAE_R_SC_W] == (r + ".conv_shortcut.weight" if r == "encoder.down_blocks.2.resnets.0" else None)
    tail = L.VAE_E_NUM_GLOBAL + 5 * L.VAE_NUM_RESNET
    assert names[tail:] == ["encoder.down_blocks.0.downsamplers.0.conv.weight", "encoder.down_blocks.0.downsamplers.0.conv.bias",
                            "encoder.down_blocks.1.downsamplers.0.conv.weight", "encoder.down_blocks.1.downsamplers.0.conv.bias"]
    assert sorted(n for n in names if n is not None) == sorted(e.packed)       # every packed tensor exactly once
    assert e.packed["encoder.conv_out.weight"].shape == (8, 3, 3, 128) and e.packed["encoder.conv_out.weight"].dtype == torch.bfloat16
    assert e.packed["quant_conv.weight"].shape == (8, 1, 1, 8) and e.packed[A + "qkv.weight"].shape == (384, 1, 1, 128)


def test_missing_unexpected_and_doubled_keys_are_named(sd_tiny):
    V = _vae()
    sd = dict(sd_tiny)
    del sd["encoder.down_blocks.1.resnets.0.norm2.bias"]
    with pytest.raises(KeyError, match=r"missing key 'encoder\.down_blocks\.1\.resnets\.0\.norm2\.bias'"):
        V.VAEEncoder.from_state_dict(sd, "cpu")
    with pytest.raises(KeyError, match=r"unexpected key 'encoder\.mid_block\.resnets\.2\.norm1\.weight'"):
        V.VAEEncoder.from_state_dict(dict(sd_tiny, **{"encoder.mid_block.resnets.2.norm1.weight": torch.zeros(128)}), "cpu")
    with pytest.raises(KeyError, match="unexpected key 'loss.logvar'"):
        V.VAEEncoder.from_state_dict(dict(sd_tiny, **{"loss.logvar": torch.zeros(1)}), "cpu")
    with pytest.raises(ValueError, match=r"'quant_conv\.weight' has shape"):
        V.VAEEncoder.from_state_dict(dict(sd_tiny, **{"quant_conv.weight": torch.zeros(8, 4, 1, 1)}), "cpu")
    with pytest.raises(KeyError, match=r"missing key 'encoder\.conv_out\.weight'"):
        V.VAEEncoder.from_state_dict({k: v for k, v in sd_tiny.items() if k != "encoder.conv_out.weight"}, "cpu")
    # both attention key generations in one state dict
    with pytest.raises(KeyError, match=r"to_q\.weight' is given twice"):
        V.VAEEncoder.from_state_dict(dict(sd_tiny, **{A + "query.weight": sd_tiny[A + "to_q.weight"]}), "cpu")
    with pytest.raises(NotImplementedError):
        V.VAEEncoder.from_state_dict(sd_tiny, "cpu").encode(torch.zeros(1, 3, 16, 24))


def test_both_attention_key_generations_pack_to_identical_bits():
    V = _vae()
    forms = [E.init_encoder_state_dict(R.TINY, seed=3, generation=g, conv_attention=c) for g in ("new", "old") for c in (False, True)]
    assert A + "query.weight" in forms[2] and forms[3][A + "proj_attn.weight"].dim() == 4
    packed = [V.VAEEncoder.from_state_dict(sd, "cpu").packed for sd in forms]
    for p in packed[1:]:
        assert p.keys() == packed[0].keys()
        assert all(p[k].dtype == packed[0][k].dtype and torch.equal(p[k], packed[0][k]) for k in p)


def test_workspace_bytes_and_shape_refusals(sd_tiny):
    import mapdit_amd
    L = mapdit_amd._lib
    lib = L.lib()
    e = _vae().VAEEncoder.from_state_dict(sd_tiny, "cpu")
    sizes = [e.workspace_bytes(n, 16, 24) for n in (1, 2, 4)]
    assert sizes[0] > 0 and sizes == sorted(set(sizes))
    # three fp32 and one 16-bit activation of E = N H W ch0 elements dominate: 14 E and the small attention / GroupNorm buffers
    E0 = 4 * 16 * 24 * 64
    assert 14 * E0 <= sizes[2] < 14 * E0 + (1 << 20)
    with pytest.raises(ValueError, match="18 x 24 is not a multiple of 4"):
        e.workspace_bytes(1, 18, 24)
    with pytest.raises(ValueError, match="9 tokens.*multiple of 8"):
        e.workspace_bytes(1, 12, 12)
    with pytest.raises(ValueError, match="positive"):
        e.workspace_bytes(0, 16, 24)
    d = L.VaeConfig(latent_channels=4, out_channels=3, num_blocks=4, ch0=128, ch1=256, ch2=500, ch3=512, layers_per_block=2, norm_num_groups=32, norm_eps=1e-6)
    assert lib.vae_encode_workspace_bytes(ctypes.byref(d), 1, 32, 32) == 0 and b"500" in lib.last_error()


def test_restated_downsample_equals_an_explicit_loop():
    """Output (y, x) reads input (2 y + ky, 2 x + kx); rows / columns at or past the size are zeros.  5 x 8: an odd and an even size."""
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 5, 8, generator=g, dtype=torch.float64)
    w = torch.randn(4, 3, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(4, generator=g, dtype=torch.float64)
    got = E.downsample(x, w, b)
    assert got.shape == (2, 4, 2, 4)
    want = torch.zeros_like(got)
    for y in range(2):
        for xx in range(4):
            acc = b.clone()[None].repeat(2, 1)
            for ky in range(3):
                for kx in range(3):
                    sy, sx = 2 * y + ky, 2 * xx + kx
                    if sy < 5 and sx < 8:
                        acc = acc + x[:, :, sy, sx] @ w[:, :, ky, kx].t()
            want[:, :, y, xx] = acc
    assert float((got - want).abs().max()) < 1e-12
    # for the odd height the pad row is never touched: the last window's rows are 2, 3, 4
    assert torch.equal(E.downsample(x, w, b), E.downsample(torch.cat([x, torch.full((2, 3, 1, 8), 7.0, dtype=torch.float64)], 2), w, b)[:, :, :2])


@pytest.mark.parametrize("dtype, bound", [(torch.float16, 5e-3), (torch.bfloat16, 5e-2)])
def test_operand_rounding_emulation_of_the_restatement(sd_tiny, dtype, bound):
    """Guards the yardstick: rounding every matmul operand to 16 bits moves the result, by less than the decoder restatement's guard."""
    x = torch.rand(2, 3, 16, 24, generator=torch.Generator().manual_seed(21)) * 2 - 1
    mean, logvar = E.encode(sd_tiny, x)
    assert mean.shape == logvar.shape == (2, 4, 4, 6) and mean.dtype == torch.float64 and torch.isfinite(mean).all()
    m2, lv2 = E.encode(sd_tiny, x, operand_dtype=dtype)
    from conftest import rel_err
    e = rel_err(m2.numpy(), mean.numpy())
    print(f"encoder e_emul {dtype}: mean {e:.3e}, logvar {rel_err(lv2.numpy(), logvar.numpy()):.3e}")
    assert 0 < e < bound
    old = E.init_encoder_state_dict(R.TINY, seed=2, generation="old", conv_attention=True)
    assert torch.equal(E.encode(old, x, cfg=R.TINY)[0], mean)


# ---- the script's refusals that need no GPU ----------------------------------------------------------------------------------------------
def _script_args(tmp_path, images, labels, extra=()):
    np.save(tmp_path / "imgs.npy", images)
    np.save(tmp_path / "labels.npy", labels)
    return ["--images", str(tmp_path / "imgs.npy"), "--labels", str(tmp_path / "labels.npy"), "--vae-weights", str(tmp_path / "nowhere.safetensors"),
            "--output-dir", str(tmp_path / "out"), *extra]


def test_script_argument_refusals(tmp_path):
    from mapdit_amd import encode_data as D
    imgs, labels = np.zeros((5, 16, 24, 3), np.uint8), np.arange(5)
    args = D.build_parser().parse_args(_script_args(tmp_path, imgs, labels))
    assert args.batch_size == 128 and args.flip is True and args.seed == 0 and args.vae_precision == "f16" and not args.overwrite
    assert D.build_parser().parse_args(_script_args(tmp_path, imgs, labels, ["--no-flip"])).flip is False
    with pytest.raises(ValueError, match="5 images and --labels 4 labels"):
        D.main(_script_args(tmp_path, imgs, labels[:4]))
    with pytest.raises(ValueError, match="float32, expected uint8"):
        D.main(_script_args(tmp_path, imgs.astype(np.float32), labels))
    with pytest.raises(ValueError, match=r"expected \[N, H, W, C\]"):
        D.main(_script_args(tmp_path, imgs[0], labels))
    with pytest.raises(ValueError, match="integer"):
        D.main(_script_args(tmp_path, imgs, labels.astype(np.float32)))
    os.makedirs(tmp_path / "out")
    (tmp_path / "out" / "stats.pt").write_bytes(b"x")
    with pytest.raises(FileExistsError, match=r"stats\.pt exists.*--overwrite"):
        D.main(_script_args(tmp_path, imgs, labels))
    (tmp_path / "out" / "stats.pt").write_bytes(b"")                           # an empty file is no data
    with pytest.raises(FileNotFoundError, match="nowhere.safetensors"):        # past the array checks: the weights come next
        D.main(_script_args(tmp_path, imgs, labels))
    with pytest.raises(FileNotFoundError, match="missing.npy"):
        D.main(["--images", str(tmp_path / "missing.npy"), "--labels", str(tmp_path / "labels.npy"), "--vae-weights", "w", "--output-dir", str(tmp_path / "o")])


def test_flip_flags_depend_on_seed_and_index_only():
    from mapdit_amd import encode_data as D
    f = D.flip_flags(1000, 0)
    assert f.dtype == torch.uint8 and f.shape == (1000,) and 400 < int(f.sum()) < 600
    assert torch.equal(D.flip_flags(1000, 0), f) and not torch.equal(D.flip_flags(1000, 1), f)
    assert torch.equal(D.flip_flags(10, 0), f[:10])                            # image i's flag does not depend on how many follow
