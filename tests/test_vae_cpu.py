"""Host side of the native VAE decoder (map-dit_amd/vae.py, mapdit_vae_workspace_bytes): key set, config inference, weight packing,
the safetensors reader, refusals, the CLI flag - and the yardstick itself (tests/vae_reference.py).  No GPU."""
import ctypes
import os
import struct
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_reference as R  # noqa: E402
from conftest import rel_err  # noqa: E402


def _vae():
    import mapdit_amd.vae as V
    return V


@pytest.fixture(scope="module")
def sd_default():
    return R.init_state_dict(R.DEFAULT, seed=1)


@pytest.fixture(scope="module")
def sd_tiny():
    return R.init_state_dict(R.TINY, seed=2)


def test_parameter_count_and_key_set_of_the_default_config(sd_default):
    V = _vae()
    assert sum(v.numel() for v in sd_default.values()) == 49_490_199          # the published 49.49 M of sd-vae-ft-mse's decoder side
    shapes = V.decoder_shapes()                                              # defaults = stabilityai/sd-vae-ft-mse
    assert set(shapes) == set(sd_default)
    assert all(tuple(sd_default[k].shape) == tuple(s) for k, s in shapes.items())
    total = 0
    for s in shapes.values():
        n = 1
        for d in s:
            n *= d
        total += n
    assert total == 49_490_199
    # 4 (post_quant_conv, conv_in) + 14 resnets x 8 + 2 shortcuts x 2 + 10 (attention) + 3 upsamplers x 2 + 4 (conv_norm_out, conv_out)
    assert len(shapes) == 140 and "decoder.up_blocks.3.upsamplers.0.conv.weight" not in shapes
    assert "decoder.up_blocks.2.resnets.0.conv_shortcut.weight" in shapes and "decoder.up_blocks.1.resnets.0.conv_shortcut.weight" not in shapes


def test_config_inference_from_shapes(sd_default, sd_tiny):
    V = _vae()
    assert V.infer_config(sd_default) == dict(block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=4, out_channels=3)
    assert V.infer_config(sd_tiny) == dict(block_out_channels=(64, 64, 128), layers_per_block=1, latent_channels=4, out_channels=3)
    d = V.VAEDecoder.from_state_dict(sd_tiny, "cpu")
    assert d.cfg["block_out_channels"] == (64, 64, 128) and d.scale == 4 and d.precision == "f16" and d.max_batch == 16
    assert (d._cfg.num_blocks, d._cfg.ch0, d._cfg.ch1, d._cfg.ch2, d._cfg.ch3, d._cfg.layers_per_block) == (3, 64, 64, 128, 0, 1)


def test_both_attention_key_generations_load_to_identical_packed_weights():
    V = _vae()
    forms = [R.init_state_dict(R.TINY, seed=3, generation=g, conv_attention=c) for g in ("new", "old") for c in (False, True)]
    assert "decoder.mid_block.attentions.0.query.weight" in forms[2] and forms[3]["decoder.mid_block.attentions.0.proj_attn.weight"].dim() == 4
    packed = [V.VAEDecoder.from_state_dict(sd, "cpu").packed for sd in forms]
    for p in packed[1:]:
        assert p.keys() == packed[0].keys()
        assert all(p[k].dtype == packed[0][k].dtype and torch.equal(p[k], packed[0][k]) for k in p)
    qkv = packed[0]["decoder.mid_block.attentions.0.qkv.weight"]
    assert qkv.shape == (384, 1, 1, 128) and qkv.dtype == torch.float16
    assert torch.equal(qkv[128:256, 0, 0], forms[0]["decoder.mid_block.attentions.0.to_k.weight"].half())
    # encoder.* and quant_conv.* are ignored; the slot table names every packed tensor exactly once
    extra = dict(forms[0], **{"encoder.conv_in.weight": torch.zeros(3), "quant_conv.bias": torch.zeros(8)})
    d = V.VAEDecoder.from_state_dict(extra, "cpu", precision="bf16")
    assert d.packed.keys() == packed[0].keys() and d.packed["decoder.conv_in.weight"].dtype == torch.bfloat16
    names = [n for n in d.slot_names() if n is not None]
    assert sorted(names) == sorted(d.packed) and len(d.slot_names()) == 14 + 10 * (2 + 3 * 2) + 2 * 2


def test_missing_and_extra_keys_are_named(sd_tiny):
    V = _vae()
    sd = dict(sd_tiny)
    del sd["decoder.up_blocks.1.resnets.0.norm2.bias"]
    with pytest.raises(KeyError, match=r"missing key 'decoder\.up_blocks\.1\.resnets\.0\.norm2\.bias'"):
        V.VAEDecoder.from_state_dict(sd, "cpu")
    with pytest.raises(KeyError, match=r"unexpected key 'decoder\.mid_block\.resnets\.2\.norm1\.weight'"):
        V.VAEDecoder.from_state_dict(dict(sd_tiny, **{"decoder.mid_block.resnets.2.norm1.weight": torch.zeros(128)}), "cpu")
    with pytest.raises(KeyError, match="unexpected key 'loss.logvar'"):
        V.VAEDecoder.from_state_dict(dict(sd_tiny, **{"loss.logvar": torch.zeros(1)}), "cpu")
    with pytest.raises(ValueError, match="shape"):
        V.VAEDecoder.from_state_dict(dict(sd_tiny, **{"decoder.conv_norm_out.bias": torch.zeros(32)}), "cpu")
    with pytest.raises(ValueError, match="precision"):
        V.VAEDecoder.from_state_dict(sd_tiny, "cpu", precision="fp8")
    with pytest.raises(NotImplementedError):
        V.VAEDecoder.from_state_dict(sd_tiny, "cpu").decode(torch.zeros(1, 4, 4, 6))


def test_packed_layout_is_cout_ky_kx_cin():
    V = _vae()
    w = torch.arange(5 * 3 * 3 * 3, dtype=torch.float32).reshape(5, 3, 3, 3)          # integers < 2048: exact in fp16
    p = V.pack_conv_weight(w, torch.float16)
    assert p.shape == (5, 3, 3, 3) and p.is_contiguous() and p.dtype == torch.float16
    flat = p.reshape(-1)
    for co in range(5):
        for ky in range(3):
            for kx in range(3):
                for c in range(3):
                    assert float(flat[((co * 3 + ky) * 3 + kx) * 3 + c]) == float(w[co, c, ky, kx])
    lin = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    assert torch.equal(V.pack_conv_weight(lin, torch.bfloat16).reshape(4, 3), lin.bfloat16())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_safetensors_round_trip(tmp_path, dtype):
    V = _vae()
    g = torch.Generator().manual_seed(5)
    sd = {"a.weight": torch.randn(3, 5, generator=g).to(dtype), "b": torch.randn(7, generator=g).to(dtype), "c.x": torch.randn(2, 1, 3, 3, generator=g).to(dtype)}
    path = tmp_path / "t.safetensors"
    R.write_safetensors(sd, path)
    back = V.read_safetensors(path)
    assert back.keys() == sd.keys()
    assert all(back[k].dtype == dtype and back[k].shape == sd[k].shape and torch.equal(back[k], sd[k]) for k in sd)
    assert V.load_state_dict_file(str(path)).keys() == sd.keys()
    tp = tmp_path / "t.pt"
    torch.save({"state_dict": sd, "epoch": 3}, tp)
    nested = V.load_state_dict_file(str(tp))
    assert all(torch.equal(nested[k], sd[k]) for k in sd)


def test_safetensors_refusals(tmp_path):
    V = _vae()
    sd = {"a": torch.arange(6, dtype=torch.float32).reshape(2, 3), "b": torch.ones(4)}
    good = tmp_path / "good.safetensors"
    R.write_safetensors(sd, good)
    raw = good.read_bytes()
    unknown = tmp_path / "i64.safetensors"
    R.write_safetensors(sd, unknown, dtype_names={"b": "I64"})
    with pytest.raises(ValueError, match="I64"):
        V.read_safetensors(unknown)
    short = tmp_path / "short.safetensors"
    short.write_bytes(raw[:-5])
    with pytest.raises(ValueError, match="truncated"):
        V.read_safetensors(short)
    (tmp_path / "stub.safetensors").write_bytes(raw[:5])
    with pytest.raises(ValueError, match="truncated"):
        V.read_safetensors(tmp_path / "stub.safetensors")
    over = tmp_path / "over.safetensors"
    over.write_bytes(struct.pack("<Q", len(raw)) + raw[8:])
    with pytest.raises(ValueError, match="overruns"):
        V.read_safetensors(over)
    wrong = tmp_path / "wrong.safetensors"
    R.write_safetensors(sd, wrong, dtype_names={"a": "F16"})                   # 24 bytes cannot be [2, 3] F16
    with pytest.raises(ValueError, match="offsets"):
        V.read_safetensors(wrong)


def test_workspace_bytes_and_refusals():
    import mapdit_amd
    L = mapdit_amd._lib
    lib = L.lib()

    def cfg(ch=(128, 256, 512, 512), groups=32, lpb=2):
        ch = list(ch) + [0] * (4 - len(ch))
        return L.VaeConfig(latent_channels=4, out_channels=3, num_blocks=sum(c > 0 for c in ch), ch0=ch[0], ch1=ch[1], ch2=ch[2], ch3=ch[3],
                           layers_per_block=lpb, norm_num_groups=groups, norm_eps=1e-6)

    def need(c, n, h, w):
        return lib.vae_workspace_bytes(ctypes.byref(c), n, h, w)
    d = cfg()
    sizes = [need(d, n, 32, 32) for n in (1, 2, 4, 16)]
    assert sizes[0] > 0 and sizes == sorted(set(sizes))
    by_area = [need(d, 2, h, w) for h, w in ((8, 8), (8, 16), (16, 16), (32, 32), (64, 64))]
    assert by_area[0] > 0 and by_area == sorted(set(by_area))
    # the formula of mapdit.h: 14 E + 6 N T C + 6 T^2 + the GroupNorm scratch (two fp64 per sample, 1,024-pixel chunk and group), with
    # E = N (8h)(8w) 256 (the first resnet of the last up block reads 256 channels)
    n, h, w = 16, 32, 32
    E, T = n * 64 * h * w * 256, h * w
    assert 0 <= need(d, n, h, w) - (14 * E + 6 * n * T * 512 + 6 * T * T + n * (64 * T // 1024) * 32 * 16) < 8 * 256
    assert need(d, 1, 6, 6) == 0 and b"multiple of 8" in lib.last_error() and b"36" in lib.last_error()
    assert need(cfg(ch=(128, 256, 500, 512)), 1, 8, 8) == 0 and b"500" in lib.last_error() and b"groups" in lib.last_error()
    assert need(d, 0, 8, 8) == 0 and b"N=0" in lib.last_error()
    assert need(d, -1, 8, 8) == 0 and b"positive" in lib.last_error()
    assert need(cfg(ch=(64, 64, 128), lpb=1), 2, 4, 6) > 0
    import mapdit_amd.vae as V
    dec = V.VAEDecoder.from_state_dict(R.init_state_dict(R.TINY, seed=2), "cpu")
    assert dec.workspace_bytes(2, 4, 6) == need(cfg(ch=(64, 64, 128), lpb=1), 2, 4, 6)
    with pytest.raises(ValueError, match="multiple of 8"):
        dec.workspace_bytes(1, 6, 6)


@pytest.mark.parametrize("cli", ["sample", "sample_fid", "sample_ema"])
def test_cli_missing_vae_weights_fails_before_any_model_is_built(cli, tmp_path):
    import importlib
    mod = importlib.import_module("mapdit_amd." + cli)
    args = mod.build_parser().parse_args(["--result-dir", "x"])
    assert args.vae_weights is None and args.vae_precision == "f16" and args.vae_norm_groups == 32
    with pytest.raises(FileNotFoundError, match="nowhere.safetensors"):       # before config.yaml of the (equally missing) run directory is read
        mod.main(["--result-dir", str(tmp_path / "no_such_run"), "--vae-weights", str(tmp_path / "nowhere.safetensors")])


def test_load_vae_without_weights_still_names_diffusers():
    from mapdit_amd import sampling as S
    try:
        import diffusers  # noqa: F401
        pytest.skip("diffusers is installed here")
    except ImportError:
        pass
    with pytest.raises(RuntimeError, match="diffusers"):
        S.load_vae(None, "cpu")


@pytest.mark.parametrize("dtype, bound", [(torch.float16, 5e-3), (torch.bfloat16, 5e-2)])
def test_operand_rounding_emulation_of_the_restatement(sd_tiny, dtype, bound):
    """Guards the yardstick: rounding every matmul operand to 16 bits moves the tiny config's output by a few 1e-4 (fp16) / 1e-3 (bf16)
    - not by nothing (the option would be dead) and not by more than five times what was measured when the tests were written."""
    z = 3 * torch.randn(2, 4, 4, 6, generator=torch.Generator().manual_seed(11))
    ref = R.decode(sd_tiny, z)
    assert ref.shape == (2, 3, 16, 24) and ref.dtype == torch.float64 and torch.isfinite(ref).all()
    e = rel_err(R.decode(sd_tiny, z, operand_dtype=dtype).numpy(), ref.numpy())
    print(f"e_emul {dtype}: {e:.3e}; output std {float(ref.std()):.3f}, max {float(ref.abs().max()):.3f}")
    assert 0 < e < bound
    # either generation of keys, with or without an explicit config, is the same function
    old = R.init_state_dict(R.TINY, seed=2, generation="old", conv_attention=True)
    assert torch.equal(R.decode(old, z, cfg=R.TINY), ref)
