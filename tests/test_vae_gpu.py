"""The native VAE decoder end to end on the GPU (map-dit_amd/vae.py -> mapdit_vae_decode) against the fp64 restatement
(tests/vae_reference.py), in both operand formats, and through the three sampler CLIs.

Tolerance: e_emul = rel_err(restatement with every matmul operand rounded to the format, fp64 restatement) is computed HERE, on the CPU;
the kernels must stay within 2 e_emul of the fp64 restatement.  The factor 2 covers what the emulation does not round the way the
kernels do (probabilities, the staged fp32 inputs, summation order); the tolerance never comes from the code under test."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_reference as R  # noqa: E402
from conftest import rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


def _decoder(sd, precision="f16", **kw):
    from mapdit_amd.vae import VAEDecoder
    return VAEDecoder.from_state_dict(sd, DEV, precision=precision, **kw)


@pytest.fixture(scope="module")
def tiny():
    sd = R.init_state_dict(R.TINY, seed=2)
    z = 3 * torch.randn(3, 4, 4, 6, generator=torch.Generator().manual_seed(11))
    return sd, z, R.decode(sd, z[:2])


@pytest.fixture(scope="module")
def full():
    sd = R.init_state_dict(R.DEFAULT, seed=1)
    z = 3 * torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(12))
    return sd, z, R.decode(sd, z)


def _check(sd, z, ref, precision):
    e_emul = rel_err(R.decode(sd, z, operand_dtype=DTYPES[precision]).numpy(), ref.numpy())
    dec = _decoder(sd, precision)
    out = dec.decode(z.to(DEV)).sample
    again = dec.decode(z.to(DEV)).sample
    assert out.shape == ref.shape and out.dtype == torch.float32 and out.is_cuda
    assert torch.isfinite(out).all()
    assert torch.equal(out, again)
    e = rel_err(out.cpu().numpy(), ref.numpy())
    print(f"vae decode {precision} {tuple(z.shape)}: rel err {e:.3e}, e_emul {e_emul:.3e}, ratio {e / e_emul:.2f}; "
          f"max abs err {float((out.cpu().double() - ref).abs().max()):.3e}")
    assert e <= 2 * e_emul


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_tiny_config_against_the_restatement(tiny, precision):
    sd, z, ref = tiny
    assert ref.shape == (2, 3, 16, 24)
    _check(sd, z[:2], ref, precision)


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_default_config_against_the_restatement(full, precision):
    sd, z, ref = full
    assert ref.shape == (1, 3, 64, 64)
    _check(sd, z, ref, precision)


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_chunked_batch_equals_single_sample_decodes(tiny, precision):
    sd, z, _ = tiny
    zd = z.to(DEV)
    chunked = _decoder(sd, precision, max_batch=2).decode(zd).sample                  # 2 + 1
    assert chunked.shape == (3, 3, 16, 24)
    one = _decoder(sd, precision, max_batch=1)
    for n in range(3):
        assert torch.equal(one.decode(zd[n:n + 1]).sample[0], chunked[n]), n


def test_refusals(tiny):
    sd, z, _ = tiny
    dec = _decoder(sd)
    with pytest.raises(ValueError, match="multiple of 8"):                             # 36 tokens in the attention
        dec.decode(torch.zeros(1, 4, 6, 6, device=DEV))
    with pytest.raises(NotImplementedError):
        dec.decode(z)                                                                  # a CPU tensor
    with pytest.raises(ValueError, match="expected"):
        dec.decode(torch.zeros(1, 3, 4, 6, device=DEV))


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_file_formats_and_key_generations_decode_to_identical_bits(tiny, tmp_path, precision):
    from mapdit_amd.vae import VAEDecoder
    _, z, _ = tiny
    zd = z[:2].to(DEV)
    want = None
    for gen in ("new", "old"):
        sd = R.init_state_dict(R.TINY, seed=2, generation=gen, conv_attention=(gen == "old"))
        pt, st = tmp_path / f"{gen}.pt", tmp_path / f"{gen}.safetensors"
        torch.save(sd if gen == "new" else {"state_dict": sd}, pt)
        R.write_safetensors(sd, st)
        for path in (pt, st):
            out = VAEDecoder.from_file(str(path), DEV, precision=precision).decode(zd).sample
            want = out if want is None else want
            assert torch.equal(out, want), (gen, path.name)
    assert torch.equal(want, _decoder(R.init_state_dict(R.TINY, seed=2), precision).decode(zd).sample)


# ---- the three CLIs -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    """A small run directory, made the way tests/test_samplers_gpu.py makes its own."""
    from mapdit_amd import train
    root = tmp_path_factory.mktemp("vae_results")
    return train.main(["--synthetic", "--results-dir", str(root), "--model", "DiT-XS/2", "--num-steps", "8", "--batch-size", "8",
                       "--log-every", "4", "--ckpt-every", "8", "--ema-snapshot-every", "2", "--num-classes", "10",
                       "--num-lin-warmup", "2", "--start-decay", "3", "--verbose", "0"])


@pytest.fixture(scope="module")
def weight_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("vae_weights") / "tiny_vae.safetensors"
    R.write_safetensors(R.init_state_dict(R.TINY, seed=2, generation="old"), path)
    return str(path)


def test_sample_fid_cli_writes_pixels(run_dir, weight_file):
    from mapdit_amd import sample_fid
    base = ["--result-dir", run_dir, "--num-classes", "10", "--num-sampling-steps", "2", "--batch-size", "4", "--num-samples", "6"]
    arr = np.load(sample_fid.main(base + ["--vae-weights", weight_file, "--output-file", "px.npz"]))["arr_0"]
    assert arr.shape == (6, 128, 128, 3) and arr.dtype == np.uint8 and arr.std() > 0            # 32 x 32 latents, two upsamplers
    arr_bf = np.load(sample_fid.main(base + ["--vae-weights", weight_file, "--vae-precision", "bf16", "--output-file", "px_bf.npz"]))["arr_0"]
    assert arr_bf.shape == arr.shape and arr_bf.dtype == np.uint8 and arr_bf.std() > 0
    # without the flag nothing changes: latents with --use-vae false, the diffusers message with --use-vae on
    lat = np.load(sample_fid.main(base + ["--use-vae", "false", "--output-file", "lat.npz"]))["arr_0"]
    assert lat.shape == (6, 32, 32, 4) and lat.dtype == np.uint8
    with pytest.raises(RuntimeError, match="diffusers"):
        sample_fid.main(base)


def test_sample_and_sample_ema_cli_write_pictures(run_dir, weight_file, tmp_path):
    from PIL import Image
    from mapdit_amd import sample, sample_ema
    out = str(tmp_path / "grid.png")
    s = sample.main(["--result-dir", run_dir, "--num-sampling-steps", "2", "--class-label", "3", "--output-file", out, "--seed", "1",
                     "--vae-weights", weight_file])
    assert s.shape == (4, 3, 128, 128) and float(s.abs().max()) <= 1.0 and float(s.std()) > 0
    img = Image.open(out)
    assert img.size == (2 * 130 + 2, 2 * 130 + 2) and img.mode == "RGB"                # 2 x 2 grid, 2-pixel padding
    assert not os.path.exists(out + ".npy")                                            # the latent dump belongs to --use-vae false
    out2 = str(tmp_path / "ema.png")
    e = sample_ema.main(["--result-dir", run_dir, "--num-sampling-steps", "2", "--class-label", "0", "--output-file", out2,
                         "--vae-weights", weight_file])
    assert e.shape == (8 * 5, 3, 128, 128)                                             # 40 images: decoded in chunks of max_batch
    assert Image.open(out2).size == (5 * 130 + 2, 8 * 130 + 2) and Image.open(out2).mode == "RGB"
    # the same command with --use-vae false writes what it wrote before
    out3 = str(tmp_path / "lat.png")
    l = sample.main(["--result-dir", run_dir, "--use-vae", "false", "--num-sampling-steps", "2", "--class-label", "3", "--output-file", out3,
                     "--seed", "1"])
    assert l.shape == (4, 4, 32, 32) and Image.open(out3).mode == "RGBA" and np.load(out3 + ".npy").shape == (4, 4, 32, 32)
