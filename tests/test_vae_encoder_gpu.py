"""The native VAE encoder end to end on the GPU (map-dit_amd/vae.py -> mapdit_vae_encode) against the fp64 restatement
(tests/vae_encoder_reference.py), in both operand formats, and the data-set script (map-dit_amd/encode_data.py).

Tolerance, the decoder's rule: e_emul = rel_err(restatement with every matmul operand rounded to the format, fp64 restatement) is computed
HERE, on the CPU, separately for the mean and the log-variance; the kernels must stay within 2 e_emul of the fp64 restatement (the
factor of tests/test_vae_gpu.py, for the same reasons).  std is compared as 2 log(std) against the reference log-variance, so the
exponential does not flatten the comparison - and the reference log-variance must lie in (-10, 10) everywhere, so that the clamp to
[-30, 20] cannot hide an error: asserted before the device is asked; the fixture seeds were chosen on the CPU so that it holds
(reference log-variance in [-1.15, 2.51] for the tiny fixture, [-1.48, 1.26] for the default one).

Measured on an MI355X when the tests were written, rel err vs fp64 / e_emul (profiles/vae_encoder_tests_gpu.log):
    tiny     f16  mean 1.16e-3 / 1.13e-3, logvar 8.08e-4 / 8.26e-4      bf16  mean 9.16e-3 / 9.01e-3, logvar 6.89e-3 / 6.91e-3
    default  f16  mean 9.71e-4 / 1.00e-3, logvar 1.16e-3 / 1.09e-3      bf16  mean 8.34e-3 / 9.25e-3, logvar 7.42e-3 / 8.89e-3
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_encoder_reference as E  # noqa: E402
import vae_reference as R  # noqa: E402
from conftest import rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


def _encoder(sd, precision="f16", **kw):
    from mapdit_amd.vae import VAEEncoder
    return VAEEncoder.from_state_dict(sd, DEV, precision=precision, **kw)


def _images(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


@pytest.fixture(scope="module")
def tiny():
    sd = E.init_encoder_state_dict(R.TINY, seed=2)
    x = _images((3, 3, 16, 24), 21)
    return sd, x, E.encode(sd, x)


@pytest.fixture(scope="module")
def full():
    sd = E.init_encoder_state_dict(R.DEFAULT, seed=1)
    x = _images((1, 3, 32, 32), 22)
    return sd, x, E.encode(sd, x)


def _check(sd, x, ref, precision, latent_shape):
    ref_mean, ref_lv = ref
    assert ref_mean.shape == ref_lv.shape == latent_shape
    assert float(ref_lv.min()) > -10.0 and float(ref_lv.max()) < 10.0, (float(ref_lv.min()), float(ref_lv.max()))   # the clamp is far away
    em_mean, em_lv = E.encode(sd, x, operand_dtype=DTYPES[precision])
    e_mean, e_lv = rel_err(em_mean.numpy(), ref_mean.numpy()), rel_err(em_lv.numpy(), ref_lv.numpy())
    enc = _encoder(sd, precision)
    dist = enc.encode(x.to(DEV)).latent_dist
    again = enc.encode(x.to(DEV)).latent_dist
    for t in (dist.mean, dist.std, dist.logvar):
        assert t.shape == latent_shape and t.dtype == torch.float32 and t.is_cuda and torch.isfinite(t).all()
    assert torch.equal(dist.mean, again.mean) and torch.equal(dist.std, again.std)
    assert dist.mode() is dist.mean and bool((dist.std > 0).all())
    g_mean = rel_err(dist.mean.cpu().numpy(), ref_mean.numpy())
    g_lv = rel_err((torch.log(dist.std.cpu().double()) * 2).numpy(), ref_lv.numpy())
    print(f"vae encode {precision} {tuple(x.shape)}: mean rel err {g_mean:.3e} (e_emul {e_mean:.3e}, ratio {g_mean / e_mean:.2f}); "
          f"logvar rel err {g_lv:.3e} (e_emul {e_lv:.3e}, ratio {g_lv / e_lv:.2f}); reference logvar in [{float(ref_lv.min()):.2f}, {float(ref_lv.max()):.2f}]")
    assert g_mean <= 2 * e_mean
    assert g_lv <= 2 * e_lv
    assert rel_err(dist.logvar.cpu().numpy(), ref_lv.numpy()) <= 2 * e_lv              # the property: 2 log(std) in fp32
    return dist


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_tiny_config_against_the_restatement(tiny, precision):
    sd, x, ref = tiny
    dist = _check(sd, x, ref, precision, (3, 4, 4, 6))                                  # 24 attention tokens
    g = torch.Generator(device=DEV).manual_seed(3)
    s = dist.sample(generator=g)
    want = dist.mean + dist.std * torch.randn(dist.mean.shape, generator=torch.Generator(device=DEV).manual_seed(3), device=DEV)
    assert torch.equal(s, want) and not torch.equal(dist.sample(), s)


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_default_config_against_the_restatement(full, precision):
    sd, x, ref = full
    _check(sd, x, ref, precision, (1, 4, 4, 4))                                         # 16 attention tokens


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_chunked_batch_equals_single_sample_encodes(tiny, precision):
    sd, x, _ = tiny
    xd = x.to(DEV)
    chunked = _encoder(sd, precision, max_batch=2).encode(xd).latent_dist              # 2 + 1
    one = _encoder(sd, precision, max_batch=1)
    for n in range(3):
        alone = one.encode(xd[n:n + 1]).latent_dist
        assert torch.equal(alone.mean[0], chunked.mean[n]) and torch.equal(alone.std[0], chunked.std[n]), n


def _u8_images(n, h, w, seed):
    return torch.randint(0, 256, (n, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _torch_prepared(u8, flags):
    """ToTensor + Normalize(0.5, 0.5) (+ the flips) in torch on the CPU: fp32 NCHW."""
    x = ((u8.float().div(255) - 0.5) / 0.5).permute(0, 3, 1, 2).contiguous()
    for n in range(len(u8)):
        if flags is not None and int(flags[n]):
            x[n] = torch.flip(x[n], dims=[2])
    return x


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_uint8_input_equals_the_torch_prepared_tensor(tiny, precision):
    sd = tiny[0]
    u8 = _u8_images(3, 16, 24, 31)
    flags = torch.tensor([0, 1, 0], dtype=torch.uint8)
    enc = _encoder(sd, precision, max_batch=2)
    got = enc.encode(u8.to(DEV), flip=flags.to(DEV)).latent_dist
    want = enc.encode(_torch_prepared(u8, flags).to(DEV)).latent_dist
    assert torch.equal(got.mean, want.mean) and torch.equal(got.std, want.std)
    plain = enc.encode(u8.to(DEV)).latent_dist
    unflipped = enc.encode(_torch_prepared(u8, None).to(DEV)).latent_dist
    assert torch.equal(plain.mean, unflipped.mean) and torch.equal(plain.mean[0], got.mean[0]) and not torch.equal(plain.mean[1], got.mean[1])


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_file_formats_and_key_generations_encode_to_identical_bits(tiny, tmp_path, precision):
    from mapdit_amd.vae import VAEDecoder, VAEEncoder
    _, x, _ = tiny
    xd = x[:2].to(DEV)
    want = None
    for gen in ("new", "old"):
        sd = E.init_encoder_state_dict(R.TINY, seed=2, generation=gen, conv_attention=(gen == "old"))
        pt, st = tmp_path / f"{gen}.pt", tmp_path / f"{gen}.safetensors"
        torch.save(sd if gen == "new" else {"state_dict": sd}, pt)
        R.write_safetensors(sd, st)
        for path in (pt, st):
            out = VAEEncoder.from_file(str(path), DEV, precision=precision).encode(xd).latent_dist
            want = out if want is None else want
            assert torch.equal(out.mean, want.mean) and torch.equal(out.std, want.std), (gen, path.name)
    assert torch.equal(want.mean, _encoder(tiny[0], precision).encode(xd).latent_dist.mean)
    # one file with both halves loads into both classes; the decoder still decodes (the shared helpers did not break it)
    both = tmp_path / "both.safetensors"
    R.write_safetensors(dict(E.init_encoder_state_dict(R.TINY, seed=2), **R.init_state_dict(R.TINY, seed=2)), both)
    enc, dec = VAEEncoder.from_file(str(both), DEV, precision=precision), VAEDecoder.from_file(str(both), DEV, precision=precision)
    dist = enc.encode(xd).latent_dist
    assert torch.equal(dist.mean, want.mean)
    img = dec.decode(dist.mode()).sample
    assert img.shape == (2, 3, 16, 24) and torch.isfinite(img).all()
    assert torch.equal(img, VAEDecoder.from_state_dict(R.init_state_dict(R.TINY, seed=2), DEV, precision=precision).decode(dist.mean).sample)


def test_refusals(tiny):
    sd, x, _ = tiny
    enc = _encoder(sd)
    with pytest.raises(ValueError, match="18 x 24 is not a multiple of 4"):
        enc.encode(torch.zeros(1, 3, 18, 24, device=DEV))
    with pytest.raises(ValueError, match="9 tokens.*multiple of 8"):
        enc.encode(torch.zeros(1, 3, 12, 12, device=DEV))
    with pytest.raises(NotImplementedError):
        enc.encode(x)                                                                  # a CPU tensor
    with pytest.raises(ValueError, match="expected"):
        enc.encode(torch.zeros(1, 4, 16, 24, device=DEV))                              # a wrong channel count
    with pytest.raises(ValueError, match="expected"):
        enc.encode(torch.zeros(1, 16, 24, 4, device=DEV, dtype=torch.uint8))
    with pytest.raises(ValueError, match="flip"):
        enc.encode(torch.zeros(2, 16, 24, 3, device=DEV, dtype=torch.uint8), flip=torch.zeros(3, dtype=torch.uint8))


# ---- encode_data end to end ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dataset_inputs(tmp_path_factory):
    root = tmp_path_factory.mktemp("encode_data")
    u8 = _u8_images(10, 16, 24, 41)
    labels = torch.randint(0, 10, (10,), generator=torch.Generator().manual_seed(42))
    np.save(root / "imgs.npy", u8.numpy())
    np.save(root / "labels.npy", labels.numpy())
    R.write_safetensors(E.init_encoder_state_dict(R.TINY, seed=2, generation="old"), root / "vae.safetensors")
    return root, u8, labels


def _run_script(root, out, *extra):
    from mapdit_amd import encode_data
    return encode_data.main(["--images", str(root / "imgs.npy"), "--labels", str(root / "labels.npy"), "--vae-weights", str(root / "vae.safetensors"),
                             "--output-dir", str(root / out), *extra])


def test_encode_data_end_to_end(dataset_inputs):
    from mapdit_amd import encode_data
    from mapdit_amd.data import DeviceLatentDataset
    root, u8, labels = dataset_inputs
    out = _run_script(root, "out4", "--batch-size", "4", "--seed", "5")
    ld = lambda d, n: torch.load(os.path.join(d, n), weights_only=True)  # noqa: E731
    means, stds, lab, stats = (ld(out, n) for n in encode_data.OUTPUTS)
    assert means.shape == stds.shape == (10, 4, 4, 6) and means.dtype == stds.dtype == torch.float32
    assert lab.dtype == torch.int64 and torch.equal(lab, labels)
    assert stats["mean"].shape == stats["std"].shape == (4,) and stats["mean"].dtype == stats["std"].dtype == torch.float32
    # bit-equal to the class on the same images and flips
    flags = encode_data.flip_flags(10, 5)
    assert 0 < int(flags.sum()) < 10
    dist = _encoder(E.init_encoder_state_dict(R.TINY, seed=2)).encode(u8.to(DEV), flip=flags.to(DEV)).latent_dist
    assert torch.equal(means, dist.mean.cpu()) and torch.equal(stds, dist.std.cpu())
    # stats.pt: download_data.py:56-58 applied to the saved tensors; 1e-6 relative is fp32 storage of an fp64 result
    m64, s64 = means.double(), stds.double()
    mean = m64.mean(dim=[0, 2, 3])
    std = (s64.square().mean(dim=[0, 2, 3]) + (m64 - mean[None, :, None, None]).square().mean(dim=[0, 2, 3])).sqrt()
    e_m, e_s = float(((stats["mean"].double() - mean) / mean).abs().max()), float(((stats["std"].double() - std) / std).abs().max())
    print(f"stats.pt vs the CPU formula: mean rel err {e_m:.3e}, std rel err {e_s:.3e} (bound 1e-6)")
    assert e_m <= 1e-6 and e_s <= 1e-6
    # the training side reads the directory
    ds = DeviceLatentDataset(out, DEV)
    assert len(ds) == 10 and ds.channels == 4
    batch = ds.batch(0, 4)
    assert batch[0].shape == (4, 4, 4, 6) and torch.isfinite(batch[0]).all() and batch[1].shape == (4,)
    # another batch size writes identical files
    out3 = _run_script(root, "out3", "--batch-size", "3", "--seed", "5")
    for n in encode_data.OUTPUTS[:3]:
        assert torch.equal(ld(out3, n), ld(out, n)), n
    s3 = ld(out3, "stats.pt")                      # (the fp64 sums are added sample by sample: the batch split does not enter)
    assert torch.equal(s3["mean"], stats["mean"]) and torch.equal(s3["std"], stats["std"])
    # no flips: the plain encode
    outn = _run_script(root, "outn", "--batch-size", "16", "--no-flip")
    assert torch.equal(ld(outn, "posterior_means.pt"), _encoder(E.init_encoder_state_dict(R.TINY, seed=2)).encode(u8.to(DEV)).latent_dist.mean.cpu())


def test_encode_data_refusals(dataset_inputs):
    root, u8, labels = dataset_inputs
    _run_script(root, "outr", "--batch-size", "8")
    with pytest.raises(FileExistsError, match="--overwrite"):
        _run_script(root, "outr", "--batch-size", "8")
    _run_script(root, "outr", "--batch-size", "8", "--overwrite")
    from mapdit_amd import encode_data
    np.save(root / "odd.npy", np.zeros((2, 18, 24, 3), np.uint8))
    np.save(root / "two.npy", np.zeros(2, np.int64))
    base = ["--labels", str(root / "two.npy"), "--vae-weights", str(root / "vae.safetensors"), "--output-dir", str(root / "never")]
    with pytest.raises(ValueError, match="18 x 24.*multiple of 4"):
        encode_data.main(["--images", str(root / "odd.npy"), *base])
    np.save(root / "small.npy", np.zeros((2, 12, 12, 3), np.uint8))
    with pytest.raises(ValueError, match="multiple of 8"):
        encode_data.main(["--images", str(root / "small.npy"), *base])
    with pytest.raises(ValueError, match="lengths must agree"):
        encode_data.main(["--images", str(root / "imgs.npy"), *base])
    np.save(root / "f32.npy", np.zeros((2, 16, 24, 3), np.float32))
    with pytest.raises(ValueError, match="expected uint8"):
        encode_data.main(["--images", str(root / "f32.npy"), *base])
    assert not os.path.exists(root / "never")
