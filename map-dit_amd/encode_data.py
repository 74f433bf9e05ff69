"""Make a latent data set: the reference's download_data.py on the native VAE encoder (map-dit_amd/vae.py -> mapdit_vae_encode).

    python -m mapdit_amd.encode_data --images imgs.npy --labels labels.npy --vae-weights vae.safetensors --output-dir DIR

Reads a uint8 [N, H, W, 3] image array (a ``.npy``, memory-mapped, or a torch file) and an integer [N] label array, encodes batch by
batch and writes what ``train.py --data-path`` and ``DeviceLatentDataset`` read: ``posterior_means.pt``, ``posterior_stds.pt`` (fp32
[N, L, h, w]), ``labels.pt`` (int64) and ``stats.pt`` ({"mean": [L], "std": [L]}, the mixture statistics of download_data.py:56-58,
summed in fp64 on the device).  ``--flip`` (the default, as the reference's RandomHorizontalFlip) bakes one random mirror per image:
the flags are a pure function of ``--seed`` and the image index, so ``--batch-size`` does not change a bit of the output.  JPEG
decoding and the hub's data-set format are out of scope (INTEGRATION.md shows the few lines that dump such a set to the two arrays).
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

OUTPUTS = ("posterior_means.pt", "posterior_stds.pt", "labels.pt", "stats.pt")


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--images", type=str, required=True, help="uint8 [N, H, W, 3]: a .npy (read memory-mapped) or a torch file")
    p.add_argument("--labels", type=str, required=True, help="integer [N]: a .npy or a torch file")
    p.add_argument("--vae-weights", type=str, required=True, help="AutoencoderKL weights (.safetensors or a torch file) holding encoder.* and quant_conv.*")
    p.add_argument("--output-dir", type=str, required=True)
    p.add_argument("--batch-size", type=int, default=128)
    p.add_argument("--vae-precision", type=str, default="f16", choices=["f16", "bf16"])
    p.add_argument("--vae-norm-groups", type=int, default=32)
    p.add_argument("--flip", action=argparse.BooleanOptionalAction, default=True, help="bake one seeded random left-right mirror per image")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--overwrite", action="store_true", help="replace existing output files")
    return p


def load_array(path):
    """A ``.npy`` memory-mapped (ImageNet at 128 px is 63 GB), anything else through torch.load; returned as a numpy array / memmap."""
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path}: no such file")
    if str(path).endswith(".npy"):
        return np.load(path, mmap_mode="r")
    t = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{path}: a torch file must hold one tensor, not {type(t).__name__}")
    return t.numpy()


def flip_flags(n: int, seed: int) -> torch.Tensor:
    """uint8 [n]: image i is mirrored iff the i-th draw of a generator seeded with ``seed`` is below one half."""
    return (torch.rand(n, generator=torch.Generator().manual_seed(int(seed))) < 0.5).to(torch.uint8)


def check_inputs(images, labels, args):
    """The refusals that need neither the weights nor a GPU."""
    if images.dtype != np.uint8:
        raise ValueError(f"--images {args.images}: dtype {images.dtype}, expected uint8 (pixels as PIL / numpy hold them; no scaling is guessed)")
    if images.ndim != 4:
        raise ValueError(f"--images {args.images}: shape {tuple(images.shape)}, expected [N, H, W, C]")
    if labels.ndim != 1 or labels.dtype.kind not in "iu":
        raise ValueError(f"--labels {args.labels}: shape {tuple(labels.shape)} of {labels.dtype}, expected an integer [N] array")
    if len(labels) != len(images):
        raise ValueError(f"--images holds {len(images)} images and --labels {len(labels)} labels: the lengths must agree")
    if len(images) < 1:
        raise ValueError(f"--images {args.images}: no images")
    if args.batch_size < 1:
        raise ValueError(f"--batch-size {args.batch_size} must be at least 1")
    for name in OUTPUTS:
        path = os.path.join(args.output_dir, name)
        if not args.overwrite and os.path.exists(path) and os.path.getsize(path) > 0:
            raise FileExistsError(f"{path} exists and is not empty: pass --overwrite to replace it")


def main(argv=None):
    args = build_parser().parse_args(argv)
    images, labels = load_array(args.images), load_array(args.labels)
    check_inputs(images, labels, args)
    if not os.path.exists(args.vae_weights):
        raise FileNotFoundError(f"--vae-weights {args.vae_weights}: no such file")
    if not torch.cuda.is_available():
        raise NotImplementedError("encode_data runs the HIP encoder: it needs the GPU, there is no CPU path")

    import ctypes as C

    from . import _lib as L
    from .vae import VAEEncoder
    dev = torch.device("cuda")
    enc = VAEEncoder.from_file(args.vae_weights, dev, precision=args.vae_precision, norm_num_groups=args.vae_norm_groups, max_batch=args.batch_size)
    n_img, H, W, Cimg = images.shape
    if Cimg != enc.cfg["out_channels"]:
        raise ValueError(f"--images {args.images}: {Cimg} channels, the encoder's conv_in takes {enc.cfg['out_channels']}")
    try:
        enc.workspace_bytes(min(n_img, args.batch_size), H, W)
    except ValueError as e:
        raise ValueError(f"--images {args.images}: images of {H} x {W}: {e}") from None
    lat, h, w = enc.cfg["latent_channels"], H // enc.scale, W // enc.scale
    flags = flip_flags(n_img, args.seed).to(dev) if args.flip else None
    means = torch.empty(n_img, lat, h, w, dtype=torch.float32)
    stds = torch.empty_like(means)
    acc = torch.zeros(lat, 3, dtype=torch.float64, device=dev)
    lib = L.lib()
    with torch.no_grad():
        for i in range(0, n_img, args.batch_size):
            j = min(i + args.batch_size, n_img)
            batch = torch.from_numpy(np.array(images[i:j])).to(dev)             # (a copy: the memory map is read-only)
            dist = enc.encode(batch, flip=None if flags is None else flags[i:j]).latent_dist
            lib.vae_stats_accumulate(dist.mean.data_ptr(), dist.std.data_ptr(), j - i, lat, h * w, acc.data_ptr(), L.cur_stream())
            means[i:j] = dist.mean.cpu()
            stds[i:j] = dist.std.cpu()
        ch_mean, ch_std = torch.empty(lat, device=dev), torch.empty(lat, device=dev)
        lib.vae_stats_finish(acc.data_ptr(), C.c_double(float(n_img) * h * w), ch_mean.data_ptr(), ch_std.data_ptr(), lat, L.cur_stream())
        stats = {"mean": ch_mean.cpu(), "std": ch_std.cpu()}
    os.makedirs(args.output_dir, exist_ok=True)
    torch.save(means, os.path.join(args.output_dir, "posterior_means.pt"))
    torch.save(stds, os.path.join(args.output_dir, "posterior_stds.pt"))
    torch.save(torch.from_numpy(np.asarray(labels).astype(np.int64)), os.path.join(args.output_dir, "labels.pt"))
    torch.save(stats, os.path.join(args.output_dir, "stats.pt"))
    print(f"encoded {n_img} images of {H} x {W} to {lat} x {h} x {w} latents in {args.output_dir}: "
          f"mean {[round(v, 4) for v in stats['mean'].tolist()]}, std {[round(v, 4) for v in stats['std'].tolist()]}")
    return args.output_dir


if __name__ == "__main__":
    main()
