"""Native FD-DINOv2 on ``libmapdit_hip.so``: the CLS feature after the final LayerNorm of a DINOv2 ViT (``mapdit_vit_features``,
include/mapdit.h; ViT-L/14: 1024 numbers per image), its fp64 sums on the device (``fid.FeatureStats``) and the Fréchet distance of
the two Gaussian fits on the host (``fid.frechet_distance``) - the metric of Stein et al. 2023 (``dgm-eval``) and of EDM2's tables.

    python -m mapdit_amd.dinov2 stats --images A.npz --dinov2-weights FILE --output ref.npz
    python -m mapdit_amd.dinov2 features --images A.npz --dinov2-weights FILE --output feats.npz
    python -m mapdit_amd.dinov2 compare a.npz b.npz [--dinov2-weights FILE]

Every image is resized to 224 x 224 with torch's antialiased bicubic map on pixel values in 0 .. 255, then normalised with the ImageNet
mean and std: EDM2's ``DINOv2Detector(resize_mode="torch")``.  Files: ``mu_dinov2`` / ``sigma_dinov2`` (and ``dinov2_features`` fp32
[N, D] in a features file); the keys do not collide with FID's ``mu`` / ``sigma`` / ``pool_3``, so one ``.npz`` may carry both sets.
EDM2's pickled reference files are not read (unpickling runs code); INTEGRATION.md shows the conversion to ``.npz``.

Parity with the hub weights and with EDM2's ``calculate_metrics.py`` is unpinned: neither the weight file nor the ``dinov2`` code is
at hand where this was written; the network is restated from its public description and checked against an independent fp64
restatement on random weights (tests/dinov2_reference.py), the resize against the installed torch.  The first number quoted needs one
cross-check; it would catch the position-table interpolation offset (``interpolate_offset``), torch's antialias map and the
CLS-after-final-norm output.
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib as L
from . import fid as FID
from .vae import PRECISIONS, load_state_dict_file

PATCH = 14
HEAD_DIM = 64
LN_EPS = 1e-6
IMAGE_SIZE = 224
STATS_KEYS = ("mu_dinov2", "sigma_dinov2")
FEATURES_KEY = "dinov2_features"
_PREFIXES = ("module.", "backbone.")                     # wrappers a checkpoint may carry; stripped
_IGNORED = ("mask_token",)

_BLOCK_LEAVES = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "ls1.gamma",
                 "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias", "ls2.gamma")


def vit_shapes(dim, depth, mlp_dim, grid) -> dict:
    """Key -> shape of the state dict of a DINOv2 ViT (patch 14, LayerScale, no registers, a GELU MLP)."""
    s = {"cls_token": (1, 1, dim), "pos_embed": (1, 1 + grid * grid, dim), "patch_embed.proj.weight": (dim, 3, PATCH, PATCH),
         "patch_embed.proj.bias": (dim,), "norm.weight": (dim,), "norm.bias": (dim,)}
    leaf = {"norm1.weight": (dim,), "norm1.bias": (dim,), "attn.qkv.weight": (3 * dim, dim), "attn.qkv.bias": (3 * dim,),
            "attn.proj.weight": (dim, dim), "attn.proj.bias": (dim,), "ls1.gamma": (dim,), "norm2.weight": (dim,), "norm2.bias": (dim,),
            "mlp.fc1.weight": (mlp_dim, dim), "mlp.fc1.bias": (mlp_dim,), "mlp.fc2.weight": (dim, mlp_dim), "mlp.fc2.bias": (dim,),
            "ls2.gamma": (dim,)}
    for i in range(depth):
        for k in _BLOCK_LEAVES:
            s[f"blocks.{i}.{k}"] = leaf[k]
    return s


def check_state_dict(sd) -> tuple:
    """The checked state dict and (dim, depth, mlp_dim, grid) read off its shapes.  A missing, unexpected or doubled key is a KeyError
    naming it, ``register_tokens`` and ``mlp.w12`` NotImplementedErrors naming the variant, a wrong shape a ValueError."""
    out = {}
    for k, v in sd.items():
        name = k
        for p in _PREFIXES:
            if name.startswith(p):
                name = name[len(p):]
        if name in out:
            raise KeyError(f"DINOv2 state dict: {name!r} is given twice (with and without a {'/'.join(_PREFIXES)} prefix)")
        out[name] = v
    for k in out:
        if k == "register_tokens" or k.endswith(".register_tokens"):
            raise NotImplementedError(f"DINOv2 state dict: {k!r}: the register variants (dinov2_*_reg) are not built; FD-DINOv2 uses dinov2_vitl14")
        if ".mlp.w12." in k or ".mlp.w3." in k:
            raise NotImplementedError(f"DINOv2 state dict: {k!r}: the SwiGLU MLP (mlp.w12, ViT-g/14) is not built; FD-DINOv2 uses dinov2_vitl14")
    out = {k: v for k, v in out.items() if k not in _IGNORED}
    for k in ("cls_token", "pos_embed", "blocks.0.mlp.fc1.weight"):
        if k not in out:
            raise KeyError(f"DINOv2 state dict: missing key {k!r}")
    if out["cls_token"].dim() != 3 or out["pos_embed"].dim() != 3 or out["blocks.0.mlp.fc1.weight"].dim() != 2:
        raise ValueError(f"DINOv2 state dict: 'cls_token' of shape {tuple(out['cls_token'].shape)}, 'pos_embed' of shape {tuple(out['pos_embed'].shape)} "
                         f"and 'blocks.0.mlp.fc1.weight' of shape {tuple(out['blocks.0.mlp.fc1.weight'].shape)} are no [1, 1, D], [1, 1 + g * g, D], [F, D]")
    dim, mlp_dim = int(out["cls_token"].shape[2]), int(out["blocks.0.mlp.fc1.weight"].shape[0])
    grid = math.isqrt(max(int(out["pos_embed"].shape[1]) - 1, 0))
    depth = 1 + max(int(k.split(".")[1]) for k in out if k.startswith("blocks.") and k.split(".")[1].isdigit())
    if dim < HEAD_DIM or dim % HEAD_DIM:
        raise ValueError(f"DINOv2 state dict: dim {dim} is no multiple of the head dimension {HEAD_DIM}")
    shapes = vit_shapes(dim, depth, mlp_dim, grid)
    missing, extra = sorted(set(shapes) - set(out)), sorted(set(out) - set(shapes))
    if missing:
        raise KeyError(f"DINOv2 state dict: missing key {missing[0]!r}" + (f" (and {len(missing) - 1} more)" if len(missing) > 1 else ""))
    if extra:
        raise KeyError(f"DINOv2 state dict: unexpected key {extra[0]!r}" + (f" (and {len(extra) - 1} more)" if len(extra) > 1 else ""))
    for k, v in out.items():
        if tuple(v.shape) != tuple(shapes[k]):
            raise ValueError(f"DINOv2 state dict: {k!r} has shape {tuple(v.shape)}, expected {tuple(shapes[k])}")
    return out, (dim, depth, mlp_dim, grid)


def feature_dim(sd) -> int:
    """``dim`` of a raw state dict (the length of a feature row), read off ``cls_token`` alone."""
    for p in ("",) + _PREFIXES:
        if p + "cls_token" in sd:
            return int(sd[p + "cls_token"].shape[-1])
    raise KeyError("DINOv2 state dict: missing key 'cls_token'")


def interpolate_pos_embed(pos_embed, g, interpolate_offset=0.1):
    """[1, 1 + M * M, D] -> fp32 [1 + g * g, D]: the class row as it is, the M x M grid by F.interpolate(mode="bicubic") with
    scale_factor = (g + interpolate_offset) / M per axis and no antialiasing, as the hub models do it (the offset moves the sampling
    grid, not the size; the size is asserted); g == M: the table as it is.  Done once at load time, on the host."""
    pos = pos_embed.detach().to(torch.float32)
    D = pos.shape[2]
    M = math.isqrt(pos.shape[1] - 1)
    if M * M != pos.shape[1] - 1:
        raise ValueError(f"DINOv2 pos_embed: {pos.shape[1] - 1} patch rows are no square grid")
    if g == M:
        return pos[0].contiguous()
    s = float(g + interpolate_offset) / M
    grid = F.interpolate(pos[0, 1:].reshape(1, M, M, D).permute(0, 3, 1, 2), scale_factor=(s, s), mode="bicubic")
    if tuple(grid.shape[-2:]) != (g, g):
        raise AssertionError(f"DINOv2 pos_embed: scale_factor {s} gives a grid of {tuple(grid.shape[-2:])}, expected ({g}, {g})")
    return torch.cat([pos[0, :1], grid.permute(0, 2, 3, 1).reshape(g * g, D)], dim=0).contiguous()


def pack_patch_weight(w, dtype):
    """[D, 3, 14, 14] -> 16-bit [D, MAPDIT_VIT_PATCH_K]: the (c, py, px) flattening, the tail zero."""
    D = w.shape[0]
    out = torch.zeros(D, L.VIT_PATCH_K, dtype=torch.float32)
    out[:, :3 * PATCH * PATCH] = w.detach().to(torch.float32).reshape(D, -1)
    return out.to(dtype)


class DinoV2Features:
    """``DinoV2Features.from_file(path, device).features(x)``: x uint8 [N, H, W, 3] as ``sample_fid.py`` stores images, or fp32
    [N, 3, H, W] in [-1, 1], on the device, any H, W >= 8 -> fp32 [N, D] on the device (D = 1024 for ViT-L/14, the metric's network;
    ViT-S and ViT-B files load too).  ``precision``: the 16-bit format of the weights and of the activations between the kernels
    ("f16" default, "bf16"); accumulation and the residual stream are fp32.  Batches above ``max_batch`` are chunked; an image alone
    gives the same bits as in a batch."""

    def __init__(self, sd, device, precision="f16", max_batch=32, image_size=IMAGE_SIZE, interpolate_offset=0.1):
        if precision not in PRECISIONS:
            raise ValueError(f"DINOv2 precision {precision!r}: one of {sorted(PRECISIONS)}")
        if max_batch < 1:
            raise ValueError(f"max_batch={max_batch} must be at least 1")
        if image_size < PATCH or image_size % PATCH:
            raise ValueError(f"DINOv2 image_size={image_size} is no multiple of the patch ({PATCH})")
        sd, (dim, depth, mlp_dim, _) = check_state_dict(sd)
        self.device, self.precision, self.max_batch = torch.device(device), precision, int(max_batch)
        if self.device.type != "cuda":
            raise NotImplementedError("DinoV2Features runs on the GPU only (HIP kernels, no CPU path): pass a CUDA device")
        self.dim, self.depth, self.mlp_dim, self.heads, self.image_size = dim, depth, mlp_dim, dim // HEAD_DIM, int(image_size)
        dt = PRECISIONS[precision]
        dev = self.device

        def f32(t):
            return t.detach().to(torch.float32).contiguous().to(dev)

        def w16(t):
            return t.detach().to(torch.float32).to(dt).contiguous().to(dev)

        slots = [None] * L.VIT_W_GLOBAL
        slots[L.VIT_W_PATCH] = pack_patch_weight(sd["patch_embed.proj.weight"], dt).to(dev)
        slots[L.VIT_W_PATCH_BIAS] = f32(sd["patch_embed.proj.bias"])
        slots[L.VIT_W_CLS] = f32(sd["cls_token"].reshape(dim))
        slots[L.VIT_W_POS] = interpolate_pos_embed(sd["pos_embed"], self.image_size // PATCH, interpolate_offset).to(dev)
        slots[L.VIT_W_NORM] = f32(sd["norm.weight"])
        slots[L.VIT_W_NORM_BIAS] = f32(sd["norm.bias"])
        order = {L.VIT_B_LN1: "norm1.weight", L.VIT_B_LN1_BIAS: "norm1.bias", L.VIT_B_QKV: "attn.qkv.weight", L.VIT_B_QKV_BIAS: "attn.qkv.bias",
                 L.VIT_B_PROJ: "attn.proj.weight", L.VIT_B_PROJ_BIAS: "attn.proj.bias", L.VIT_B_LS1: "ls1.gamma", L.VIT_B_LN2: "norm2.weight",
                 L.VIT_B_LN2_BIAS: "norm2.bias", L.VIT_B_FC1: "mlp.fc1.weight", L.VIT_B_FC1_BIAS: "mlp.fc1.bias", L.VIT_B_FC2: "mlp.fc2.weight",
                 L.VIT_B_FC2_BIAS: "mlp.fc2.bias", L.VIT_B_LS2: "ls2.gamma"}
        assert sorted(order) == list(range(L.VIT_W_BLOCK))
        for i in range(depth):
            for slot in range(L.VIT_W_BLOCK):
                t = sd[f"blocks.{i}.{order[slot]}"]
                slots.append(w16(t) if t.dim() == 2 else f32(t))
        self.packed = slots
        self._cfg = L.VitConfig(image_size=self.image_size, patch=PATCH, dim=dim, depth=depth, heads=self.heads, mlp_dim=mlp_dim, ln_eps=LN_EPS)
        self.workspace_bytes(1)                                # a configuration the library refuses ends here, with its message
        self._table = None
        self._ws = None

    @classmethod
    def from_state_dict(cls, sd, device, precision="f16", max_batch=32, image_size=IMAGE_SIZE, interpolate_offset=0.1):
        return cls(sd, device, precision, max_batch, image_size, interpolate_offset)

    @classmethod
    def from_file(cls, path, device, precision="f16", max_batch=32, image_size=IMAGE_SIZE, interpolate_offset=0.1):
        if torch.device(device).type != "cuda":                # (before a gigabyte of weights is read)
            raise NotImplementedError("DinoV2Features runs on the GPU only (HIP kernels, no CPU path): pass a CUDA device")
        return cls(load_state_dict_file(path), device, precision, max_batch, image_size, interpolate_offset)

    def workspace_bytes(self, n) -> int:
        lib = L.lib()
        need = lib.vit_workspace_bytes(C.byref(self._cfg), int(n))
        if need == 0:
            raise ValueError(f"DINOv2 features refused: {lib.last_error().decode()}")
        return need

    def _run(self, x, what, out16=False):
        """The walk over chunks of max_batch images: ``what`` = "features" (CLS rows, fp32 [N, D]) or "tokens" ([N, T, D])."""
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise NotImplementedError(f"DinoV2Features.{what} runs on the GPU only (HIP kernels, no CPU path): pass a CUDA tensor")
        u8 = x.dtype == torch.uint8
        if x.dim() != 4 or x.shape[3 if u8 else 1] != 3:
            raise ValueError(f"DINOv2 {what}: x has shape {tuple(x.shape)} ({x.dtype}), expected uint8 [N, H, W, 3] or float [N, 3, H, W]")
        x = x.detach().to(self.device).contiguous() if u8 else x.detach().to(self.device, torch.float32).contiguous()
        N, H, W = (x.shape[0], x.shape[1], x.shape[2]) if u8 else (x.shape[0], x.shape[2], x.shape[3])
        if H < 8 or W < 8:
            raise ValueError(f"DINOv2 {what}: images of {H} x {W} (8 x 8 at the least)")
        if what == "tokens":
            T = 1 + (self.image_size // PATCH) ** 2
            out = torch.empty(N, T, self.dim, dtype=PRECISIONS[self.precision] if out16 else torch.float32, device=self.device)
        else:
            out = torch.empty(N, self.dim, dtype=torch.float32, device=self.device)
        if N == 0:
            return out
        chunk = min(N, self.max_batch)
        need = self.workspace_bytes(chunk)
        lib = L.lib()
        if self._table is None:
            self._table = (C.c_void_p * len(self.packed))(*[t.data_ptr() for t in self.packed])
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        fn = getattr(lib, "vit_" + what + ("_f16" if self.precision == "f16" else ""))
        extra = (L.VIT_OUT_16 if out16 else L.VIT_OUT_F32,) if what == "tokens" else ()
        kind = L.VIT_IMG_U8_NHWC if u8 else L.VIT_IMG_F32_NCHW
        with torch.cuda.device(self.device):
            stream = L.cur_stream()
            for i in range(0, N, chunk):
                n = min(chunk, N - i)
                fn(C.byref(self._cfg), self._table, x[i:i + n].data_ptr(), kind, n, H, W, out[i:i + n].data_ptr(), *extra, self._ws.data_ptr(),
                   self._ws.numel(), stream)
        return out

    @torch.no_grad()
    def features(self, x):
        return self._run(x, "features")

    @torch.no_grad()
    def tokens(self, x, out16=False):
        """Every token after the final LayerNorm (``mapdit_vit_tokens``): [N, 1 + g * g, D], g = image_size / 14; row 0 the CLS token (fp32:
        the bits of ``features``), rows 1 + p the patches in row-major grid order.  ``out16``: in the network's 16-bit format."""
        return self._run(x, "tokens", out16)


# ---- files --------------------------------------------------------------------------------------------------------------------------
def _kept(path, drop) -> dict:
    """The arrays an existing ``.npz`` at ``path`` holds under other keys (FID's ``mu`` / ``sigma`` / ``pool_3``): they stay."""
    if not os.path.isfile(path):
        return {}
    try:
        with np.load(path) as z:
            return {k: z[k] for k in z.files if k not in drop}
    except (OSError, ValueError):
        return {}


def save_stats(path, mu, sigma, keep=False):
    """``mu_dinov2``, ``sigma_dinov2`` as fp64; ``keep=True``: beside whatever other arrays the file holds already."""
    old = _kept(path, STATS_KEYS + (FEATURES_KEY,)) if keep else {}
    with open(path, "wb") as f:
        np.savez(f, mu_dinov2=np.asarray(mu, np.float64), sigma_dinov2=np.asarray(sigma, np.float64), **old)


def save_features(path, feat, mu, sigma, keep=False):
    old = _kept(path, STATS_KEYS + (FEATURES_KEY,)) if keep else {}
    with open(path, "wb") as f:
        np.savez(f, **{FEATURES_KEY: np.asarray(feat, np.float32)}, mu_dinov2=np.asarray(mu, np.float64), sigma_dinov2=np.asarray(sigma, np.float64),
                 **old)


def load_stats(path):
    """``mu_dinov2`` [D] and ``sigma_dinov2`` [D, D] of an ``.npz``; other keys (FID's) are ignored."""
    with np.load(path) as z:
        for k in STATS_KEYS:
            if k not in z.files:
                raise KeyError(f"{path}: no {k!r} in the file (it holds {sorted(z.files)}); write the statistics with "
                               "`python -m mapdit_amd.dinov2 stats --images A.npz --dinov2-weights FILE --output ref.npz`")
        mu, sigma = (np.asarray(z[k], np.float64) for k in STATS_KEYS)
    if mu.ndim != 1 or sigma.shape != (mu.shape[0], mu.shape[0]):
        raise ValueError(f"{path}: mu_dinov2 of shape {mu.shape} and sigma_dinov2 of shape {sigma.shape} are no [D] and [D, D]")
    return mu, sigma


def load_features(path):
    """fp32 [N, D] ``dinov2_features`` of a file written by the ``features`` subcommand (what ``metrics.precision_recall`` and
    ``metrics.kid`` take, once on the device)."""
    with np.load(path) as z:
        if FEATURES_KEY not in z.files:
            raise KeyError(f"{path}: no {FEATURES_KEY!r} in the file (it holds {sorted(z.files)}): write one with "
                           "`python -m mapdit_amd.dinov2 features --images A.npz --dinov2-weights FILE --output feats.npz`")
        feat = np.ascontiguousarray(z[FEATURES_KEY], np.float32)
    if feat.ndim != 2:
        raise ValueError(f"{path}: {FEATURES_KEY} of shape {feat.shape} is no [N, D]")
    return feat


def _is_stats(path) -> bool:
    if not str(path).endswith(".npz"):
        return False
    with np.load(path) as z:
        return all(k in z.files for k in STATS_KEYS)


class FeaturePass:
    """One pass of the network over batches of uint8 images: the FeatureStats of the CLS features and, with ``keep``, the rows."""

    def __init__(self, net, device="cuda", keep=False):
        self.net, self.device = net, device
        self.stats = FID.FeatureStats(net.dim, device)
        self.feats = [] if keep else None

    def update(self, images):
        feat = self.net.features(torch.from_numpy(np.ascontiguousarray(images)).to(self.device))
        self.stats.update(feat)
        if self.feats is not None:
            self.feats.append(feat)
        return self

    def over(self, images, batch_size):
        for i in range(0, len(images), batch_size):
            self.update(images[i:i + batch_size])
        return self


def stats_of_images(images, net, batch_size=64, device="cuda"):
    return FeaturePass(net, device).over(images, batch_size).stats


def features_of_images(images, net, batch_size=64, device="cuda"):
    p = FeaturePass(net, device, keep=True).over(images, batch_size)
    return torch.cat(p.feats), p.stats


def fd_dinov2(mu1, sigma1, mu2, sigma2) -> float:
    return FID.frechet_distance(mu1, sigma1, mu2, sigma2)


def tokens_flip_flags(num, flip_seed):
    """Which images the ``tokens`` subcommand mirrors: none, or those ``encode_data --flip --seed S`` mirrored."""
    if flip_seed is None:
        return np.zeros(num, dtype=bool)
    from .encode_data import flip_flags
    return flip_flags(num, flip_seed).numpy().astype(bool)


def write_tokens(args):
    """``tokens``: fp16 [num, G * G, dim] through a memory map, a batch at a time (ImageNet at G = 16, ViT-B: 503 GB)."""
    if args.grid < 1 or args.grid > 128:
        raise ValueError(f"--grid {args.grid}: the token grid must lie in 1 .. 128")
    if args.batch_size < 1:
        raise ValueError(f"--batch-size {args.batch_size} must be at least 1")
    if not str(args.output).endswith(".npy"):
        raise ValueError(f"--output {args.output!r}: the tokens are written as one .npy (train.py --repa-features memory-maps it)")
    if args.dinov2_weights is None:
        raise ValueError("tokens needs --dinov2-weights")
    images = FID.load_images(args.images)                      # (a bad array ends the run before the weights are read)
    num = len(images)
    flips = tokens_flip_flags(num, args.flip_seed)
    net = DinoV2Features.from_file(args.dinov2_weights, "cuda", args.precision, min(args.batch_size, 32), image_size=PATCH * args.grid)
    out = np.lib.format.open_memmap(args.output, mode="w+", dtype=np.float16, shape=(num, args.grid * args.grid, net.dim))
    for i in range(0, num, args.batch_size):
        batch = np.ascontiguousarray(images[i:i + args.batch_size])
        fl = flips[i:i + args.batch_size]
        if fl.any():
            batch = batch.copy()
            batch[fl] = batch[fl][:, :, ::-1]
        tok = net.tokens(torch.from_numpy(batch).to("cuda"))
        out[i:i + len(batch)] = tok[:, 1:].to(torch.float16).cpu().numpy()
    out.flush()
    del out
    print(f"{args.output}: fp16 [{num}, {args.grid * args.grid}, {net.dim}] patch tokens" + (f", flips of seed {args.flip_seed}" if args.flip_seed is not None else ""))
    return args.output


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(prog="python -m mapdit_amd.dinov2")
    sub = p.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("stats", help="feature statistics (mu_dinov2, sigma_dinov2) of an image array")
    f = sub.add_parser("features", help="the DINOv2 features of an image array, with their mu_dinov2 and sigma_dinov2")
    for q in (s, f):
        q.add_argument("--images", required=True, help=".npz / .npy of uint8 [N, H, W, 3]")
        q.add_argument("--output", required=True, help="an existing .npz keeps its other arrays (FID's mu, sigma, pool_3)")
    t = sub.add_parser("tokens", help="the patch tokens of an image array as an fp16 .npy [num, G * G, dim]: REPA's targets (train.py --repa-features)")
    t.add_argument("--images", required=True, help=".npz / .npy of uint8 [N, H, W, 3]")
    t.add_argument("--output", required=True, help="the .npy to write (fp16 [num, G * G, dim], CLS dropped)")
    t.add_argument("--grid", type=int, required=True, help="G: the images are resized to 14 G pixels; G * G must equal the DiT's token count")
    t.add_argument("--flip-seed", type=int, default=None, help="mirror image i iff encode_data.flip_flags(num, S)[i] (the latents of encode_data --flip --seed S)")
    c = sub.add_parser("compare", help="FD-DINOv2 of two statistics or features files or image arrays")
    c.add_argument("a", help="the reference (real) side")
    c.add_argument("b", help="the samples")
    for q in (s, f, c, t):
        q.add_argument("--dinov2-weights", default=None, help="dinov2_vitl14_pretrain weights (.safetensors, or a torch state dict)")
        q.add_argument("--batch-size", type=int, default=64)
        q.add_argument("--precision", choices=sorted(PRECISIONS), default="f16")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    net = None

    def network():
        nonlocal net
        if args.dinov2_weights is None:
            raise ValueError("an image array needs --dinov2-weights (only statistics and features files compare without the network)")
        if net is None:
            net = DinoV2Features.from_file(args.dinov2_weights, "cuda", args.precision, min(args.batch_size, 32))
        return net

    if args.cmd == "tokens":
        return write_tokens(args)
    if args.cmd == "stats":
        images = FID.load_images(args.images)                  # (a bad array ends the run before the weights are read)
        st = stats_of_images(images, network(), args.batch_size)
        save_stats(args.output, *st.mean_cov(), keep=True)
        print(f"{args.output}: mu_dinov2, sigma_dinov2 of {st.n} images")
        return args.output
    if args.cmd == "features":
        images = FID.load_images(args.images)
        feat, st = features_of_images(images, network(), args.batch_size)
        save_features(args.output, feat.cpu().numpy(), *st.mean_cov(), keep=True)
        print(f"{args.output}: {FEATURES_KEY}, mu_dinov2, sigma_dinov2 of {st.n} images")
        return args.output
    pairs = [load_stats(f) if _is_stats(f) else stats_of_images(FID.load_images(f), network(), args.batch_size).mean_cov() for f in (args.a, args.b)]
    value = fd_dinov2(*pairs[0], *pairs[1])
    print(f"fd_dinov2: {value:.6f}")
    return value


if __name__ == "__main__":
    main()
