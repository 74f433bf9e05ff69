"""Native FID on ``libmapdit_hip.so``: the 2048 ``pool_3`` features of the 2015 Inception-v3 in the layout of ``pytorch-fid``'s
``pt_inception-2015-12-05`` weights (``mapdit_inc_features``, include/mapdit.h), their fp64 sums on the device
(``mapdit_inc_stats_accumulate``) and the Fréchet distance of the two Gaussian fits on the host.

    python -m mapdit_amd.fid stats --images A.npz --inception-weights FILE --output ref.npz
    python -m mapdit_amd.fid features --images A.npz --inception-weights FILE --output feats.npz
    python -m mapdit_amd.fid compare a.npz b.npz [--inception-weights FILE] [--metrics fid,fid_s,isc,pr,kid]

``features`` writes the ``pool_3`` features [N, 2048] fp32 beside ``mu`` and ``sigma``, so the file still loads as a statistics file.
``--metrics``: ``pr`` (precision, recall, density, coverage) and ``kid`` (metrics.py) need the features of both sides - an image
array with the weights, or a file that holds ``pool_3``; ``a`` is the reference (real) side, ``b`` the samples.
``fid_s`` (sFID): the same Fréchet distance on the spatial features, the first 7 channels of the ``Mixed_6d.branch1x1`` unit
(17 x 17 x 7 = 2023 numbers per image; ``mapdit_inc_features_tap``).  ``stats --spatial`` / ``features --spatial`` add their
statistics as ``mu_s``, ``sigma_s`` (the keys of ADM's reference batches); ``compare`` needs them, or images, on both sides.
``isc`` (Inception Score, ``metrics.inception_score``): of side ``b``, from its ``pool_3`` and the classifier head (``fc.weight``) of
``--inception-weights``; printed as ``isc: mean ± std`` over splits of 5000.

Parity with the hub weights is unpinned: the network is restated from its public description and checked against an independent
fp64 restatement on random weights (tests/inception_reference.py), not against ``pytorch-fid``.  The first FID quoted from this
code needs one cross-check against ``pytorch-fid`` on a machine that has the weight file.  The same holds for ``fid_s`` and ``isc``
against ADM's ``evaluator.py``: ``mixed_6/conv:0`` is TAKEN to be the ``Mixed_6d.branch1x1`` unit's output after BatchNorm and ReLU,
and its channel order to be the port's (a permutation of the 2023 coordinates would not change the distance, another choice of 7
channels would); neither is checked here.
"""
from __future__ import annotations

import argparse
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import metrics as M
from .metrics import METRICS, add_metric_flags, parse_metrics  # noqa: F401  (the --metrics flags, shared with sample_fid.py)
from .vae import PRECISIONS, load_state_dict_file

BN_EPS = 1e-3
FEATURE_DIM = 2048
IMAGE_SIZE = 299


# ---- the key set: every BasicConv2d in execution order (the order of mapdit_inc_features' weight table) ----------------------------
def conv_units() -> list:
    """(name, cin, cout, (kh, kw), stride, (pad_h, pad_w)) of the 94 ``BasicConv2d`` units, in execution order."""
    u = [("Conv2d_1a_3x3", 3, 32, (3, 3), 2, (0, 0)), ("Conv2d_2a_3x3", 32, 32, (3, 3), 1, (0, 0)), ("Conv2d_2b_3x3", 32, 64, (3, 3), 1, (1, 1)),
         ("Conv2d_3b_1x1", 64, 80, (1, 1), 1, (0, 0)), ("Conv2d_4a_3x3", 80, 192, (3, 3), 1, (0, 0))]

    def one(name, cin, cout, k=(1, 1), stride=1, pad=(0, 0)):
        u.append((name, cin, cout, k, stride, pad))

    for blk, cin, pool in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        one(f"{blk}.branch1x1", cin, 64)
        one(f"{blk}.branch5x5_1", cin, 48)
        one(f"{blk}.branch5x5_2", 48, 64, (5, 5), 1, (2, 2))
        one(f"{blk}.branch3x3dbl_1", cin, 64)
        one(f"{blk}.branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1))
        one(f"{blk}.branch3x3dbl_3", 96, 96, (3, 3), 1, (1, 1))
        one(f"{blk}.branch_pool", cin, pool)
    one("Mixed_6a.branch3x3", 288, 384, (3, 3), 2)
    one("Mixed_6a.branch3x3dbl_1", 288, 64)
    one("Mixed_6a.branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1))
    one("Mixed_6a.branch3x3dbl_3", 96, 96, (3, 3), 2)
    for blk, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        one(f"{blk}.branch1x1", 768, 192)
        one(f"{blk}.branch7x7_1", 768, c7)
        one(f"{blk}.branch7x7_2", c7, c7, (1, 7), 1, (0, 3))
        one(f"{blk}.branch7x7_3", c7, 192, (7, 1), 1, (3, 0))
        one(f"{blk}.branch7x7dbl_1", 768, c7)
        one(f"{blk}.branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0))
        one(f"{blk}.branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3))
        one(f"{blk}.branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0))
        one(f"{blk}.branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))
        one(f"{blk}.branch_pool", 768, 192)
    one("Mixed_7a.branch3x3_1", 768, 192)
    one("Mixed_7a.branch3x3_2", 192, 320, (3, 3), 2)
    one("Mixed_7a.branch7x7x3_1", 768, 192)
    one("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3))
    one("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
    one("Mixed_7a.branch7x7x3_4", 192, 192, (3, 3), 2)
    for blk, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        one(f"{blk}.branch1x1", cin, 320)
        one(f"{blk}.branch3x3_1", cin, 384)
        one(f"{blk}.branch3x3_2a", 384, 384, (1, 3), 1, (0, 1))
        one(f"{blk}.branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
        one(f"{blk}.branch3x3dbl_1", cin, 448)
        one(f"{blk}.branch3x3dbl_2", 448, 384, (3, 3), 1, (1, 1))
        one(f"{blk}.branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1))
        one(f"{blk}.branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
        one(f"{blk}.branch_pool", cin, 192)
    return u


_BN_LEAVES = ("bn.weight", "bn.bias", "bn.running_mean", "bn.running_var")
_IGNORED = ("fc.", "AuxLogits.")


def inception_shapes() -> dict:
    """Key -> shape of the feature network's state dict (``fc.*``, ``AuxLogits.*`` and ``num_batches_tracked`` are not part of it)."""
    s = {}
    for name, cin, cout, (kh, kw), _, _ in conv_units():
        s[f"{name}.conv.weight"] = (cout, cin, kh, kw)
        for leaf in _BN_LEAVES:
            s[f"{name}.{leaf}"] = (cout,)
    return s


def fold_bn(w, gamma, beta, mean, var, eps=BN_EPS):
    """conv (no bias) + eval BatchNorm -> conv + bias: w' = w * g / sqrt(var + eps), b' = beta - mean * g / sqrt(var + eps).  fp64."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    return w.double() * s[:, None, None, None], beta.double() - mean.double() * s


def fold_state_dict(sd) -> dict:
    """Checked and folded: {unit name: (w' fp64 [Cout, Cin, kh, kw], b' fp64 [Cout])} in execution order.  A missing or unexpected key
    is a KeyError naming it, a wrong shape a ValueError; a missing ``bn.weight`` counts as ones."""
    shapes = inception_shapes()
    sd = {k: v for k, v in sd.items() if not k.startswith(_IGNORED) and not k.endswith("num_batches_tracked")}
    optional = {k for k in shapes if k.endswith(".bn.weight")}
    missing, extra = sorted(set(shapes) - set(sd) - optional), sorted(set(sd) - set(shapes))
    if missing:
        raise KeyError(f"Inception state dict: missing key {missing[0]!r}" + (f" (and {len(missing) - 1} more)" if len(missing) > 1 else ""))
    if extra:
        raise KeyError(f"Inception state dict: unexpected key {extra[0]!r}" + (f" (and {len(extra) - 1} more)" if len(extra) > 1 else ""))
    for k, v in sd.items():
        if tuple(v.shape) != tuple(shapes[k]):
            raise ValueError(f"Inception state dict: {k!r} has shape {tuple(v.shape)}, expected {tuple(shapes[k])}")
    out = {}
    for name, _, cout, _, _, _ in conv_units():
        gamma = sd.get(f"{name}.bn.weight")
        gamma = torch.ones(cout, dtype=torch.float64) if gamma is None else gamma
        out[name] = fold_bn(sd[f"{name}.conv.weight"], gamma, sd[f"{name}.bn.bias"], sd[f"{name}.bn.running_mean"], sd[f"{name}.bn.running_var"])
    return out


NUM_LOGITS = 1008


def classifier_head(sd):
    """(W fp32 [1008, 2048], b fp32 [1008]) of the raw state dict: the ``fc`` layer on ``pool_3`` that ``fold_state_dict`` leaves out,
    for ``metrics.inception_score``.  A missing key is a KeyError naming it, a wrong shape a ValueError."""
    for k, shape in (("fc.weight", (NUM_LOGITS, FEATURE_DIM)), ("fc.bias", (NUM_LOGITS,))):
        if k not in sd:
            raise KeyError(f"Inception state dict: missing key {k!r} (the classifier head; the Inception Score needs it)")
        if tuple(sd[k].shape) != shape:
            raise ValueError(f"Inception state dict: {k!r} has shape {tuple(sd[k].shape)}, expected {shape}")
    return sd["fc.weight"].detach().to(torch.float32).contiguous(), sd["fc.bias"].detach().to(torch.float32).contiguous()


def pack_conv_weight(w, dtype):
    """[Cout, Cin, kh, kw] -> 16-bit [Cout][kh][kw][Cin], the B operand of mapdit_inc_conv."""
    return w.permute(0, 2, 3, 1).contiguous().to(torch.float32).to(dtype)


class InceptionFeatures:
    """``InceptionFeatures.from_file(path, device).features(x)``: x uint8 [N, H, W, 3] as ``sample_fid.py`` stores images, or fp32
    [N, 3, H, W] in [-1, 1], on the device, any H, W >= 8 -> fp32 [N, 2048] on the device.  Every image is resized to 299 x 299
    (bilinear, align_corners=False) first.  ``precision``: the 16-bit format of the weights and of the activations between the
    layers ("f16" default: 10 mantissa bits; "bf16"); accumulation is fp32.  Batches above ``max_batch`` are chunked; an image alone
    gives the same bits as in a batch."""

    def __init__(self, folded, device, precision="f16", max_batch=32, image_size=IMAGE_SIZE):
        if precision not in PRECISIONS:
            raise ValueError(f"Inception precision {precision!r}: one of {sorted(PRECISIONS)}")
        if max_batch < 1:
            raise ValueError(f"max_batch={max_batch} must be at least 1")
        self.device, self.precision, self.max_batch = torch.device(device), precision, int(max_batch)
        units = conv_units()
        if list(folded) != [u[0] for u in units]:
            raise KeyError("Inception weights: the folded units are not the network's 94 in execution order")
        self._check_plan(units)
        dt = PRECISIONS[precision]
        self.packed = []
        for name in folded:
            w, b = folded[name]
            self.packed += [pack_conv_weight(w, dt).to(self.device), b.to(torch.float32).contiguous().to(self.device)]
        self._cfg = L.IncConfig(image_size=int(image_size))
        self._table = None
        self._ws = None

    @staticmethod
    def _check_plan(units):
        """This module's table against the library's plan (host only): slot by slot the same shapes, or nothing runs."""
        if len(units) != L.INC_NUM_CONV:
            raise L.MapditError(f"fid.py lists {len(units)} convolutions, mapdit.h {L.INC_NUM_CONV}")
        lib = L.lib()
        v = [C.c_int() for _ in range(5)]
        for i, (name, cin, cout, (kh, kw), stride, _) in enumerate(units):
            lib.inc_layer_shape(i, *[C.byref(x) for x in v])
            if [x.value for x in v] != [cin, cout, kh, kw, stride]:
                raise L.MapditError(f"weight slot {i} ({name}): fid.py has {[cin, cout, kh, kw, stride]}, the library's plan {[x.value for x in v]}")

    @classmethod
    def from_state_dict(cls, sd, device, precision="f16", max_batch=32):
        return cls(fold_state_dict(sd), device, precision, max_batch)

    @classmethod
    def from_file(cls, path, device, precision="f16", max_batch=32):
        return cls.from_state_dict(load_state_dict_file(path), device, precision, max_batch)

    def workspace_bytes(self, n) -> int:
        lib = L.lib()
        need = lib.inc_workspace_bytes(C.byref(self._cfg), int(n))
        if need == 0:
            raise ValueError(f"Inception features refused: {lib.last_error().decode()}")
        return need

    @property
    def spatial_dim(self) -> int:
        """The length of a spatial feature row: 17 * 17 * 7 = 2023 at 299 (``mapdit_inc_spatial_shape``, host only)."""
        return spatial_dim(self._cfg.image_size)

    @torch.no_grad()
    def features(self, x, spatial=False):
        """``spatial=True`` -> (feat, fp32 [N, spatial_dim]): sFID's features, the first 7 channels of Mixed_6d.branch1x1 in (h, w, c)
        order, from the same pass; ``feat`` has the same bits either way."""
        if not isinstance(x, torch.Tensor) or not x.is_cuda or self.device.type != "cuda":
            raise NotImplementedError("InceptionFeatures.features runs on the GPU only (HIP kernels, no CPU path): pass a CUDA tensor to a network on the device")
        u8 = x.dtype == torch.uint8
        if x.dim() != 4 or x.shape[3 if u8 else 1] != 3:
            raise ValueError(f"Inception features: x has shape {tuple(x.shape)} ({x.dtype}), expected uint8 [N, H, W, 3] or float [N, 3, H, W]")
        x = x.detach().to(self.device).contiguous() if u8 else x.detach().to(self.device, torch.float32).contiguous()
        N, H, W = (x.shape[0], x.shape[1], x.shape[2]) if u8 else (x.shape[0], x.shape[2], x.shape[3])
        if H < 8 or W < 8:
            raise ValueError(f"Inception features: images of {H} x {W} (8 x 8 at the least)")
        feat = torch.empty(N, FEATURE_DIM, dtype=torch.float32, device=self.device)
        sdim = self.spatial_dim if spatial else 0
        spat = torch.empty(N, sdim, dtype=torch.float32, device=self.device) if spatial else None
        if N == 0:
            return (feat, spat) if spatial else feat
        chunk = min(N, self.max_batch)
        need = self.workspace_bytes(chunk)
        lib = L.lib()
        if self._table is None:
            self._table = (C.c_void_p * len(self.packed))(*[t.data_ptr() for t in self.packed])
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        fn = lib.inc_features_tap_f16 if self.precision == "f16" else lib.inc_features_tap       # (a null tap is mapdit_inc_features)
        kind = L.INC_IMG_U8_NHWC if u8 else L.INC_IMG_F32_NCHW
        with torch.cuda.device(self.device):
            stream = L.cur_stream()
            for i in range(0, N, chunk):
                n = min(chunk, N - i)
                fn(C.byref(self._cfg), self._table, x[i:i + n].data_ptr(), kind, n, H, W, feat[i:i + n].data_ptr(),
                   L.ptr(spat[i:i + n] if spatial else None), self._ws.data_ptr(), self._ws.numel(), stream)
        return (feat, spat) if spatial else feat


class FeatureStats:
    """Running fp64 sums of x and x x^T on the device; ``mean_cov`` -> the mean and the unbiased covariance (``np.cov``'s N - 1) as
    fp64 numpy arrays.  Every element adds its samples in the order they arrive, so the result does not depend on the batching."""

    def __init__(self, D=FEATURE_DIM, device="cuda"):
        self.D, self.device, self.n = int(D), torch.device(device), 0
        if self.device.type != "cuda":
            raise NotImplementedError("FeatureStats accumulates on the GPU only (HIP kernels, no CPU path)")
        self.sum = torch.zeros(self.D, dtype=torch.float64, device=self.device)
        self.outer = torch.zeros(self.D, self.D, dtype=torch.float64, device=self.device)

    def update(self, feat):
        if not isinstance(feat, torch.Tensor) or not feat.is_cuda:
            raise NotImplementedError("FeatureStats.update runs on the GPU only (HIP kernels, no CPU path): pass a CUDA tensor")
        if feat.dim() != 2 or feat.shape[1] != self.D:
            raise ValueError(f"FeatureStats.update: features of shape {tuple(feat.shape)}, expected [N, {self.D}]")
        feat = feat.detach().to(self.device, torch.float32).contiguous()
        if feat.shape[0] == 0:
            return self
        with torch.cuda.device(self.device):
            L.lib().inc_stats_accumulate(feat.data_ptr(), feat.shape[0], self.D, self.sum.data_ptr(), self.outer.data_ptr(), L.cur_stream())
        self.n += int(feat.shape[0])
        return self

    def mean_cov(self):
        if self.n < 2:
            raise ValueError(f"FeatureStats: {self.n} samples; a covariance needs two at the least")
        s, o = self.sum.cpu().numpy(), self.outer.cpu().numpy()
        mu = s / self.n
        sigma = (o - np.outer(s, mu)) / (self.n - 1)
        return mu, (sigma + sigma.T) / 2                      # (the sums are symmetric already; the subtraction's rounding need not be)

    def save(self, path):
        mu, sigma = self.mean_cov()
        save_stats(path, mu, sigma)


SPATIAL_KEYS = ("mu_s", "sigma_s")                             # the keys of ADM's reference batches


def _spatial_arrays(mu_s, sigma_s) -> dict:
    if (mu_s is None) != (sigma_s is None):
        raise ValueError("mu_s and sigma_s go together")
    return {} if mu_s is None else {"mu_s": np.asarray(mu_s, np.float64), "sigma_s": np.asarray(sigma_s, np.float64)}


def save_stats(path, mu, sigma, mu_s=None, sigma_s=None):
    """``mu``, ``sigma`` and, when given, the spatial statistics ``mu_s``, ``sigma_s`` (sFID) as fp64."""
    with open(path, "wb") as f:                                # (an open file: np.savez appends no second ".npz" to the name)
        np.savez(f, mu=np.asarray(mu, np.float64), sigma=np.asarray(sigma, np.float64), **_spatial_arrays(mu_s, sigma_s))


def load_stats(path, spatial=False):
    """``mu`` [D] and ``sigma`` [D, D] of any ``.npz`` that holds them (``pytorch-fid`` statistics, ADM's ``VIRTUAL_*`` reference
    batches); other keys are ignored.  ``spatial=True`` -> (mu, sigma, mu_s, sigma_s): the spatial statistics too, under the keys
    ADM's reference batches carry."""
    keys = ("mu", "sigma") + (SPATIAL_KEYS if spatial else ())
    with np.load(path) as z:
        for k in keys:
            if k in z.files:
                continue
            if k in SPATIAL_KEYS:
                raise KeyError(f"{path}: no {k!r} in the file (it holds {sorted(z.files)}); the spatial statistics are written by "
                               "`python -m mapdit_amd.fid stats --spatial --images A.npz --inception-weights FILE --output ref.npz`")
            raise KeyError(f"{path}: no {k!r} in the file (it holds {sorted(z.files)}); statistics need 'mu' and 'sigma'")
        out = [np.asarray(z[k], np.float64) for k in keys]
    for km, ks, mu, sigma in zip(keys[0::2], keys[1::2], out[0::2], out[1::2]):
        if mu.ndim != 1 or sigma.shape != (mu.shape[0], mu.shape[0]):
            raise ValueError(f"{path}: {km} of shape {mu.shape} and {ks} of shape {sigma.shape} are no [D] and [D, D]")
    return tuple(out)


def has_spatial(path) -> bool:
    """Whether an ``.npz`` carries ``mu_s`` and ``sigma_s`` (the member names alone are read)."""
    import zipfile
    if not str(path).endswith(".npz"):
        return False
    try:
        with zipfile.ZipFile(path) as z:
            return all(k + ".npy" in z.namelist() for k in SPATIAL_KEYS)
    except zipfile.BadZipFile:                                 # (no archive: it carries nothing; the caller's refusal names the command)
        return False


FeatureStats.load = staticmethod(load_stats)

FEATURES_KEY = "pool_3"


def save_features(path, feat, mu, sigma, mu_s=None, sigma_s=None):
    """``pool_3`` fp32 [N, D] beside ``mu`` and ``sigma`` (and ``mu_s``, ``sigma_s`` when given): a statistics file that also carries
    what precision / recall, KID and the Inception Score need."""
    with open(path, "wb") as f:
        np.savez(f, **{FEATURES_KEY: np.asarray(feat, np.float32)}, mu=np.asarray(mu, np.float64), sigma=np.asarray(sigma, np.float64),
                 **_spatial_arrays(mu_s, sigma_s))


def features_rows(path):
    """The number of rows of ``pool_3`` in an ``.npz``, read from the array's header alone; None when the file holds none."""
    import zipfile
    if not str(path).endswith(".npz"):
        return None
    with zipfile.ZipFile(path) as z:
        if FEATURES_KEY + ".npy" not in z.namelist():
            return None
        with z.open(FEATURES_KEY + ".npy") as f:
            np.lib.format.read_magic(f)                        # (np.savez writes format 1.0 for arrays of this size)
            shape = np.lib.format.read_array_header_1_0(f)[0]
    if len(shape) != 2:
        raise ValueError(f"{path}: {FEATURES_KEY} of shape {shape} is no [N, D]")
    return int(shape[0])


def has_features(path) -> bool:
    return features_rows(path) is not None


def load_features(path):
    """fp32 [N, D] ``pool_3`` of a file written by the ``features`` subcommand."""
    with np.load(path) as z:
        if FEATURES_KEY not in z.files:
            raise KeyError(f"{path}: no {FEATURES_KEY!r} in the file (it holds {sorted(z.files)}): write one with "
                           "`python -m mapdit_amd.fid features --images A.npz --inception-weights FILE --output feats.npz`")
        feat = np.ascontiguousarray(z[FEATURES_KEY], np.float32)
    if feat.ndim != 2:
        raise ValueError(f"{path}: {FEATURES_KEY} of shape {feat.shape} is no [N, D]")
    return feat


# ---- metrics beside the FID ---------------------------------------------------------------------------------------------------------
FEATURE_METRICS = ("isc", "pr", "kid")                        # the names that need pool_3 itself, not its statistics


def load_head(path):
    """``classifier_head`` of a weight file: what ``isc`` reads of it."""
    return classifier_head(load_state_dict_file(path))


def spatial_dim(image_size=IMAGE_SIZE) -> int:
    """The length of a spatial feature row at an image size, from the library's plan (host only): 2023 at 299."""
    v = [C.c_int() for _ in range(3)]
    L.lib().inc_spatial_shape(C.byref(L.IncConfig(image_size=int(image_size))), *[C.byref(x) for x in v])
    return v[0].value * v[1].value * v[2].value


def extra_metrics(real, fake, names, args, head=None) -> dict:
    """The values of ``isc``, ``pr`` and ``kid`` (those in ``names``) of two fp32 CUDA feature tensors, in printing order.  ``isc`` is
    the score of ``fake`` alone (``real`` may be None) on ``head``'s weight: the unbiased logits, as in ADM's evaluator."""
    out = {}
    if "isc" in names:
        out["isc"], out["isc_std"] = M.inception_score(fake, head[0].to(fake.device))
    if "pr" in names:
        out.update(M.precision_recall(real, fake))
    if "kid" in names:
        out["kid"], out["kid_std"] = M.kid(real, fake, args.kid_subsets, args.kid_subset_size)
    return out


def frechet_distance(mu1, sigma1, mu2, sigma2) -> float:
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2) in fp64 on the host.  tr (S1 S2)^(1/2) is the sum of the square roots of the
    eigenvalues of S1^(1/2) S2 S1^(1/2), a symmetric positive semi-definite matrix with the spectrum of S1 S2: two symmetric eigh
    solves, no complex arithmetic, no scipy.  Eigenvalues that rounding made negative count as 0."""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, np.float64)), np.atleast_1d(np.asarray(mu2, np.float64))
    s1, s2 = np.atleast_2d(np.asarray(sigma1, np.float64)), np.atleast_2d(np.asarray(sigma2, np.float64))
    if mu1.shape != mu2.shape or s1.shape != s2.shape or s1.shape != (mu1.shape[0], mu1.shape[0]):
        raise ValueError(f"frechet_distance: shapes {mu1.shape}, {s1.shape}, {mu2.shape}, {s2.shape}")
    lam, q = np.linalg.eigh((s1 + s1.T) / 2)
    root = (q * np.sqrt(np.clip(lam, 0.0, None))) @ q.T                    # S1^(1/2)
    m = root @ ((s2 + s2.T) / 2) @ root
    ev = np.linalg.eigvalsh((m + m.T) / 2)
    d = mu1 - mu2
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(np.clip(ev, 0.0, None)).sum())


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def load_images(path):
    """A uint8 [N, H, W, 3] array: an ``.npy``, or the first array of an ``.npz`` (``arr_0``, as ``sample_fid.py`` writes it)."""
    a = np.load(path)
    if not isinstance(a, np.ndarray):
        with a:
            if not a.files:
                raise ValueError(f"{path}: an empty .npz")
            a = a["arr_0" if "arr_0" in a.files else a.files[0]]
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3:
        raise ValueError(f"{path}: an array of shape {a.shape} and dtype {a.dtype}; images are uint8 [N, H, W, 3]")
    return a


def print_metrics(values):
    """One line per metric; the Inception Score with its standard deviation over the splits."""
    for k, v in values.items():
        if k == "isc":
            print(f"isc: {v:.6f} ± {values['isc_std']:.6f}")
        elif k != "isc_std":
            print(f"{k}: {v:.6f}")


class FeaturePass:
    """One pass of the network over batches of uint8 images: the FeatureStats of ``pool_3``, with ``spatial`` those of the spatial
    features from the same walk, and with ``keep`` the ``pool_3`` rows themselves (on the device)."""

    def __init__(self, net, device="cuda", spatial=False, keep=False):
        self.net, self.device = net, device
        self.stats = FeatureStats(FEATURE_DIM, device)
        self.stats_s = FeatureStats(net.spatial_dim, device) if spatial else None
        self.feats = [] if keep else None

    def update(self, images):
        x = torch.from_numpy(np.ascontiguousarray(images)).to(self.device)
        if self.stats_s is None:
            feat = self.net.features(x)
        else:
            feat, spat = self.net.features(x, spatial=True)
            self.stats_s.update(spat)
        self.stats.update(feat)
        if self.feats is not None:
            self.feats.append(feat)
        return self

    def over(self, images, batch_size):
        for i in range(0, len(images), batch_size):
            self.update(images[i:i + batch_size])
        return self


def stats_of_images(images, net, batch_size=64, device="cuda", spatial=False):
    """The FeatureStats of the pool features; ``spatial=True`` -> (that, the FeatureStats of the spatial features) from one pass."""
    p = FeaturePass(net, device, spatial).over(images, batch_size)
    return (p.stats, p.stats_s) if spatial else p.stats


def features_of_images(images, net, batch_size=64, device="cuda", spatial=False):
    """(fp32 [N, 2048] on the device, FeatureStats): stats_of_images that keeps the features.  ``spatial=True`` adds the FeatureStats
    of the spatial features, accumulated in the same pass, as a third value."""
    p = FeaturePass(net, device, spatial, keep=True).over(images, batch_size)
    return (torch.cat(p.feats), p.stats, p.stats_s) if spatial else (torch.cat(p.feats), p.stats)


def _is_stats(path) -> bool:
    if not str(path).endswith(".npz"):
        return False
    with np.load(path) as z:
        return "mu" in z.files and "sigma" in z.files


def build_parser():
    p = argparse.ArgumentParser(prog="python -m mapdit_amd.fid")
    sub = p.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("stats", help="feature statistics (mu, sigma) of an image array")
    s.add_argument("--images", required=True, help=".npz / .npy of uint8 [N, H, W, 3]")
    s.add_argument("--output", required=True)
    f = sub.add_parser("features", help="pool_3 features of an image array, with their mu and sigma")
    f.add_argument("--images", required=True, help=".npz / .npy of uint8 [N, H, W, 3]")
    f.add_argument("--output", required=True)
    for q in (s, f):
        q.add_argument("--spatial", action="store_true", help="add mu_s, sigma_s: the statistics of the spatial features (sFID, --metrics fid_s)")
    c = sub.add_parser("compare", help="FID (and with --metrics sFID, Inception Score, precision / recall, KID) of two statistics or feature "
                                       "files or image arrays")
    c.add_argument("a", help="the reference (real) side")
    c.add_argument("b", help="the samples")
    add_metric_flags(c)
    for q in (s, f, c):
        q.add_argument("--inception-weights", default=None, help="pt_inception-2015-12-05 weights (.safetensors, or a torch state dict)")
        q.add_argument("--batch-size", type=int, default=64)
        q.add_argument("--precision", choices=sorted(PRECISIONS), default="f16")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    net = None

    def network():
        nonlocal net
        if args.inception_weights is None:
            raise ValueError("an image array needs --inception-weights (only statistics files compare without the network)")
        if net is None:
            net = InceptionFeatures.from_file(args.inception_weights, "cuda", args.precision, args.batch_size)
        return net

    if args.cmd == "stats":
        images = load_images(args.images)                      # (a bad array ends the run before the weights are read)
        if args.spatial:
            st, st_s = stats_of_images(images, network(), args.batch_size, spatial=True)
            save_stats(args.output, *st.mean_cov(), *st_s.mean_cov())
            print(f"{args.output}: mu, sigma, mu_s, sigma_s of {st.n} images")
            return args.output
        st = stats_of_images(images, network(), args.batch_size)
        st.save(args.output)
        print(f"{args.output}: mu, sigma of {st.n} images")
        return args.output
    if args.cmd == "features":
        images = load_images(args.images)
        if args.spatial:
            feat, st, st_s = features_of_images(images, network(), args.batch_size, spatial=True)
            save_features(args.output, feat.cpu().numpy(), *st.mean_cov(), *st_s.mean_cov())
            print(f"{args.output}: {FEATURES_KEY}, mu, sigma, mu_s, sigma_s of {st.n} images")
            return args.output
        feat, st = features_of_images(images, network(), args.batch_size)
        save_features(args.output, feat.cpu().numpy(), *st.mean_cov())
        print(f"{args.output}: {FEATURES_KEY}, mu, sigma of {st.n} images")
        return args.output
    names = parse_metrics(args.metrics)
    if names == ("fid",):
        pairs = [load_stats(f) if _is_stats(f) else stats_of_images(load_images(f), network(), args.batch_size).mean_cov() for f in (args.a, args.b)]
        fid = frechet_distance(*pairs[0], *pairs[1])
        print(f"fid: {fid:.6f}")
        return fid
    kinds = ["features" if has_features(f) else "stats" if _is_stats(f) else "images" for f in (args.a, args.b)]
    both = "pr" in names or "kid" in names                     # pool_3 of both sides; isc: of the samples (b) alone
    need_feat = (both, both or "isc" in names)
    for f, kind, need in zip((args.a, args.b), kinds, need_feat):          # refused before the network is built or a kernel runs
        if kind == "stats" and need:
            raise ValueError(f"{f} holds statistics only: --metrics {args.metrics} needs the features of " + ("both sides" if both else "the samples") +
                             "; write them with `python -m mapdit_amd.fid features --images A.npz --inception-weights FILE --output feats.npz`")
        if kind == "images" and args.inception_weights is None:
            raise ValueError(f"{f} is an image array: it needs --inception-weights")
        if "fid_s" in names and kind != "images" and not has_spatial(f):
            raise ValueError(f"{f} holds no 'mu_s' / 'sigma_s': fid_s compares the spatial statistics, which " +
                             ("pool_3 does not give; " if kind == "features" else "the file lacks; ") +
                             "write them with `python -m mapdit_amd.fid stats --spatial --images A.npz --inception-weights FILE --output ref.npz`")
    if "isc" in names and args.inception_weights is None:
        raise ValueError("--metrics isc needs --inception-weights: the Inception Score reads the classifier head (fc.weight) of the file")
    head = load_head(args.inception_weights) if "isc" in names else None   # (the head alone: no network for two feature files)
    feats, pairs, pairs_s = [], [], []
    for f, kind, need in zip((args.a, args.b), kinds, need_feat):
        if kind == "images":
            feat, st, *st_s = features_of_images(load_images(f), network(), args.batch_size, spatial="fid_s" in names)
            feats.append(feat)
            pairs.append(st.mean_cov() if "fid" in names else None)
            pairs_s.append(st_s[0].mean_cov() if st_s else None)
        else:
            feats.append(torch.from_numpy(load_features(f)).to("cuda") if need else None)
            pairs.append(load_stats(f) if "fid" in names else None)
            pairs_s.append(load_stats(f, spatial=True)[2:] if "fid_s" in names else None)
    values = {}
    if "fid" in names:
        values["fid"] = frechet_distance(*pairs[0], *pairs[1])
    if "fid_s" in names:
        values["fid_s"] = frechet_distance(*pairs_s[0], *pairs_s[1])
    values.update(extra_metrics(feats[0], feats[1], names, args, head))
    print_metrics(values)
    return values


if __name__ == "__main__":
    main()
