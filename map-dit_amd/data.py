"""Device-resident latent data set: the reference's four files (train.py:144-176) held in HBM, and a batch - epoch shuffle, gather,
posterior draw and standardisation - as ONE launch of csrc/dataset.hip.

A batch is a pure function of (seed, optimiser step): the same bits for any world size, micro-batch split and rank, no host
processes, no copies, no loader state.  Continuing a run needs the step number and nothing else, so there is no state_dict.  The
random-number layout is a contract (include/mapdit.h, "Device-resident latent data set").

Two deviations from the reference's DataLoader, both inherent: the epoch permutation is a stateless Feistel network instead of
torch.randperm, and a sample's noise is a function of (seed, epoch, position in the epoch) instead of a worker's generator.
"""
from __future__ import annotations

import math
import os

import torch

from . import _lib, parallel
from ._lib import MapditError, ptr

FILES = ("posterior_means.pt", "posterior_stds.pt", "labels.pt", "stats.pt")


def position(step: int, global_batch: int, n_samples: int):
    """(epoch, first) of the 0-based optimiser step: E = N // B whole batches make an epoch and the last N % B positions of every
    epoch's permutation are dropped (the reference loader's drop_last=True; another permutation, other samples)."""
    if step < 0 or global_batch < 1:
        raise ValueError(f"step {step} / global batch {global_batch}: step >= 0 and batch >= 1")
    per_epoch = n_samples // global_batch
    if per_epoch < 1:
        raise ValueError(f"the data set holds {n_samples} samples, fewer than the global batch {global_batch}")
    return step // per_epoch, (step % per_epoch) * global_batch


class DeviceLatentDataset:
    """`source`: a directory with posterior_means.pt / posterior_stds.pt / labels.pt / stats.pt, or the tuple
    (means [N, C, H, W], stds [N, C, H, W], labels [N], stats {"mean": [C], "std": [C]})."""

    def __init__(self, source, device, seed: int = 0):
        device = torch.device(device)
        if device.type != "cuda":
            raise NotImplementedError("DeviceLatentDataset keeps the data in HBM and draws batches with a HIP kernel: no CPU path")
        if isinstance(source, (str, os.PathLike)):
            ld = lambda n: torch.load(os.path.join(source, n), weights_only=True)
            means, stds, labels, stats = (ld(n) for n in FILES)
        else:
            means, stds, labels, stats = source
        if means.dim() != 4 or stds.shape != means.shape or labels.shape != means.shape[:1] or means.shape[0] < 1:
            raise ValueError(f"means {tuple(means.shape)} / stds {tuple(stds.shape)} must be one [N, C, H, W] shape and labels "
                             f"{tuple(labels.shape)} [N], N >= 1")
        if means.shape[0] >= 1 << 32:
            raise ValueError(f"{means.shape[0]} samples: positions are 32-bit counter words (N < 2^32)")
        ch_mean = torch.as_tensor(stats["mean"], dtype=torch.float32).reshape(-1).cpu()
        ch_std = torch.as_tensor(stats["std"], dtype=torch.float32).reshape(-1).cpu()
        if ch_mean.numel() != means.shape[1] or ch_std.numel() != means.shape[1]:
            raise ValueError(f"stats hold {ch_mean.numel()} means / {ch_std.numel()} stds for {means.shape[1]} channels")
        if not all(math.isfinite(v) and v > 0 for v in ch_std.tolist()) or not all(math.isfinite(v) for v in ch_mean.tolist()):
            raise ValueError(f"stats must be finite with std > 0 (the kernel divides by it): mean {ch_mean.tolist()}, std {ch_std.tolist()}")
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.device = device
        self.stats = {"mean": ch_mean.clone(), "std": ch_std.clone()}
        want = [(means, torch.float32), (stds, torch.float32), (labels, torch.int64)]
        resident = lambda t, dt: t.device == device and t.dtype == dt and t.is_contiguous()
        need = sum(t.numel() * dt.itemsize for t, dt in want if not resident(t, dt))
        free = torch.cuda.mem_get_info(device)[0]
        if need > free:
            raise MapditError(f"the data set needs {need:,} bytes of device memory and {free:,} are free on {device}: it must fit "
                              f"HBM (sharding over ranks and 16-bit storage are not built)")
        self.means, self.stds, self.labels = (t if resident(t, dt) else t.to(device=device, dtype=dt).contiguous() for t, dt in want)
        self.ch_mean, self.ch_std = ch_mean.to(device), ch_std.to(device)

    channels = property(lambda self: self.means.shape[1])
    data_size = property(lambda self: self.means.shape[2])

    def __len__(self):
        return self.means.shape[0]

    def position(self, step: int, global_batch: int):
        return position(int(step), int(global_batch), len(self))

    def batch(self, step: int, global_batch: int, rank: int = 0, world: int = 1):
        """This rank's slots (parallel.shard_batch) of the global batch of 0-based optimiser step `step`: x [n, C, H, W] fp32
        standardised draws from the samples' posteriors, y [n] int64."""
        epoch, first = self.position(step, global_batch)
        if epoch >= 1 << 32:
            raise ValueError(f"step {step} lies in epoch {epoch}: the epoch is a 32-bit counter word")
        lo, hi = parallel.shard_batch(int(global_batch), rank, world)
        n, (_, C, H, W) = hi - lo, self.means.shape
        x = torch.empty((n, C, H, W), dtype=torch.float32, device=self.device)
        y = torch.empty((n,), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.lib().data_batch(ptr(self.means), ptr(self.stds), ptr(self.labels), len(self), C, H * W, ptr(self.ch_mean), ptr(self.ch_std),
                                  self.seed, epoch, first + lo, n, None, ptr(x), ptr(y), None, _lib.cur_stream())
        return x, y
