"""Counter-based draws of the samplers: the initial latent, the label and every reverse step's noise of sample `s` as a pure function
of (seed, s) - csrc/samplerng.hip on the library's Philox4x32-10.

A sample's draws depend on neither the batch it sits in, the process that makes it nor anything drawn before it, so a sampling run can
be split over processes, stopped and continued (sample_fid.py --sample-rng counter).  The random-number layout is a contract
(include/mapdit.h, "Counter-based sampler draws").  The sample index of a row travels as a DEVICE int64 array: the two halves of a
classifier-free-guidance batch carry the same indices, and a captured graph is re-aimed by copying into its index buffer.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import ptr

INDEX_END = 1 << 32                                                     # the sample index is a 32-bit counter word


def pair(rng, index):
    """The loops' `rng=` / `index=` keywords go together: (None, None), or an rng and its checked int64 device index."""
    if (rng is None) != (index is None):
        raise ValueError("rng= and index= go together: a SampleRNG draws by sample index, and an index means nothing without one "
                         f"(got rng={'None' if rng is None else type(rng).__name__}, index={'None' if index is None else 'given'})")
    if rng is None:
        return None, None
    check_index(index)                                                  # (before the rng is touched: a bad index needs no device to refuse)
    return rng, rng.check_index(index)


def check_index(index):
    """The range rule: a non-empty 1-d integer sequence with every entry in [0, 2^32) - the kernels read the low 32 bits of an index,
    so anything else is refused -> the index as a tensor.  Reads the values on the host: call it outside a capture."""
    idx = torch.as_tensor(index)
    if idx.dim() != 1 or idx.numel() < 1 or idx.dtype.is_floating_point or idx.dtype.is_complex or idx.dtype == torch.bool:
        raise ValueError(f"index must be a non-empty 1-d integer sequence; got shape {tuple(idx.shape)}, {idx.dtype}")
    lo, hi = int(idx.min()), int(idx.max())
    if lo < 0 or hi >= INDEX_END:
        raise ValueError(f"sample index {lo if lo < 0 else hi} does not lie in [0, 2^32): the index is a 32-bit counter word")
    return idx


def rows_index(index, rows: int):
    """The index of a batch of `rows` rows: one entry per row, or one per row of HALF the batch - the classifier-free-guidance layout
    [conditional | unconditional], whose halves carry the same sample indices and so the same noise."""
    n = index.numel()
    if rows == n:
        return index
    if rows == 2 * n:
        return torch.cat([index, index])
    raise ValueError(f"{n} sample indices for a batch of {rows} rows: pass one per row, or one per row of one half of a guidance batch")


class SampleRNG:
    """`seed`: the run's --seed (its low 64 bits are the Philox key)."""

    def __init__(self, seed: int, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise NotImplementedError("SampleRNG draws with a HIP kernel (csrc/samplerng.hip): no CPU path")
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.device = device

    def check_index(self, index):
        """The module's `check_index`, then int64 [N] on this rng's device."""
        return check_index(index).to(device=self.device, dtype=torch.int64).contiguous()

    def _draw(self, index, per, num_classes, want_z, want_y):
        n = index.numel()
        z = torch.empty(n, per, dtype=torch.float32, device=self.device) if want_z else None
        y = torch.empty(n, dtype=torch.int64, device=self.device) if want_y else None
        with torch.cuda.device(self.device):
            _lib.lib().sample_draw(self.seed, index.data_ptr(), n, per, int(num_classes), ptr(z), ptr(y), _lib.cur_stream())
        return z, y

    def latents(self, index, shape):
        """fp32 [len(index), *shape]: the initial latent of each sample index."""
        index = self.check_index(index)
        per = 1
        for d in shape:
            per *= int(d)
        return self._draw(index, per, 1, True, False)[0].view(index.numel(), *shape)

    def labels(self, index, num_classes: int):
        """int64 [len(index)] in [0, num_classes)."""
        return self._draw(self.check_index(index), 1, num_classes, False, True)[1]

    def noise(self, index, t, shape):
        """fp32 [len(index), *shape]: the noise of the step row j takes at schedule index t[j] (int64 [len(index)])."""
        index = self.check_index(index)
        return self.noise_checked(index, t, (index.numel(), *shape))

    def noise_checked(self, index, t, full_shape):
        """`noise` for an index check_index has returned already (no host read: what the loops call per step)."""
        t = t.to(device=self.device, dtype=torch.int64).contiguous()
        if t.shape != index.shape:
            raise ValueError(f"t has shape {tuple(t.shape)}, the index {tuple(index.shape)}")
        out = torch.empty(*full_shape, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.lib().sample_noise(self.seed, index.data_ptr(), t.data_ptr(), index.numel(), out[0].numel(), out.data_ptr(), _lib.cur_stream())
        return out
