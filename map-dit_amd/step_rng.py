"""Counter-based draws of a training step: noise, timesteps, label drops and the --synthetic batch as ONE launch of csrc/steprng.hip.

Every draw is a pure function of (seed, optimiser step, slot in the global batch): the same bits for any world size, micro-batch
split and rank, and no generator state to carry - continuing a run needs the step number and nothing else.  The random-number layout
is a contract (include/mapdit.h, "Counter-based step draws").
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from ._lib import ptr

OUTPUTS = ("eps", "x_syn", "t", "u", "z", "drop", "y_syn")             # in the order of mapdit_step_draw's parameters
_DTYPES = {"eps": torch.float32, "x_syn": torch.float32, "t": torch.int64, "u": torch.float64, "z": torch.float64,
           "drop": torch.int64, "y_syn": torch.int64}


def drop_threshold(drop_prob: float) -> int:
    """thr of the contract's label drop: ceil(float32(p) * 2^24); slot drops its label where (a1 >> 8) < thr."""
    p = float(np.float32(drop_prob))
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"drop_prob must lie in [0, 1], got {drop_prob!r}")
    return math.ceil(p * 2.0 ** 24)                                     # (exact: an fp32 value times a power of two)


def first_slot(lo: int, k: int, micro: int) -> int:
    """Slot in the global batch of the first sample of micro-batch k of the rank whose share starts at `lo` (parallel.shard_batch)."""
    return int(lo) + int(k) * int(micro)


class StepRNG:
    """`seed`: the run's --seed (its low 64 bits are the Philox key)."""

    def __init__(self, seed: int, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise NotImplementedError("StepRNG draws with a HIP kernel (csrc/steprng.hip): no CPU path")
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.device = device

    def draw(self, step: int, first_slot: int, count: int, per: int | None = None, T: int | None = None, num_classes: int | None = None,
             drop_prob: float | None = None, want=OUTPUTS):
        """The draws of slots [first_slot, first_slot + count) of 0-based optimiser step `step`, one launch on the current stream.
        `want` names the outputs (OUTPUTS); the namespace returned holds exactly those: eps / x_syn fp32 [count, per] (needs `per`),
        t int64 [count] in [0, T) (needs `T`), u fp64 [count] in [0, 1), z fp64 [count] standard normal, drop int64 [count], 1 = drop
        the label (needs `drop_prob`), y_syn int64 [count] in [0, num_classes) (needs `num_classes`)."""
        want = tuple(want)
        unknown = [w for w in want if w not in OUTPUTS]
        if unknown or not want:
            raise ValueError(f"want names {unknown or 'nothing'}; the outputs are {OUTPUTS}")
        needs = {"eps": ("per", per), "x_syn": ("per", per), "t": ("T", T), "drop": ("drop_prob", drop_prob), "y_syn": ("num_classes", num_classes)}
        for w in want:
            if w in needs and needs[w][1] is None:
                raise ValueError(f"draw(want={w!r}) needs {needs[w][0]}")
        if not 0 <= int(step) < 1 << 32:
            raise ValueError(f"step {step}: the step is a 32-bit counter word")
        count = int(count)
        out = {w: torch.empty((count, int(per)) if w in ("eps", "x_syn") else (count,), dtype=_DTYPES[w], device=self.device)
               for w in want if count >= 1 and (per is None or int(per) >= 1)}             # (a bad count / per is the entry's to refuse)
        with torch.cuda.device(self.device):
            _lib.lib().step_draw(self.seed, int(step), int(first_slot), count, 1 if per is None else int(per), 1 if T is None else int(T),
                                 1 if num_classes is None else int(num_classes), 0.0 if drop_prob is None else float(drop_prob),
                                 *(ptr(out.get(w)) for w in OUTPUTS), _lib.cur_stream())
        return SimpleNamespace(**out)
