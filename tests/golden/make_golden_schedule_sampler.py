#!/usr/bin/env python3
"""Golden vectors for the schedule samplers (runs ONLY where a checkout of the reference exists; see make_golden.py).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_schedule_sampler.py REFERENCE_ROOT      (or MAPDIT_REFERENCE=...)

Imports the reference's diffusion/timestep_sampler.py UNCHANGED (np.int, which its constructor needs and numpy >= 1.24 no longer has, is
set here first) and writes tests/golden/schedule_sampler.npz: inputs and recorded results only, nothing of the reference is copied.

For each setting (T, H) - (37, 3) and (1000, 10), uniform_prob 0.001 - under the keys "<tag>_...":
  batch<i>_ts / batch<i>_losses   the update batches (int16 timesteps, fp32 losses) fed to update_with_all_losses one after the other as
                                  lists of Python numbers, as update_with_local_losses does.  Every batch is a permutation of all
                                  timesteps followed by repeats, so every batch names some timesteps several times; in the (37, 3)
                                  setting one timestep occurs more than H times in a batch (its row fills and shifts inside one batch).
  points                          after how many batches the three snapshots were taken: before warm-up, at the first warmed-up
                                  batch, and after further shifts
  p<k>_hist / p<k>_counts         _loss_history (stored as fp32: every entry IS an fp32 loss, asserted) and _loss_counts
  p<k>_weights / p<k>_cdf         weights() and the cdf np.random.choice(p = weights / sum) builds from it
  p<k>_seed / p<k>_u / p<k>_idx / p<k>_w
                                  np.random.seed(s); u = random_sample(N), and np.random.seed(s); sampler.sample(N, "cpu"): the indices
                                  are searchsorted(cdf, u, "right") (asserted), and every u lies further than 1e-9 from every cdf edge
                                  (asserted; a seed that violates it is replaced by the next), so no draw is excluded from an exact
                                  comparison.
"""
import importlib.util
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SETTINGS = [(37, 3, 64), (1000, 10, 256)]            # (T, H, draws per snapshot)
UNIFORM_PROB = 0.001
GAP = 1e-9


def load_reference(root):
    np.int = int                                      # the reference's constructor: np.zeros(..., dtype=np.int)
    spec = importlib.util.spec_from_file_location("ref_timestep_sampler", os.path.join(root, "diffusion", "timestep_sampler.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_batches(rng, T, H):
    """H + 2 batches: a permutation of all timesteps, then repeats.  After H - 1 batches no history is warmed up, batch H completes every
    row (rows with repeats have shifted already), two more shift every row twice or more."""
    out = []
    extra = max(13, T // 40)
    for b in range(H + 2):
        rep = rng.integers(0, T, size=extra)
        if T < 100:
            rep[:H + 2] = rep[0]                      # one timestep H + 3 times in this batch: fills and shifts inside one batch
        ts = np.concatenate([rng.permutation(T), rep]).astype(np.int16)
        losses = (rng.lognormal(mean=-2.0, sigma=1.5, size=ts.size) * (1.0 + 4.0 * ts / T)).astype(np.float32)
        out.append((ts, losses))
    return out


def main(root):
    ref = load_reference(root)
    rng = np.random.default_rng(20240611)
    data = {}
    for T, H, N in SETTINGS:
        tag = f"t{T}h{H}"
        sampler = ref.LossSecondMomentResampler(types.SimpleNamespace(num_timesteps=T), history_per_term=H, uniform_prob=UNIFORM_PROB)
        batches = make_batches(rng, T, H)
        points = [H - 1, H, H + 2]
        data[f"{tag}_points"] = np.asarray(points, dtype=np.int64)
        data[f"{tag}_uniform_prob"] = np.float64(UNIFORM_PROB)
        seed = 1000 * T
        for i, (ts, losses) in enumerate(batches):
            assert len(np.unique(ts)) < ts.size
            data[f"{tag}_batch{i}_ts"], data[f"{tag}_batch{i}_losses"] = ts, losses
            sampler.update_with_all_losses([int(t) for t in ts], [float(x) for x in losses])
            if i + 1 not in points:
                continue
            k = points.index(i + 1)
            assert sampler._warmed_up() == (k > 0), (tag, k)
            hist = sampler._loss_history.copy()
            assert np.array_equal(hist.astype(np.float32).astype(np.float64), hist)
            w = sampler.weights()
            p = w / np.sum(w)
            cdf = np.cumsum(p)
            cdf /= cdf[-1]
            while True:
                seed += 1
                np.random.seed(seed)
                u = np.random.random_sample(N)
                if np.abs(u[:, None] - cdf[None, :]).min() > GAP:
                    break
            np.random.seed(seed)
            idx, sw = sampler.sample(N, "cpu")
            idx, sw = idx.numpy(), sw.numpy()
            assert np.array_equal(idx, np.searchsorted(cdf, u, side="right")), (tag, k)
            assert idx.max() < T and sw.dtype == np.float32
            print(f"{tag} point {k}: after {i + 1} batches, warmed {sampler._warmed_up()}, seed {seed}, "
                  f"smallest gap {np.abs(u[:, None] - cdf[None, :]).min():.2e}, weights {sw.min():.3g} .. {sw.max():.3g}")
            data.update({f"{tag}_p{k}_hist": hist.astype(np.float32), f"{tag}_p{k}_counts": sampler._loss_counts.astype(np.int64),
                         f"{tag}_p{k}_weights": w.astype(np.float64), f"{tag}_p{k}_cdf": cdf, f"{tag}_p{k}_seed": np.int64(seed),
                         f"{tag}_p{k}_u": u, f"{tag}_p{k}_idx": idx.astype(np.int64), f"{tag}_p{k}_w": sw})
    out = os.path.join(HERE, "schedule_sampler.npz")
    np.savez_compressed(out, **data)
    print(f"wrote {out}: {os.path.getsize(out) / 1024:.1f} kB")


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MAPDIT_REFERENCE")
    if not root or not os.path.isdir(root):
        sys.exit("usage: make_golden_schedule_sampler.py REFERENCE_ROOT (a checkout of the reference; or MAPDIT_REFERENCE)")
    main(root)
