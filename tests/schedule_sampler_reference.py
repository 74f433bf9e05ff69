"""fp64 numpy restatement of the schedule sampler kernels (csrc/timestep_sampler.hip), written from the definitions in the reference's
diffusion/timestep_sampler.py and numpy's np.random.choice, with the two deliberate deviations of the kernels:

    update    LossSecondMomentResampler.update_with_all_losses over the entries in index order: a row that is not full takes the loss at
              hist[t][counts[t]++], a full row is shifted left by one and takes it in its last slot.  DEVIATIONS: an entry with t outside
              [0, T) is skipped (and counted: the kernel records it for mapdit_device_error_poll); an entry whose loss is inf / NaN is skipped.
    prepare   weights(): ones -> p = 1 / T until all(counts == H); then w = sqrt(mean(hist^2, -1)), p = w / sum(w) * (1 - uniform_prob) +
              uniform_prob / T.  DEVIATION: sum(w) zero or not finite gives p = 1 / T (the reference divides and raises inside numpy).
              cdf = cumsum(p) / cumsum(p)[-1], the table np.random.choice(p=p) builds.
    draw      t = min(searchsorted(cdf, u, side="right"), T - 1), w = float32(1 / (T p[t])): np.random.choice's draw for the uniforms
              random_sample gave it, and ScheduleSampler.sample's importance weights.

The sums here run in numpy's order, the kernel's in its own fixed order: probabilities and cdf agree within TABLE_TOL(T) relative, two
summation orders of T positive fp64 terms plus a few roundings.  History and counts involve no arithmetic and agree exactly.

numpy and fp64 only; nothing here imports the library or touches a device.
"""
import numpy as np

W_TOL = 2.0 ** -22                                   # fp32 sample weights: one fp32 rounding of an fp64 quotient, and the table's error


def TABLE_TOL(T):
    return (T + 8) * 2.0 ** -52


def new_state(T, H):
    return np.zeros([T, H], dtype=np.float64), np.zeros([T], dtype=np.int64)


def update(hist, counts, ts, losses):
    """In place; returns the number of entries skipped for an out-of-range timestep."""
    T, H = hist.shape
    bad = 0
    for t, loss in zip(np.asarray(ts).reshape(-1).tolist(), np.asarray(losses, dtype=np.float32).reshape(-1).tolist()):
        if t < 0 or t >= T:
            bad += 1
            continue
        if not np.isfinite(loss):
            continue
        if counts[t] == H:
            hist[t, :-1] = hist[t, 1:].copy()
            hist[t, -1] = loss
        else:
            hist[t, counts[t]] = loss
            counts[t] += 1
    return bad


def warmed_up(hist, counts):
    return bool((counts == hist.shape[1]).all())


def table(p):
    """(p, cdf) of an unnormalised positive vector, as ScheduleSampler.sample and np.random.choice build them."""
    p = np.asarray(p, dtype=np.float64)
    cdf = np.cumsum(p)
    return p, cdf / cdf[-1]


def prepare(hist, counts, uniform_prob):
    T = hist.shape[0]
    flat = np.full([T], 1.0 / T, dtype=np.float64)
    if not warmed_up(hist, counts):
        return table(flat)
    with np.errstate(all="ignore"):
        w = np.sqrt(np.mean(hist ** 2, axis=-1))
        s = np.sum(w)
        if not (s > 0.0 and np.isfinite(s)):
            return table(flat)
        w = w / s
        w = w * (1.0 - uniform_prob)
        w = w + uniform_prob / T
    return table(w)


def weights(hist, counts, uniform_prob):
    """The reference's weights() vector: ones until warmed up, then prepare()'s probabilities."""
    if not warmed_up(hist, counts):
        return np.ones([hist.shape[0]], dtype=np.float64)
    return prepare(hist, counts, uniform_prob)[0]


def prepare_weights(w):
    """(p, cdf, bad): bad = some weight is <= 0 or not finite (the kernel records it and falls back to the uniform table)."""
    w = np.asarray(w, dtype=np.float64)
    with np.errstate(all="ignore"):
        s = np.sum(w)
        bad = bool((~(w > 0.0) | ~np.isfinite(w)).any()) or not (s > 0.0 and np.isfinite(s))
    if bad:
        return table(np.full(w.shape, 1.0 / w.size)) + (True,)
    return table(w / s) + (False,)


def draw(prob, cdf, u):
    T = prob.size
    t = np.minimum(np.searchsorted(cdf, np.asarray(u, dtype=np.float64), side="right"), T - 1).astype(np.int64)
    return t, (1.0 / (T * prob[t])).astype(np.float32)
