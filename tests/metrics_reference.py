"""Independent fp64 numpy restatement of map-dit_amd/metrics.py, the yardstick of tests/test_manifold_gpu.py and
tests/test_metrics_cpu.py.  Nothing here shares a formula with the library: squared distances are brute-force ``((x - y)^2).sum``
(no norm expansion), neighbours come from a sort, and the KID estimator is written from its definition."""
import numpy as np


def sqdist(q, r):
    """fp64 [Nq, Nr]: sum_d (q_i[d] - r_j[d])^2, one query row at a time."""
    q, r = np.asarray(q, np.float64), np.asarray(r, np.float64)
    out = np.empty((q.shape[0], r.shape[0]), np.float64)
    for i in range(q.shape[0]):
        diff = r - q[i]
        out[i] = (diff * diff).sum(1)
    return out


def knn_radii(x, k):
    """The k-th smallest squared distance to a row at another index."""
    d = sqdist(x, x)
    out = np.empty(d.shape[0], np.float64)
    for i in range(d.shape[0]):
        out[i] = np.sort(np.delete(d[i], i))[k - 1]
    return out


def count_ref_radius(q, r, rad_r, d=None):
    d = sqdist(q, r) if d is None else d
    return (d <= np.asarray(rad_r, np.float64)[None, :]).sum(1)


def count_query_radius(q, r, rad_q, d=None):
    d = sqdist(q, r) if d is None else d
    return (d <= np.asarray(rad_q, np.float64)[:, None]).sum(1)


def precision_recall(real, fake, k=3):
    """Kynkäänniemi et al. 2019 (precision, recall) and Naeem et al. 2020 (density, coverage), on squared distances."""
    r_real, r_fake = knn_radii(real, k), knn_radii(fake, k)
    d_fr = sqdist(fake, real)
    in_real = count_ref_radius(fake, real, r_real, d_fr)
    in_fake = count_ref_radius(real, fake, r_fake, d_fr.T)
    covered = count_query_radius(real, fake, r_real, d_fr.T)
    return {"precision": float((in_real > 0).mean()), "recall": float((in_fake > 0).mean()), "density": float(in_real.mean() / k),
            "coverage": float((covered > 0).mean())}


def poly_kernel(a, b, gamma, coef0=1.0, degree=3):
    return (gamma * (np.asarray(a, np.float64) @ np.asarray(b, np.float64).T) + coef0) ** degree


def poly_kernel_sum(a, b, gamma, coef0=1.0, degree=3, skip_diag=False):
    k = poly_kernel(a, b, gamma, coef0, degree)
    return float(k.sum() - (np.trace(k) if skip_diag else 0.0))


def mmd2_unbiased(x, y):
    """1 / (m (m - 1)) sum_{i != j} k(x_i, x_j) + the same for y - 2 / m^2 sum_{i, j} k(x_i, y_j), k = (x.y / D + 1)^3: a double loop
    over the pairs, as the definition reads."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    m, D = x.shape[0], x.shape[1]
    assert y.shape[0] == m
    kxx = kyy = kxy = 0.0
    for i in range(m):
        for j in range(m):
            if i != j:
                kxx += (x[i] @ x[j] / D + 1.0) ** 3
                kyy += (y[i] @ y[j] / D + 1.0) ** 3
            kxy += (x[i] @ y[j] / D + 1.0) ** 3
    return kxx / (m * (m - 1)) + kyy / (m * (m - 1)) - 2.0 * kxy / (m * m)


def kid(real, fake, index_pairs):
    """(mean, std) of mmd2_unbiased over the given (real indices, fake indices) subsets."""
    est = np.array([mmd2_unbiased(np.asarray(real)[i], np.asarray(fake)[j]) for i, j in index_pairs])
    return float(est.mean()), float(est.std())


def clusters(seed, D, n_a=200, n_b=333):
    """The numerics fixture: eight centres standard_normal((8, D)); rows relu(0.5 centre[randint] + s standard_normal), s = 0.5 for
    set A (n_a rows) and 0.55 for set B (n_b rows), drawn in that order from default_rng(seed) and cast to fp32."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((8, D))
    out = []
    for n, s in ((n_a, 0.5), (n_b, 0.55)):
        which = rng.integers(0, 8, n)
        out.append(np.maximum(0.5 * centres[which] + s * rng.standard_normal((n, D)), 0.0).astype(np.float32))
    return out


def ambiguous_pairs(q, r, rad, mode, eps=4 * 3.5e-7):
    """Number of pairs whose fp64 d2 lies within eps (n_q + n_r) of the radius it is compared with (mode "ref": rad[r], "query":
    rad[q]): the pairs an fp32 evaluation of the norm expansion may place on the other side."""
    q64, r64 = np.asarray(q, np.float64), np.asarray(r, np.float64)
    d = sqdist(q64, r64)
    band = eps * ((q64 * q64).sum(1)[:, None] + (r64 * r64).sum(1)[None, :])
    rad = np.asarray(rad, np.float64)
    thr = rad[None, :] if mode == "ref" else rad[:, None]
    return int((np.abs(d - thr) <= band).sum())
