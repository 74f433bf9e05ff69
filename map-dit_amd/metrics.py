"""Sample-quality metrics beside the FID, on ``libmapdit_hip.so``'s pairwise-Gram kernel (csrc/manifold.hip; include/mapdit.h,
"Sample-quality metrics on feature sets"): improved precision / recall (Kynkäänniemi et al. 2019), density / coverage (Naeem et al.
2020) and the Kernel Inception Distance (Bińkowski et al. 2018).  Inputs are fp32 CUDA tensors ``[N, D]`` (the ``pool_3`` features of
``fid.py``: D = 2048), D a multiple of 4.  The N x M distance matrix is never stored; everything is on squared distances.

    knn_radii(x, k=3)                       fp32 [N]: the k-th smallest squared distance to another row
    precision_recall(real, fake, k=3)       {"precision", "recall", "density", "coverage"}
    kid(real, fake, subsets=100, subset_size=1000, seed=0)     (mean, std) of the unbiased MMD^2 estimate, kernel (x.y / D + 1)^3
    inception_score(feat, fc_weight, fc_bias=None, split_size=5000)    (mean, std) over the splits of exp(mean KL(p_n || p_bar)):
                                            the softmax over feat . fc_weight^T is reduced on the Gram tile, never stored

``chunks`` (0: chosen by the library) only cuts the work differently; no result depends on it.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L

_MODES = {"ref": L.BALL_REF_RADIUS, "query": L.BALL_QUERY_RADIUS}


def _features(x, name):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise NotImplementedError(f"metrics: {name} must be a CUDA tensor (HIP kernels, no CPU path)")
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"metrics: {name} has shape {tuple(x.shape)} and dtype {x.dtype}, expected fp32 [N, D]")
    return x.detach().contiguous()


def _workspace(need, device, what):
    if need == 0:
        raise ValueError(f"metrics: {what} refused: {L.lib().last_error().decode()}")
    return torch.empty(need, dtype=torch.uint8, device=device)


def knn_radii(x, k=3, chunks=0):
    """fp32 [N] on the device: the k-th smallest squared distance from each row to another row (1 <= k <= 8, k < N).  The row itself
    is left out by index: a duplicate row elsewhere is a neighbour at distance 0."""
    x = _features(x, "x")
    N, D = x.shape
    lib = L.lib()
    radii = torch.empty(N, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        ws = _workspace(lib.knn_radii_workspace_bytes(N, D, chunks), x.device, "knn_radii")
        lib.knn_radii(x.data_ptr(), N, D, int(k), radii.data_ptr(), chunks, ws.data_ptr(), ws.numel(), L.cur_stream())
    return radii


def ball_count(q, r, rad, mode="ref", exclude_self=False, chunks=0):
    """int64 [Nq] on the device: per query the number of references r with d2(q, r) <= rad[r] (mode "ref", rad [Nr]) or <= rad[q]
    (mode "query", rad [Nq]).  ``exclude_self`` skips r == q by index and needs q and r to be the same tensor."""
    q, r = _features(q, "q"), _features(r, "r")
    if mode not in _MODES:
        raise ValueError(f"metrics: mode {mode!r}: one of {sorted(_MODES)}")
    if q.shape[1] != r.shape[1]:
        raise ValueError(f"metrics: q has {q.shape[1]} dimensions, r {r.shape[1]}")
    if not isinstance(rad, torch.Tensor) or not rad.is_cuda:
        raise NotImplementedError("metrics: rad must be a CUDA tensor (HIP kernels, no CPU path)")
    want = r.shape[0] if mode == "ref" else q.shape[0]
    if rad.dtype != torch.float32 or tuple(rad.shape) != (want,):
        raise ValueError(f"metrics: rad has shape {tuple(rad.shape)} and dtype {rad.dtype}, mode {mode!r} expects fp32 [{want}]")
    rad = rad.detach().contiguous()
    Nq, Nr, D = q.shape[0], r.shape[0], q.shape[1]
    lib = L.lib()
    count = torch.empty(Nq, dtype=torch.int32, device=q.device)           # (the library writes uint32: the same bits below 2^31)
    with torch.cuda.device(q.device):
        ws = _workspace(lib.ball_count_workspace_bytes(Nq, Nr, D, chunks), q.device, "ball_count")
        lib.ball_count(q.data_ptr(), Nq, r.data_ptr(), Nr, D, rad.data_ptr(), _MODES[mode], 1 if exclude_self else 0, count.data_ptr(), chunks,
                       ws.data_ptr(), ws.numel(), L.cur_stream())
    return count.to(torch.int64)


def poly_kernel_sum(a, b, gamma, coef0=1.0, degree=3, skip_diag=False, chunks=0):
    """fp64 0-dim tensor on the device: sum over i, j of (gamma * a_i . b_j + coef0)^degree, the fp32 dot product widened to fp64
    before the polynomial.  ``skip_diag`` drops i == j and needs a and b to be the same tensor."""
    a, b = _features(a, "a"), _features(b, "b")
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"metrics: a has {a.shape[1]} dimensions, b {b.shape[1]}")
    Na, Nb, D = a.shape[0], b.shape[0], a.shape[1]
    lib = L.lib()
    out = torch.empty((), dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        ws = _workspace(lib.poly_kernel_sum_workspace_bytes(Na, Nb, D, chunks), a.device, "poly_kernel_sum")
        lib.poly_kernel_sum(a.data_ptr(), Na, b.data_ptr(), Nb, D, float(gamma), float(coef0), int(degree), 1 if skip_diag else 0, out.data_ptr(),
                            chunks, ws.data_ptr(), ws.numel(), L.cur_stream())
    return out


def precision_recall(real, fake, k=3, chunks=0) -> dict:
    """precision: the share of fake samples inside some real sample's k-NN ball; recall: the same with the roles swapped; density: the
    mean number of real balls that hold a fake sample, over k; coverage: the share of real samples whose own ball holds a fake one."""
    real, fake = _features(real, "real"), _features(fake, "fake")
    r_real, r_fake = knn_radii(real, k, chunks), knn_radii(fake, k, chunks)
    in_real = ball_count(fake, real, r_real, "ref", chunks=chunks)
    in_fake = ball_count(real, fake, r_fake, "ref", chunks=chunks)
    covered = ball_count(real, fake, r_real, "query", chunks=chunks)
    nf, nr = fake.shape[0], real.shape[0]
    return {"precision": int((in_real > 0).sum()) / nf, "recall": int((in_fake > 0).sum()) / nr,
            "density": int(in_real.sum()) / (k * nf), "coverage": int((covered > 0).sum()) / nr}


def kid_subsets(n_real, n_fake, subsets=100, subset_size=1000, seed=0) -> list:
    """[(indices into real, indices into fake)] per subset: a function of the arguments only."""
    if subset_size < 2 or subset_size > min(n_real, n_fake):
        raise ValueError(f"kid: subset_size={subset_size} with {n_real} real and {n_fake} fake samples (2 .. the smaller set)")
    if subsets < 1:
        raise ValueError(f"kid: subsets={subsets} (at least 1)")
    rng = np.random.RandomState(seed)
    return [(rng.choice(n_real, subset_size, replace=False), rng.choice(n_fake, subset_size, replace=False)) for _ in range(subsets)]


def mmd2_unbiased(sum_xx, sum_yy, sum_xy, m) -> float:
    """The unbiased MMD^2 estimate of two sets of m samples from the kernel sums: xx and yy without their diagonals, xy whole."""
    return float(sum_xx) / (m * (m - 1)) + float(sum_yy) / (m * (m - 1)) - 2.0 * float(sum_xy) / (m * m)


def kid(real, fake, subsets=100, subset_size=1000, seed=0, chunks=0):
    """(mean, std) over ``subsets`` draws of ``subset_size`` samples per set of the unbiased MMD^2 with the kernel (x.y / D + 1)^3.
    Rows are gathered on the device, each subset is three kernel sums, the estimator runs on the host in fp64."""
    real, fake = _features(real, "real"), _features(fake, "fake")
    if real.shape[1] != fake.shape[1]:
        raise ValueError(f"metrics: real has {real.shape[1]} dimensions, fake {fake.shape[1]}")
    D, m = real.shape[1], int(subset_size)
    sums = []
    for ir, jf in kid_subsets(real.shape[0], fake.shape[0], subsets, m, seed):
        x = real[torch.from_numpy(ir).to(real.device)]
        y = fake[torch.from_numpy(jf).to(fake.device)]
        sums.append(torch.stack([poly_kernel_sum(x, x, 1.0 / D, 1.0, 3, True, chunks), poly_kernel_sum(y, y, 1.0 / D, 1.0, 3, True, chunks),
                                 poly_kernel_sum(x, y, 1.0 / D, 1.0, 3, False, chunks)]))
    est = np.array([mmd2_unbiased(*row, m) for row in torch.stack(sums).cpu().numpy()], np.float64)
    return float(est.mean()), float(est.std())


# ---- Inception Score ----------------------------------------------------------------------------------------------------------------
def softmax_score(x, weight, bias=None, chunks=0):
    """(ent fp64 0-dim, marg fp64 [C]) on the device: sum_n sum_c p log p and sum_n p_nc of p_n = softmax(x_n . w_c + bias_c), one
    ``mapdit_softmax_score`` call (fp32 only inside the dot products; bias, exp and log in fp64)."""
    x, weight = _features(x, "x"), _features(weight, "weight")
    if x.shape[1] != weight.shape[1]:
        raise ValueError(f"metrics: x has {x.shape[1]} dimensions, weight {weight.shape[1]}")
    N, D, C = x.shape[0], x.shape[1], weight.shape[0]
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or not bias.is_cuda:
            raise NotImplementedError("metrics: bias must be a CUDA tensor (HIP kernels, no CPU path)")
        if bias.dtype != torch.float32 or tuple(bias.shape) != (C,):
            raise ValueError(f"metrics: bias has shape {tuple(bias.shape)} and dtype {bias.dtype}, expected fp32 [{C}]")
        bias = bias.detach().contiguous()
    lib = L.lib()
    ent = torch.empty((), dtype=torch.float64, device=x.device)
    marg = torch.empty(C, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        ws = _workspace(lib.softmax_score_workspace_bytes(N, C, D, chunks), x.device, "softmax_score")
        lib.softmax_score(x.data_ptr(), N, weight.data_ptr(), C, D, L.ptr(bias), ent.data_ptr(), marg.data_ptr(), chunks, ws.data_ptr(), ws.numel(),
                          L.cur_stream())
    return ent, marg


def inception_score_from_sums(ent, marg, n) -> float:
    """exp(KL) of one split of n samples from its two sums, in fp64 on the host: with P_c = marg[c] (the class marginal times n),
    KL = (ent - sum_c P_c log(P_c / n)) / n, the mean over the samples of KL(p_n || p_bar).  A class with P_c = 0 adds 0."""
    p = np.asarray(marg, np.float64)
    nz = p > 0
    cross = float(np.sum(p[nz] * np.log(p[nz] / n)))
    return float(np.exp((float(ent) - cross) / n))


def inception_score(feat, fc_weight, fc_bias=None, split_size=5000, chunks=0):
    """(mean, std) over the splits of exp(mean_n KL(p_n || p_bar)): ADM's ``compute_inception_score`` - rows [i, i + split_size) per
    split, the last one may be short, ``np.std`` (N) over the splits.  ``feat`` fp32 [N, 2048] ``pool_3``, ``fc_weight`` fp32
    [1008, 2048] (``fid.classifier_head``), both CUDA tensors.  ``fc_bias=None``: the unbiased logits, as in ADM's evaluator and
    torch-fidelity's ``logits_unbiased``.  One ``mapdit_softmax_score`` call per split; the host finishes each in fp64."""
    feat, fc_weight = _features(feat, "feat"), _features(fc_weight, "fc_weight")
    if split_size < 1:
        raise ValueError(f"inception_score: split_size={split_size} (at least 1)")
    if feat.shape[0] < 1:
        raise ValueError("inception_score: no samples")
    sums = []
    for i in range(0, feat.shape[0], int(split_size)):
        rows = feat[i:i + int(split_size)]
        ent, marg = softmax_score(rows, fc_weight, fc_bias, chunks)
        sums.append((ent, marg, rows.shape[0]))
    scores = np.array([inception_score_from_sums(float(ent.cpu()), marg.cpu().numpy(), n) for ent, marg, n in sums], np.float64)
    return float(scores.mean()), float(scores.std())


# ---- the --metrics flags of fid.py and sample_fid.py --------------------------------------------------------------------------------
METRICS = ("fid", "fid_s", "isc", "pr", "kid")


def parse_metrics(text) -> tuple:
    """"fid,fid_s,isc,pr,kid" -> the names in METRICS order; None or "" is the default, ("fid",)."""
    names = [m.strip() for m in (text or "fid").split(",") if m.strip()]
    bad = [m for m in names if m not in METRICS]
    if bad or not names:
        raise ValueError(f"--metrics {text!r}: a comma-separated list of {', '.join(METRICS)}")
    return tuple(m for m in METRICS if m in names)


def add_metric_flags(p):
    p.add_argument("--metrics", default=None, help="comma-separated: fid (default), fid_s (sFID: the Fréchet distance of the spatial features), "
                                                   "isc (Inception Score), pr (precision, recall, density, coverage), kid")
    p.add_argument("--kid-subsets", type=int, default=100)
    p.add_argument("--kid-subset-size", type=int, default=1000, help="at most the smaller set's size")
