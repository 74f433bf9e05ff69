"""The yardstick of the Inception Score and of the spatial (sFID) features: numpy fp64 restatements written from the definitions.

    softmax_sums(x, w, bias)           (ent, marg, logp): sum_n sum_c p log p, sum_n p_nc and the log-probabilities themselves
    inception_score(x, w, bias, split) ADM's compute_inception_score on the softmax of x w^T (+ bias): (mean, std, per-split scores)
    log_is_bound(x, w, logp)           the bound of the GPU tests on |log IS - log IS_64| for fp32 dot products (derivation there)
    spatial(sd, images, image_size)    the first 7 channels of the Mixed_6d.branch1x1 unit in (h, w, c) order, fp64 [N, hs * ws * 7],
                                       by the walk of tests/inception_reference.py up to that block
"""
import numpy as np
import torch
import torch.nn.functional as F

import inception_reference as R

SPATIAL_CHANNELS = 7


def softmax_sums(x, w, bias=None):
    """fp64 throughout: logits l = x w^T (+ bias), log p = l - logsumexp(l) -> (sum p log p, sum_n p, log p)."""
    l = np.asarray(x, np.float64) @ np.asarray(w, np.float64).T
    if bias is not None:
        l = l + np.asarray(bias, np.float64)[None, :]
    m = l.max(axis=1, keepdims=True)
    logp = l - (m + np.log(np.exp(l - m).sum(axis=1, keepdims=True)))
    p = np.exp(logp)
    return float((p * logp).sum()), p.sum(axis=0), logp


def split_score(logp):
    """exp(mean_n KL(p_n || p_bar)) of one split, ADM's formula on the probabilities: sum_c p (log p - log mean_n p)."""
    p = np.exp(logp)
    with np.errstate(divide="ignore", invalid="ignore"):
        kl = p * (logp - np.log(p.mean(axis=0, keepdims=True)))
    return float(np.exp(np.where(p > 0, kl, 0.0).sum(axis=1).mean()))


def inception_score(x, w, bias=None, split_size=5000):
    logp = softmax_sums(x, w, bias)[2]
    scores = np.array([split_score(logp[i:i + split_size]) for i in range(0, len(logp), split_size)])
    return float(scores.mean()), float(scores.std()), scores


def log_is_bound(x, w, logp):
    """|log IS - log IS_64| when every logit carries an error of at most eps = gamma_K max_{n,c} sum_k |x_nk w_ck| (gamma_K =
    K u / (1 - K u), u = 2^-24: an fp32 chain of K steps on exact products): each log p_nc then moves by at most 2 eps (the logit and
    the log-sum-exp), each p_nc and each marginal by a factor within e^{+-2 eps}, and with T = max |log p - log p_bar|
        |log IS - log IS_64| = |mean_n sum_c (p' (log p' - log p_bar') - p (log p - log p_bar))| <= 4 eps + (e^{2 eps} - 1) T.
    -> (bound, eps, T), all from the reference's own numbers."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    K = x.shape[1]
    gamma = K * 2.0 ** -24 / (1.0 - K * 2.0 ** -24)
    eps = gamma * float((np.abs(x) @ np.abs(w).T).max())
    logpbar = np.log(np.exp(logp).mean(axis=0, keepdims=True))
    T = float(np.abs(logp - logpbar).max())
    return 4.0 * eps + np.expm1(2.0 * eps) * T, eps, T


def prepare(images, size):
    """inception_reference.prepare at another square size."""
    x = images.permute(0, 3, 1, 2).to(torch.float64)
    x = F.interpolate(x, size=(size, size), mode="bilinear", align_corners=False)
    return x / 255.0 * 2.0 - 1.0


@torch.no_grad()
def spatial(sd, images, image_size=299, operand_dtype=None) -> torch.Tensor:
    """fp64 [N, hs * ws * 7]: the stem and Mixed_5b .. Mixed_6c of the restatement, then Mixed_6d's branch1x1 unit alone (convolution,
    BatchNorm, ReLU), its first 7 channels, (h, w, c) order.  ``operand_dtype`` as in inception_reference.features."""
    net = R._Net(sd, operand_dtype=operand_dtype)
    x = R.prepare(images) if image_size == 299 else prepare(images, image_size)
    x = net.unit(x, "Conv2d_1a_3x3", 3, 32, 3, 2)
    x = net.unit(x, "Conv2d_2a_3x3", 32, 32, 3)
    x = net.unit(x, "Conv2d_2b_3x3", 32, 64, 3, 1, 1)
    x = net.max2(x)
    x = net.unit(x, "Conv2d_3b_1x1", 64, 80)
    x = net.unit(x, "Conv2d_4a_3x3", 80, 192, 3)
    x = net.max2(x)
    x = net.inception_a(x, "Mixed_5b", 192, 32)
    x = net.inception_a(x, "Mixed_5c", 256, 64)
    x = net.inception_a(x, "Mixed_5d", 288, 64)
    x = net.inception_b(x, "Mixed_6a")
    x = net.inception_c(x, "Mixed_6b", 128)
    x = net.inception_c(x, "Mixed_6c", 160)
    b1 = net.unit(x, "Mixed_6d.branch1x1", 768, 192)
    return b1[:, :SPATIAL_CHANNELS].permute(0, 2, 3, 1).reshape(b1.shape[0], -1)
