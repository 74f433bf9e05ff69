"""The yardstick of the DINOv2 feature network: an independent fp64 restatement, in numpy / torch on the CPU, of every step of
``mapdit_vit_features`` - the antialiased bicubic resize, the patch rows, the embed, LayerNorm, softmax attention, exact GELU, the
whole pre-norm ViT with LayerScale - and the generator of a random state dict in the public ``dinov2_vit*14`` layout.  Written from
the network's public description, step by step with explicit sums, not through torch.nn modules; tests/test_dinov2_cpu.py pins the
pieces to torch.nn.functional in fp64.

``emulate="f16" | "bf16"`` rounds every operand the kernels round to 16 bits - the patch rows, the LayerNorm output, the qkv rows,
the softmax probabilities (relative to the row maximum), the attention output, fc1's output, the GELU output and every linear weight -
and keeps everything else fp64, so that what is left between it and the kernels is fp32 accumulation; ``emulate=None`` is the exact
network."""
import math

import numpy as np
import torch

PATCH = 14
PATCH_K = 592
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
_DT = {"f16": torch.float16, "bf16": torch.bfloat16}
UNIT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8, None: 0.0}       # the relative rounding error of the operand formats


def rnd(t, emulate):
    """fp64 -> the 16-bit operand format (fp16 saturated at +-65504, as the kernels convert) -> fp64."""
    if emulate is None:
        return t
    t = torch.as_tensor(t, dtype=torch.float64)
    if emulate == "f16":
        t = t.clamp(-65504.0, 65504.0)
    return t.to(torch.float32).to(_DT[emulate]).to(torch.float64)


# ---- the resize -----------------------------------------------------------------------------------------------------------------------
def _cubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def aa_matrix(I, S):
    """fp64 [S, I]: row d holds the normalised weights of destination d - F.interpolate(mode="bicubic", antialias=True,
    align_corners=False): scale = I / S, centre = scale (d + 1/2), support = 2 max(scale, 1), taps [trunc(centre - support + 1/2),
    trunc(centre + support + 1/2)) cut to the image, weight cubic((t + 1/2 - centre) / max(scale, 1))."""
    scale = I / S
    wide = max(scale, 1.0)
    m = np.zeros((S, I), np.float64)
    for d in range(S):
        centre = scale * (d + 0.5)
        lo = max(int(centre - 2.0 * wide + 0.5), 0)
        hi = min(int(centre + 2.0 * wide + 0.5), I)
        w = np.array([_cubic((t + 0.5 - centre) / wide) for t in range(lo, hi)], np.float64)
        m[d, lo:hi] = w / w.sum()
    return m


def resize_aa(x, S):
    """fp64 [N, C, H, W] -> [N, C, S, S]: the horizontal pass, then the vertical one; no clamping."""
    x = np.asarray(x, np.float64)
    my, mx = aa_matrix(x.shape[2], S), aa_matrix(x.shape[3], S)
    return np.einsum("yh,nchx->ncyx", my, np.einsum("xw,nchw->nchx", mx, x))


def pixels_255(images):
    """uint8 [N, H, W, 3] or float [N, 3, H, W] in [-1, 1] -> fp64 [N, 3, H, W] in 0 .. 255."""
    a = images.numpy() if isinstance(images, torch.Tensor) else np.asarray(images)
    if a.dtype == np.uint8:
        return a.astype(np.float64).transpose(0, 3, 1, 2)
    return (a.astype(np.float64) + 1.0) * 127.5


def patch_rows(images, S, emulate=None):
    """-> fp64 [N * P, 592]: resize on 0 .. 255, / 255, - mean, / std, the patches in (gy, gx) order, each (c, py, px), the tail zero."""
    x = resize_aa(pixels_255(images), S) / 255.0
    x = (x - np.array(MEAN)[None, :, None, None]) / np.array(STD)[None, :, None, None]
    N, g = x.shape[0], S // PATCH
    p = x.reshape(N, 3, g, PATCH, g, PATCH).transpose(0, 2, 4, 1, 3, 5).reshape(N * g * g, 3 * PATCH * PATCH)
    out = np.zeros((N * g * g, PATCH_K), np.float64)
    out[:, :3 * PATCH * PATCH] = p
    return rnd(torch.from_numpy(out), emulate)


# ---- the pieces -------------------------------------------------------------------------------------------------------------------------
def linear(x, w, b, emulate=None):
    """x [M, K] (taken as it is: the caller rounds what the kernels round), w [O, K] rounded here, b fp64."""
    return x @ rnd(w.double(), emulate).T + b.double()


def embed(patch, cls, pos, N):
    """patch [N * P, D], cls [D], pos [1 + P, D] -> [N, 1 + P, D]."""
    D = patch.shape[1]
    tok = torch.cat([cls.double().reshape(1, 1, D).expand(N, 1, D), patch.reshape(N, -1, D)], dim=1)
    return tok + pos.double()[None]


def layernorm(x, w, b, eps=1e-6):
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * w.double() + b.double()


def attention(qkv, heads, emulate=None, absolute=False):
    """qkv [N, T, 3 D] (q | k | v thirds, head h the columns [64 h, 64 h + 64) of each) -> [N, T, D]: softmax(q k^T / 8) v.  With
    ``absolute`` also sum_j p_j |v_j| / sum_j p_j per output element: the scale of an output's rounding error."""
    N, T, D3 = qkv.shape
    D = D3 // 3
    hd = D // heads
    q, k, v = (qkv[:, :, i * D:(i + 1) * D].reshape(N, T, heads, hd).permute(0, 2, 1, 3) for i in range(3))
    s = torch.einsum("nhqd,nhkd->nhqk", q, k) / math.sqrt(hd)
    p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    den = p.sum(dim=-1, keepdim=True)
    pr = rnd(p, emulate)
    o = (torch.einsum("nhqk,nhkd->nhqd", pr, v) / den).permute(0, 2, 1, 3).reshape(N, T, D)
    if not absolute:
        return o
    return o, (torch.einsum("nhqk,nhkd->nhqd", pr, v.abs()) / den).permute(0, 2, 1, 3).reshape(N, T, D)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


# ---- the network ------------------------------------------------------------------------------------------------------------------------
def make_state_dict(dim=128, depth=2, mlp_dim=512, grid=37, seed=0, gamma=(0.05, 1.0)):
    """A random state dict in the public layout (fp32 tensors): linears at 1 / sqrt(fan_in), LayerNorm weights around 1, LayerScale
    gammas uniform in ``gamma``, a ``mask_token`` the loader must ignore."""
    g = torch.Generator().manual_seed(seed)

    def n(*shape, s=1.0):
        return (torch.randn(*shape, generator=g, dtype=torch.float64) * s).float()

    def u(*shape, lo=0.0, hi=1.0):
        return (lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64)).float()

    sd = {"cls_token": n(1, 1, dim, s=0.5), "pos_embed": n(1, 1 + grid * grid, dim, s=0.3), "mask_token": n(1, dim),
          "patch_embed.proj.weight": n(dim, 3, PATCH, PATCH, s=1.0 / math.sqrt(3 * PATCH * PATCH)), "patch_embed.proj.bias": n(dim, s=0.1)}
    for i in range(depth):
        p = f"blocks.{i}."
        sd[p + "norm1.weight"], sd[p + "norm1.bias"] = u(dim, lo=0.7, hi=1.3), n(dim, s=0.1)
        sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"] = n(3 * dim, dim, s=1.5 / math.sqrt(dim)), n(3 * dim, s=0.1)
        sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"] = n(dim, dim, s=1.0 / math.sqrt(dim)), n(dim, s=0.1)
        sd[p + "ls1.gamma"] = u(dim, lo=gamma[0], hi=gamma[1])
        sd[p + "norm2.weight"], sd[p + "norm2.bias"] = u(dim, lo=0.7, hi=1.3), n(dim, s=0.1)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = n(mlp_dim, dim, s=1.0 / math.sqrt(dim)), n(mlp_dim, s=0.1)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = n(dim, mlp_dim, s=1.0 / math.sqrt(mlp_dim)), n(dim, s=0.1)
        sd[p + "ls2.gamma"] = u(dim, lo=gamma[0], hi=gamma[1])
    sd["norm.weight"], sd["norm.bias"] = u(dim, lo=0.7, hi=1.3), n(dim, s=0.1)
    return sd


def interpolate_pos(pos_embed, g, offset=0.1):
    """The hub models' position table at a g x g grid, restated with an explicit bicubic (a = -0.75, torch's non-antialiased
    kernel, border taps clamped) at source coordinate (d + 1/2) / s - 1/2 with s = (g + offset) / M: the scale FACTOR, not the size
    ratio, places the samples.  g == M: the table itself.  fp64 [1 + g * g, D]."""
    pos = pos_embed.double()[0]
    M = math.isqrt(pos.shape[0] - 1)
    if g == M:
        return pos
    D = pos.shape[1]
    grid = pos[1:].reshape(M, M, D).numpy()
    s = (g + offset) / M
    w = np.zeros((g, M), np.float64)
    for d in range(g):
        c = (d + 0.5) / s - 0.5
        i0 = math.floor(c)
        t = c - i0
        for k in range(-1, 3):
            w[d, min(max(i0 + k, 0), M - 1)] += _cubic(k - t, a=-0.75)
    out = np.einsum("yh,xw,hwd->yxd", w, w, grid).reshape(g * g, D)
    return torch.cat([pos[:1], torch.from_numpy(out)], dim=0)


def vit_forward(sd, images, image_size, emulate=None, offset=0.1):
    """-> fp64 [N, D]: the CLS row after the final LayerNorm."""
    D = sd["cls_token"].shape[-1]
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    heads = D // 64
    rows = patch_rows(images, image_size, emulate)
    N = rows.shape[0] // (image_size // PATCH) ** 2
    wp = torch.zeros(D, PATCH_K, dtype=torch.float64)
    wp[:, :3 * PATCH * PATCH] = sd["patch_embed.proj.weight"].double().reshape(D, -1)
    pos = interpolate_pos(sd["pos_embed"], image_size // PATCH, offset).float().double()      # (the table is held in fp32)
    x = embed(linear(rows, wp, sd["patch_embed.proj.bias"], emulate), sd["cls_token"].reshape(D), pos, N)
    for i in range(depth):
        p = f"blocks.{i}."
        h = rnd(layernorm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"]), emulate)
        qkv = rnd(linear(h, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"], emulate), emulate)
        a = rnd(attention(qkv, heads, emulate), emulate)
        x = x + sd[p + "ls1.gamma"].double() * linear(a, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"], emulate)
        h = rnd(layernorm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"]), emulate)
        f = rnd(linear(h, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"], emulate), emulate)
        f = rnd(gelu(f), emulate)
        x = x + sd[p + "ls2.gamma"].double() * linear(f, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"], emulate)
    return layernorm(x[:, 0], sd["norm.weight"], sd["norm.bias"])


def e_emul(fn, emulate):
    """max |fn(emulate) - fn(None)| / max |fn(None)|: what the 16-bit operands alone cost a case."""
    exact = fn(None)
    return float((fn(emulate) - exact).abs().max() / exact.abs().max())


# ---- the cases of the GPU tests: built here once, so that tests/test_dinov2_cpu.py measures e_emul on the very inputs they run -------
RESIZE_CASES = {"32to28": (32, 32, 28), "64to28": (64, 64, 28), "16to28": (16, 16, 28), "40x24to28": (40, 24, 28), "256to224": (256, 256, 224),
                "28to28": (28, 28, 28)}
ATTN_T = (2, 5, 63, 64, 65, 256, 257, 258, 513)
WALK_CASES = {"walk28": (28, 3), "walk224": (224, 2)}         # image_size, N (dim 128, 2 heads, depth 2, mlp 512)


def case_images(name, n=2, f32=False):
    """uint8 [n, H, W, 3] of a resize case: a smooth ramp plus noise, so that a resize has something to average; ``f32``: fp32
    [n, 3, H, W] in [-1, 1] holding the same picture (v / 127.5 - 1 rounded to fp32)."""
    H, W, _ = RESIZE_CASES[name]
    g = torch.Generator().manual_seed(1000 + H * 7 + W)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    base = 128 + 80 * torch.sin(yy / 5.0)[None, :, :, None] * torch.cos(xx / 7.0)[None, :, :, None]
    img = (base + 60 * torch.randn(n, H, W, 3, generator=g, dtype=torch.float64)).clamp(0, 255).round().to(torch.uint8)
    if not f32:
        return img
    return (img.permute(0, 3, 1, 2).double() / 127.5 - 1.0).float().contiguous()


def case_layernorm(D, M=6):
    """fp32 rows with a 300-fold outlier in one channel (DINOv2's residual stream has such), LayerNorm weight and bias."""
    g = torch.Generator().manual_seed(2000 + D)
    x = torch.randn(M, D, generator=g, dtype=torch.float64)
    x[:, 7] = 300.0 * (1.0 + 0.1 * torch.randn(M, generator=g, dtype=torch.float64))
    w = 0.7 + 0.6 * torch.rand(D, generator=g, dtype=torch.float64)
    b = 0.1 * torch.randn(D, generator=g, dtype=torch.float64)
    return x.float(), w.float(), b.float()


def case_attention(T, prec, N=3, heads=2, scale=1.0):
    """qkv fp64 [N, T, 3 D] holding values of the operand format.  ``scale`` multiplies q and k: 9 puts logits near +-80."""
    D = 64 * heads
    g = torch.Generator().manual_seed(3000 + T)
    qkv = torch.randn(N, T, 3 * D, generator=g, dtype=torch.float64)
    qkv[:, :, :2 * D] *= scale
    return rnd(qkv, prec)


def case_gelu(prec):
    g = torch.Generator().manual_seed(4000)
    x = torch.cat([torch.tensor([0.0, -0.0, 10.0, -10.0, 65504.0, -65504.0, 300.0, -300.0], dtype=torch.float64),
                   3.0 * torch.randn(1016, generator=g, dtype=torch.float64)])
    return rnd(x, prec)


def case_walk(name):
    size, n = WALK_CASES[name]
    g = torch.Generator().manual_seed(5000 + size)
    return make_state_dict(128, 2, 512, seed=11), torch.randint(0, 256, (n, size + 8, size + 8, 3), generator=g, dtype=torch.uint8), size


def measure_e_emul(prec) -> dict:
    """case name -> e_emul for one operand format: everything the GPU tests hold to 2 x e_emul."""
    out = {}
    for name, (_, _, S) in RESIZE_CASES.items():
        out[f"prepare_{name}"] = e_emul(lambda e: patch_rows(case_images(name), S, e), prec)
    out["prepare_f32_32to28"] = e_emul(lambda e: patch_rows(case_images("32to28", f32=True), 28, e), prec)
    for D in (128, 1024):
        x, w, b = case_layernorm(D)
        out[f"layernorm_{D}"] = e_emul(lambda e: rnd(layernorm(x.double(), w, b), e), prec)
    for T in ATTN_T:
        qkv = case_attention(T, prec)
        out[f"attention_{T}"] = e_emul(lambda e: rnd(attention(qkv, 2, e), e), prec)
    qkv = case_attention(65, prec, scale=9.0)
    out["attention_65_big"] = e_emul(lambda e: rnd(attention(qkv, 2, e), e), prec)
    x = case_gelu(prec)
    out["gelu"] = e_emul(lambda e: rnd(gelu(x), e), prec)
    for name in WALK_CASES:
        sd, images, size = case_walk(name)
        out[name] = e_emul(lambda e: vit_forward(sd, images, size, e), prec)
    return out
