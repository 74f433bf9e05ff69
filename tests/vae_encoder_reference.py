"""Plain-torch CPU restatement of the AutoencoderKL encoder (encoder + quant_conv) from its state-dict keys: the reference of the
VAE encoder tests.  fp64 throughout; ``operand_dtype`` rounds every conv / linear / matmul operand to that 16-bit format and back, as
vae_reference.decode does - the tolerances of the GPU tests come from it, never from the kernels.  Independent of map-dit_amd/vae.py
on purpose: it builds its own key names and shapes.  The downsample is written literally as the pad + strided convolution of
Downsample2D(padding=0)."""
import torch
import torch.nn.functional as F

from vae_reference import DEFAULT, OLD_NAMES, TINY, _rnd  # noqa: F401  (DEFAULT / TINY: the configs the tests name)

ATTN = "encoder.mid_block.attentions.0."


def _resnets(cfg):
    """(prefix, cin, cout) of every resnet in execution order: the down blocks, then the mid block's two."""
    ch = list(cfg["block_out_channels"])
    out, cin = [], ch[0]
    for i, c in enumerate(ch):
        for j in range(cfg["layers_per_block"]):
            out.append((f"encoder.down_blocks.{i}.resnets.{j}", cin, c))
            cin = c
    return out + [("encoder.mid_block.resnets.0", cin, cin), ("encoder.mid_block.resnets.1", cin, cin)]


def init_encoder_state_dict(cfg=DEFAULT, seed=0, generation="new", conv_attention=False):
    """Random weights from a seed, in the pattern of vae_reference.init_state_dict: uniform fan-in-scaled conv / linear weights, biases in
    +-0.1, gamma = 1 + 0.2 randn, beta = 0.2 randn.  ``generation="old"``: the attention keys query / key / value / proj_attn;
    ``conv_attention``: their weights as [C, C, 1, 1].  ``cfg["out_channels"]`` is the image's channel count."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(name, cout, cin, k):
        bound = (3.0 / (cin * k * k)) ** 0.5
        sd[name + ".weight"] = (torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * bound
        sd[name + ".bias"] = (torch.rand(cout, generator=g) * 2 - 1) * 0.1

    def norm(name, c):
        sd[name + ".weight"] = 1 + 0.2 * torch.randn(c, generator=g)
        sd[name + ".bias"] = 0.2 * torch.randn(c, generator=g)

    ch = list(cfg["block_out_channels"])
    lat2 = 2 * cfg["latent_channels"]
    conv("encoder.conv_in", ch[0], cfg["out_channels"], 3)
    for prefix, cin, cout in _resnets(cfg):
        norm(prefix + ".norm1", cin)
        conv(prefix + ".conv1", cout, cin, 3)
        norm(prefix + ".norm2", cout)
        conv(prefix + ".conv2", cout, cout, 3)
        if cin != cout:
            conv(prefix + ".conv_shortcut", cout, cin, 1)
    for i in range(len(ch) - 1):
        conv(f"encoder.down_blocks.{i}.downsamplers.0.conv", ch[i], ch[i], 3)
    norm(ATTN + "group_norm", ch[-1])
    for name in ("to_q", "to_k", "to_v", "to_out.0"):
        conv(ATTN + "@" + name, ch[-1], ch[-1], 1)
    norm("encoder.conv_norm_out", ch[-1])
    conv("encoder.conv_out", lat2, ch[-1], 3)
    conv("quant_conv", lat2, lat2, 1)
    out = {}
    for k, v in sd.items():
        if "@" in k:
            head, leaf = k.split("@")[1].rsplit(".", 1)
            k = ATTN + (OLD_NAMES[head] if generation == "old" else head) + "." + leaf
            if leaf == "weight" and not conv_attention:
                v = v[:, :, 0, 0].clone()
        out[k] = v
    return out


def downsample(x, w, b):
    """Downsample2D(padding=0): one zero row below, one zero column to the right, then 3 x 3 / stride 2 without padding."""
    return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)


def encode(sd, x, cfg=None, operand_dtype=None, norm_num_groups=32, eps=1e-6):
    """x [N, C, H, W] in [-1, 1] -> (mean, logvar), each [N, latent, H / s, W / s] in fp64; logvar clamped to [-30, 20]."""
    sd = {k: v.to(torch.float64) for k, v in sd.items() if not k.startswith(("decoder.", "post_quant_conv."))}
    for new, old in OLD_NAMES.items():                      # accept either generation of attention keys
        for leaf in ("weight", "bias"):
            if ATTN + f"{old}.{leaf}" in sd:
                sd[ATTN + f"{new}.{leaf}"] = sd.pop(ATTN + f"{old}.{leaf}")
    if cfg is None:
        nb = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.down_blocks."))
        cfg = dict(block_out_channels=tuple(sd[f"encoder.down_blocks.{i}.resnets.0.conv1.weight"].shape[0] for i in range(nb)),
                   layers_per_block=1 + max(int(k.split(".")[4]) for k in sd if k.startswith("encoder.down_blocks.0.resnets.")),
                   latent_channels=sd["encoder.conv_out.weight"].shape[0] // 2, out_channels=sd["encoder.conv_in.weight"].shape[1])
    G = norm_num_groups

    def conv(t, name, pad):
        return F.conv2d(_rnd(t, operand_dtype), _rnd(sd[name + ".weight"], operand_dtype), sd[name + ".bias"], padding=pad)

    def gn(t, name):
        return F.group_norm(t, G, sd[name + ".weight"], sd[name + ".bias"], eps)

    def resnet(t, p, cin, cout):
        h = conv(F.silu(gn(t, p + ".norm1")), p + ".conv1", 1)
        h = conv(F.silu(gn(h, p + ".norm2")), p + ".conv2", 1)
        return (conv(t, p + ".conv_shortcut", 0) if cin != cout else t) + h

    def attention(t):
        n, c, hh, ww = t.shape
        u = gn(t, ATTN + "group_norm").reshape(n, c, hh * ww).transpose(1, 2)                    # [N, T, C]

        def lin(v, name):
            w = sd[ATTN + name + ".weight"].reshape(c, c)
            return _rnd(v, operand_dtype) @ _rnd(w, operand_dtype).t() + sd[ATTN + name + ".bias"]
        q, k, v = lin(u, "to_q"), lin(u, "to_k"), lin(u, "to_v")
        s = _rnd(q, operand_dtype) @ _rnd(k, operand_dtype).transpose(1, 2) / c ** 0.5
        o = _rnd(torch.softmax(s, dim=-1), operand_dtype) @ _rnd(v, operand_dtype)
        return t + lin(o, "to_out.0").transpose(1, 2).reshape(n, c, hh, ww)

    t = conv(x.to(torch.float64), "encoder.conv_in", 1)
    rs = _resnets(cfg)
    per, nb = cfg["layers_per_block"], len(cfg["block_out_channels"])
    for i in range(nb):
        for r in rs[i * per:(i + 1) * per]:
            t = resnet(t, *r)
        if i < nb - 1:
            p = f"encoder.down_blocks.{i}.downsamplers.0.conv"
            t = downsample(_rnd(t, operand_dtype), _rnd(sd[p + ".weight"], operand_dtype), sd[p + ".bias"])
    t = resnet(t, *rs[-2])
    t = attention(t)
    t = resnet(t, *rs[-1])
    t = conv(F.silu(gn(t, "encoder.conv_norm_out")), "encoder.conv_out", 1)
    mean, logvar = conv(t, "quant_conv", 0).chunk(2, dim=1)
    return mean, torch.clamp(logvar, -30.0, 20.0)
