"""Plain-torch CPU restatement of the AutoencoderKL decoder (post_quant_conv + decoder) from its state-dict keys: the reference of the
VAE tests.  fp64 throughout; ``operand_dtype`` rounds every conv / linear / matmul operand to that 16-bit format and back, which
emulates what 16-bit MFMA operands with wide accumulation do - the tolerances of the GPU tests come from it, never from the kernels.
Independent of map-dit_amd/vae.py on purpose: it builds its own key names and shapes."""
import json
import struct

import torch
import torch.nn.functional as F

DEFAULT = dict(block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=4, out_channels=3)
TINY = dict(block_out_channels=(64, 64, 128), layers_per_block=1, latent_channels=4, out_channels=3)
ATTN = "decoder.mid_block.attentions.0."
OLD_NAMES = {"to_q": "query", "to_k": "key", "to_v": "value", "to_out.0": "proj_attn"}


def _resnets(cfg):
    """(prefix, cin, cout) of every resnet in execution order."""
    ch = list(reversed(cfg["block_out_channels"]))
    out = [("decoder.mid_block.resnets.0", ch[0], ch[0]), ("decoder.mid_block.resnets.1", ch[0], ch[0])]
    cin = ch[0]
    for i, c in enumerate(ch):
        for j in range(cfg["layers_per_block"] + 1):
            out.append((f"decoder.up_blocks.{i}.resnets.{j}", cin, c))
            cin = c
    return out


def init_state_dict(cfg=DEFAULT, seed=0, generation="new", conv_attention=False):
    """Random weights from a seed: uniform fan-in-scaled conv / linear weights, biases in +-0.1, gamma = 1 + 0.2 randn, beta = 0.2 randn.
    ``generation="old"``: the attention keys query / key / value / proj_attn; ``conv_attention``: their weights as [C, C, 1, 1]."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(name, cout, cin, k):
        bound = (3.0 / (cin * k * k)) ** 0.5
        sd[name + ".weight"] = (torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * bound
        sd[name + ".bias"] = (torch.rand(cout, generator=g) * 2 - 1) * 0.1

    def norm(name, c):
        sd[name + ".weight"] = 1 + 0.2 * torch.randn(c, generator=g)
        sd[name + ".bias"] = 0.2 * torch.randn(c, generator=g)

    ch = list(reversed(cfg["block_out_channels"]))
    lat = cfg["latent_channels"]
    conv("post_quant_conv", lat, lat, 1)
    conv("decoder.conv_in", ch[0], lat, 3)
    for prefix, cin, cout in _resnets(cfg):
        norm(prefix + ".norm1", cin)
        conv(prefix + ".conv1", cout, cin, 3)
        norm(prefix + ".norm2", cout)
        conv(prefix + ".conv2", cout, cout, 3)
        if cin != cout:
            conv(prefix + ".conv_shortcut", cout, cin, 1)
    norm(ATTN + "group_norm", ch[0])
    for name in ("to_q", "to_k", "to_v", "to_out.0"):
        conv(ATTN + "@" + name, ch[0], ch[0], 1)
    for i in range(len(ch) - 1):
        conv(f"decoder.up_blocks.{i}.upsamplers.0.conv", ch[i], ch[i], 3)
    norm("decoder.conv_norm_out", ch[-1])
    conv("decoder.conv_out", cfg["out_channels"], ch[-1], 3)
    out = {}
    for k, v in sd.items():                                 # insertion order = execution-independent; rename the attention linears last
        if "@" in k:
            head, leaf = k.split("@")[1].rsplit(".", 1)
            k = ATTN + (OLD_NAMES[head] if generation == "old" else head) + "." + leaf
            if leaf == "weight" and not conv_attention:
                v = v[:, :, 0, 0].clone()
        out[k] = v
    return out


def _rnd(t, operand_dtype):
    return t if operand_dtype is None else t.to(operand_dtype).to(torch.float64)


def decode(sd, z, cfg=None, norm_num_groups=32, eps=1e-6, operand_dtype=None):
    """z [N, latent, h, w] -> [N, out_channels, h * 2^(blocks-1), w * 2^(blocks-1)] in fp64."""
    sd = {k: v.to(torch.float64) for k, v in sd.items() if not k.startswith(("encoder.", "quant_conv."))}
    for new, old in OLD_NAMES.items():                      # accept either generation of attention keys
        for leaf in ("weight", "bias"):
            if ATTN + f"{old}.{leaf}" in sd:
                sd[ATTN + f"{new}.{leaf}"] = sd.pop(ATTN + f"{old}.{leaf}")
    if cfg is None:
        nb = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("decoder.up_blocks."))
        cfg = dict(block_out_channels=tuple(reversed([sd[f"decoder.up_blocks.{i}.resnets.0.conv1.weight"].shape[0] for i in range(nb)])),
                   layers_per_block=max(int(k.split(".")[4]) for k in sd if k.startswith("decoder.up_blocks.0.resnets.")),
                   latent_channels=sd["decoder.conv_in.weight"].shape[1], out_channels=sd["decoder.conv_out.weight"].shape[0])
    G = norm_num_groups

    def conv(x, name, pad):
        return F.conv2d(_rnd(x, operand_dtype), _rnd(sd[name + ".weight"], operand_dtype), sd[name + ".bias"], padding=pad)

    def gn(x, name):
        return F.group_norm(x, G, sd[name + ".weight"], sd[name + ".bias"], eps)

    def resnet(x, p, cin, cout):
        h = conv(F.silu(gn(x, p + ".norm1")), p + ".conv1", 1)
        h = conv(F.silu(gn(h, p + ".norm2")), p + ".conv2", 1)
        return (conv(x, p + ".conv_shortcut", 0) if cin != cout else x) + h

    def attention(x):
        n, c, hh, ww = x.shape
        t = gn(x, ATTN + "group_norm").reshape(n, c, hh * ww).transpose(1, 2)                    # [N, T, C]

        def lin(v, name):
            w = sd[ATTN + name + ".weight"].reshape(c, c)
            return _rnd(v, operand_dtype) @ _rnd(w, operand_dtype).t() + sd[ATTN + name + ".bias"]
        q, k, v = lin(t, "to_q"), lin(t, "to_k"), lin(t, "to_v")
        s = _rnd(q, operand_dtype) @ _rnd(k, operand_dtype).transpose(1, 2) / c ** 0.5
        o = _rnd(torch.softmax(s, dim=-1), operand_dtype) @ _rnd(v, operand_dtype)
        o = lin(o, "to_out.0")
        return x + o.transpose(1, 2).reshape(n, c, hh, ww)

    x = conv(z.to(torch.float64), "post_quant_conv", 0)
    x = conv(x, "decoder.conv_in", 1)
    rs = _resnets(cfg)
    x = resnet(x, *rs[0])
    x = attention(x)
    x = resnet(x, *rs[1])
    per = cfg["layers_per_block"] + 1
    nb = len(cfg["block_out_channels"])
    for i in range(nb):
        for r in rs[2 + i * per: 2 + (i + 1) * per]:
            x = resnet(x, *r)
        if i < nb - 1:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = conv(x, f"decoder.up_blocks.{i}.upsamplers.0.conv", 1)
    return conv(F.silu(gn(x, "decoder.conv_norm_out")), "decoder.conv_out", 1)


ST_NAMES = {torch.float32: "F32", torch.float16: "F16", torch.bfloat16: "BF16"}


def write_safetensors(sd, path, dtype_names=None):
    """A minimal writer of the safetensors container for the tests: 8-byte little-endian header length, JSON header, raw tensors.
    ``dtype_names`` overrides the header's dtype string per key (to write a file the reader must refuse)."""
    header, blobs, off = {}, [], 0
    for k, v in sd.items():
        v = v.contiguous()
        raw = v.view(torch.uint8).numpy().tobytes() if v.numel() else b""
        header[k] = {"dtype": (dtype_names or {}).get(k, ST_NAMES[v.dtype]), "shape": list(v.shape), "data_offsets": [off, off + len(raw)]}
        blobs.append(raw)
        off += len(raw)
    hj = json.dumps(header).encode()
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(hj)) + hj + b"".join(blobs))
