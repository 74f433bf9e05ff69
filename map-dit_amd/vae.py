"""Native VAE decoder: ``vae.decode(samples).sample`` of the reference's sampler scripts (sample.py:72-74, sample_fid.py:83-84,
sample_ema.py:73) on ``libmapdit_hip.so`` - ``mapdit_vae_decode`` (include/mapdit.h), for weights in the ``AutoencoderKL`` layout
(Stable Diffusion's decoder; the defaults are those of ``stabilityai/sd-vae-ft-mse``).  The encoder is not built: ``encoder.*`` and
``quant_conv.*`` are ignored.  Parity with the hub weights is unpinned: the network is restated from its public description and
checked against an independent restatement (tests/vae_reference.py), not against the ``diffusers`` package.
"""
from __future__ import annotations

import ctypes as C
import json
import re
import struct
from types import SimpleNamespace

import torch

from . import _lib as L

PRECISIONS = {"f16": torch.float16, "bf16": torch.bfloat16}
# the older generation of attention keys (what the hub's own file carries) -> the current one
_OLD_ATTN = {"query": "to_q", "key": "to_k", "value": "to_v", "proj_attn": "to_out.0"}
_ATTN = "decoder.mid_block.attentions.0."


# ---- safetensors: 8-byte little-endian header length, a JSON header, raw little-endian tensors -------------------------------------
_ST_DTYPES = {"F32": (torch.float32, 4), "F16": (torch.float16, 2), "BF16": (torch.bfloat16, 2)}


def read_safetensors(path) -> dict:
    """A reader of our own (the package is not a dependency).  F32, F16 and BF16 tensors; anything else, a short file or offsets
    that do not fit is an error, never a guess."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 8:
        raise ValueError(f"{path}: truncated safetensors file ({len(raw)} bytes: no header length)")
    (n,) = struct.unpack("<Q", raw[:8])
    if n > len(raw) - 8:
        raise ValueError(f"{path}: the safetensors header ({n} bytes) overruns the file ({len(raw)} bytes)")
    try:
        header = json.loads(raw[8:8 + n].decode("utf-8"))
    except (UnicodeDecodeError, json.JSONDecodeError) as e:
        raise ValueError(f"{path}: the safetensors header is not JSON ({e})") from None
    if not isinstance(header, dict):
        raise ValueError(f"{path}: the safetensors header is not a JSON object")
    data = memoryview(raw)[8 + n:]
    out = {}
    for name, meta in header.items():
        if name == "__metadata__":
            continue
        try:
            dtype, shape, (lo, hi) = meta["dtype"], [int(s) for s in meta["shape"]], meta["data_offsets"]
        except (KeyError, TypeError, ValueError):
            raise ValueError(f"{path}: malformed safetensors entry for {name!r}") from None
        if dtype not in _ST_DTYPES:
            raise ValueError(f"{path}: tensor {name!r} has dtype {dtype}; this reader knows {sorted(_ST_DTYPES)}")
        tdtype, size = _ST_DTYPES[dtype]
        numel = 1
        for s in shape:
            numel *= s
        if not (0 <= lo <= hi) or hi - lo != numel * size:
            raise ValueError(f"{path}: tensor {name!r}: offsets [{lo}, {hi}) do not hold {shape} {dtype}")
        if hi > len(data):
            raise ValueError(f"{path}: truncated safetensors file: tensor {name!r} ends at byte {hi} of {len(data)}")
        t = torch.frombuffer(bytearray(data[lo:hi]), dtype=tdtype) if numel else torch.empty(0, dtype=tdtype)
        out[name] = t.reshape(shape).clone()
    return out


def load_state_dict_file(path) -> dict:
    """A ``.safetensors`` file, or a torch file (``weights_only=True``; a nested ``"state_dict"`` is taken)."""
    if str(path).endswith(".safetensors"):
        return read_safetensors(path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and isinstance(sd.get("state_dict"), dict):
        sd = sd["state_dict"]
    if not isinstance(sd, dict) or not all(isinstance(v, torch.Tensor) for v in sd.values()):
        raise ValueError(f"{path}: not a state dict of tensors")
    return sd


# ---- the key set of a config --------------------------------------------------------------------------------------------------------
def _resnet_shapes(prefix, cin, cout):
    s = {f"{prefix}.norm1.weight": (cin,), f"{prefix}.norm1.bias": (cin,), f"{prefix}.conv1.weight": (cout, cin, 3, 3),
         f"{prefix}.conv1.bias": (cout,), f"{prefix}.norm2.weight": (cout,), f"{prefix}.norm2.bias": (cout,),
         f"{prefix}.conv2.weight": (cout, cout, 3, 3), f"{prefix}.conv2.bias": (cout,)}
    if cin != cout:
        s[f"{prefix}.conv_shortcut.weight"] = (cout, cin, 1, 1)
        s[f"{prefix}.conv_shortcut.bias"] = (cout,)
    return s


def decoder_shapes(block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=4, out_channels=3) -> dict:
    """Key -> shape of ``post_quant_conv`` and ``decoder`` for a config, attention keys in the current generation (to_q ...)."""
    ch = list(reversed(block_out_channels))
    c0 = ch[0]
    s = {"post_quant_conv.weight": (latent_channels, latent_channels, 1, 1), "post_quant_conv.bias": (latent_channels,),
         "decoder.conv_in.weight": (c0, latent_channels, 3, 3), "decoder.conv_in.bias": (c0,)}
    s.update(_resnet_shapes("decoder.mid_block.resnets.0", c0, c0))
    s[_ATTN + "group_norm.weight"] = s[_ATTN + "group_norm.bias"] = (c0,)
    for k in ("to_q", "to_k", "to_v", "to_out.0"):
        s[_ATTN + k + ".weight"] = (c0, c0)
        s[_ATTN + k + ".bias"] = (c0,)
    s.update(_resnet_shapes("decoder.mid_block.resnets.1", c0, c0))
    cin = c0
    for i, cout in enumerate(ch):
        for j in range(layers_per_block + 1):
            s.update(_resnet_shapes(f"decoder.up_blocks.{i}.resnets.{j}", cin, cout))
            cin = cout
        if i < len(ch) - 1:
            s[f"decoder.up_blocks.{i}.upsamplers.0.conv.weight"] = (cout, cout, 3, 3)
            s[f"decoder.up_blocks.{i}.upsamplers.0.conv.bias"] = (cout,)
    s["decoder.conv_norm_out.weight"] = s["decoder.conv_norm_out.bias"] = (cin,)
    s["decoder.conv_out.weight"] = (out_channels, cin, 3, 3)
    s["decoder.conv_out.bias"] = (out_channels,)
    return s


def _normalise_keys(sd) -> dict:
    """Decoder-side tensors under the current generation's names; encoder.* / quant_conv.* dropped; anything else is an error."""
    out = {}
    for k, v in sd.items():
        if k.startswith(("encoder.", "quant_conv.")):
            continue
        if not k.startswith(("decoder.", "post_quant_conv.")):
            raise KeyError(f"VAE state dict: unexpected key {k!r} (neither decoder.*, post_quant_conv.*, encoder.* nor quant_conv.*)")
        if k.startswith(_ATTN):
            head, _, leaf = k[len(_ATTN):].rpartition(".")
            k = _ATTN + _OLD_ATTN.get(head, head) + "." + leaf
        if k in out:
            raise KeyError(f"VAE state dict: {k!r} is given twice (both attention key generations)")
        out[k] = v
    return out


def infer_config(sd) -> dict:
    """block_out_channels, layers_per_block, latent_channels, out_channels from the tensor shapes and key indices."""
    need = ("decoder.conv_in.weight", "decoder.conv_out.weight")
    for k in need:
        if k not in sd:
            raise KeyError(f"VAE state dict: missing key {k!r}")
    ups = sorted({int(m.group(1)) for k in sd for m in [re.match(r"decoder\.up_blocks\.(\d+)\.", k)] if m})
    if not ups or ups != list(range(len(ups))) or len(ups) > 4:
        raise KeyError(f"VAE state dict: decoder.up_blocks indices {ups} (1 to 4 consecutive blocks expected)")
    res0 = sorted({int(m.group(1)) for k in sd for m in [re.match(r"decoder\.up_blocks\.0\.resnets\.(\d+)\.", k)] if m})
    if len(res0) < 2 or res0 != list(range(len(res0))):
        raise KeyError(f"VAE state dict: decoder.up_blocks.0.resnets indices {res0}")
    widths = []
    for i in ups:
        k = f"decoder.up_blocks.{i}.resnets.0.conv1.weight"
        if k not in sd:
            raise KeyError(f"VAE state dict: missing key {k!r}")
        widths.append(int(sd[k].shape[0]))
    return dict(block_out_channels=tuple(reversed(widths)), layers_per_block=len(res0) - 1,
                latent_channels=int(sd["decoder.conv_in.weight"].shape[1]), out_channels=int(sd["decoder.conv_out.weight"].shape[0]))


def pack_conv_weight(w: torch.Tensor, dtype) -> torch.Tensor:
    """[Cout, Cin, k, k] (or a linear's [Cout, Cin]) -> 16-bit [Cout][ky][kx][Cin], the B operand of mapdit_vae_conv."""
    if w.dim() == 2:
        w = w[:, :, None, None]
    return w.float().permute(0, 2, 3, 1).contiguous().to(dtype)


class VAEDecoder:
    """``VAEDecoder.from_file(path, device).decode(z).sample``: z [N, latent_channels, h, w] fp32 on the device, de-normalised by the
    caller -> [N, out_channels, 8h, 8w] fp32 NCHW on the device, unclamped.  ``precision``: the 16-bit operand format of every conv /
    matmul ("f16" default: 10 mantissa bits; "bf16"); accumulation and the residual stream are fp32 in both."""

    def __init__(self, packed, cfg, device, precision, norm_num_groups, max_batch):
        self.cfg, self.precision, self.norm_num_groups, self.max_batch = dict(cfg), precision, int(norm_num_groups), int(max_batch)
        self.device = torch.device(device)
        self.packed = {k: v.to(self.device) for k, v in packed.items()}
        ch = list(cfg["block_out_channels"]) + [0] * (4 - len(cfg["block_out_channels"]))
        self._cfg = L.VaeConfig(latent_channels=cfg["latent_channels"], out_channels=cfg["out_channels"], num_blocks=len(cfg["block_out_channels"]),
                                ch0=ch[0], ch1=ch[1], ch2=ch[2], ch3=ch[3], layers_per_block=cfg["layers_per_block"],
                                norm_num_groups=self.norm_num_groups, norm_eps=1e-6)
        self.scale = 2 ** (len(cfg["block_out_channels"]) - 1)
        self._table = None
        self._ws = None

    # -- construction --------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd, device, precision="f16", norm_num_groups=32, max_batch=16):
        if precision not in PRECISIONS:
            raise ValueError(f"VAE precision {precision!r}: one of {sorted(PRECISIONS)}")
        if max_batch < 1:
            raise ValueError(f"max_batch={max_batch} must be at least 1")
        sd = _normalise_keys(sd)
        cfg = infer_config(sd)
        shapes = decoder_shapes(**cfg)
        missing, extra = sorted(set(shapes) - set(sd)), sorted(set(sd) - set(shapes))
        if missing:
            raise KeyError(f"VAE state dict: missing key {missing[0]!r}" + (f" (and {len(missing) - 1} more)" if len(missing) > 1 else ""))
        if extra:
            raise KeyError(f"VAE state dict: unexpected key {extra[0]!r}" + (f" (and {len(extra) - 1} more)" if len(extra) > 1 else ""))
        dt, packed = PRECISIONS[precision], {}
        for k, want in shapes.items():
            v = sd[k]
            if k.startswith(_ATTN) and k.endswith(".weight") and v.dim() == 4 and tuple(v.shape[2:]) == (1, 1):
                v = v[:, :, 0, 0]                                   # the older generation stores the linears as 1 x 1 convs
            if tuple(v.shape) != tuple(want):
                raise ValueError(f"VAE state dict: {k!r} has shape {tuple(sd[k].shape)}, expected {tuple(want)}")
            if k.startswith(_ATTN + "to_") and not k.startswith(_ATTN + "to_out"):
                continue                                            # stacked below
            packed[k] = pack_conv_weight(v, dt) if v.dim() in (2, 4) else v.float().contiguous()
        qkv = [sd[_ATTN + n + ".weight"] for n in ("to_q", "to_k", "to_v")]
        packed[_ATTN + "qkv.weight"] = pack_conv_weight(torch.cat([w.reshape(w.shape[0], w.shape[1]) for w in qkv], 0), dt)
        packed[_ATTN + "qkv.bias"] = torch.cat([sd[_ATTN + n + ".bias"].float() for n in ("to_q", "to_k", "to_v")], 0).contiguous()
        return cls(packed, cfg, device, precision, norm_num_groups, max_batch)

    @classmethod
    def from_file(cls, path, device, precision="f16", norm_num_groups=32, max_batch=16):
        return cls.from_state_dict(load_state_dict_file(path), device, precision, norm_num_groups, max_batch)

    # -- the library's weight table ----------------------------------------------------------------------------------------------------
    def slot_names(self):
        """Packed-tensor name (or None) of every slot of mapdit_vae_decode's weight table, in the header's order."""
        g = [None] * L.VAE_NUM_GLOBAL
        for slot, name in (("PQ", "post_quant_conv"), ("CONV_IN", "decoder.conv_in"), ("ATTN_QKV", _ATTN + "qkv"), ("ATTN_OUT", _ATTN + "to_out.0"),
                           ("CONV_OUT", "decoder.conv_out")):
            g[getattr(L, f"VAE_W_{slot}_W")], g[getattr(L, f"VAE_W_{slot}_B")] = name + ".weight", name + ".bias"
        for slot, name in (("ATTN_GN", _ATTN + "group_norm"), ("NORM_OUT", "decoder.conv_norm_out")):
            g[getattr(L, f"VAE_W_{slot}_G")], g[getattr(L, f"VAE_W_{slot}_B")] = name + ".weight", name + ".bias"
        nb, lpb = len(self.cfg["block_out_channels"]), self.cfg["layers_per_block"]
        resnets = ["decoder.mid_block.resnets.0", "decoder.mid_block.resnets.1"]
        resnets += [f"decoder.up_blocks.{i}.resnets.{j}" for i in range(nb) for j in range(lpb + 1)]
        for r in resnets:
            s = [None] * L.VAE_NUM_RESNET
            for slot, name in (("N1_G", "norm1.weight"), ("N1_B", "norm1.bias"), ("C1_W", "conv1.weight"), ("C1_B", "conv1.bias"), ("N2_G", "norm2.weight"),
                               ("N2_B", "norm2.bias"), ("C2_W", "conv2.weight"), ("C2_B", "conv2.bias"), ("SC_W", "conv_shortcut.weight"),
                               ("SC_B", "conv_shortcut.bias")):
                s[getattr(L, f"VAE_R_{slot}")] = f"{r}.{name}" if f"{r}.{name}" in self.packed else None
            g += s
        for i in range(nb - 1):
            s = [None] * L.VAE_NUM_UP
            s[L.VAE_U_W], s[L.VAE_U_B] = f"decoder.up_blocks.{i}.upsamplers.0.conv.weight", f"decoder.up_blocks.{i}.upsamplers.0.conv.bias"
            g += s
        return g

    def workspace_bytes(self, n, h, w) -> int:
        lib = L.lib()
        need = lib.vae_workspace_bytes(C.byref(self._cfg), int(n), int(h), int(w))
        if need == 0:
            raise ValueError(f"VAE decode refused: {lib.last_error().decode()}")
        return need

    # -- decode ------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def decode(self, z):
        if not isinstance(z, torch.Tensor) or not z.is_cuda or self.device.type != "cuda":
            raise NotImplementedError("VAEDecoder.decode runs on the GPU only (HIP kernels, no CPU path): pass a CUDA tensor to a decoder on the device")
        if z.dim() != 4 or z.shape[1] != self.cfg["latent_channels"]:
            raise ValueError(f"VAE decode: z has shape {tuple(z.shape)}, expected [N, {self.cfg['latent_channels']}, h, w]")
        z = z.detach().to(self.device, torch.float32).contiguous()
        N, _, h, w = z.shape
        if N == 0:
            return SimpleNamespace(sample=z.new_empty(0, self.cfg["out_channels"], h * self.scale, w * self.scale))
        chunk = min(N, self.max_batch)
        need = self.workspace_bytes(chunk, h, w)
        lib = L.lib()
        if self._table is None:
            names = self.slot_names()
            self._table = (C.c_void_p * len(names))(*[None if n is None else self.packed[n].data_ptr() for n in names])
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        out = torch.empty(N, self.cfg["out_channels"], h * self.scale, w * self.scale, dtype=torch.float32, device=self.device)
        fn = lib.vae_decode_f16 if self.precision == "f16" else lib.vae_decode
        with torch.cuda.device(self.device):
            stream = L.cur_stream()
            for i in range(0, N, chunk):
                n = min(chunk, N - i)
                fn(C.byref(self._cfg), self._table, z[i:i + n].data_ptr(), out[i:i + n].data_ptr(), n, h, w, self._ws.data_ptr(), self._ws.numel(), stream)
        return SimpleNamespace(sample=out)
