"""Native VAE, both directions, on ``libmapdit_hip.so`` for weights in the ``AutoencoderKL`` layout (Stable Diffusion's; the defaults are
those of ``stabilityai/sd-vae-ft-mse``).  ``VAEDecoder``: ``vae.decode(samples).sample`` of the reference's sampler scripts
(sample.py:72-74, sample_fid.py:83-84, sample_ema.py:73) - ``mapdit_vae_decode`` (include/mapdit.h).  ``VAEEncoder``:
``vae.encode(imgs).latent_dist`` of the reference's download_data.py - ``mapdit_vae_encode``.  Each class takes its half of a state
dict and ignores the other's, so one hub file serves both.  Parity with the hub weights is unpinned: the network is restated from its
public description and checked against independent restatements (tests/vae_reference.py, tests/vae_encoder_reference.py), not
against the ``diffusers`` package.
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
_ENC_ATTN = "encoder.mid_block.attentions.0."
# the two halves of the network: (key prefixes, attention prefix)
_SIDES = {"decoder": (("decoder.", "post_quant_conv."), _ATTN), "encoder": (("encoder.", "quant_conv."), _ENC_ATTN)}


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


def encoder_shapes(block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=4, out_channels=3) -> dict:
    """Key -> shape of ``encoder`` and ``quant_conv`` for a config (``out_channels``: the image's channels), attention keys in the
    current generation (to_q ...)."""
    ch = list(block_out_channels)
    s = {"encoder.conv_in.weight": (ch[0], out_channels, 3, 3), "encoder.conv_in.bias": (ch[0],)}
    cin = ch[0]
    for i, cout in enumerate(ch):
        for j in range(layers_per_block):
            s.update(_resnet_shapes(f"encoder.down_blocks.{i}.resnets.{j}", cin, cout))
            cin = cout
        if i < len(ch) - 1:
            s[f"encoder.down_blocks.{i}.downsamplers.0.conv.weight"] = (cout, cout, 3, 3)
            s[f"encoder.down_blocks.{i}.downsamplers.0.conv.bias"] = (cout,)
    s.update(_resnet_shapes("encoder.mid_block.resnets.0", cin, cin))
    s[_ENC_ATTN + "group_norm.weight"] = s[_ENC_ATTN + "group_norm.bias"] = (cin,)
    for k in ("to_q", "to_k", "to_v", "to_out.0"):
        s[_ENC_ATTN + k + ".weight"] = (cin, cin)
        s[_ENC_ATTN + k + ".bias"] = (cin,)
    s.update(_resnet_shapes("encoder.mid_block.resnets.1", cin, cin))
    s["encoder.conv_norm_out.weight"] = s["encoder.conv_norm_out.bias"] = (cin,)
    s["encoder.conv_out.weight"] = (2 * latent_channels, cin, 3, 3)
    s["encoder.conv_out.bias"] = (2 * latent_channels,)
    s["quant_conv.weight"] = (2 * latent_channels, 2 * latent_channels, 1, 1)
    s["quant_conv.bias"] = (2 * latent_channels,)
    return s


def _normalise_keys(sd, side="decoder") -> dict:
    """One side's tensors (decoder.* + post_quant_conv.*, or encoder.* + quant_conv.*) under the current generation's names; the other
    side's dropped; anything else is an error."""
    mine, attn = _SIDES[side]
    theirs = _SIDES["encoder" if side == "decoder" else "decoder"][0]
    out = {}
    for k, v in sd.items():
        if k.startswith(theirs):
            continue
        if not k.startswith(mine):
            raise KeyError(f"VAE state dict: unexpected key {k!r} (neither decoder.*, post_quant_conv.*, encoder.* nor quant_conv.*)")
        if k.startswith(attn):
            head, _, leaf = k[len(attn):].rpartition(".")
            k = attn + _OLD_ATTN.get(head, head) + "." + leaf
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


def infer_encoder_config(sd) -> dict:
    """The same four entries from the encoder's tensors: ``out_channels`` is the image's channel count, ``latent_channels`` half of
    conv_out's outputs (mean and log-variance)."""
    for k in ("encoder.conv_in.weight", "encoder.conv_out.weight"):
        if k not in sd:
            raise KeyError(f"VAE state dict: missing key {k!r}")
    downs = sorted({int(m.group(1)) for k in sd for m in [re.match(r"encoder\.down_blocks\.(\d+)\.", k)] if m})
    if not downs or downs != list(range(len(downs))) or len(downs) > 4:
        raise KeyError(f"VAE state dict: encoder.down_blocks indices {downs} (1 to 4 consecutive blocks expected)")
    res0 = sorted({int(m.group(1)) for k in sd for m in [re.match(r"encoder\.down_blocks\.0\.resnets\.(\d+)\.", k)] if m})
    if not res0 or res0 != list(range(len(res0))):
        raise KeyError(f"VAE state dict: encoder.down_blocks.0.resnets indices {res0}")
    widths = []
    for i in downs:
        k = f"encoder.down_blocks.{i}.resnets.0.conv1.weight"
        if k not in sd:
            raise KeyError(f"VAE state dict: missing key {k!r}")
        widths.append(int(sd[k].shape[0]))
    two_l = int(sd["encoder.conv_out.weight"].shape[0])
    if two_l % 2:
        raise ValueError(f"VAE state dict: 'encoder.conv_out.weight' has {two_l} outputs; mean and log-variance need an even count")
    return dict(block_out_channels=tuple(widths), layers_per_block=len(res0), latent_channels=two_l // 2,
                out_channels=int(sd["encoder.conv_in.weight"].shape[1]))


def pack_conv_weight(w: torch.Tensor, dtype) -> torch.Tensor:
    """[Cout, Cin, k, k] (or a linear's [Cout, Cin]) -> 16-bit [Cout][ky][kx][Cin], the B operand of mapdit_vae_conv."""
    if w.dim() == 2:
        w = w[:, :, None, None]
    return w.float().permute(0, 2, 3, 1).contiguous().to(dtype)


_RESNET_SLOTS = (("N1_G", "norm1.weight"), ("N1_B", "norm1.bias"), ("C1_W", "conv1.weight"), ("C1_B", "conv1.bias"), ("N2_G", "norm2.weight"),
                 ("N2_B", "norm2.bias"), ("C2_W", "conv2.weight"), ("C2_B", "conv2.bias"), ("SC_W", "conv_shortcut.weight"),
                 ("SC_B", "conv_shortcut.bias"))


class _VAEHalf:
    """What the two directions share: the checked, packed weights of one half of the network, the library's config struct, the
    weight table and the workspace."""
    _side = None                      # "decoder" / "encoder": the key prefixes and the attention prefix (_SIDES)
    _shapes = None                    # config -> {key: shape}
    _infer = None                     # normalised state dict -> config

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
        attn = _SIDES[cls._side][1]
        sd = _normalise_keys(sd, cls._side)
        cfg = cls._infer(sd)
        shapes = cls._shapes(**cfg)
        missing, extra = sorted(set(shapes) - set(sd)), sorted(set(sd) - set(shapes))
        if missing:
            raise KeyError(f"VAE state dict: missing key {missing[0]!r}" + (f" (and {len(missing) - 1} more)" if len(missing) > 1 else ""))
        if extra:
            raise KeyError(f"VAE state dict: unexpected key {extra[0]!r}" + (f" (and {len(extra) - 1} more)" if len(extra) > 1 else ""))
        dt, packed = PRECISIONS[precision], {}
        for k, want in shapes.items():
            v = sd[k]
            if k.startswith(attn) and k.endswith(".weight") and v.dim() == 4 and tuple(v.shape[2:]) == (1, 1):
                v = v[:, :, 0, 0]                                   # the older generation stores the linears as 1 x 1 convs
            if tuple(v.shape) != tuple(want):
                raise ValueError(f"VAE state dict: {k!r} has shape {tuple(sd[k].shape)}, expected {tuple(want)}")
            if k.startswith(attn + "to_") and not k.startswith(attn + "to_out"):
                continue                                            # stacked below
            packed[k] = pack_conv_weight(v, dt) if v.dim() in (2, 4) else v.float().contiguous()
        qkv = [sd[attn + n + ".weight"] for n in ("to_q", "to_k", "to_v")]
        packed[attn + "qkv.weight"] = pack_conv_weight(torch.cat([w.reshape(w.shape[0], w.shape[1]) for w in qkv], 0), dt)
        packed[attn + "qkv.bias"] = torch.cat([sd[attn + n + ".bias"].float() for n in ("to_q", "to_k", "to_v")], 0).contiguous()
        return cls(packed, cfg, device, precision, norm_num_groups, max_batch)

    @classmethod
    def from_file(cls, path, device, precision="f16", norm_num_groups=32, max_batch=16):
        return cls.from_state_dict(load_state_dict_file(path), device, precision, norm_num_groups, max_batch)

    # -- the library's weight table ----------------------------------------------------------------------------------------------------
    def _slot_names(self, prefix, num_global, pairs, norms, resnets, tails):
        """Global slots (``prefix`` + W / B or G / B), MAPDIT_VAE_NUM_RESNET slots per resnet, a weight / bias pair per tail conv."""
        g = [None] * num_global
        for slot, name in pairs:
            g[getattr(L, f"{prefix}{slot}_W")], g[getattr(L, f"{prefix}{slot}_B")] = name + ".weight", name + ".bias"
        for slot, name in norms:
            g[getattr(L, f"{prefix}{slot}_G")], g[getattr(L, f"{prefix}{slot}_B")] = name + ".weight", name + ".bias"
        for r in resnets:
            s = [None] * L.VAE_NUM_RESNET
            for slot, name in _RESNET_SLOTS:
                s[getattr(L, f"VAE_R_{slot}")] = f"{r}.{name}" if f"{r}.{name}" in self.packed else None
            g += s
        for t in tails:
            g += [t + ".weight", t + ".bias"]       # MAPDIT_VAE_U_W, _B / MAPDIT_VAE_D_W, _B
        return g

    def _pointers(self):
        if self._table is None:
            names = self.slot_names()
            self._table = (C.c_void_p * len(names))(*[None if n is None else self.packed[n].data_ptr() for n in names])
        return self._table

    def _workspace(self, need):
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws


class VAEDecoder(_VAEHalf):
    """``VAEDecoder.from_file(path, device).decode(z).sample``: z [N, latent_channels, h, w] fp32 on the device, de-normalised by the
    caller -> [N, out_channels, 8h, 8w] fp32 NCHW on the device, unclamped.  ``precision``: the 16-bit operand format of every conv /
    matmul ("f16" default: 10 mantissa bits; "bf16"); accumulation and the residual stream are fp32 in both."""
    _side, _shapes, _infer = "decoder", staticmethod(decoder_shapes), staticmethod(infer_config)

    def slot_names(self):
        """Packed-tensor name (or None) of every slot of mapdit_vae_decode's weight table, in the header's order."""
        nb, lpb = len(self.cfg["block_out_channels"]), self.cfg["layers_per_block"]
        resnets = ["decoder.mid_block.resnets.0", "decoder.mid_block.resnets.1"]
        resnets += [f"decoder.up_blocks.{i}.resnets.{j}" for i in range(nb) for j in range(lpb + 1)]
        assert (L.VAE_U_W, L.VAE_U_B, L.VAE_NUM_UP) == (0, 1, 2)
        return self._slot_names("VAE_W_", L.VAE_NUM_GLOBAL,
                                (("PQ", "post_quant_conv"), ("CONV_IN", "decoder.conv_in"), ("ATTN_QKV", _ATTN + "qkv"),
                                 ("ATTN_OUT", _ATTN + "to_out.0"), ("CONV_OUT", "decoder.conv_out")),
                                (("ATTN_GN", _ATTN + "group_norm"), ("NORM_OUT", "decoder.conv_norm_out")), resnets,
                                [f"decoder.up_blocks.{i}.upsamplers.0.conv" for i in range(nb - 1)])

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
        table, ws = self._pointers(), self._workspace(need)
        out = torch.empty(N, self.cfg["out_channels"], h * self.scale, w * self.scale, dtype=torch.float32, device=self.device)
        fn = lib.vae_decode_f16 if self.precision == "f16" else lib.vae_decode
        with torch.cuda.device(self.device):
            stream = L.cur_stream()
            for i in range(0, N, chunk):
                n = min(chunk, N - i)
                fn(C.byref(self._cfg), table, z[i:i + n].data_ptr(), out[i:i + n].data_ptr(), n, h, w, ws.data_ptr(), ws.numel(), stream)
        return SimpleNamespace(sample=out)


class LatentDist:
    """``DiagonalGaussianDistribution`` as far as the reference uses it: ``mean``, ``std`` fp32 [N, L, h, w] on the device as the
    kernel wrote them; ``logvar`` = 2 log(std), the clamped log-variance up to the rounding of exp and log (the library call
    returns mean and std only)."""

    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    @property
    def logvar(self):
        return 2.0 * torch.log(self.std)

    def mode(self):
        return self.mean

    def sample(self, generator=None):
        return self.mean + self.std * torch.randn(self.mean.shape, generator=generator, device=self.mean.device, dtype=self.mean.dtype)


class VAEEncoder(_VAEHalf):
    """``VAEEncoder.from_file(path, device).encode(x).latent_dist``: x fp32 [N, C, H, W] in [-1, 1] on the device, or uint8 [N, H, W, C]
    as PIL / numpy hold it (prepared by mapdit_vae_prepare_u8: ToTensor + Normalize(0.5, 0.5), with ``flip`` [N] mirroring the
    flagged samples left-right) -> mean, std fp32 [N, latent_channels, H / s, W / s].  Batches above ``max_batch`` are chunked; a
    sample alone gives the same bits as in a batch."""
    _side, _shapes, _infer = "encoder", staticmethod(encoder_shapes), staticmethod(infer_encoder_config)

    def slot_names(self):
        """Packed-tensor name (or None) of every slot of mapdit_vae_encode's weight table, in the header's order."""
        nb, lpb = len(self.cfg["block_out_channels"]), self.cfg["layers_per_block"]
        resnets = [f"encoder.down_blocks.{i}.resnets.{j}" for i in range(nb) for j in range(lpb)]
        resnets += ["encoder.mid_block.resnets.0", "encoder.mid_block.resnets.1"]
        assert (L.VAE_D_W, L.VAE_D_B, L.VAE_NUM_DOWN) == (0, 1, 2)
        return self._slot_names("VAE_E_", L.VAE_E_NUM_GLOBAL,
                                (("CONV_IN", "encoder.conv_in"), ("ATTN_QKV", _ENC_ATTN + "qkv"), ("ATTN_OUT", _ENC_ATTN + "to_out.0"),
                                 ("CONV_OUT", "encoder.conv_out"), ("QUANT", "quant_conv")),
                                (("ATTN_GN", _ENC_ATTN + "group_norm"), ("NORM_OUT", "encoder.conv_norm_out")), resnets,
                                [f"encoder.down_blocks.{i}.downsamplers.0.conv" for i in range(nb - 1)])

    def workspace_bytes(self, n, H, W) -> int:
        lib = L.lib()
        need = lib.vae_encode_workspace_bytes(C.byref(self._cfg), int(n), int(H), int(W))
        if need == 0:
            raise ValueError(f"VAE encode refused: {lib.last_error().decode()}")
        return need

    # -- encode ------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def encode(self, x, flip=None):
        if not isinstance(x, torch.Tensor) or not x.is_cuda or self.device.type != "cuda":
            raise NotImplementedError("VAEEncoder.encode runs on the GPU only (HIP kernels, no CPU path): pass a CUDA tensor to an encoder on the device")
        Cimg, lat = self.cfg["out_channels"], self.cfg["latent_channels"]
        u8 = x.dtype == torch.uint8
        if x.dim() != 4 or x.shape[3 if u8 else 1] != Cimg:
            raise ValueError(f"VAE encode: x has shape {tuple(x.shape)} ({x.dtype}), expected " +
                             (f"uint8 [N, H, W, {Cimg}]" if u8 else f"[N, {Cimg}, H, W]"))
        if flip is not None and not u8:
            raise ValueError("VAE encode: flip belongs to the uint8 input (the image preparation mirrors); flip a float tensor with torch.flip")
        x = x.detach().to(self.device).contiguous() if u8 else x.detach().to(self.device, torch.float32).contiguous()
        N, H, W = (x.shape[0], x.shape[1], x.shape[2]) if u8 else (x.shape[0], x.shape[2], x.shape[3])
        if flip is not None:
            flip = torch.as_tensor(flip, device=self.device)
            if flip.shape != (N,):
                raise ValueError(f"VAE encode: flip has shape {tuple(flip.shape)}, expected [{N}]")
            flip = (flip != 0).to(torch.uint8).contiguous()
        chunk = max(1, min(N, self.max_batch))
        need = self.workspace_bytes(chunk, H, W)                     # (refuses the shape before anything is allocated)
        h, w = H // self.scale, W // self.scale
        mean = torch.empty(N, lat, h, w, dtype=torch.float32, device=self.device)
        std = torch.empty_like(mean)
        if N == 0:
            return SimpleNamespace(latent_dist=LatentDist(mean, std))
        lib = L.lib()
        table, ws = self._pointers(), self._workspace(need)
        prep = torch.empty(chunk, H, W, Cimg, dtype=torch.float32, device=self.device) if u8 else None
        fn = lib.vae_encode_f16 if self.precision == "f16" else lib.vae_encode
        with torch.cuda.device(self.device):
            stream = L.cur_stream()
            for i in range(0, N, chunk):
                n = min(chunk, N - i)
                src, kind = x[i:i + n].data_ptr(), L.VAE_IN_F32_NCHW
                if u8:
                    lib.vae_prepare_u8(src, None if flip is None else flip[i:i + n].data_ptr(), prep.data_ptr(), n, H, W, Cimg, stream)
                    src, kind = prep.data_ptr(), L.VAE_IN_F32
                fn(C.byref(self._cfg), table, src, kind, mean[i:i + n].data_ptr(), std[i:i + n].data_ptr(), n, H, W, ws.data_ptr(), ws.numel(), stream)
        return SimpleNamespace(latent_dist=LatentDist(mean, std))
