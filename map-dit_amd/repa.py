"""REPA, representation alignment (Yu et al. 2024), on ``libmapdit_hip.so``: a three-layer MLP projects the DiT's hidden state after
an early block (``model.hidden_tap``, ``model.tapped_hidden``), and every projected token is pulled toward the DINOv2 patch token of the
clean image (``python -m mapdit_amd.dinov2 tokens``) by a negative cosine similarity.

    head = RepaHead(model.hidden_size, feat_dim, precision=model.gemm_precision).to(device)
    model.hidden_tap = 7                                      # after 8 blocks
    out = model(x, t, y)
    loss = diffusion_loss(out) + 0.5 * head.loss(model.tapped_hidden, feats).mean()
    loss.backward()                                           # head.loss's backward hands d loss / d hidden to the engine

``z = W3 silu(W2 silu(W1 h + b1) + b2) + b3``: plain biased linears with fp32 masters in one flat buffer (``_pflat`` / ``_gflat``, the
layout ``optim.FusedAdamEMA`` steps), 16-bit GEMM operands (the library's GEMMs: NT forward, NN for dX, TN for dW), fp32 accumulation,
fp32 pre-activations.  No compute runs in torch.  The projector is the paper's plain (not magnitude-preserving) one; its effect on this
network's convergence is not measured.
"""
from __future__ import annotations

import ctypes as C
import math

import torch
import torch.nn as nn

from . import _lib as L

PRECISIONS = {"bf16": torch.bfloat16, "f16": torch.float16}


def check_features(feats, n, tokens, feat_dim):
    """``feats`` [n, tokens, feat_dim] fp16 or fp32 on the device, contiguous: what ``RepaHead.loss`` takes."""
    if not isinstance(feats, torch.Tensor) or feats.dtype not in (torch.float16, torch.float32):
        raise ValueError(f"REPA features must be an fp16 or fp32 tensor, got {getattr(feats, 'dtype', type(feats))}")
    if tuple(feats.shape) != (n, tokens, feat_dim):
        raise ValueError(f"REPA features of shape {tuple(feats.shape)}, expected [{n}, {tokens}, {feat_dim}] (samples, tokens, feature width)")
    return feats.contiguous()


class _RepaLossFunction(torch.autograd.Function):
    """loss [N] = -(1 / T) sum_t cos(projector(hidden)[n, t], feats[n, t]).  The parameter gradients go straight into the head's flat
    gradient buffer (``p.grad`` are views of it, accumulated into when they are still set); d loss / d hidden is returned to autograd."""

    @staticmethod
    def forward(ctx, head, hidden, feats, anchor):
        N, T, D = hidden.shape
        ctx.head, ctx.saved = head, head._forward(hidden.contiguous().float(), feats)
        ctx.shape = (N, T, D)
        return ctx.saved["loss"]

    @staticmethod
    def backward(ctx, gloss):
        dh = ctx.head._backward(ctx.saved, gloss.contiguous().float(), ctx.needs_input_grad[1])
        ctx.saved = None
        return None, (dh.view(ctx.shape) if dh is not None else None), None, None


class RepaHead(nn.Module):
    """The alignment head.  ``in_dim``: the DiT's hidden size; ``feat_dim``: the feature width P (a multiple of 8); ``hidden``: the width
    of the two inner layers (a multiple of 8).  Initialised like ``nn.Linear`` (U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)) for weights and
    biases) from a generator seeded with ``seed``.  ``loss_scale`` ("f16" only): the power of two the backward multiplies the cosine
    gradient by so that the 16-bit activation gradients sit in fp16's normal range; 0 = 2^floor(log2(rows x feat_dim))."""

    def __init__(self, in_dim, feat_dim, hidden=2048, precision="f16", seed=0):
        super().__init__()
        if precision not in PRECISIONS:
            raise ValueError(f"RepaHead precision {precision!r}: one of {sorted(PRECISIONS)} (bf16x3 is not built)")
        for name, v in (("in_dim", in_dim), ("feat_dim", feat_dim), ("hidden", hidden)):
            if v < 8 or v % 8:
                raise ValueError(f"RepaHead {name}={v} must be a positive multiple of 8")
        self.in_dim, self.feat_dim, self.hidden, self.gemm_precision = int(in_dim), int(feat_dim), int(hidden), precision
        self.loss_scale = 0.0
        self._last_scale = 1.0
        g = torch.Generator().manual_seed(int(seed))
        dims = [(self.hidden, self.in_dim), (self.hidden, self.hidden), (self.feat_dim, self.hidden)]
        for i, (o, k) in enumerate(dims, 1):
            bound = 1.0 / math.sqrt(k)
            setattr(self, f"w{i}", nn.Parameter((torch.rand(o, k, generator=g) * 2 - 1) * bound))
            setattr(self, f"b{i}", nn.Parameter((torch.rand(o, generator=g) * 2 - 1) * bound))
        self._pflat = self._gflat = self._gviews = None
        self._w_epoch = 0
        self._flatten_parameters()

    # ---- flat storage (the layout FusedAdamEMA reads) ----------------------------------------------------------------------------
    def _flatten_parameters(self):
        params = list(self.parameters())
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + 31) // 32 * 32
        flat = torch.zeros(total, device=params[0].device, dtype=torch.float32)
        for p, o in zip(params, offs):
            flat[o:o + p.numel()].view(p.shape).copy_(p.data)
            p.data = flat[o:o + p.numel()].view(p.shape)
        self._pflat, self._poffs = flat, offs
        self._gflat = self._gviews = None

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._flatten_parameters()
        return out

    def _attach_grads(self) -> bool:
        if self._gflat is None or self._gflat.device != self._pflat.device:
            self._gflat = torch.zeros_like(self._pflat)
            self._gviews = [self._gflat[o:o + p.numel()].view(p.shape) for p, o in zip(self.parameters(), self._poffs)]
        fresh, accumulate = [], False
        for p, g in zip(self.parameters(), self._gviews):
            if p.grad is None:
                p.grad = g
                fresh.append(g)
            else:
                if p.grad.data_ptr() != g.data_ptr():
                    g.copy_(p.grad)
                    p.grad = g
                accumulate = True
        if accumulate:
            for g in fresh:
                g.zero_()
        return accumulate

    def mark_weights_changed(self):
        self._w_epoch += 1

    def effective_loss_scale(self) -> float:
        """The loss scale the most recent backward ran with (1.0 in bf16 and before any backward)."""
        return float(self._last_scale)

    # ---- the kernels ---------------------------------------------------------------------------------------------------------------
    def _fn(self, name):
        return getattr(L.lib(), name + ("_f16" if self.gemm_precision == "f16" else ""))

    def _gemm(self, layout, M, N, K, A, lda, B, ldb, out, ldo, alpha=1.0, split_k=1, slab=0):
        ep = L.Epilogue(kind=L.EPI_STORE_F32, out=out.data_ptr(), ldo=ldo, alpha=alpha, split_k=split_k, slab_stride=slab)
        fn = L.lib().gemm_f16 if self.gemm_precision == "f16" else L.lib().gemm_bf16
        fn(layout, M, N, K, A.data_ptr(), lda, B.data_ptr(), ldb, C.byref(ep), L.cur_stream())

    def _to16(self, x, n=None):
        out = torch.empty(x.shape, dtype=PRECISIONS[self.gemm_precision], device=x.device)
        (L.lib().f32_to_f16 if self.gemm_precision == "f16" else L.lib().f32_to_bf16)(x.data_ptr(), out.data_ptr(), x.numel(), 1.0, L.cur_stream())
        return out

    def _forward(self, hidden, feats):
        if not hidden.is_cuda:
            raise L.MapditError("RepaHead runs on the MI355X only: there is no CPU path")
        N, T, D = hidden.shape
        if D != self.in_dim:
            raise ValueError(f"RepaHead: hidden states of width {D}, built for {self.in_dim}")
        feats = check_features(feats, N, T, self.feat_dim).to(hidden.device)
        lib, M, H, P = L.lib(), N * T, self.hidden, self.feat_dim
        dev, dt = hidden.device, PRECISIONS[self.gemm_precision]
        with torch.cuda.device(dev):
            st = L.cur_stream()
            w16 = [self._to16(w.data) for w in (self.w1, self.w2, self.w3)]
            x16 = self._to16(hidden.view(M, D))
            pre1, pre2 = torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)
            act1, act2 = torch.empty(M, H, dtype=dt, device=dev), torch.empty(M, H, dtype=dt, device=dev)
            z, loss = torch.empty(M, P, device=dev), torch.empty(N, device=dev)
            self._gemm(L.NT, M, H, D, x16, D, w16[0], D, pre1, H)
            self._fn("repa_bias_silu_fwd")(pre1.data_ptr(), self.b1.data_ptr(), act1.data_ptr(), M, H, st)
            self._gemm(L.NT, M, H, H, act1, H, w16[1], H, pre2, H)
            self._fn("repa_bias_silu_fwd")(pre2.data_ptr(), self.b2.data_ptr(), act2.data_ptr(), M, H, st)
            self._gemm(L.NT, M, P, H, act2, H, w16[2], H, z, P)
            self._fn("repa_bias_silu_fwd")(z.data_ptr(), self.b3.data_ptr(), None, M, P, st)
            kind = L.REPA_F_F16 if feats.dtype == torch.float16 else L.REPA_F_F32
            lib.repa_cos_loss(z.data_ptr(), feats.data_ptr(), kind, None, 1.0, loss.data_ptr(), None, M, T, P, st)
        return dict(loss=loss, z=z, feats=feats, kind=kind, x16=x16, w16=w16, pre1=pre1, pre2=pre2, act1=act1, act2=act2, dims=(N, T, D))

    def _split_k(self, rows, cols, K):
        """Slabs of a weight-gradient product: one round of the chip, four K-tiles per workgroup at the least (the engine's rule)."""
        if K % 64 or rows % 8 or cols % 8:
            return 1
        edge = L.lib().gemm_tile_size_k(rows, cols, K, 1)
        tiles = -(-rows // edge) * -(-cols // edge)
        return max(1, min((256 if edge == 256 else 512) // tiles, (K // 64) // 4))

    def _dw(self, dy16, x16, M, rows, cols, grad, scale, accumulate):
        """grad [rows, cols] (+)= scale * dy16^T x16 over M token rows: split-K slabs, summed in slab order."""
        lib, s = L.lib(), self._split_k(rows, cols, M)
        slab = rows * cols
        G = torch.empty(s * slab, device=grad.device)
        self._gemm(L.TN, rows, cols, M, dy16, rows, x16, cols, G, cols, alpha=scale, split_k=s, slab=slab)
        (lib.sum_slabs if accumulate else lib.reduce_slabs)(grad.data_ptr(), G.data_ptr(), s, slab, slab, L.cur_stream())

    def _backward(self, sv, gloss, want_dh):
        N, T, D = sv["dims"]
        lib, M, H, P = L.lib(), N * T, self.hidden, self.feat_dim
        dev, dt = gloss.device, PRECISIONS[self.gemm_precision]
        accumulate = self._attach_grads()
        g = dict(zip(("w1", "b1", "w2", "b2", "w3", "b3"), self._gviews))
        scale = 1.0
        if self.gemm_precision == "f16":
            scale = float(self.loss_scale) or 2.0 ** math.floor(math.log2(M * P))
        self._last_scale = scale
        inv = 1.0 / scale
        bwd = self._fn("repa_bias_silu_bwd")
        with torch.cuda.device(dev):
            st = L.cur_stream()
            dz = torch.empty(M, P, device=dev)
            lib.repa_cos_loss(sv["z"].data_ptr(), sv["feats"].data_ptr(), sv["kind"], gloss.data_ptr(), 1.0, None, dz.data_ptr(), M, T, P, st)
            part = torch.empty(-(-M // L.REPA_PART_ROWS) * max(H, P), device=dev)
            dz16 = torch.empty(M, P, dtype=dt, device=dev)
            bwd(dz.data_ptr(), None, dz16.data_ptr(), g["b3"].data_ptr(), part.data_ptr(), scale, inv, int(accumulate), M, P, st)
            self._dw(dz16, sv["act2"], M, P, H, g["w3"], inv, accumulate)
            dact = torch.empty(M, H, device=dev)
            dpre16 = torch.empty(M, H, dtype=dt, device=dev)
            self._gemm(L.NN, M, H, P, dz16, P, sv["w16"][2], H, dact, H)
            bwd(dact.data_ptr(), sv["pre2"].data_ptr(), dpre16.data_ptr(), g["b2"].data_ptr(), part.data_ptr(), 1.0, inv, int(accumulate), M, H, st)
            self._dw(dpre16, sv["act1"], M, H, H, g["w2"], inv, accumulate)
            dpre1 = torch.empty(M, H, dtype=dt, device=dev)
            self._gemm(L.NN, M, H, H, dpre16, H, sv["w16"][1], H, dact, H)
            bwd(dact.data_ptr(), sv["pre1"].data_ptr(), dpre1.data_ptr(), g["b1"].data_ptr(), part.data_ptr(), 1.0, inv, int(accumulate), M, H, st)
            self._dw(dpre1, sv["x16"], M, H, D, g["w1"], inv, accumulate)
            dh = None
            if want_dh:
                dh = torch.empty(M, D, device=dev)
                self._gemm(L.NN, M, D, H, dpre1, H, sv["w16"][0], D, dh, D, alpha=inv)
        return dh

    def _anchor(self):
        a = getattr(self, "_anchor_t", None)
        if a is None or a.device != self._pflat.device:
            a = torch.zeros(1, device=self._pflat.device, requires_grad=True)
            self._anchor_t = a
        return a

    def loss(self, hidden, feats):
        """hidden fp32 [N, T, in_dim] (``model.tapped_hidden``), feats fp16 or fp32 [N, T, feat_dim] -> the per-sample alignment loss [N]."""
        if hidden.dim() != 3:
            raise ValueError(f"RepaHead.loss: hidden of shape {tuple(hidden.shape)}, expected [N, T, {self.in_dim}]")
        return _RepaLossFunction.apply(self, hidden, feats, self._anchor())

    def forward(self, hidden, feats):
        return self.loss(hidden, feats)

    def __getstate__(self):
        st = dict(super().__getstate__() if hasattr(super(), "__getstate__") else self.__dict__)
        for k in ("_gflat", "_gviews", "_anchor_t"):
            st[k] = None
        return st
