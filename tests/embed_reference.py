"""fp64 references of the embedding, conditioning and output kernels (csrc/embed.hip) and of the converters beside them
(csrc/pointwise.hip), written from the model's semantics: patchify / unpatchify / mp_sum of the oracle on float64 tensors, the backward
formulas stated in closed form (tests/test_embed_reference_cpu.py holds each of them to fp64 autograd), and the helpers the GPU tests
need to speak about the 16-bit formats: the correctly rounded 16-bit value of an fp64 number and the spacing of the format there.

Nothing here imports the library or touches a device.
"""
import math

import numpy as np
import torch

from oracle.dit_oracle import MP_SILU_DIV, mp_sum, patchify, unpatchify

C5 = float(np.float32(0.70710678118654752))          # the fp32 constant of mp_sum(a, b, 0.5) = (a + b) * 0.5 / sqrt(0.5), as a double
SQRT2_F32 = float(np.float32(1.41421356237309515))
INV_SQRT8 = 1.0 / math.sqrt(8.0)
U24 = 2.0 ** -24                                     # unit roundoff of fp32


def grid(shape, rng):
    """Integers in [-128, 128] divided by 64, as float64: exact in bf16 (8 significant bits), fp16 and fp32.  A product of two is a
    multiple of 2^-12 of magnitude <= 4; a sum of up to 257 of them plus one more value stays below 2^11 in magnitude, so every partial
    sum in any order needs at most 11 + 12 = 23 bits below its leading one: exact in fp32, fused multiply-add or not."""
    return torch.from_numpy(rng.integers(-128, 129, size=tuple(shape)).astype(np.float64) / 64)


# ---- the 16-bit formats ------------------------------------------------------------------------------------------------------------
FORMATS = {"bf16": dict(dtype=torch.bfloat16, mant=7, emin=-126, emax=127), "f16": dict(dtype=torch.float16, mant=10, emin=-14, emax=15)}


def ulp16(v, fmt):
    """Spacing of the 16-bit format `fmt` in the binade of |v| (float64 array in, float64 array out; the subnormal spacing below emin)."""
    f = FORMATS[fmt]
    v = np.abs(np.asarray(v, dtype=np.float64))
    e = np.frexp(v)[1] - 1                                        # v = m 2^(e+1), 0.5 <= m < 1  ->  floor(log2 v) = e
    e = np.where(v == 0, f["emin"], np.clip(e, f["emin"], None))
    return np.ldexp(1.0, (e - f["mant"]).astype(np.int64))


def round16(v, fmt):
    """The fp64 value `v` rounded ONCE to the 16-bit format, ties to even, returned as float64 (torch's .to(bfloat16) of a double goes
    through fp32 first: two roundings).  Finite values inside the format's range only."""
    f = FORMATS[fmt]
    v = np.asarray(v, dtype=np.float64)
    q = ulp16(v, fmt)
    r = np.rint(v / q) * q                                        # v / q is exact (q a power of two); rint rounds half to even
    assert np.all(np.abs(r) < np.ldexp(2.0, f["emax"])), "round16: value outside the format's finite range"
    return r


def ulp_report(got, want64, fmt):
    """(worst |got - want| / ulp16(want), share of elements that differ from the correctly rounded value)."""
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    worst = float(np.max(np.abs(got - want64) / ulp16(want64, fmt)))
    share = float(np.mean(got != round16(want64, fmt)))
    return worst, share


# ---- patch embedding ---------------------------------------------------------------------------------------------------------------
def patch_rows(x, p):
    """[N, C, S, S] -> [N T, P + 1]: the patch rows with the ones column at index P."""
    h = patchify(x, p)
    h = torch.cat([h, torch.ones_like(h[:, :, :1])], -1)
    return h.reshape(-1, h.shape[-1])


def patch_embed_sum(x, w, pos, p):
    """rows W^T + pos (per sample): the plain sum of the embedding and the positional table, [N T, D]."""
    N = x.shape[0]
    y = patch_rows(x, p) @ w.t()
    return (y.reshape(N, -1, w.shape[0]) + pos.unsqueeze(0)).reshape(-1, w.shape[0])


def patch_embed_mp(x, w, pos, p):
    """mp_sum(embedding, pos, 0.5) of the model, [N T, D]."""
    N = x.shape[0]
    y = (patch_rows(x, p) @ w.t()).reshape(N, -1, w.shape[0])
    return mp_sum(y, pos.unsqueeze(0), 0.5).reshape(-1, w.shape[0])


# ---- timestep Fourier features -------------------------------------------------------------------------------------------------------
def fourier_arg_f32(t, scale, shift):
    """The fp32 argument as torch forms it (outer(), then +): the product rounded to fp32, then the add rounded.  numpy float32 arrays."""
    prod = (np.asarray(t).astype(np.float32)[:, None] * np.asarray(scale, dtype=np.float32)[None, :]).astype(np.float32)
    return (prod + np.asarray(shift, dtype=np.float32)[None, :]).astype(np.float32)


def fourier_ref(t, scale, shift):
    """sqrt(2) cos(arg) in fp64 of the fp32-emulated argument, [n, F] float64 numpy."""
    return math.sqrt(2.0) * np.cos(fourier_arg_f32(t, scale, shift).astype(np.float64))


# ---- conditioning --------------------------------------------------------------------------------------------------------------------
def mp_silu64(c):
    return torch.nn.functional.silu(c) / MP_SILU_DIV


def dmp_silu64(c):
    """d/dc [silu(c) / 0.596] in closed form."""
    s = torch.sigmoid(c)
    return s * (1 + c * (1 - s)) / MP_SILU_DIV


def cond_combine_ref(temb, table, y):
    """c = mp_sum(t_emb, y_emb, 0.5) = (t_emb + table[y]) * sqrt(0.5)."""
    return mp_sum(temb, table[y], 0.5)


def cond_combine_bwd_ref(c, dcs, dcd, y, table_rows):
    """Gradients of  sum(mp_silu(c) dcs) + sum(c dcd)  with c = (temb + table[y]) C5:  dc = dcs f'(c) + dcd,  dtemb = C5 dc,
    dtable[r] = sum over the samples that carry label r of C5 dc.  Returns (dtemb, dtable [table_rows, D], terms) where
    terms[o] = |dcs f'(c)| + |dcd| of sample o (what the error bound of dtable is stated in)."""
    a = dcs * dmp_silu64(c)
    dtemb = (a + dcd) * math.sqrt(0.5)
    dtable = torch.zeros(table_rows, c.shape[1], dtype=c.dtype)
    dtable.index_add_(0, y, dtemb)
    return dtemb, dtable, a.abs() + dcd.abs()


# ---- final layer tail ----------------------------------------------------------------------------------------------------------------
def gates_ref(a, ref):
    """MPScale gate per sample: sigmoid(a . ref / sqrt(8)), a [N, 8], ref [8]."""
    return torch.sigmoid(a @ ref * INV_SQRT8)


def final_out_ref(lin, gm, gs, N, S, p):
    """lin [N T, 2P] (mean chunk, sigma chunk), gates gm, gs [N] -> [N, 2C, S, S]."""
    mean, sigma = lin.reshape(N, -1, lin.shape[-1]).chunk(2, -1)
    return torch.cat([unpatchify(mean * gm.view(-1, 1, 1), S, p), unpatchify(sigma * gs.view(-1, 1, 1), S, p)], 1)


def final_out_bwd_ref(dout, lin, a_mean, a_sigma, ref_mean, ref_sigma, gm, gs, p):
    """Closed-form backward of final_out_ref(lin, gates_ref(a_mean, ref_mean), gates_ref(a_sigma, ref_sigma)) for the upstream gradient
    dout, at the GIVEN gate values gm, gs (so that a test can hand in the gates a device computed).  Returns a dict:
    dlin [N T, 2P]; da_mean, da_sigma [N, 8]; dref_mean, dref_sigma [8]; dg_mean, dg_sigma [N] = sum(dout lin) over the chunk (the
    gradient of the gate); and for the error bounds abs_mean, abs_sigma [N] = sum |dout lin| over the chunk (what the reduction adds)
    and kap_mean, kap_sigma [N] = g (1 - g) / sqrt(8)."""
    N, C2 = dout.shape[0], dout.shape[1]
    Cc = C2 // 2
    dm, ds = patchify(dout[:, :Cc], p), patchify(dout[:, Cc:], p)                  # [N, T, P]
    mean, sigma = lin.reshape(N, -1, lin.shape[-1]).chunk(2, -1)
    r = dict(dlin=torch.cat([dm * gm.view(-1, 1, 1), ds * gs.view(-1, 1, 1)], -1).reshape(-1, lin.shape[-1]))
    for name, d, l, g, a, ref in (("mean", dm, mean, gm, a_mean, ref_mean), ("sigma", ds, sigma, gs, a_sigma, ref_sigma)):
        dg = (d * l).sum((1, 2))
        kap = g * (1 - g) * INV_SQRT8
        dang = dg * kap
        r["da_" + name] = dang.unsqueeze(1) * ref.unsqueeze(0)
        r["dref_" + name] = (dang.unsqueeze(1) * a).sum(0)
        r["dg_" + name] = dg
        r["abs_" + name] = (d * l).abs().sum((1, 2))
        r["kap_" + name] = kap
    return r


# ---- classifier-free guidance tail -----------------------------------------------------------------------------------------------------
def cfg_combine_ref(x, C, s):
    """x [n_total, 2C, HW]: eps = u + s (c - u) on the first C channels, written to both halves; the other channels pass through."""
    half = x.shape[0] // 2
    cond, unc = x[:half, :C], x[half:, :C]
    eps = unc + s * (cond - unc)
    return torch.cat([torch.cat([eps, eps], 0), x[:, C:]], 1)


def cfg_combine_bwd_ref(dout, C, s):
    """Adjoint of cfg_combine_ref in closed form: with g = dout[n] + dout[n + half] on the first C channels the conditional rows take
    s g and the unconditional rows (1 - s) g."""
    half = dout.shape[0] // 2
    g = dout[:half, :C] + dout[half:, :C]
    return torch.cat([torch.cat([s * g, (1 - s) * g], 0), dout[:, C:]], 1)
