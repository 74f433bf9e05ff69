"""The embedding, conditioning and output kernels (csrc/embed.hip) and the converters beside them (csrc/pointwise.hip) through the C
ABI, one by one, on every code path: against the fp64 references of tests/embed_reference.py (checked on the CPU by
tests/test_embed_reference_cpu.py), element by element.

Conventions of every case.  Outputs are pre-filled with NaN (16-bit padding columns with a sentinel), every output carries GUARD = 64
rows after its last legal row and those rows - like all padding - must come back with the bits they had.  Where the operands come from
R.grid (integers / 64) every fp32 sum the kernel forms is exact, so the result is compared with torch.equal.  Elsewhere the bound is
stated in the test's docstring, derived from the operation count and the formats; "within 1 ulp" of a 16-bit format means
|got - want64| <= spacing of the format at want64, and the share of elements that are not THE correctly rounded value of want64 must
not exceed 1 %.  Every test prints the worst ratio to its bounds ("ratio ..." lines, pytest -s).
"""
import math

import numpy as np
import pytest
import torch

import embed_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
NAN = float("nan")
SENTINEL = 7.0
U24 = R.U24
FMT = pytest.mark.parametrize("fmt", ["bf16", "f16"])
TWINS = {"f32_to_bf16": "f32_to_f16", "f32_to_bf16_2d": "f32_to_f16_2d", "mpsilu_to_bf16": "mpsilu_to_f16"}


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------
def entry(name, fmt="bf16"):
    from mapdit_amd import _lib as L
    if fmt == "f16":
        name = TWINS.get(name, name + "_f16")
    return getattr(L.lib(), name)


def st():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


def dt_of(fmt):
    return R.FORMATS[fmt]["dtype"]


def dev32(t64):
    """An fp64 host tensor on the device as fp32; the value must survive (grid operands, or values already rounded to fp32)."""
    t = t64.float()
    assert torch.equal(t.double(), t64)
    return t.to(DEV).contiguous()


def padded(t, ld, fill=NAN):
    """[rows, cols] -> device [rows, ld] with `fill` in the padding columns."""
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype, device=DEV)
    out[:, :t.shape[1]] = t.to(DEV)
    return out


def guarded(rows, cols, dtype=torch.float32, fill=NAN):
    return torch.full((rows + GUARD, cols), fill, dtype=dtype, device=DEV)


def bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def all_sentinel(t):
    return same_bits(t, torch.full_like(t.contiguous(), SENTINEL))


def f64(t):
    return t.detach().double().cpu()


def within(got, want, tol):
    """Worst |got - want| / tol over the elements (0 / 0 counts as 0); tensors or arrays, fp64."""
    got, want, tol = (np.asarray(z, dtype=np.float64) for z in (got, want, tol))
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300))))


class Ulps:
    """Accumulates the 1-ulp checks of one test: worst distance in ulps and the share of not correctly rounded elements."""

    def __init__(self, fmt):
        self.fmt, self.worst, self.bad, self.total = fmt, 0.0, 0, 0

    def add(self, got16, want64):
        got, want = f64(got16).numpy(), np.asarray(want64, dtype=np.float64)
        assert got.shape == want.shape and np.isfinite(got).all()
        self.worst = max(self.worst, float(np.max(np.abs(got - want) / R.ulp16(want, self.fmt))))
        self.bad += int(np.sum(got != R.round16(want, self.fmt)))
        self.total += got.size

    def check(self, what):
        share = self.bad / max(self.total, 1)
        print(f"ratio {what} {self.fmt}: worst {self.worst:.3f} ulp (limit 1), not correctly rounded {self.bad}/{self.total} = {share:.2e} (limit 1e-2)")
        assert self.worst <= 1.0
        assert share <= 0.01


# ---- patch_embed_fwd -------------------------------------------------------------------------------------------------------------------
PE_SHAPES = [((3, 4, 16, 2, 128), "reg_full_tiles"), ((5, 4, 12, 2, 384), "reg_T36_M180_three_passes"), ((1, 4, 8, 2, 128), "reg_M16"),
             ((1, 1, 16, 4, 128), "reg_C1_p4"), ((5, 3, 12, 2, 128), "generic_P13_tail"), ((2, 8, 8, 2, 256), "generic_P33_two_tiles"),
             ((3, 4, 20, 4, 256), "generic_P65_T25_M75"), ((3, 4, 16, 8, 128), "f64tile_P257_M12"), ((40, 4, 16, 8, 256), "f64tile_P257_M160")]


@FMT
@pytest.mark.parametrize("shape", [s for s, _ in PE_SHAPES], ids=[i for _, i in PE_SHAPES])
def test_patch_embed_fwd(shape, fmt):
    """Grid operands: every product is a multiple of 2^-12, every partial sum of the P + 1 <= 257 products and the positional value is
    below 2^11 - exact in fp32 in any order, with or without contraction.  out_scale 1 is therefore the fp64 sum itself; out_scale 0
    multiplies the exact sum by float32(0.70710678118654752): one rounding.  The patch rows are copies (exact in both 16-bit formats)."""
    N, C_, S, p_, D = shape
    P, T = p_ * p_ * C_, (S // p_) ** 2
    M = N * T
    rng = np.random.default_rng(list(shape))
    x, w, pos = R.grid((N, C_, S, S), rng), R.grid((D, P + 1), rng), R.grid((T, D), rng)
    rows, want1 = R.patch_rows(x, p_), R.patch_embed_sum(x, w, pos, p_)
    assert rows.shape == (M, P + 1) and want1.shape == (M, D) and torch.equal(want1.float().double(), want1)
    want0 = (want1.float() * torch.tensor(R.C5, dtype=torch.float32)).double()              # one fp32 rounding of the exact sum
    mp = R.patch_embed_mp(x, w, pos, p_)
    assert float((want0 - mp).abs().max()) <= 2.0 ** -23 * float(mp.abs().max())            # ... and it is the model's mp_sum
    xd, wd, pd = dev32(x), dev32(w), guarded(T, D)                                          # pos: T rows, NaN in the rows after them
    pd[:T] = dev32(pos)
    ldp0 = (P + 1 + 7) // 8 * 8
    fn = entry("patch_embed_fwd", fmt)
    for ldp in (ldp0, ldp0 + 8, None):
        for out_scale, want in ((1.0, want1), (0.0, want0)):
            out = guarded(M, D)
            patches = None if ldp is None else guarded(M, ldp, dt_of(fmt))
            fn(p(xd), p(wd), p(pd), p(out), p(patches), ldp or ldp0, N, C_, S, p_, D, out_scale, st())
            torch.cuda.synchronize()
            assert torch.equal(f64(out[:M]), want), (ldp, out_scale)
            assert bool(torch.isnan(out[M:]).all())
            if patches is not None:
                assert torch.equal(f64(patches[:M, :P + 1]), rows)                          # (the ones column at index P included)
                assert float(f64(patches[:M, P]).min()) == 1.0
                assert float(f64(patches[:M, P + 1:]).abs().max()) == 0.0 and not bool(torch.isnan(patches[:M, P + 1:]).any())
                assert bool(torch.isnan(patches[M:]).all())


# ---- final_out_fwd / final_out_bwd -------------------------------------------------------------------------------------------------------
FO_SHAPES = [((3, 4, 16, 2), "N3"), ((16, 3, 6, 2), "N16_one_round_per216"), ((35, 4, 8, 2), "N35_two_rounds_plus3"), ((17, 4, 16, 8), "N17_p8"),
             ((2, 4, 20, 4), "N2_p4_T25")]


def run_final_out(fmt, shape, lin, am, asg, rm, rs, dout, prior_m, prior_s, gscale, ldl, ldd):
    """One forward and one backward on fresh buffers; every output returned with its guard rows checked."""
    N, C_, S, p_ = shape
    P, T = p_ * p_ * C_, (S // p_) ** 2
    M, dt = N * T, dt_of(fmt)
    lind = padded(lin, ldl)                                                                 # NaN in the padding columns of lin
    d = [z.to(DEV).contiguous() for z in (am, asg, rm, rs, dout)]
    out = guarded(N, 2 * C_ * S * S)
    entry("final_out_fwd")(p(lind), ldl, p(d[0]), p(d[1]), p(d[2]), p(d[3]), p(out), N, C_, S, p_, st())
    dlin = guarded(M, ldd, dt, SENTINEL)
    da = guarded(2 * N, 8, dt)
    part = guarded(N, 16)
    drm, drs = guarded(1, 8), guarded(1, 8)
    drm[0], drs[0] = prior_m.to(DEV), prior_s.to(DEV)
    entry("final_out_bwd", fmt)(p(d[4]), p(lind), ldl, p(d[0]), p(d[1]), p(d[2]), p(d[3]), p(dlin), ldd, p(da), p(part), p(drm), p(drs),
                                gscale, N, C_, S, p_, st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[N:]).all()) and bool(torch.isnan(da[2 * N:]).all()) and bool(torch.isnan(part[N:]).all())
    assert bool(torch.isnan(drm[1:]).all()) and bool(torch.isnan(drs[1:]).all())
    assert all_sentinel(dlin[M:]) and all_sentinel(dlin[:M, 2 * P:])                        # columns >= 2P are not this kernel's
    return dict(out=out[:N].reshape(N, 2 * C_, S, S), dlin=dlin[:M, :2 * P], da=da[:2 * N].reshape(2, N, 8), part=part[:N], drm=drm[0], drs=drs[0])


def leading_dims(P):
    ldd0 = max(2 * P, 64)
    return [(2 * P, ldd0), (2 * P + 8, ldd0 + 8)]


@FMT
@pytest.mark.parametrize("gscale", [1.0, 2.0 ** -3], ids=["gs1", "gs2^-3"])
@pytest.mark.parametrize("shape", [s for s, _ in FO_SHAPES], ids=[i for _, i in FO_SHAPES])
def test_final_out_index_mode(shape, gscale, fmt):
    """a_mean = a_sigma = 0: both gates are 1 / (1 + exp(-0)) = 0.5 exactly, so with grid lin / dout and a power-of-two grad_scale the
    kernels only MOVE values: out = 0.5 lin rearranged and dlin = grad_scale 0.5 dout rearranged, exact in fp32 and in both 16-bit
    formats.  dg = sum(dout lin) is a sum of multiples of 2^-12 whose absolute values add up to less than 2^12 (asserted): exact in any
    order, so da = cvt16((grad_scale ((dg 0.5) 0.5) float32(1/sqrt 8)) ref) is reproduced rounding by rounding in numpy float32, and
    dref_part = dang * 0 leaves dref at its prior contents, bit for bit."""
    N, C_, S, p_ = shape
    P, T = p_ * p_ * C_, (S // p_) ** 2
    rng = np.random.default_rng(list(shape))
    lin, dout = R.grid((N * T, 2 * P), rng), R.grid((N, 2 * C_, S, S), rng)
    rm, rs = R.grid((8,), rng), R.grid((8,), rng)
    prior_m, prior_s = R.grid((8,), rng) + 3, R.grid((8,), rng) - 3                         # non-zero
    zero = torch.zeros(N, 8, dtype=torch.float64)
    half = torch.full((N,), 0.5, dtype=torch.float64)
    want_out = R.final_out_ref(lin, half, half, N, S, p_)
    r = R.final_out_bwd_ref(dout, lin, zero, zero, rm, rs, half, half, p_)
    want_dlin = r["dlin"] * gscale
    assert float(r["abs_mean"].max()) < 4096 and float(r["abs_sigma"].max()) < 4096
    k32 = np.float32(0.35355339059327379)
    want_da = []
    for name, ref in (("mean", rm), ("sigma", rs)):
        dg = r["dg_" + name].numpy()
        dg32 = dg.astype(np.float32)
        assert np.array_equal(dg32.astype(np.float64), dg)
        dang = ((dg32 * np.float32(0.5)) * np.float32(0.5)) * k32
        want_da.append((np.float32(gscale) * dang)[:, None] * ref.numpy().astype(np.float32)[None, :])
    want_da = torch.from_numpy(np.stack(want_da)).to(dt_of(fmt))
    first = None
    for ldl, ldd in leading_dims(P):
        for rep in range(2):
            o = run_final_out(fmt, shape, lin.float(), zero.float(), zero.float(), rm.float(), rs.float(), dout.float(), prior_m.float(),
                              prior_s.float(), gscale, ldl, ldd)
            assert torch.equal(f64(o["out"]), want_out), (ldl, ldd)
            assert torch.equal(f64(o["dlin"]), want_dlin), (ldl, ldd)
            assert same_bits(o["da"].cpu(), want_da), (ldl, ldd)
            assert float(f64(o["part"]).abs().max()) == 0.0
            assert torch.equal(f64(o["drm"]), prior_m) and torch.equal(f64(o["drs"]), prior_s)
            if first is None:
                first = o
            for k in o:                                                                     # no atomics: a repeat, and another row pitch, give the same bits
                assert same_bits(o[k], first[k]), (k, ldl, ldd, rep)


@FMT
@pytest.mark.parametrize("shape", [s for s, _ in FO_SHAPES], ids=[i for _, i in FO_SHAPES])
def test_final_out_value_mode(shape, fmt):
    """Random a_*, ref_*, lin, dout; grad_scale 0.37.

    Gates (read off a call with lin = 1, where out IS the gate), in units of u = 2^-24 and with A = sum |a ref| / sqrt 8:  s is 8 fp32
    products, 8 adds and the multiply by float32(1/sqrt 8): 17 roundings of partial results bounded by A, |ds| <= 17 u A.  The fast
    exponential is exp2(-s log2 e): the rounding of its argument is a relative error |s| u <= A u of e, the hardware adds 1 ulp (2 u);
    1 + e rounds once and the division is at most 2.5 ulp (5 u) in its fast form.  The gate's slope in s is at most 1/4 and a relative
    error of e reaches g through g (1 - g) <= 1/4:  |dg| <= (17 A + A + 2) u / 4 + (1 + 5) u g <= (4.5 A + 6.5) u <= 8 u (1 + A) =
    2^-21 (1 + A).  out itself is one fp32 product of lin and that gate: bit-equal to the host's fp32 product.

    The backward is compared with the fp64 formulas evaluated at the DEVICE's gates (the gates are pinned on their own above; like c in the
    cond_combine tests, what a kernel read is what its reference reads).  dlin = cvt16((grad_scale dout) g): two fp32 roundings in front of
    the 16-bit one - within 1 ulp.  dg = sum over the chunk's n = C S S products dout lin, in whatever order the block reduces them:
    |error| <= n 2^-24 sum |dout lin|; the six multiplications that follow (g, 1 - g and its subtraction, 1/sqrt 8, grad_scale, ref; or a)
    are relative roundings of a value bounded by the same sum: da within (n + 8) 2^-24 kap |grad_scale ref_j| sum |dout lin| plus the 16-bit
    rounding (1 ulp), kap = g (1 - g) / sqrt 8.  dref_j = prior + sum over the N samples, in sample order: the N additions round partial
    sums bounded by the absolute sum of everything added, the prior included: within (n + N + 8) 2^-24 (|prior_j| + sum_n kap_n |a_nj| sum |dout lin|_n).
    """
    N, C_, S, p_ = shape
    P, T = p_ * p_ * C_, (S // p_) ** 2
    n_terms = C_ * S * S
    g = torch.Generator().manual_seed(1000 + N * S)
    rn = lambda *s: torch.randn(*s, generator=g).double()                                  # fp32 values, held as fp64
    lin, dout, am, asg, rm, rs = rn(N * T, 2 * P), rn(N, 2 * C_, S, S), rn(N, 8), rn(N, 8), rn(8), rn(8)
    prior_m, prior_s = rn(8) + 2, rn(8) - 2
    gscale = float(np.float32(0.37))
    f = lambda *ts: [t.float() for t in ts]
    # the gates
    ones = torch.ones_like(lin)
    o1 = run_final_out(fmt, shape, *f(ones, am, asg, rm, rs, dout, prior_m, prior_s), gscale, 2 * P, max(2 * P, 64))
    gd = f64(o1["out"]).reshape(N, 2, -1)
    assert torch.equal(gd, gd[:, :, :1].expand_as(gd))                                      # one value per (sample, chunk)
    gm_d, gs_d = gd[:, 0, 0].clone(), gd[:, 1, 0].clone()
    worst_gate = 0.0
    for got, a, ref in ((gm_d, am, rm), (gs_d, asg, rs)):
        A = (a * ref).abs().sum(1) * R.INV_SQRT8
        worst_gate = max(worst_gate, within(got, R.gates_ref(a, ref), 2.0 ** -21 * (1 + A)))
    print(f"ratio final_out gate {fmt}: {worst_gate:.3f}")
    assert worst_gate <= 1.0
    # forward and backward at the device's gates
    want_out = R.final_out_ref(lin.float(), gm_d.float(), gs_d.float(), N, S, p_)          # fp32 on the host: the same single rounding
    r = R.final_out_bwd_ref(dout, lin, am, asg, rm, rs, gm_d, gs_d, p_)
    ul, first = Ulps(fmt), None
    worst_da = worst_dref = lit_da = lit_dref = 0.0
    for ldl, ldd in leading_dims(P):
        for rep in range(2):
            o = run_final_out(fmt, shape, *f(lin, am, asg, rm, rs, dout, prior_m, prior_s), gscale, ldl, ldd)
            if first is None:
                first = o
            for k in o:
                assert same_bits(o[k], first[k]), (k, ldl, ldd, rep)
        assert same_bits(o["out"].cpu(), want_out), (ldl, ldd)
        ul.add(o["dlin"], (r["dlin"] * gscale).numpy())
        for w, (name, ref, a, prior, got_ref) in enumerate((("mean", rm, am, prior_m, o["drm"]), ("sigma", rs, asg, prior_s, o["drs"]))):
            want_da = r["da_" + name] * gscale
            scale = (r["abs_" + name] * r["kap_" + name]).unsqueeze(1)                      # [N, 1]
            tol_da = (n_terms + 8) * U24 * scale * (gscale * ref).abs().unsqueeze(0) + torch.from_numpy(R.ulp16(want_da.numpy(), fmt))
            worst_da = max(worst_da, within(f64(o["da"][w]), want_da, tol_da))
            tol_ref = (n_terms + N + 8) * U24 * (prior.abs() + (scale * a.abs()).sum(0))
            worst_dref = max(worst_dref, within(f64(got_ref), prior + r["dref_" + name], tol_ref))
            # reported only: the same figures against the count of the reduction's terms alone, without the roundings that follow it
            lit_da = max(lit_da, within(f64(o["da"][w]), want_da, tol_da - 8 * U24 * scale * (gscale * ref).abs().unsqueeze(0)))
            lit_dref = max(lit_dref, within(f64(got_ref), prior + r["dref_" + name], tol_ref * n_terms / (n_terms + N + 8)))
            # the per-sample parts: the same bound without the sum over samples
            want_part = (r["dg_" + name] * r["kap_" + name]).unsqueeze(1) * a
            worst_dref = max(worst_dref, within(f64(o["part"]).reshape(N, 2, 8)[:, w], want_part, (n_terms + 8) * U24 * scale * a.abs()))
    print(f"ratio final_out da {fmt}: {worst_da:.3f}   dref {fmt}: {worst_dref:.3f}   (with n_terms = C S S alone: da {lit_da:.3f}, dref {lit_dref:.3f})")
    ul.check("final_out dlin")
    assert worst_da <= 1.0
    assert worst_dref <= 1.0


# ---- cond_combine_fwd / cond_combine_bwd -------------------------------------------------------------------------------------------------
def label_patterns(n, rows, rng):
    """The label vectors of one (n, table_rows): who owns a table row, and which later samples it has to add, is decided by these."""
    null = rows - 1
    distinct = rng.permutation(rows)[:n] if rows >= n else rng.permutation(np.arange(n) % rows)      # n > rows: every label n / rows times, scattered
    others = rng.integers(1, null, size=n)
    among = np.where(np.arange(n) % 2 == 0, null, others)                                   # the null row at 0, 2, 4, ... among other labels
    ends = np.where(rng.integers(0, 2, size=n) == 0, 0, null)
    if n > 1:
        ends[0], ends[-1] = null, 0
    return {"distinct": distinct, "all_equal": np.full(n, 3), "null_among_others": among, "first_and_null_row": ends}


@FMT
@pytest.mark.parametrize("n", [1, 5, 33])
@pytest.mark.parametrize("D", [128, 384, 1152])
def test_cond_combine(D, n, fmt):
    """Grid temb / table: temb + row is exact, c = (temb + row) float32(0.70710678118654752) is one fp32 rounding (bit-equal to the host's), c_bf its
    16-bit rounding (bit-equal), c_silu = cvt16(c / (1 + exp(-c)) / 0.596): a handful of fp32 roundings in front of the 16-bit one.

    Backward, from the device's fp32 c.  The upstream gradients are built so that dc = dcs f'(c) + dcd does not cancel: with a random sign
    sg per element, dcd = sg (1 + u), u in [0, 1], and dcs = sg v, v in [0, 2]; f' = d mp_silu lies in [-0.17, 1.85], so |dc| >= 1 - 0.34
    while |dcs f'| + |dcd| <= 5.7: the fp32 evaluation (error below 2^-20 of the terms, next paragraph) stays far inside one 16-bit ulp of
    dc, and dtemb = cvt16(dc C5) is held to 1 ulp.
    dtable[r] = prior + sum over the samples o with label r, in sample order, of dc_o C5, held to 2^-20 sum_o T_o with T_o = |dcs_o f'(c_o)|
    + |dcd_o|: a budget of 16 roundings of 2^-24 T each, counted as follows.  A term passes through twelve fp32 roundings (the exponential's
    argument, the exponential, 1 + e, the reciprocal, 1 - s, c (1 - s), 1 + ., s ., / 0.596, dcs ., + dcd, . C5), each relative to an
    intermediate; the intermediates of f' reach s (1 + |c| (1 - s)) / 0.596 <= 1.5 also where f' itself is near zero, which is why the bound
    needs |dcd_o| >= 1 inside T_o (|dcs| <= 2, |c| <= 2.9 here): 12 u T_o per term, u = 2^-24.  The sample-order sum rounds each of its k
    partial sums once, sum_i u |s_i| <= u C5 sum_j (k - j + 1) T_j - for terms of like size C5 (k + 1) / 2 u sum T - and the += rounds
    |prior + sum| <= 2 + C5 sum T once more.  Up to k = 5 (n = 1, 5; every pattern but the repeated labels at n = 33) that is 12 + 2.2 + 1.5
    <= 16 roundings: a first-order worst case, and there the limit is derived.  For the repeated labels at n = 33 (k up to 33) it is NOT:
    the same count gives 12 + 12 + 1.5 = 25.5 u sum T, so at those cases the limit 2^-20 sum T is the issue's figure, kept as set, and not
    a worst-case envelope.  What can be said for it there is a second-moment estimate: with the roundings taken as independent and uniform
    (rms u / sqrt 3 of the value rounded), the variance is at most u^2 / 3 (12 sum T_o^2 + C5^2 sum_i (sum T)^2) <= u^2 / 3 (12 + k / 2)
    (sum T)^2, an rms error of at most 3.1 u sum T at k = 33 - the limit of 16 u sits five such deviations out, and a kernel that drops or
    doubles one of k terms is off by about sum T / k = 2^19 u sum T / k.  The measured ratio is printed."""
    dt = dt_of(fmt)
    ul_silu, ul_dtemb, worst_dtable = Ulps(fmt), Ulps(fmt), 0.0
    c5 = torch.tensor(R.C5, dtype=torch.float32)
    fwd, bwd = entry("cond_combine_fwd", fmt), entry("cond_combine_bwd", fmt)
    for rows in (11, 1001):
        rng = np.random.default_rng([D, n, rows])
        temb, table = R.grid((n, D), rng), R.grid((rows, D), rng)
        sg = torch.from_numpy(rng.integers(0, 2, size=(n, D)) * 2.0 - 1)
        dcd = sg * (1 + torch.from_numpy(rng.integers(0, 65, size=(n, D)) / 64))
        dcs = sg * torch.from_numpy(rng.integers(0, 129, size=(n, D)) / 64)
        prior = R.grid((rows, D), rng)
        prior[prior == 0] = 0.5
        td, tabd, dcsd, dcdd = dev32(temb), dev32(table), dev32(dcs), dev32(dcd)
        for pattern, y in label_patterns(n, rows, rng).items():
            y = torch.from_numpy(np.asarray(y, dtype=np.int64))
            assert int(y.min()) >= 0 and int(y.max()) < rows
            yd = y.to(DEV)
            want_c = (temb + table[y]).float() * c5
            assert float((want_c.double() - R.cond_combine_ref(temb, table, y)).abs().max()) <= 2.0 ** -23 * 4
            runs = []
            for rep in range(2):
                c, cs, cb = guarded(n, D), guarded(n, D, dt), guarded(n, D, dt)
                fwd(p(td), p(tabd), p(yd), p(c), p(cs), p(cb), n, D, rows, st())
                dtemb = guarded(n, D, dt)
                dtable = guarded(rows, D)
                dtable[:rows] = prior.float().to(DEV)
                bwd(p(c), p(dcsd), p(dcdd), p(yd), p(dtemb), p(dtable), n, D, rows, st())
                torch.cuda.synchronize()
                for buf, legal in ((c, n), (cs, n), (cb, n), (dtemb, n), (dtable, rows)):
                    assert bool(torch.isnan(buf[legal:]).all()), pattern
                runs.append([z.clone() for z in (c[:n], cs[:n], cb[:n], dtemb[:n], dtable[:rows])])
            for a, b in zip(*runs):
                assert same_bits(a, b), pattern                                             # no atomics
            c, cs, cb, dtemb, dtable = runs[0]
            assert same_bits(c.cpu(), want_c), pattern
            assert same_bits(cb.cpu(), want_c.to(dt)), pattern
            c64 = f64(c)
            ul_silu.add(cs, R.mp_silu64(c64).numpy())
            want_dtemb, want_dtable, terms = R.cond_combine_bwd_ref(c64, dcs, dcd, y, rows)
            ul_dtemb.add(dtemb, want_dtemb.numpy())
            used = torch.zeros(rows, dtype=torch.bool)
            used[y] = True
            assert same_bits(dtable[~used.to(DEV)].cpu(), prior.float()[~used]), pattern    # rows of unused labels: bit-unchanged
            tsum = torch.zeros(rows, D, dtype=torch.float64).index_add_(0, y, terms)
            worst_dtable = max(worst_dtable, within(f64(dtable)[used], (prior + want_dtable)[used], 2.0 ** -20 * tsum[used]))
    print(f"ratio cond_combine dtable {fmt}: {worst_dtable:.3f}")
    ul_silu.check("cond_combine c_silu")
    ul_dtemb.check("cond_combine dtemb")
    assert worst_dtable <= 1.0


# ---- fourier_fwd ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,F", [(5, 256), (3, 96), (1, 256), (7, 32)])
def test_fourier_fwd(n, F):
    """The argument is reproduced rounding by rounding (product rounded, then the add: tests/test_embed_reference_cpu.py); the device's
    cosf and the multiply by float32(sqrt 2) are a few fp32 ulps in front of the bf16 rounding: within 1 bf16 ulp of sqrt 2 cos in fp64,
    all but 1 % of the elements the correctly rounded value.  (One format: the Fourier features are bf16 in every engine precision.)"""
    g = torch.Generator().manual_seed(14 + n)
    scale, shift = 2 * math.pi * torch.randn(F, generator=g), 2 * math.pi * torch.rand(F, generator=g)
    t = torch.randint(0, 1000, (n,), generator=g)
    t[-1] = 999
    if n > 1:
        t[0] = 0
    want = R.fourier_ref(t.numpy(), scale.numpy(), shift.numpy())
    out = guarded(n, F, torch.bfloat16)
    td, sd, hd = t.to(DEV), scale.to(DEV), shift.to(DEV)
    entry("fourier_fwd")(p(td), p(sd), p(hd), p(out), n, F, st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[n:]).all())
    ul = Ulps("bf16")
    ul.add(out[:n], want)
    ul.check("fourier_fwd")


# ---- cfg_combine / cfg_combine_bwd -----------------------------------------------------------------------------------------------------------
def run_cfg(which, x, n, C_, HW, s):
    xd = x.float().to(DEV).contiguous()
    out = guarded(n, 2 * C_ * HW)
    entry(which)(p(xd), p(out), n, C_, HW, s, st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[n:]).all())
    return f64(out[:n]).reshape(n, 2 * C_, HW)


@pytest.mark.parametrize("n,C_,HW", [(2, 4, 64), (6, 4, 64), (10, 3, 25), (4, 4, 1024)])
def test_cfg_combine_both_directions(n, C_, HW):
    """Grid operands and a dyadic scale: c - u, s (c - u), u + s (c - u), g = a + b, s g and (1 - s) g are all exact in fp32 - torch.equal
    to fp64, in both directions.  s = 1.37 (random operands): forward u + s (c - u) is three roundings (two with contraction), each
    relative to an intermediate bounded by |u| + |s| (|c| + |u|): within 3 2^-24 (|u| + |s| (|c| + |u|)); backward k (a + b) with k = s
    or 1 - s: the add, 1 - s and the product, three relative roundings: within 3 2^-24 |k| (|a| + |b|).  The channels past C pass through
    bit for bit.  The adjoint identity <dout, fwd(x)> = <bwd(dout), x>, evaluated in fp64 on the device's results, holds to the sum of those
    element bounds weighted by |dout| and |x|."""
    half = n // 2
    rng = np.random.default_rng([n, C_, HW])
    x, dout = R.grid((n, 2 * C_, HW), rng), R.grid((n, 2 * C_, HW), rng)
    for s in (1.5, 1.0, 0.0, 4.0, -0.5):
        assert torch.equal(run_cfg("cfg_combine", x, n, C_, HW, s), R.cfg_combine_ref(x, C_, s)), s
        assert torch.equal(run_cfg("cfg_combine_bwd", dout, n, C_, HW, s), R.cfg_combine_bwd_ref(dout, C_, s)), s
    g = torch.Generator().manual_seed(n * HW)
    x, dout = torch.randn(n, 2 * C_, HW, generator=g).double(), torch.randn(n, 2 * C_, HW, generator=g).double()
    s = float(np.float32(1.37))
    fx, bd = run_cfg("cfg_combine", x, n, C_, HW, 1.37), run_cfg("cfg_combine_bwd", dout, n, C_, HW, 1.37)
    want_f, want_b = R.cfg_combine_ref(x, C_, s), R.cfg_combine_bwd_ref(dout, C_, s)
    assert torch.equal(fx[:, C_:], x[:, C_:]) and torch.equal(bd[:, C_:], dout[:, C_:])
    c, u = x[:half, :C_].abs(), x[half:, :C_].abs()
    tol_f = 3 * U24 * (u + abs(s) * (c + u)).repeat(2, 1, 1)
    gsum = dout[:half, :C_].abs() + dout[half:, :C_].abs()
    tol_b = 3 * U24 * torch.cat([abs(s) * gsum, abs(1 - s) * gsum], 0)
    rf, rb = within(fx[:, :C_], want_f[:, :C_], tol_f), within(bd[:, :C_], want_b[:, :C_], tol_b)
    lhs, rhs = float((dout * fx).sum()), float((bd * x).sum())
    tol_adj = float((dout[:, :C_].abs() * tol_f).sum() + (x[:, :C_].abs() * tol_b).sum())
    print(f"ratio cfg_combine fwd {rf:.3f}  bwd {rb:.3f}  adjoint {abs(lhs - rhs) / tol_adj:.3f}")
    assert rf <= 1.0
    assert rb <= 1.0
    assert abs(lhs - rhs) <= tol_adj


# ---- converters ------------------------------------------------------------------------------------------------------------------------------
EDGES = [0.0, -0.0, float("inf"), -float("inf"), NAN,
         1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -23,          # bf16 ties (to even: down, up), just above a tie
         1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 3 * 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -23,  # fp16 ties
         65504.0, -65504.0, 65519.0, 65520.0, 65536.0, 1e5, -1e5,                               # fp16: largest finite, below / on / above the overflow tie
         3.3895313892515355e38, 3.4028234663852886e38, -3.4028234663852886e38,                  # bf16's largest finite; fp32's (rounds to bf16 inf)
         2.0 ** -14, 2.0 ** -15, 1e-5, 6e-8, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -10), 3 * 2.0 ** -25, 1e-8,   # normal fp32, subnormal fp16
         -1e-5, 2.0 ** -14 * (1 - 2.0 ** -11), 2.0 ** -126]


@FMT
def test_f32_to_16_matches_the_host_cast(fmt):
    """v_cvt rounds to nearest even, keeps the sign of zero, overflows to inf and (fp16) produces subnormals: every result is the bit
    pattern of torch's CPU cast.  NaN payloads are not compared (isnan on both sides)."""
    dt = dt_of(fmt)
    g = torch.Generator().manual_seed(21)
    for x in (torch.randn(1000, generator=g) * 3, torch.tensor(EDGES, dtype=torch.float32)):
        n = x.numel()
        out = torch.full((n + GUARD,), SENTINEL, dtype=dt, device=DEV)
        xd = x.to(DEV)
        entry("f32_to_bf16", fmt)(p(xd), p(out), n, 1.0, st())
        torch.cuda.synchronize()
        got, want = out[:n].cpu(), x.to(dt)
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan)
        wrong = (bits(got) != bits(want)) & ~nan
        assert not bool(wrong.any()), [(float(a), float(b), float(c)) for a, b, c in zip(x[wrong], got[wrong], want[wrong])]
        assert all_sentinel(out[n:])


@FMT
def test_f32_to_16_2d_strided(fmt):
    dt = dt_of(fmt)
    rows, cols, ldx, ldo, alpha = 7, 33, 40, 48, 0.5
    g = torch.Generator().manual_seed(22)
    x = torch.randn(rows, cols, generator=g)
    xd = padded(x, ldx)
    out = guarded(rows, ldo, dt, SENTINEL)
    entry("f32_to_bf16_2d", fmt)(p(xd), ldx, p(out), ldo, rows, cols, alpha, st())
    torch.cuda.synchronize()
    assert same_bits(out[:rows, :cols].cpu(), (x * 0.5).to(dt))                               # 0.5 x is exact: one rounding
    assert all_sentinel(out[:rows, cols:]) and all_sentinel(out[rows:])


@FMT
def test_mpsilu_to_16(fmt):
    """x / (1 + exp(-x)) / 0.596 in fp32 with the fast exponential and reciprocal: a few fp32 ulps in front of the 16-bit rounding."""
    g = torch.Generator().manual_seed(23)
    x = torch.randn(1000, generator=g) * 2
    out = torch.full((1000 + GUARD,), SENTINEL, dtype=dt_of(fmt), device=DEV)
    xd = x.to(DEV)
    entry("mpsilu_to_bf16", fmt)(p(xd), p(out), 1000, st())
    torch.cuda.synchronize()
    ul = Ulps(fmt)
    ul.add(out[:1000], R.mp_silu64(x.double()).numpy())
    ul.check("mpsilu_to_16")
    assert all_sentinel(out[1000:])


@pytest.mark.parametrize("nslabs", [1, 3])
def test_sum_slabs(nslabs):
    """acc += sum of the slabs in slab order, on grid operands: exact, so bit-equal to fp64; the slabs' own padding (NaN) is never read."""
    n, stride = 1001, 1024
    rng = np.random.default_rng(nslabs)
    prior, slabs = R.grid((n,), rng) + 5, R.grid((nslabs, n), rng)
    acc = torch.full((n + GUARD,), NAN, device=DEV)
    acc[:n] = prior.float().to(DEV)
    sd = padded(slabs.float(), stride)
    entry("sum_slabs")(p(acc), p(sd), nslabs, stride, n, st())
    torch.cuda.synchronize()
    assert torch.equal(f64(acc[:n]), prior + slabs.sum(0))
    assert bool(torch.isnan(acc[n:]).all())
