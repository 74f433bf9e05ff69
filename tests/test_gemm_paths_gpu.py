"""Every fused GEMM epilogue, per element against fp64, on every dispatch path of ``launch()`` (csrc/gemm.hip) - and each case asserts
the path it reached through ``mapdit_gemm_last_plan``, so a change of the tile rule cannot quietly take a case off its kernel.

Operands.  A holds integers in [-2, 2] (thinned so that the accumulator's standard deviation is about 1), a few rows scaled by 8; B holds
{-1, 0, 1} / 4.  Every product and partial sum is exact in fp32 in any order: the accumulator is an exact multiple of 1/4 with |acc| <= 40
(asserted), the same number on every kernel, and its fp64 value (one CPU matmul per shape, shared by all cases of that shape and by both
16-bit formats) is THE accumulator.  The reference of an output is the epilogue's formula (mapdit.h, the functors of gemm.hip) evaluated in
fp64 on it; the pointwise fp64 arithmetic and the comparisons run in torch on the device so that the 50 M-element cases stay at seconds.
Stream operands are random, exact in their storage format, in rows wider than the result with NaN in the padding; outputs start as NaN
and their padding must still hold the fill pattern afterwards.

Bounds (u = 2^-24; counted from the functor source, written beside each use):
 * STORE_F32 (alpha a power of two): == ; accumulate: one fp32 rounding.  STORE_BF16, `pre` of SILU2, `y` of RESID, v of the head kinds
   (and q, k of QKV_HEADS_RAW): == the accumulator rounded to the format - which also pins placement: a permuted head is an equality failure.
   The accumulator of this recipe has 8 significant bits, so it is exact in bf16 and fp16 and these equalities see no rounding: STORE_BF16
   therefore runs a second time with alpha = 171 / 8192 (alpha acc exact in fp32 with up to 16 significant bits), where the stored value
   must be its round-to-nearest-even.  `pre`, `y` and the head kinds' v go through the same pack16 conversion with nothing to round.
 * fp32 outputs of arithmetic epilogues: |got - ref| <= e32 = n u sum|terms| (+ 4 u relative per v_exp / v_rcp / v_sqrt).
 * 16-bit outputs of arithmetic epilogues: |got - ref| < ulp16(ref) - one of the two neighbours of the fp64 value (subnormal spacing below
   the smallest normal, +-0 equal).  Where e32 exceeds half a 16-bit ulp - results that cancel: out3 of RESID near ka o c = -kb h (or
   o A = -o' B), the derivative factor next to its zero at h = -1.278 (DSILU, `dact`) - the bound is e32 + ulp16(|ref| + e32) instead.
   The same e32 also gives the sharper |got - ref| <= e32 + ulp16(|ref| + e32) / 2 (the store rounds an fp32 value within e32 of the
   reference to nearest), asserted too: the neighbour bound alone cannot see an error below a bf16 ulp.
 * RESID promises equal bits on the 128^2, 64-row and 256^2 kernels, STORE_BF16 on the 64-row and 128^2 forms: torch.equal
   (test_equal_bits_across_kernel_forms).  SILU2 and SILU2_GRAD are different instruction sequences: no equality is asserted between them.

Paths x kinds covered (NT / NN / TN = layouts; "all" = STORE_BF16 at alpha 1/2 and 171/8192, STORE_F32 plain and alpha = 2 + accumulate, SILU2, SILU2_COND,
SILU2_GRAD with and without `out`, MUL_AUX, DSILU, RESID {no out3 | AdaLN out3 at rows_per_sample 256, 64, 96 (tiles straddle samples) |
rot2 out3 | no `out`}; "large" = STORE_BF16 (both alphas), SILU2_GRAD with out, MUL_AUX, DSILU, RESID with AdaLN out3; "heads" = QKV_HEADS,
QKV_HEADS_RAW at head_dim 72 and 64):

  path                                  shapes (M, N, K)                                          kinds
  scalar fallback                       (72, 40, 24) NT NN TN; (72, 40, 12) for STORE_F32          all; heads at N = 192 / 216, T = 24
  128^2, fast / not                     (128, 256, 128) / (200, 136, 192) NT NN TN                 all; heads
  64-row form, fast / not               (320, 384, 64) / (1000, 256, 128) NT NN                    STORE_BF16, every RESID form
  256^2 forced, interior / guarded      (512, 512, 128) / (600, 264, 128) NT NN TN                 all (wave-private; shared-image for RESID
                                                                                                   - FE and guarded - and STORE_F32); heads
  256^2 forced, K > 1024                (512, 256, 1088) NT NN                                     STORE_BF16 (shared-image)
  256^2 by the tile rule                (8192, 1024, 64) / (8136, 1032, 64) NT NN                  all; heads at (11008, 768), (8192, 1152),
                                                                                                   (2560, 3456: head_dim 72)
  persistent grid                       (196608, 256, 64) / (196360, 256, 64) NT                   large (RESID: stagger 2); QKV_HEADS and RAW-64 (65536, 768),
                                                                                                   RAW-72 (14080, 3456)
  column split                          (49152, 384, 64) NT NN TN; (12288, 1152, 64) NT            large; QKV_HEADS (12288, 1152), RAW-72 (3840, 3456)
                                        (second launch on the 64-row form: STORE_BF16, RESID)
Left off: the persistent and column-split rows run the "large" kinds and heads only (the other kinds share their functor's code with a
covered one on those kernels and cross every other path); QKV_HEADS_RAW at head_dim 64 is not run on the column split (head_dim 72 is);
RMB is held to the unfused pass by test_gemm_fused_resid_mod_backward.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
NT, NN, TN = 0, 1, 2
LAYOUT_NAME = {NT: "NT", NN: "NN", TN: "TN"}


class _Fmt:
    def __init__(self, f16):
        import mapdit_amd
        self.mod = mapdit_amd._lib
        self.f16 = f16
        self.dt = torch.float16 if f16 else torch.bfloat16
        self.bits = 11 if f16 else 8                       # significand bits
        self.emin = -14 if f16 else -126                   # exponent of the smallest normal

    def gemm(self, *args):
        lib = self.mod.lib()
        (lib.gemm_f16 if self.f16 else lib.gemm_bf16)(*args)

    def plan(self):
        pl = self.mod.GemmPlan()
        self.mod.lib().gemm_last_plan(C.byref(pl))
        return pl

    def ulp(self, x):
        """Spacing of the 16-bit format at |x| (fp64 tensor): 2^(e - bits + 1), e = floor(log2 |x|) clamped at the smallest normal."""
        _, ex = torch.frexp(x.abs())                       # |x| = m 2^ex, m in [0.5, 1); 0 -> ex = 0
        e = torch.where(x == 0, torch.full_like(ex, self.emin), ex - 1).clamp(min=self.emin)
        return ((e.long() - (self.bits - 1) + 1023) << 52).view(torch.float64)      # the power of two, as its fp64 bit pattern


@pytest.fixture(scope="module", params=["bf16", "f16"])
def F(request):
    return _Fmt(request.param == "f16")


# ---- operands and the accumulator: once per shape ------------------------------------------------------------------------------------
_OPERANDS = {}          # holds ONE shape (cases of a shape are consecutive): the fp32 accumulator of the largest is 200 MB of device memory


@pytest.fixture(scope="module", autouse=True)
def _drop_operands():
    yield
    _OPERANDS.clear()


def operands(M, N, K):
    key = (M, N, K)
    if key not in _OPERANDS:
        _OPERANDS.clear()
        g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
        q = min(1.0, 12.0 / K)                                                      # var of a term = 2 q / 24: the sum has variance ~1
        A = torch.randint(-2, 3, (M, K), generator=g).float() * (torch.rand(M, K, generator=g) < q).float()
        B = torch.randint(-1, 2, (N, K), generator=g).float() / 4
        acc = A.double() @ B.double().t()                                           # fp64, CPU
        big = (torch.arange(M) % 29 == 3) & (8 * acc.abs().amax(1) <= 40)           # rows scaled by 8: pre-activations to about +-30
        s = torch.where(big, 8.0, 1.0)
        A, acc = A * s[:, None], acc * s[:, None].double()                          # (a power of two: still THE fp64 product)
        assert float(acc.abs().max()) <= 40 and torch.equal(acc, acc.float().double()) and torch.equal(acc * 4, (acc * 4).round())
        if M * N >= 128 * 128:
            assert float(acc.abs().max()) >= 16, "no large pre-activation in this shape"
        _OPERANDS[key] = (A, B, acc.float().to(DEV))                                # (exact in fp32: 8 significant bits)
    return _OPERANDS[key]


def st():
    return torch.cuda.current_stream().cuda_stream


def padded(values, ld, dtype=None):
    """values [R, W] in rows of ld elements, NaN in the padding."""
    t = torch.full((values.shape[0], ld), float("nan"), device=DEV, dtype=dtype or values.dtype)
    t[:, :values.shape[1]] = values
    return t


def nan_out(rows, ld, dtype):
    return torch.full((rows, ld), float("nan"), device=DEV, dtype=dtype)


def untouched(t, width):
    """The padding of an output still holds the fill pattern, bit for bit."""
    pad = t[:, width:].contiguous()
    fill = torch.full_like(pad, float("nan"))
    it = torch.int16 if t.element_size() == 2 else torch.int32
    return pad.numel() == 0 or torch.equal(pad.view(it), fill.view(it))


class Ctx:
    """What a failure reports: the case, the plan, the first failing element and its tile."""

    def __init__(self, what, plan, N):
        self.what, self.pl, self.N = what, plan, N

    def tile_text(self, m, n):
        """Where element (m, n) of the GEMM result lies in the launch that wrote it."""
        pl = self.pl
        if pl.tile == 0:
            return "scalar fallback (no tiles)"
        if pl.col_split and n >= self.N - 128:
            return f"tile row {m // 128} (64-row form: {m // 64}) of the column-split strip from column {self.N - 128}, family {pl.family2}"
        tn = 256 if pl.tile == 256 else 128
        return f"tile ({m // pl.tile}, {n // tn}) of {pl.tile} x {tn}"

    def plan_text(self):
        return ", ".join(f"{n}={getattr(self.pl, n)}" for n, _ in self.pl._fields_)

    def check(self, name, got, ref, tol=None, strict=False, col0=0, colw=1):
        """col0, colw: column j of `got` is column col0 + j * colw of the GEMM result (the k and v blocks of the head kinds; out4's heads)."""
        got, ref = got.double(), ref.double()
        if tol is None:
            ok = got == ref                                   # (+-0 equal; a NaN left in the output fails)
        elif strict:
            ok = (got - ref).abs() < tol
        else:
            ok = (got - ref).abs() <= tol
        if bool(ok.all()):
            return
        bad = torch.nonzero(~ok)
        m, n = (int(v) for v in bad[0])
        t = float(tol[m, n]) if torch.is_tensor(tol) else tol
        ng = col0 + n * colw
        pytest.fail(f"{self.what}: {name}: {bad.shape[0]} of {ok.numel()} elements fail, first at (m, n) = ({m}, {ng}) of the result, {self.tile_text(m, ng)}: "
                    f"got {float(got[m, n])!r}, fp64 reference {float(ref[m, n])!r}, bound {t!r}; plan: {self.plan_text()}")

    def check16(self, F, name, got, ref, e32, col0=0):
        """A 16-bit output of an arithmetic epilogue: one of the two neighbours of the fp64 value; widened by the fp32 bound e32 only
        where that exceeds half a 16-bit ulp.  Then the sharper statement the same e32 gives: the stored value is the round-to-nearest
        of an fp32 value within e32 of the reference, |got - ref| <= e32 + ulp16(|ref| + e32) / 2 - a relative error of a tenth of a
        bf16 ulp in a functor's constant moves a fifth of the outputs across a rounding boundary and past this bound, while every one
        of them still is a neighbour."""
        ulp, ulp_hi = F.ulp(ref), F.ulp(ref.abs() + e32)
        wide = e32 > 0.5 * ulp
        self.check(name, got, ref, torch.where(wide, e32 + ulp_hi, ulp), strict=True, col0=col0)
        self.check(name + " (as a rounded fp32 value)", got, ref, e32 + 0.5 * ulp_hi, col0=col0)


# ---- the epilogues' formulas in fp64, with their fp32 error bounds ------------------------------------------------------------------------
def silu_ref(v):
    """act = silu(v) / 0.596 and the derivative factor d/dv act = s (1 + v (1 - s)) / 0.596, with absolute fp32 bounds.
    act: e^-v = v_exp(v * -log2 e): the rounded constant and the product's rounding move the exponent by |v| log2 e u each, 2 |v| u on
    e^-v together, v_exp 4 u; then 1 + e or the fma 0.596 e + 0.596 (1) with its rounded constant (1), v_rcp 4 u, v * s (1), and in
    SILU2 the product with the rounded 1 / 0.596 (2): (2 |v| + 12) u relative in both instruction sequences.
    dact: with r = (2 |v| + 11) u the relative error of s: (1 - s) to s r + u, v (1 - s) to |v| (r + 2 u), 1 + .. one more rounding of at
    most (1 + |v|) u, the product with s: r + u, with 1 / 0.596: 2 u  ->  (2 r + 6 u) s (1 + |v|) / 0.596; the SILU2_GRAD sequence
    (sc + ac (1 - 0.596 sc)) gives (2 r + 4 u) of the same magnitude: (4 |v| + 28) u s (1 + |v|) / 0.596 covers both."""
    s = torch.sigmoid(v)
    act = v * s / 0.596
    dact = s * (1 + v * (1 - s)) / 0.596
    return act, (2 * v.abs() + 12) * U * act.abs(), dact, (4 * v.abs() + 28) * U * s * (1 + v.abs()) / 0.596


FULL = [("store16", 0), ("store16_r", 0), ("f32", 0), ("f32_acc", 0), ("silu2", 0), ("silu2_cond", 0), ("grad", 0), ("grad_noout", 0), ("mulaux", 0),
        ("dsilu", 0), ("resid", 256), ("resid_adaln", 256), ("resid_adaln", 64), ("resid_adaln", 96), ("resid_rot", 64), ("resid_noy", 256)]
F32_ONLY = [k for k in FULL if k[0].startswith("f32")]
NOT_F32 = [k for k in FULL if not k[0].startswith("f32")]
STRIPS = [k for k in FULL if k[0].startswith("store16") or k[0].startswith("resid")]
LARGE = [("store16", 0), ("store16_r", 0), ("grad", 0), ("mulaux", 0), ("dsilu", 0), ("resid_adaln", 256)]


def expected_plan(F, path, kind, T, M, N, K, layout):
    """The plan a case was written for: (family, flags).  Written from the rules DESIGN.md states, not read back from the library."""
    L = F.mod
    resid, shared_kind = kind.startswith("resid"), kind.startswith("resid") or kind.startswith("f32")
    want = dict(split_k=1, ktail=0, fe=0, persistent=0, stagger=0, col_split=0, family2=L.GEMM_NONE)
    if path == "scalar":
        return dict(want, family=L.GEMM_SCALAR, tile=0, fast=0)
    if path == "128":
        return dict(want, family=L.GEMM_128, tile=128, fast=int(M % 128 == 0 and N % 128 == 0 and K % 64 == 0))
    if path == "64row":
        return dict(want, family=L.GEMM_64ROW, tile=64, fast=int(M % 64 == 0 and N % 128 == 0))
    n256 = N - 128 if path == "colsplit" else N
    tiles = -(-M // 256) * -(-n256 // 256)
    want.update(tile=256, tiles=tiles, fast=int(M % 256 == 0 and n256 % 256 == 0),
                family=L.GEMM_256_SHARED if shared_kind or (kind.startswith("store16") and K > 1024) else L.GEMM_256_WAVE)
    if kind == "resid_adaln" and T % 256 == 0 and M % 256 == 0 and n256 % 256 == 0:
        want["fe"] = 1                                     # every optional output there, AdaLN form, every tile inside one sample
    if path == "persistent":
        assert tiles >= 768
        want.update(persistent=1, grid=256, stagger=2 if resid else 0)
    else:
        want["grid"] = tiles
    if path == "colsplit":
        strip64 = (resid or kind.startswith("store16")) and layout != TN and -(-M // 128) <= 160
        want.update(col_split=1, family2=L.GEMM_64ROW if strip64 else L.GEMM_128)
    return want


def assert_plan(pl, want, what):
    got = {k: getattr(pl, k) for k in want}
    assert got == want, f"{what}: the call was not served as this case was written for: {got} != {want}"
    assert pl.family2 != 0 or pl.col_split == 0
    if pl.tile == 256:
        assert 1 <= pl.band


def launch(F, layout, M, N, K, forced, **fields):
    A, B, acc = operands(M, N, K)
    a = (A if layout != TN else A.t()).contiguous().to(DEV).to(F.dt)
    b = (B if layout == NT else B.t()).contiguous().to(DEV).to(F.dt)
    ep = F.mod.Epilogue()
    for k, v in fields.items():
        setattr(ep, k, v)
    if forced:
        F.mod.lib().gemm_tuning(256, 2, 0)
    try:
        F.gemm(layout, M, N, K, a.data_ptr(), a.shape[1], b.data_ptr(), b.shape[1], C.byref(ep), st())
        pl = F.plan()
    finally:
        if forced:
            F.mod.lib().gemm_tuning(0, 2, 0)
    torch.cuda.synchronize()
    return acc.double(), pl


def run_pointwise(F, path, kind, T, M, N, K, layout, forced=False):
    L = F.mod
    what = f"{path} {kind} T={T} ({M}, {N}, {K}) {LAYOUT_NAME[layout]} {'f16' if F.f16 else 'bf16'}"
    g = torch.Generator(device=DEV).manual_seed(7 * M + 3 * N + K + T)
    rnd = lambda *shape: torch.randn(*shape, device=DEV, generator=g)
    ld = N + 8
    p = lambda t: t.data_ptr()
    want = lambda: expected_plan(F, path, kind, T, M, N, K, layout)
    r16 = lambda x: x.float().to(F.dt).double()            # (x exact in fp32)

    if kind in ("store16", "store16_r"):
        # alpha = 1/2: the accumulator itself (8 significant bits: it is exact in either format, the store rounds nothing).  alpha =
        # 171 / 8192: alpha * acc has up to 16 significant bits - exact in fp32, so the reference is its round-to-nearest-even in the
        # format (torch's conversion), and a store that truncated or rounded twice fails
        alpha = 0.5 if kind == "store16" else 171.0 / 8192
        out = nan_out(M, ld, F.dt)
        acc, pl = launch(F, layout, M, N, K, forced, kind=L.EPI_STORE_BF16, out=p(out), ldo=ld, alpha=alpha)
        assert_plan(pl, want(), what)
        c = Ctx(what, pl, N)
        ref = r16(alpha * acc)
        assert kind == "store16" or bool((ref != alpha * acc).any()), "no value of this case needs rounding"
        c.check("out", out[:, :N], ref)
        assert untouched(out, N), what
    elif kind in ("f32", "f32_acc"):
        if kind == "f32":
            out = nan_out(M, ld, torch.float32)
            acc, pl = launch(F, layout, M, N, K, forced, kind=L.EPI_STORE_F32, out=p(out), ldo=ld, alpha=0.25)
            tol, ref = None, 0.25 * acc                    # exact
        else:
            base = rnd(M, N)
            out = padded(base, ld)
            acc, pl = launch(F, layout, M, N, K, forced, kind=L.EPI_STORE_F32, out=p(out), ldo=ld, alpha=2.0, accumulate=1)
            ref = base.double() + 2 * acc
            tol = U * ref.abs()                            # 2 acc exact; the sum with the stored base: 1 rounding
        assert_plan(pl, want(), what)
        Ctx(what, pl, N).check("out", out[:, :N], ref, tol)
        assert untouched(out, N), what
    elif kind in ("silu2", "silu2_cond"):
        pre, act = nan_out(M, ld, F.dt), nan_out(M, ld, F.dt)
        acc, pl = launch(F, layout, M, N, K, forced, kind=L.EPI_SILU2 if kind == "silu2" else L.EPI_SILU2_COND, out=p(pre), out2=p(act), ldo=ld)
        assert_plan(pl, want(), what)
        c = Ctx(what, pl, N)
        a_ref, a_e, _, _ = silu_ref(acc)
        c.check("pre", pre[:, :N], r16(acc))
        c.check16(F, "act", act[:, :N], a_ref, a_e)
        assert untouched(pre, N) and untouched(act, N), what
    elif kind in ("grad", "grad_noout"):
        dact, act = nan_out(M, ld, F.dt), nan_out(M, ld, F.dt)
        acc, pl = launch(F, layout, M, N, K, forced, kind=L.EPI_SILU2_GRAD, out=p(dact) if kind == "grad" else None, out2=p(act), ldo=ld)
        assert_plan(pl, want(), what)
        c = Ctx(what, pl, N)
        a_ref, a_e, d_ref, d_e = silu_ref(acc)
        c.check16(F, "act", act[:, :N], a_ref, a_e)
        if kind == "grad":
            c.check16(F, "dact", dact[:, :N], d_ref, d_e)
        else:
            assert untouched(dact, 0), what                # no `out`: nothing written
        assert untouched(dact, N) and untouched(act, N), what
    elif kind == "mulaux":
        aux_v = rnd(M, N).to(F.dt)
        aux, out = padded(aux_v, ld), nan_out(M, ld, F.dt)
        acc, pl = launch(F, layout, M, N, K, forced, kind=L.EPI_MUL_AUX, out=p(out), aux=p(aux), ldo=ld)
        assert_plan(pl, want(), what)
        ref = acc * aux_v.double()
        Ctx(what, pl, N).check16(F, "out", out[:, :N], ref, U * ref.abs())            # v * aux: 1 rounding
        assert untouched(out, N), what
    elif kind == "dsilu":
        h_v = (3 * rnd(M, N)).to(F.dt)
        h, out = padded(h_v, ld), nan_out(M, ld, F.dt)
        acc, pl = launch(F, layout, M, N, K, forced, kind=L.EPI_DSILU, out=p(out), aux=p(h), ldo=ld)
        assert_plan(pl, want(), what)
        _, _, d_ref, d_e = silu_ref(h_v.double())
        ref = acc * d_ref
        Ctx(what, pl, N).check16(F, "out", out[:, :N], ref, acc.abs() * d_e + U * ref.abs())   # the factor's bound, v * factor: 1 rounding
        assert untouched(out, N), what
    else:
        S = -(-M // T)
        ldg, ld2 = 3 * N + 4, 2 * N + 12
        x_v, gate_v = rnd(M, N), rnd(S, N)
        x, gate_t = padded(x_v, ld), torch.full((S, ldg), float("nan"), device=DEV)
        gate_t[:, N:2 * N] = gate_v
        sh_v, sc_v = rnd(S, N), rnd(S, N)
        mod = torch.full((S, ld2), float("nan"), device=DEV)
        mod[:, 4:4 + N], mod[:, 8 + N:8 + 2 * N] = sh_v, sc_v
        gain = torch.tensor([0.3], device=DEV)
        y = nan_out(M, ld, F.dt) if kind != "resid_noy" else None
        xm = nan_out(M, ld, F.dt) if kind != "resid" else None
        xo = nan_out(M, ld, torch.float32)
        fields = dict(kind=L.EPI_RESID, out=y.data_ptr() if y is not None else None, out2=p(xo), aux=p(x), gate=p(gate_t) + 4 * N, ldg=ldg,
                      rows_per_sample=T, ldo=ld, alpha=0.7, beta=0.3)
        if xm is not None:
            fields.update(out3=p(xm), shift2=p(mod) + 4 * 4, scale2=p(mod) + 4 * (8 + N), ld2=ld2)
            fields.update(dict(rot2=1) if kind == "resid_rot" else dict(gain2=p(gain)))
        acc, pl = launch(F, layout, M, N, K, forced, **fields)
        assert_plan(pl, want(), what)
        c = Ctx(what, pl, N)
        smp = torch.arange(M, device=DEV) // T
        ca, cb = float(np.float32(0.7)), float(np.float32(0.3))
        gv, xv = gate_v.double()[smp], x_v.double()
        o_ref = cb * gv * acc + ca * xv
        o_e = 3 * U * ((cb * gv * acc).abs() + (ca * xv).abs())                  # fma(cb g, v, ca x): cb g (1), ca x (1), the fma (1)
        c.check("out2", xo[:, :N], o_ref, o_e)
        assert untouched(xo, N), what
        if y is not None:
            c.check("y", y[:, :N], r16(acc))
            assert untouched(y, N), what
        if xm is not None:
            cv, hv = sc_v.double()[smp], sh_v.double()[smp]
            if kind == "resid_rot":
                sw = o_ref.view(M, N // 2, 2).flip(-1).reshape(M, N)
                sw_e = o_e.view(M, N // 2, 2).flip(-1).reshape(M, N)
                ref = o_ref * cv + sw * hv
                # fma(o, A, o' B): o' B (1), the fma (1), on inputs that carry out2's error
                e = cv.abs() * o_e + hv.abs() * sw_e + 2 * U * ((o_ref * cv).abs() + (sw * hv).abs())
            else:
                gg = float(np.float32(0.3))
                den = math.sqrt((1 - gg) ** 2 + gg * gg)
                ka, kb = (1 - gg) / den, gg / den
                ref = ka * o_ref * cv + kb * hv
                # ka, kb: 1 - g (1), two squares and their sum (3), sqrtf (1), the division (1) = 6 u each; fma(ka o, c, kb h): ka o (1),
                # kb h (1), the fma (1): 8 u on each term, on an o that carries out2's error
                e = (ka * cv).abs() * o_e + 8 * U * ((ka * o_ref * cv).abs() + (kb * hv).abs())
            c.check16(F, "out3", xm[:, :N], ref, e)
            assert untouched(xm, N), what


def heads_major(t, M, T, H, hd):
    """[M / T * H][T][hd] head-major -> [M, H * hd] in the GEMM's (row, column) coordinates."""
    return t.view(M // T, H, T, hd).permute(0, 2, 1, 3).reshape(M, H * hd)


def run_heads(F, path, kind, T, M, N, K, layout, forced=False):
    L = F.mod
    what = f"{path} {kind} T={T} ({M}, {N}, {K}) {LAYOUT_NAME[layout]} {'f16' if F.f16 else 'bf16'}"
    hd = 72 if kind == "raw72" else 64
    D = N // 3
    H = D // hd
    rows = M // T * H * T
    guard = 64                                             # elements behind each head-major tensor that must stay untouched
    q, k, v = (torch.full((rows * hd + guard,), float("nan"), device=DEV, dtype=F.dt) for _ in range(3))
    p = lambda t: t.data_ptr()
    r16 = lambda x: x.float().to(F.dt).double()
    if kind == "heads":
        s = torch.full((2 * rows + guard,), float("nan"), device=DEV)
        acc, pl = launch(F, layout, M, N, K, forced, kind=L.EPI_QKV_HEADS, out=p(q), out2=p(k), out3=p(v), out4=p(s), rows_per_sample=T)
    else:
        acc, pl = launch(F, layout, M, N, K, forced, kind=L.EPI_QKV_HEADS_RAW, out=p(q), out2=p(k), out3=p(v), rows_per_sample=T, ld2=hd)
    assert_plan(pl, expected_plan(F, path, kind, T, M, N, K, layout), what)
    c = Ctx(what, pl, N)
    got = [heads_major(t[:rows * hd], M, T, H, hd) for t in (q, k, v)]
    # placement, exactly: v (and the raw q, k) is the rounded accumulator at (sample, head, token, d)
    c.check("v", got[2], r16(acc[:, 2 * D:]), col0=2 * D)
    for t in (q, k, v):
        assert untouched(t[None, :], rows * hd), what
    if kind != "heads":
        c.check("q", got[0], r16(acc[:, :D]))
        c.check("k", got[1], r16(acc[:, D:2 * D]), col0=D)
        return
    assert untouched(s[None, :], 2 * rows), what
    eps = float(np.float32(1e-4))
    for w, name in ((0, "q"), (1, "k")):
        a = acc[:, w * D:(w + 1) * D].view(M, H, 64)
        # the 64 squares and their sum are exact in fp32 for these operands (multiples of 1/16 below 2^24 / 16); v_sqrt 4 u, + eps (1),
        # v_rcp 4 u, the product with 8 exact: 9 u relative
        sc = 8.0 / (a.pow(2).sum(-1).sqrt() + eps)                                 # [M, H]
        s_got = s[w * rows:(w + 1) * rows].view(M // T, H, T).permute(0, 2, 1).reshape(M, H)
        c.check(f"out4[{name}]", s_got, sc, 9 * U * sc, col0=w * D, colw=64)
        ref = (a * sc[..., None]).reshape(M, D)
        c.check16(F, f"{name}^", got[w], ref, 10 * U * ref.abs(), col0=w * D)                  # a * sc: 1 more


# ---- the matrix --------------------------------------------------------------------------------------------------------------------------
def _cases():
    rows = []

    def add(path, shapes, layouts, kinds, forced=False):
        for (M, N, K) in shapes:
            for lay in layouts:
                for kind, T in kinds:
                    rows.append(pytest.param(path, kind, T, M, N, K, lay, forced, id=f"{path}-{kind}{T or ''}-{M}x{N}x{K}-{LAYOUT_NAME[lay]}"))

    add("scalar", [(72, 40, 24)], (NT, NN, TN), NOT_F32)
    add("scalar", [(72, 40, 12)], (NT, NN, TN), F32_ONLY)
    add("128", [(128, 256, 128), (200, 136, 192)], (NT, NN, TN), FULL)
    add("64row", [(320, 384, 64), (1000, 256, 128)], (NT, NN), STRIPS)
    add("256", [(512, 512, 128), (600, 264, 128)], (NT, NN, TN), FULL, forced=True)
    add("256", [(512, 256, 1088)], (NT, NN), [("store16", 0), ("store16_r", 0)], forced=True)
    add("256", [(8192, 1024, 64), (8136, 1032, 64)], (NT, NN), FULL)
    add("persistent", [(196608, 256, 64), (196360, 256, 64)], (NT,), LARGE)
    add("colsplit", [(49152, 384, 64)], (NT, NN, TN), LARGE)
    add("colsplit", [(12288, 1152, 64)], (NT,), [("store16", 0), ("resid_adaln", 256)])
    return rows


def _head_cases():
    rows = []

    def add(path, kind, T, M, N, K, layouts, forced=False):
        for lay in layouts:
            rows.append(pytest.param(path, kind, T, M, N, K, lay, forced, id=f"{path}-{kind}-T{T}-{M}x{N}x{K}-{LAYOUT_NAME[lay]}"))

    all3 = (NT, NN, TN)
    for kind, n1 in (("heads", 192), ("raw72", 216), ("raw64", 192)):
        add("scalar", kind, 24, 48, n1, 24, all3)
        add("128", kind, 64, 128, 2 * n1, 64, all3)                 # interior (raw72: 432 columns, ragged)
        add("128", kind, 40, 200, n1, 64, all3)                     # ragged rows, samples of 40 rows
        add("256", kind, 256, 512, 4 * n1, 128, all3, forced=True)  # 768 / 864 columns
        add("256", kind, 120, 600, 2 * n1, 128, all3, forced=True)  # ragged both ways, five samples over three row tiles
    add("256", "heads", 256, 11008, 768, 64, (NT,))
    add("256", "heads", 256, 8192, 1152, 64, (NT, NN))              # ragged last tile column
    add("256", "raw64", 256, 8192, 1152, 64, (NT,))
    add("256", "raw72", 256, 2560, 3456, 64, (NT,))
    add("persistent", "heads", 256, 65536, 768, 64, (NT,))
    add("persistent", "raw64", 256, 65536, 768, 64, (NT,))
    add("persistent", "raw72", 256, 14080, 3456, 64, (NT,))         # DiT-XL's QKV width: 55 x 14 = 770 tiles, ragged last tile column
    add("colsplit", "heads", 256, 12288, 1152, 64, (NT,))
    add("colsplit", "raw72", 256, 3840, 3456, 64, (NT,))
    return rows


@pytest.mark.parametrize("path,kind,T,M,N,K,layout,forced", _cases())
def test_epilogue_per_element(F, path, kind, T, M, N, K, layout, forced):
    run_pointwise(F, path, kind, T, M, N, K, layout, forced)


@pytest.mark.parametrize("path,kind,T,M,N,K,layout,forced", _head_cases())
def test_head_epilogues_per_element(F, path, kind, T, M, N, K, layout, forced):
    run_heads(F, path, kind, T, M, N, K, layout, forced)


@pytest.mark.parametrize("T", [256, 64])
def test_equal_bits_across_kernel_forms(F, T):
    """RESID (AdaLN out3) gives the same bits on the 128^2 kernel, the 64-row form and the shared-image 256^2 kernel (straight-line at
    T = 256, guarded at T = 64: four samples per tile); STORE_BF16 on the 64-row and 128^2 forms.  A row's result does not depend on M, so
    the 64-row form - which the dispatcher takes instead of the 128^2 kernel up to 160 tiles - runs the first 1024 rows of the operands
    whose 5376 rows (168 tiles of 128^2) take the 128^2 kernel by shape and the 256^2 kernel forced."""
    L = F.mod
    M, M64, N, K = 5376, 1024, 512, 128
    g = torch.Generator().manual_seed(77)
    A = (torch.randn(M, K, generator=g)).bfloat16().float().to(DEV).to(F.dt)
    B = (0.2 * torch.randn(N, K, generator=g)).bfloat16().float().to(DEV).to(F.dt)
    S = M // T
    x, gate, mod = (torch.randn(r, c, generator=g).to(DEV) for r, c in ((M, N), (S, N), (S, 2 * N)))
    gain = torch.tensor([0.3], device=DEV)

    def run(rows, kind, forced):
        outs = [torch.full((rows, N), float("nan"), device=DEV, dtype=d) for d in (F.dt, torch.float32, F.dt)]
        ep = L.Epilogue()
        ep.kind, ep.out, ep.ldo, ep.alpha = kind, outs[0].data_ptr(), N, 1.0
        if kind == L.EPI_RESID:
            ep.out2, ep.aux, ep.gate, ep.ldg, ep.rows_per_sample, ep.alpha, ep.beta = outs[1].data_ptr(), x.data_ptr(), gate.data_ptr(), N, T, 0.7, 0.3
            ep.out3, ep.shift2, ep.scale2, ep.gain2, ep.ld2 = outs[2].data_ptr(), mod.data_ptr(), mod.data_ptr() + 4 * N, gain.data_ptr(), 2 * N
        if forced:
            L.lib().gemm_tuning(256, 2, 0)
        try:
            F.gemm(NT, rows, N, K, A.data_ptr(), K, B.data_ptr(), K, C.byref(ep), st())
            pl = F.plan()
        finally:
            if forced:
                L.lib().gemm_tuning(0, 2, 0)
        torch.cuda.synchronize()
        return outs, pl

    for kind, forms in ((L.EPI_RESID, ((M, False, L.GEMM_128), (M64, False, L.GEMM_64ROW), (M, True, L.GEMM_256_SHARED))),
                        (L.EPI_STORE_BF16, ((M, False, L.GEMM_128), (M64, False, L.GEMM_64ROW)))):
        res = []
        for rows, forced, family in forms:
            outs, pl = run(rows, kind, forced)
            assert pl.family == family and (family != L.GEMM_256_SHARED or pl.fe == int(T == 256)), (kind, rows, forced, pl.family, pl.fe)
            res.append(outs)
        n_out = 3 if kind == L.EPI_RESID else 1
        for other, (rows, _, family) in zip(res[1:], forms[1:]):
            for i in range(n_out):
                assert not torch.isnan(other[i].float()).any()
                assert torch.equal(res[0][i][:rows], other[i]), (kind, family, i, int((res[0][i][:rows] != other[i]).sum()))


def test_last_plan_reports_refusals_and_the_group_launch(F):
    """A refused call leaves family NONE; the group entry point reports the group kernel; the query needs an output."""
    L = F.mod
    a = torch.zeros(256, 256, device=DEV, dtype=F.dt)
    out = torch.zeros(2, 256, 256, device=DEV)
    ep = L.Epilogue()
    ep.kind, ep.out, ep.ldo, ep.alpha, ep.split_k = L.EPI_STORE_F32, out.data_ptr(), 256, 1.0, 9      # more slabs than K-tiles: refused
    with pytest.raises(L.MapditError):
        F.gemm(TN, 256, 256, 256, a.data_ptr(), 256, a.data_ptr(), 256, C.byref(ep), st())
    assert F.plan().family == L.GEMM_NONE
    items = (L.GemmGroupItem * 1)()
    items[0] = L.GemmGroupItem(A=a.data_ptr(), lda=256, B=a.data_ptr(), ldb=256, M=256, N=256, out=out.data_ptr(), ldo=256, alpha=1.0, slab_stride=65536)
    lib = L.lib()
    (lib.gemm_group_tn_f16 if F.f16 else lib.gemm_group_tn_bf16)(1, C.cast(items, C.c_void_p), 256, 2, st())
    torch.cuda.synchronize()
    pl = F.plan()
    assert (pl.family, pl.tile, pl.split_k, pl.grid, pl.tiles, pl.fast) == (L.GEMM_GROUP, 256, 2, 2, 1, 1)
    with pytest.raises(L.MapditError):
        lib.gemm_last_plan(None)
