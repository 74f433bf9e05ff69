"""The rotation-modulation kernels (mapdit_rot_coef_fwd / _fwd_all / _bwd, mapdit_rot_modulate_fwd, the rot2 form of the RESID GEMM epilogue,
mapdit_resid_mod_bwd with rot), the AdaLN form of mapdit_resid_mod_bwd on the paths no other test runs, and mapdit_scale_accumulate: each
through the C ABI, element by element against the fp64 references and bounds of tests/rotation_reference.py, which
tests/test_rotation_reference_cpu.py holds to the oracle and to an fp32 evaluation of the same operands.

Conventions as in tests/test_embed_kernels_gpu.py.  Outputs are pre-filled with NaN (16-bit ones with a sentinel), every output carries GUARD
rows behind its last legal row, inputs carry NaN in the padding columns of their strided rows, and everything outside an output's own rows
and columns must come back with the bits it had.  Every bound is a rule of rotation_reference (none is read off a kernel's output); what
depends on an upstream output of the same launch (dy_up and dg_up on dx) is compared at the kernel's own upstream value.  Every check prints
its worst error / bound ("ratio ..." lines, pytest -s); the measured figures stand in the docstrings.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import embed_reference as E
import rotation_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
NAN = float("nan")
SENTINEL = 7.0
FMT = pytest.mark.parametrize("fmt", ["bf16", "f16"])
TWINS = {"gemm_bf16": "gemm_f16"}


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------
def lib_mod():
    from mapdit_amd import _lib as L
    return L


def entry(name, fmt="bf16"):
    if fmt == "f16":
        name = TWINS.get(name, name + "_f16")
    return getattr(lib_mod().lib(), name)


def st():
    return torch.cuda.current_stream().cuda_stream


def p(t, col=0):
    return None if t is None else t.data_ptr() + col * t.element_size()


def dt_of(fmt):
    return E.FORMATS[fmt]["dtype"]


def fill_of(dtype):
    return NAN if dtype == torch.float32 else SENTINEL


def held(a64, ld=None, col0=0, dtype=torch.float32, guard=0, fill=NAN):
    """A [rows, cols] float64 array on the device as [rows + guard, ld] of `dtype`, at column col0, `fill` everywhere else; the values
    must survive the conversion."""
    if a64 is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a64, dtype=np.float64)).reshape(-1, a64.shape[-1])
    v = t.to(dtype)
    assert torch.equal(v.double(), t)
    out = torch.full((t.shape[0] + guard, ld or t.shape[1]), fill, dtype=dtype, device=DEV)
    out[:t.shape[0], col0:col0 + t.shape[1]] = v.to(DEV)
    return out


def blank(rows, ld, dtype=torch.float32, guard=GUARD):
    return torch.full((rows + guard, ld), fill_of(dtype), dtype=dtype, device=DEV)


def bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def kept_outside(buf, rows, col0, cols):
    """Everything of an output buffer outside [0, rows) x [col0, col0 + cols) has the bits it was filled with."""
    m = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    m[:rows, col0:col0 + cols] = False
    return torch.equal(bits(buf)[m], bits(torch.full_like(buf, fill_of(buf.dtype)))[m])


def f64(t):
    return t.detach().double().cpu().numpy()


def show(what, r):
    print("ratio", what, " ".join(f"{k} {v:.3f}" for k, v in r.items()))


def refused(fn, *args):
    with pytest.raises(lib_mod().MapditError):
        fn(*args)


# ---- rot_coef_fwd / rot_coef_fwd_all ---------------------------------------------------------------------------------------------------
def coef_layout(D):
    """theta at a non-zero offset of the modulation row and scale behind it (the engine's layout), both narrower than the row."""
    h = D // 2
    return dict(ldm=h + D + 24, theta_off=8, scale_off=8 + h + 2, ldc=D + 8)


def mod_rows(theta, scale, lay):
    n = theta.shape[0]
    mod = torch.full((n, lay["ldm"]), NAN, device=DEV)
    mod[:, lay["theta_off"]:lay["theta_off"] + theta.shape[1]] = held(theta)
    mod[:, lay["scale_off"]:lay["scale_off"] + scale.shape[1]] = held(scale)
    return mod


@pytest.mark.parametrize("D", R.COEF_DS)
def test_rot_coef_fwd(D):
    """A, B within 2 (|g theta| + 4) u |sc| of the fp64 coefficients at |g theta| up to 51; at g = 0 and in the sample whose angles are 0, A
    has the bits of scale and B is 0.  Measured on the MI355X (profiles/rotation_kernels_tests_gpu.log): A 0.42, B 0.41 of the bound at most -
    the device sincosf stays inside its documented 2 ulp at these angles."""
    c, lay, n = R.coef_case(D), coef_layout(D), R.COEF_N
    mod = mod_rows(c["theta"], c["scale"], lay)
    scale32 = held(c["scale"])
    for g in (c["g"], 0.0):
        gain = torch.tensor([g], device=DEV)
        A, B = blank(n, lay["ldc"]), blank(n, lay["ldc"])
        entry("rot_coef_fwd")(p(mod, lay["theta_off"]), p(mod, lay["scale_off"]), lay["ldm"], p(gain), p(A), p(B), lay["ldc"], n, D, st())
        torch.cuda.synchronize()
        assert kept_outside(A, n, 0, D) and kept_outside(B, n, 0, D)
        r = R.coef_ratios(c["theta"], c["scale"], g, f64(A[:n, :D]), f64(B[:n, :D]))
        show(f"rot_coef_fwd D={D} g={g:.2f}", r)
        assert max(r.values()) <= 1.0
        exact = slice(0, n) if g == 0.0 else slice(1, 2)
        assert same_bits(A[exact, :D], scale32[exact]) and float(B[exact, :D].abs().max()) == 0.0
    refused(entry("rot_coef_fwd"), p(mod, lay["theta_off"]), p(mod, lay["scale_off"]), lay["ldm"], p(gain), p(A), p(B), lay["ldc"], n, D - 1, st())


@pytest.mark.parametrize("D", R.COEF_DS)
def test_rot_coef_fwd_all(D):
    """Five slots at distinct offsets of one modulation row with distinct device gains (one of them 0): every slot's column block has the bits
    of mapdit_rot_coef_fwd called with that slot's pointers (whose values test_rot_coef_fwd pins) and lies within the coefficient bound; a
    call with three slots leaves the columns of the other two untouched.  Measured: A 0.43, B 0.42 of the bound at most."""
    a, h, n, S = R.coef_all_case(D), D // 2, R.COEF_N, R.ALL_SLOTS
    chunk = h + D
    ld_mod, ldc = S * chunk + 16, S * D + 8
    order = [3, 0, 4, 1, 2]
    theta_off = [4 + order[s] * chunk for s in range(S)]
    scale_off = [t + h for t in theta_off]
    mod = torch.full((n, ld_mod), NAN, device=DEV)
    for s in range(S):
        mod[:, theta_off[s]:theta_off[s] + h] = held(a["theta"][s])
        mod[:, scale_off[s]:scale_off[s] + D] = held(a["scale"][s])
    gains = torch.tensor(a["gains"], device=DEV)
    ints = lambda v: (C.c_int * len(v))(*v)
    gptr = lambda k: (C.c_void_p * k)(*[p(gains, s % S) for s in range(k)])
    fn = entry("rot_coef_fwd_all")
    for slots in (S, 3):
        A, B = blank(n, ldc), blank(n, ldc)
        fn(p(mod), ld_mod, ints(theta_off), ints(scale_off), gptr(S), slots, p(A), p(B), ldc, n, D, st())
        torch.cuda.synchronize()
        assert kept_outside(A, n, 0, slots * D) and kept_outside(B, n, 0, slots * D)
        worst = {}
        for s in range(slots):
            A1, B1 = blank(n, D + 8), blank(n, D + 8)
            entry("rot_coef_fwd")(p(mod, theta_off[s]), p(mod, scale_off[s]), ld_mod, p(gains, s), p(A1), p(B1), D + 8, n, D, st())
            torch.cuda.synchronize()
            assert same_bits(A[:n, s * D:(s + 1) * D], A1[:n, :D]) and same_bits(B[:n, s * D:(s + 1) * D], B1[:n, :D]), s
            r = R.coef_ratios(a["theta"][s], a["scale"][s], a["gains"][s], f64(A[:n, s * D:(s + 1) * D]), f64(B[:n, s * D:(s + 1) * D]))
            worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
            if a["gains"][s] == 0.0:
                assert same_bits(A[:n, s * D:(s + 1) * D], held(a["scale"][s])) and float(B[:n, s * D:(s + 1) * D].abs().max()) == 0.0
        show(f"rot_coef_fwd_all D={D} slots={slots}", worst)
        assert max(worst.values()) <= 1.0
    big = lib_mod().ROT_MAX_SLOTS + 1
    refused(fn, p(mod), ld_mod, ints(theta_off), ints(scale_off), gptr(S), S, p(A), p(B), ldc, n, D - 1, st())                  # odd D
    odd = [scale_off[0] + 1] + scale_off[1:]
    refused(fn, p(mod), ld_mod, ints(theta_off), ints(odd), gptr(S), S, p(A), p(B), ldc, n, D, st())                             # odd scale_off
    refused(fn, p(mod), ld_mod, ints([4] * big), ints([4 + h] * big), gptr(big), big, p(A), p(B), ldc, n, D, st())               # too many slots


# ---- rot_modulate_fwd --------------------------------------------------------------------------------------------------------------------
def run_rot_modulate(x64, A, B, ldc, colA, colB, fmt):
    """x64 [n, T, D]; A / B device rows of stride ldc with the coefficients at columns colA / colB."""
    n, T, D = x64.shape
    out, x = blank(n * T, D, dt_of(fmt)), held(x64)
    entry("rot_modulate_fwd", fmt)(p(x), p(A, colA), p(B, colB), ldc, p(out), n, T, D, st())
    torch.cuda.synchronize()
    assert kept_outside(out, n * T, 0, D)
    return out[:n * T]


@FMT
@pytest.mark.parametrize("shape", R.MOD_SHAPES)
def test_rot_modulate_fwd(shape, fmt):
    """out = 16-bit(x A + pairswap(x) B) with random A, B: within 2 * 3 u (|x A| + |x' B|) + the 16-bit store of the fp64 value; the same
    kernel output lies orders of magnitude outside the bound of the references with B[j ^ 1] for B[j] and with -B.  Measured: 0.96 to 1.00
    of the bound (the store's half ulp is attained; the fp32 part of the bound is met at 0.31 by an fp32 evaluation on the CPU), the wrong
    references at 1.7e4 to 2.5e6 times the bound."""
    n, T, D = shape
    c = R.modulate_case(n, T, D)
    ldc = D + 8
    out = run_rot_modulate(c["x"], held(c["A"], ldc), held(c["B"], ldc), ldc, 0, 0, fmt)
    got = f64(out).reshape(n, T, D)
    r, m = R.modulate_ratio(c, got, fmt), R.modulate_mutant_ratios(c, got, fmt)
    show(f"rot_modulate_fwd {shape} {fmt}", dict(out=r, **m))
    assert r <= 1.0
    assert min(m.values()) > 100.0


# ---- the RESID epilogue with rot2 ----------------------------------------------------------------------------------------------------------
@FMT
@pytest.mark.parametrize("rows", R.EPI_ROWS)
def test_resid_epilogue_rot2(rows, fmt):
    """[512, 256] x K = 64 on the 128^2 and the 256^2 kernel, tiles that span samples (64 rows per sample: per-row operand loads) and tiles
    inside one sample (256): xm lies within the modulate bound of the reference evaluated at the call's own out2, has the same bits on both
    kernels and the bits of mapdit_rot_modulate_fwd applied to that out2 (both spell fma(x, A, x' B) and round the fp32 value to 16 bits);
    out and out2 have the bits of the same call without out3.  Measured: xm 1.00 (bf16) / 0.999 (f16) of the bound, the wrong references
    at 2.4e6 times the bound or more.  (Before mapdit_rot_modulate_fwd pinned its fp32 value like the epilogue does, its fp16 build
    converted inside the fma - one rounding against the epilogue's two.)"""
    L = lib_mod()
    M, N, K = R.EPI_M, R.EPI_N, R.EPI_K
    e, s, dt = R.epilogue_case(rows, fmt), R.EPI_M // rows, dt_of(fmt)
    a, b, x = held(e["a"], dtype=dt), held(e["b"], dtype=dt), held(e["x"])
    ldg, ld2, colA, colB = N + 4, 2 * N + 16, 4, N + 12
    gate = held(e["gate"], ldg, 4)
    coef = torch.full((s, ld2), NAN, device=DEV)
    coef[:, colA:colA + N], coef[:, colB:colB + N] = held(e["A"]), held(e["B"])
    res = {}
    try:
        for tile in (128, 256):
            for with_xm in (True, False):
                L.lib().gemm_tuning(tile, 2, 0)
                y, xo, xm = blank(M, N, dt), blank(M, N), blank(M, N, dt)
                ep = L.Epilogue()
                ep.kind, ep.out, ep.out2, ep.aux, ep.ldo = L.EPI_RESID, p(y), p(xo), p(x), N
                ep.gate, ep.ldg, ep.rows_per_sample, ep.alpha, ep.beta = p(gate, 4), ldg, rows, R.CA, R.CB
                if with_xm:
                    ep.out3, ep.scale2, ep.shift2, ep.gain2, ep.ld2, ep.rot2 = p(xm), p(coef, colA), p(coef, colB), None, ld2, 1
                entry("gemm_bf16", fmt)(0, M, N, K, p(a), K, p(b), K, C.byref(ep), st())
                torch.cuda.synchronize()
                assert kept_outside(y, M, 0, N) and kept_outside(xo, M, 0, N) and kept_outside(xm, M if with_xm else 0, 0, N)
                res[tile, with_xm] = (y[:M], xo[:M], xm[:M])
    finally:
        L.lib().gemm_tuning(0, 2, 0)
    for tile in (128, 256):
        y, xo, xm = res[tile, True]
        assert same_bits(y, res[tile, False][0]) and same_bits(xo, res[tile, False][1]), tile
        assert bool(torch.isfinite(xo).all())
        c = dict(x=f64(xo).reshape(s, rows, N), A=e["A"], B=e["B"])
        got = f64(xm).reshape(s, rows, N)
        r, m = R.modulate_ratio(c, got, fmt), R.modulate_mutant_ratios(c, got, fmt)
        show(f"resid_epilogue_rot2 rows={rows} tile={tile} {fmt}", dict(xm=r, **m))
        assert r <= 1.0 and min(m.values()) > 100.0
        assert same_bits(xm, run_rot_modulate(c["x"], coef, coef, ld2, colA, colB, fmt)), tile
    assert same_bits(res[128, True][2], res[256, True][2]) and same_bits(res[128, True][1], res[256, True][1])


# ---- resid_mod_bwd -------------------------------------------------------------------------------------------------------------------------
def run_rmb(name, fmt, rot, o=None, scratch=False, dgain_out=False, dgain_scale=0.0):
    """One call of case `name` on fresh buffers, every output's surroundings checked.  Returns the results as float64 arrays (dx, dx16, dy_up
    [n, T, D]; the column sums [n, D]; part = the written gain partials, nparts their reported count) and the raw device tensors."""
    L = lib_mod()
    c, dt = R.RMB_CASES[name], dt_of(fmt)
    o = o or R.rmb_case(name, fmt)
    n, T, D = o["x"].shape
    ldx, col0, dx32 = c.get("ldx", D), c.get("col0", 0), c.get("dx32", True)
    rows, mod_on, up_on = n * T, o["dxm"] is not None, o["y_up"] is not None
    ldmod, ldg, ldd, ldd_up, cS, cH = 2 * D + 16, D + 12, 2 * D + 16, D + 8, 4, D + 8
    tok = lambda v, dtype: held(v, ldx, col0, dtype)
    a = L.ResidModBwd()
    keep = [tok(o["dxo"], torch.float32 if c["dxo"] == "f32" else dt), tok(o["dxm"], dt), tok(o["x"], torch.float32), tok(o["y_up"], dt)]
    a.dxo, a.dxo_bf = (p(keep[0], col0), None) if c["dxo"] == "f32" else (None, p(keep[0], col0))
    a.dxm, a.x, a.y_up = p(keep[1], col0), p(keep[2], col0) if mod_on else None, p(keep[3], col0)
    mod = torch.full((n, ldmod), NAN, device=DEV)
    mod[:, cS:cS + D], mod[:, cH:cH + D] = held(o["scale"]), held(o["shift"])
    gain = torch.tensor([0.0 if rot else o["gain"]], device=DEV)
    gup = held(o["g_up"], ldg, 8)
    dx, dx16, dy = (blank(rows, ldx) if dx32 else None), blank(rows, ldx, dt), blank(rows, ldx, dt)
    dmod, dgup = blank(n, ldd), blank(n, ldd_up)
    part = torch.full((8 * n * (D // 128) + GUARD,), NAN, device=DEV)
    if mod_on:
        a.scale, a.shift, a.gain, a.ldmod = p(mod, cS), p(mod, cH), p(gain), ldmod
        a.dscale, a.dshift, a.ldd, a.dgain_part = p(dmod, cS), p(dmod, cH), ldd, p(part)
    if up_on:
        a.g_up, a.ldg_up, a.dy_up, a.dg_up, a.ldd_up = p(gup, 8), ldg, p(dy, col0), p(dgup, 4), ldd_up
    a.dx, a.dx_bf = p(dx, col0), p(dx16, col0)
    a.n_samples, a.T, a.D, a.ca, a.cb, a.rot, a.dgain_scale = n, T, D, o["ca"], o["cb"], rot, dgain_scale
    a.ldx = ldx if "ldx" in c else 0
    nparts = C.c_int(-1)
    a.gain_partials_out = C.addressof(nparts)
    if scratch:
        scr = torch.full((8 * n * 3 * D,), NAN, device=DEV)
        a.part_scratch, a.part_scratch_bytes = p(scr), scr.numel() * 4
    gout = torch.full((1 + GUARD,), NAN, device=DEV)
    if dgain_out:
        a.dgain_out = p(gout)
    entry("resid_mod_bwd", fmt)(C.byref(a), st())
    torch.cuda.synchronize()
    assert (dx is None or kept_outside(dx, rows, col0, D)) and kept_outside(dx16, rows, col0, D) and kept_outside(dy, rows if up_on else 0, col0, D)
    assert kept_outside(dgup, n if up_on else 0, 4, D) and bool(torch.isnan(gout[1:]).all())
    m = torch.ones(dmod.shape, dtype=torch.bool, device=DEV)
    if mod_on:
        m[:n, cS:cS + D], m[:n, cH:cH + D] = False, False
    assert bool(torch.isnan(dmod[m]).all())
    Z = c.get("Z", 1) if scratch else 1
    count = Z * n * (D // (128 if scratch and Z > 1 else c["cols"])) if mod_on else 0
    assert bool(torch.isfinite(part[:count]).all()) and bool(torch.isnan(part[count:]).all())
    tokv = lambda t: None if t is None else f64(t[:rows, col0:col0 + D]).reshape(n, T, D)
    sums = (("dA", cS), ("dB", cH)) if rot else (("dscale", cS), ("dshift", cH))
    got = dict(dx=tokv(dx), dx16=tokv(dx16), dy_up=tokv(dy) if up_on else None, dg_up=f64(dgup[:n, 4:4 + D]) if up_on else None,
               part=part[:count].clone(), nparts=nparts.value, count=count, Z=Z, gout=gout[0].clone())
    if mod_on:
        got.update({k: f64(dmod[:n, col:col + D]) for k, col in sums})
    got["raw"] = dict(dx=dx, dx16=dx16, dy=dy, dmod=dmod, dgup=dgup)
    return o, got


def raw_equal(g1, g2, names=("dx", "dx16", "dy", "dmod", "dgup")):
    for k in names:
        u, v = g1["raw"][k], g2["raw"][k]
        if (u is None) != (v is None) or (u is not None and not same_bits(u, v)):
            return False
    return True


@FMT
@pytest.mark.parametrize("name", list(R.RMB_CASES))
def test_resid_mod_bwd_rotation_form(name, fmt):
    """rot = 1 with `gain` pointing at a zero, the cases of rotation_reference.RMB_CASES: dx within 2 * 5 u of its absolute terms, dA / dB / dg_up
    within 2 T u, the 16-bit outputs within their store bound; cases 3 and 3b (row split by 8 and by 2) return the bits of the unsplit call in
    dx / dx_bf / dy_up and the documented count of gain partials; every written gain partial is 0; case 5b (dxm = NULL) has the bits of the
    same call with rot = 0; case 4 (columns 256..383 of 384-wide tensors) leaves columns 0..255 with the sentinel (run_rmb checks).
    Measured worst ratios: dx 0.24, dA 0.10, dB 0.10, dg_up 0.10, the 16-bit outputs 1.00 (the half ulp of a correct store)."""
    c = R.RMB_CASES[name]
    split = "Z" in c
    o, got = run_rmb(name, fmt, 1, scratch=split)
    r = R.rmb_ratios(o, got, fmt, 1, c["cols"])
    show(f"resid_mod_bwd rot {name} {fmt}", r)
    assert r and max(r.values()) <= 1.0
    assert got["nparts"] == got["count"] and float(got["part"].abs().sum()) == 0.0
    if split:
        _, one = run_rmb(name, fmt, 1, o=o)
        assert got["Z"] == c["Z"] and got["count"] == c["Z"] * one["count"] == c["Z"] * c["n"] * (c["D"] // 128)
        assert raw_equal(got, one, ("dx", "dx16", "dy"))
        r1 = R.rmb_ratios(o, one, fmt, 1, c["cols"])
        show(f"resid_mod_bwd rot {name} {fmt} unsplit", r1)
        assert max(r1.values()) <= 1.0
    if o["dxm"] is None:
        _, plain = run_rmb(name, fmt, 0, o=o)
        assert raw_equal(got, plain)


@FMT
@pytest.mark.parametrize("name", ["1_wide_ragged", "2_lanes32", "3_split8", "4_column_range"])
def test_resid_mod_bwd_adaln_form(name, fmt):
    """rot = 0 per element against the formulas above resid_mod_bwd_kernel: the 32-lane kernel without the row split (D = 384), the column range
    of wider tensors with a 16-bit dxo and no fp32 dx, the 64-lane kernel on a ragged row count and the row split by 8.  dx within 2 * 9 u of
    its absolute terms, dscale / dshift / dg_up within 2 T u, the gain partials (summed over the row slices) within 2 (T cols) u of the
    absolute terms of a block.  Measured worst ratios: dx 0.16, dscale 0.15, dshift 0.08, dg_up 0.08, gain partials below 0.001, the
    16-bit outputs 1.00."""
    c = R.RMB_CASES[name]
    o, got = run_rmb(name, fmt, 0, scratch="Z" in c)
    assert got["nparts"] == got["count"] == got["Z"] * c["n"] * (c["D"] // c["cols"])
    got["dgain_part"] = f64(got["part"]).reshape(got["Z"], c["n"], c["D"] // c["cols"]).sum(0)
    r = R.rmb_ratios(o, got, fmt, 0, c["cols"])
    show(f"resid_mod_bwd adaln {name} {fmt}", r)
    assert max(r.values()) <= 1.0


@FMT
@pytest.mark.parametrize("name", ["2_lanes32", "3_split8"])
def test_resid_mod_bwd_gain_sum_and_scale(name, fmt):
    """dgain_out at Z = 1 and at Z = 8: *gain_partials_out is 0 and the value has the bits of mapdit_reduce_partials over the partials the
    same call writes without dgain_out (whose values test_resid_mod_bwd_adaln_form bounds); every other output keeps its bits.
    dgain_scale = 2^-10: the partials are 2^-10 times the unscaled ones, bit for bit."""
    c = R.RMB_CASES[name]
    split = "Z" in c
    o, base = run_rmb(name, fmt, 0, scratch=split)
    _, own = run_rmb(name, fmt, 0, o=o, scratch=split, dgain_out=True)
    assert base["Z"] == c.get("Z", 1) and base["nparts"] == base["count"] > 0 and own["nparts"] == 0
    assert raw_equal(base, own) and same_bits(base["part"], own["part"]) and bool(torch.isnan(base["gout"]))
    want = torch.full((1,), NAN, device=DEV)
    entry("reduce_partials")(p(base["part"]), base["count"], p(want), 0, st())
    torch.cuda.synchronize()
    assert same_bits(own["gout"].reshape(1), want)
    total = float(f64(base["part"]).sum())
    assert abs(float(own["gout"]) - total) <= 2.0 * base["count"] * R.U24 * float(np.abs(f64(base["part"])).sum())
    _, scaled = run_rmb(name, fmt, 0, o=o, scratch=split, dgain_scale=2.0 ** -10)
    assert same_bits(scaled["part"], base["part"] * 2.0 ** -10) and raw_equal(base, scaled)


# ---- rot_coef_bwd ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", R.COEF_DS)
def test_rot_coef_bwd(D):
    """dscale within 2 * 2 u of its absolute terms and dtheta within 2 * 8 u, each plus the coefficient rule for c and s; exactly
    ceil(D / 512) * n gain partials at index sample * ceil(D / 512) + block, each within 2 * 256 u sum |theta dphi| plus the propagated
    dphi bound, the slot behind them untouched; dgain_scale = 2^-10 scales the partials exactly and 0 means 1; at g = 0 dtheta is 0 and
    dscale has the bits of dA.  Measured worst ratios: dscale 0.36, dtheta 0.30, gain partials 0.03."""
    c, lay, n, h = R.coef_bwd_case(D), coef_layout(D), R.COEF_N, D // 2
    nb = -(-h // 256)
    ldc, ldd = D + 6, D + 10
    mod = mod_rows(c["theta"], c["scale"], lay)
    dA, dB = held(c["dA"], ldc), held(c["dB"], ldc)
    parts = {}
    for g, gscale in ((c["g"], 0.0), (c["g"], 1.0), (c["g"], 2.0 ** -10), (0.0, 0.0)):
        gain = torch.tensor([g], device=DEV)
        dth, dsc = blank(n, ldd), blank(n, ldd)
        part = torch.full((n * nb + GUARD,), NAN, device=DEV)
        entry("rot_coef_bwd")(p(dA), p(dB), ldc, p(mod, lay["theta_off"]), p(mod, lay["scale_off"]), lay["ldm"], p(gain), p(dth), p(dsc), ldd,
                              p(part), gscale, n, D, st())
        torch.cuda.synchronize()
        assert kept_outside(dth, n, 0, h) and kept_outside(dsc, n, 0, D)
        assert bool(torch.isfinite(part[:n * nb]).all()) and bool(torch.isnan(part[n * nb:]).all())
        if gscale == 0.0:
            r = R.coef_bwd_ratios(c, g, f64(dsc[:n, :D]), f64(dth[:n, :h]), f64(part[:n * nb]).reshape(n, nb))
            show(f"rot_coef_bwd D={D} g={g:.2f}", r)
            assert max(r.values()) <= 1.0
        if g == 0.0:
            assert float(dth[:n, :h].abs().max()) == 0.0 and same_bits(dsc[:n, :D], dA[:n, :D])
        else:
            parts[gscale] = (part[:n * nb].clone(), dth.clone(), dsc.clone())
    assert all(same_bits(parts[0.0][i], parts[1.0][i]) for i in range(3))
    assert same_bits(parts[2.0 ** -10][0], parts[1.0][0] * 2.0 ** -10) and all(same_bits(parts[2.0 ** -10][i], parts[1.0][i]) for i in (1, 2))
    refused(entry("rot_coef_bwd"), p(dA), p(dB), ldc, p(mod, lay["theta_off"]), p(mod, lay["scale_off"]), lay["ldm"], p(gain), p(dth), p(dsc), ldd,
            p(part), 0.0, n, D - 1, st())


# ---- scale_accumulate --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", R.ACC_ALPHAS)
@pytest.mark.parametrize("n", R.ACC_NS)
def test_scale_accumulate(n, alpha):
    """out += alpha x with the product rounded to fp32 before the addition: the bits of that evaluation in numpy float32 (a fused multiply-add
    differs in some elements at alpha = 0.3, tests/test_rotation_reference_cpu.py); the elements behind n keep their bits.  (This test
    found the kernel fusing the two: `__fmul_rn` did not keep the product apart under -ffp-contract=fast.)"""
    c = R.accumulate_case(n)
    out = torch.full((n + GUARD,), NAN, device=DEV)
    out[:n] = held(c["out"][None, :])[0]
    x = torch.full((n + GUARD,), NAN, device=DEV)
    x[:n] = held(c["x"][None, :])[0]
    entry("scale_accumulate")(p(out), p(x), n, alpha, st())
    torch.cuda.synchronize()
    want = torch.from_numpy(R.scale_accumulate_f32(c["out"], c["x"], alpha))
    assert same_bits(out[:n].cpu(), want) and bool(torch.isnan(out[n:]).all())
    refused(entry("scale_accumulate"), p(out), p(x), 0, alpha, st())
    refused(entry("scale_accumulate"), p(out), p(x), -5, alpha, st())
