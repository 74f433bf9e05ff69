"""Global gradient-norm clipping through the C ABI (csrc/weights.hip: grad_sqnorm_kernel, grad_sqnorm_ranges_kernel, grad_sqnorm_sum_kernel,
grad_clip_coef_kernel and the clip argument of adam_ema_kernel / adam_ema_ranges_kernel) against tests/grad_clip_reference.py (checked on
the CPU by tests/test_grad_clip_cpu.py).

The bound is derived there: fp64 squares and sums err by at most n 2^-53, so the fp32 norm and coefficient the device writes are within
TOL = 2^-23 relative (one ulp) of clip64.  The step kernels are held to the existing entry points bit for bit.  Every gradient buffer
carries GUARD elements of NaN behind its n elements, which must not be read (a NaN would reach the norm).
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import grad_clip_reference as G
import optimizer_reference as R
from test_optimizer_kernels_gpu import (B1, B2, EPS, KEYS, N0, STDS, bits, clean_status, device_state, equal_bits, mask_of, run, scalars, stress,
                                        table)

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
INF_BITS, NAN_BITS = 0x7F800000, 0x7FC00000


def L():
    from mapdit_amd import _lib
    return _lib


def entry(name):
    return getattr(L().lib(), name)


def st():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


@functools.lru_cache(maxsize=None)
def family():
    return G.family()


def to_device(g):
    """n gradients + GUARD NaNs behind them."""
    t = torch.full((len(g) + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    t[:len(g)] = torch.from_numpy(np.ascontiguousarray(g)).to(DEV)
    return t


def blocks_of(n):
    return (n + 4095) // 4096


def device_clip(g, n, gs, mx, status=None, step=0, via_sum=False):
    """grad_sqnorm over the first n elements of the device buffer g [-> grad_sqnorm_sum] -> grad_clip_coef; returns (clip, partials)."""
    nb = blocks_of(n)
    partials = torch.full((nb + 1,), float("nan"), dtype=torch.float64, device=DEV)          # one guard word
    clip = torch.full((2,), float("nan"), dtype=torch.float32, device=DEV)
    entry("grad_sqnorm")(p(g), n, p(partials), st())
    if via_sum:
        sqsum = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
        entry("grad_sqnorm_sum")(p(partials), nb, p(sqsum), st())
        entry("grad_clip_coef")(p(sqsum), 1, gs, mx, p(clip), p(status), step, st())
    else:
        entry("grad_clip_coef")(p(partials), nb, gs, mx, p(clip), p(status), step, st())
    torch.cuda.synchronize()
    assert math.isnan(float(partials[nb]))
    return clip, partials[:nb]


def close(got, want):
    return abs(float(got) - want) <= G.TOL * abs(want)


# ---- every case of the input family ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["position", "range", "accuracy", "coef"])
def test_norm_and_coef_against_clip64(group):
    """positions: one non-zero element at index 0 / 4,095 / 4,096 / n - 1 of n in {4, 4,096, 4,100, 3 * 4,096 + 8} - a missed tail, a missed
    block, an off-by-one block; range: one 3e19 / one 1e-30 at three gradient scales - finite, correct norms; accuracy: n = 2^22 stress
    gradients; coef: the clamp at exactly 1.0f, max_norm = inf, the visible 1e-6.  Norm and coef within 2^-23 of clip64, directly and
    through grad_sqnorm_sum (the ZeRO-1 form, grad_clip_coef(sqsum, 1): the same fixed-order sum, then s + 0 - the same two words bit for
    bit)."""
    cases = {k: v for k, v in family().items() if k.startswith(group)}
    assert len(cases) >= 2
    worst = 0.0
    for name, (g, gs, mx) in cases.items():
        n = len(g)
        want_norm, want_coef = G.clip64(g, gs, mx)
        dg = to_device(g)
        first = None
        for via_sum in (False, True):
            clip, partials = device_clip(dg, n, gs, mx, via_sum=via_sum)
            first = clip if first is None else first
            assert torch.equal(bits(clip), bits(first)), name
            norm, coef = clip.tolist()
            e = max(G.rel_diff(norm, want_norm), G.rel_diff(coef, want_coef))
            worst = max(worst, e)
            print(f"{name} via_sum={via_sum}: norm {norm:.9g} (want {want_norm:.17g}), coef {coef:.9g} (want {want_coef:.17g}), rel {e:.3e}")
            assert math.isfinite(norm) and close(norm, want_norm) and close(coef, want_coef), (name, via_sum, norm, want_norm, coef, want_coef)
            if want_coef == 1.0:
                assert coef == 1.0, name
            total = float(partials.sum(dtype=torch.float64))
            assert abs(total - G.sqsum64(g)) <= max(n * 2.0 ** -53, 2.0 ** -52) * G.sqsum64(g), name
        if group == "position":
            assert close(norm, 1.5 * gs) and int((partials != 0).sum()) == 1
    print(f"{group}: worst relative deviation {worst:.3e} (bound {G.TOL:.3e})")
    if group == "coef":
        assert abs(float(device_clip(to_device(family()["coef eps visible"][0]), 8, 1.0, G.f32(1e-5))[0][1]) - 0.476) < 5e-4
        below = float(device_clip(to_device(family()["coef just below"][0]), 8, 1.0, G.f32(0.5))[0][1])
        assert below < 1.0


# ---- range tables ----------------------------------------------------------------------------------------------------------------------
def _layouts():
    one = [(8, 8 + 4096 * 2 + 12)]
    # ZeRO-1-like: 14 stage slices, each cut into 2 equal 4-aligned parts; rank 1's parts
    parts, pos = [], 0
    for i in range(14):
        half = 4 * (300 + 517 * i % 2100)
        parts.append((pos + half, pos + 2 * half))
        pos += 2 * half
    n14 = pos
    # ragged: ~85 ranges of mixed lengths with gaps between them
    lens = [4, 128, 4092, 4096, 4100, 8192, 12292, 1024, 20, 16388, 4096, 8, 2048, 6000, 4096 * 3, 12, 5000]
    gaps = [4, 5000, 12, 4096, 100, 1024, 8, 2500, 36, 4]
    ragged, pos = [], 8
    for i in range(85):
        ragged.append((pos, pos + lens[i % len(lens)]))
        pos += lens[i % len(lens)] + gaps[i % len(gaps)]
    return {"one": (one, 10000), "zero1_14": (parts, n14), "ragged85": (ragged, pos + 40)}


@pytest.mark.parametrize("name", ["one", "zero1_14", "ragged85"])
def test_range_tables(name):
    """grad_sqnorm_ranges over one range, 14 ZeRO-1-like parts and 85 ragged 4-aligned ranges whose gaps (and the elements before the
    first and behind the last range) hold NaN: norm and coef within 2^-23 of clip64 over the covered elements - a NaN read anywhere would
    make them NaN - every workgroup's partial sum finite, and two runs give equal bits (partials, norm, coef)."""
    ranges, n = _layouts()[name]
    assert len(ranges) == {"one": 1, "zero1_14": 14, "ragged85": 85}[name]
    g = np.array(G.stress_gradient(n, seed=23))
    cov = mask_of(ranges, n)
    assert not cov.all()
    g[~cov] = np.nan
    covered = g[cov]
    gs, mx = G.f32(1.0 / 3), G.f32(2.5)
    want_norm, want_coef = G.clip64(covered, gs, mx)
    assert want_coef < 1.0
    dg = to_device(g)
    tab, nblk = table(ranges)
    runs = []
    for _ in range(2):
        partials = torch.full((nblk + 1,), float("nan"), dtype=torch.float64, device=DEV)
        clip = torch.full((2,), float("nan"), dtype=torch.float32, device=DEV)
        entry("grad_sqnorm_ranges")(p(dg), p(tab), len(ranges), nblk, p(partials), st())
        entry("grad_clip_coef")(p(partials), nblk, gs, mx, p(clip), None, 0, st())
        torch.cuda.synchronize()
        assert math.isnan(float(partials[nblk])) and bool(torch.isfinite(partials[:nblk]).all())
        runs.append((partials[:nblk].clone(), clip.clone()))
    norm, coef = runs[0][1].tolist()
    print(f"{name}: norm {norm:.9g} (want {want_norm:.17g}), coef {coef:.9g} (want {want_coef:.17g})")
    assert close(norm, want_norm) and close(coef, want_coef), (norm, want_norm, coef, want_coef)
    assert torch.equal(runs[0][0].view(torch.int64), runs[1][0].view(torch.int64)) and torch.equal(bits(runs[0][1]), bits(runs[1][1]))
    # a partial per workgroup: block b of range r covers [lo + 4096 b, min(lo + 4096 (b + 1), hi))
    want_partials = [G.sqsum64(g[lo + 4096 * b:min(lo + 4096 * (b + 1), hi)]) for lo, hi in ranges for b in range(blocks_of(hi - lo))]
    got = runs[0][0].cpu().numpy()
    assert len(want_partials) == nblk and np.all(np.abs(got - want_partials) <= 4096 * 2.0 ** -53 * np.asarray(want_partials))
    if name == "one":                                                          # the contiguous form over the same elements: the same bits
        lo, hi = ranges[0]
        c2, p2 = device_clip(dg[lo:], hi - lo, gs, mx)
        assert torch.equal(p2.view(torch.int64), runs[0][0].view(torch.int64)) and torch.equal(bits(c2), bits(runs[0][1]))


# ---- the status contract ---------------------------------------------------------------------------------------------------------------
def test_nonfinite_sum_records_the_verdict_of_the_check():
    """n = 3 * 4,096 + 8.  A finite buffer writes nothing to status (clean words stay [0, 0], foreign words stay what they are).  An inf, a
    -inf or a NaN at index 0 / 4,095 / 4,096 / n - 1 records {step, 1}; a second call with the same step leaves the count at 1; the next
    step number makes it 2.  With status == NULL the outputs follow the formulas: inf norm -> coef 0, NaN norm -> NaN coef."""
    n = 3 * 4096 + 8
    g = np.array(G.stress_gradient(n, seed=29))
    dg = to_device(g)
    gi = bits(dg)
    gs, mx = G.f32(1.0 / 8), G.f32(1.0)
    status = clean_status()
    clip, _ = device_clip(dg, n, gs, mx, status=status, step=7)
    assert status.tolist() == [0, 0] and math.isfinite(float(clip[0]))
    foreign = torch.tensor([9, 2], dtype=torch.int32, device=DEV)
    device_clip(dg, n, gs, mx, status=foreign, step=7)
    assert foreign.tolist() == [9, 2]
    step = 10
    for i in (0, 4095, 4096, n - 1):
        for what, word in (("+inf", INF_BITS), ("-inf", INF_BITS - 0x80000000), ("NaN", NAN_BITS)):
            old = int(gi[i])
            gi[i] = word
            status = clean_status()
            clip, _ = device_clip(dg, n, gs, mx, status=status, step=step)
            assert status.tolist() == [step, 1], (i, what)
            norm, coef = clip.tolist()
            assert (math.isnan(norm) and math.isnan(coef)) if what == "NaN" else (norm == math.inf and coef == 0.0), (i, what, norm, coef)
            device_clip(dg, n, gs, mx, status=status, step=step, via_sum=True)      # the same step again: counted once
            assert status.tolist() == [step, 1], (i, what)
            device_clip(dg, n, gs, mx, status=status, step=step + 1)
            assert status.tolist() == [step + 1, 2], (i, what)
            clip, _ = device_clip(dg, n, gs, mx)                                    # status NULL: the formulas
            norm, coef = clip.tolist()
            assert (math.isnan(norm) and math.isnan(coef)) if what == "NaN" else (norm == math.inf and coef == 0.0), (i, what, norm, coef)
            gi[i] = old
            step += 2
    status = clean_status()
    device_clip(dg, n, gs, mx, status=status, step=step)
    assert status.tolist() == [0, 0]                                                # everything was put back


# ---- the step ----------------------------------------------------------------------------------------------------------------------------
RANGES = [(0, 4096), (8192, N0 - 4)]


def clipped(s, hy, coef, ranges=None, status=None, step=0):
    """One launch of adam_ema_step_clipped (or _ranges_clipped) from the host state `s` with clip = {NaN, coef} written by the test."""
    d = device_state(s)
    clip = torch.tensor([float("nan"), coef], dtype=torch.float32, device=DEV)
    ptr = [d[k].data_ptr() for k in KEYS]
    hs = scalars(hy)
    if ranges is None:
        entry("adam_ema_step_clipped")(*ptr, len(s["p"]), C.byref(hs), B1, B2, EPS, p(status), step, p(clip), st())
    else:
        tab, blk = table(ranges)
        entry("adam_ema_step_ranges_clipped")(*ptr, p(tab), len(ranges), blk, C.byref(hs), B1, B2, EPS, p(status), step, p(clip), st())
    torch.cuda.synchronize()
    assert math.isnan(float(clip[0])) and float(clip[1]) == float(np.float32(coef))
    return d


@pytest.mark.parametrize("gs", [1.0, 1.0 / 3], ids=["gs1", "gs1_3"])
def test_clipped_step_is_the_existing_step_bit_for_bit(gs):
    """stress_state, n = 65,536 + 4.  clip[1] == 1.0f: _clipped equals adam_ema_step_guarded (clean status) and adam_ema_step_scalars
    (status NULL), _ranges_clipped equals adam_ema_step_ranges, all six buffers.  clip[1] in {0.5, 1/3}: equal to the existing entry
    points called with grad_scale' = fp32(grad_scale * clip[1]) - the kernel's one fp32 multiplication."""
    s = stress()
    hy = R.hyper(10, 1e-2, 0.9, 0.99, STDS, gs)
    for coef in (1.0, 0.5, float(np.float32(1.0 / 3))):
        hy2 = hy.copy()
        hy2[4] = np.float32(hy[4]) * np.float32(coef)
        assert (coef == 1.0) == (hy2[4] == hy[4])
        want = run("guarded", s, hy2)
        assert equal_bits(want, run("scalars", s, hy2))
        assert equal_bits(want, clipped(s, hy, coef, status=clean_status(), step=3)), coef
        assert equal_bits(want, clipped(s, hy, coef)), coef
        want_r = run("ranges", s, hy2, ranges=RANGES)
        assert not equal_bits(want_r, want)
        assert equal_bits(want_r, clipped(s, hy, coef, ranges=RANGES)), coef
        assert equal_bits(want_r, clipped(s, hy, coef, ranges=RANGES, status=clean_status(), step=3)), coef
    assert not equal_bits(run("guarded", s, hy), clipped(s, hy, 0.5))               # (and a coefficient below 1 does change the step)


def test_clipped_step_refuses_a_recorded_bad_step():
    """status[0] == step: parameters, gradients, moments and both EMA copies keep their bits, contiguous and range form; the verdict of
    another step is ignored."""
    s = stress()
    hy = R.hyper(10, 1e-2, 0.9, 0.99, STDS, 1.0 / 3)
    before = device_state(s)
    for ranges in (None, RANGES):
        status = torch.tensor([41, 3], dtype=torch.int32, device=DEV)
        d = clipped(s, hy, 0.5, ranges=ranges, status=status, step=41)
        assert equal_bits(d, before) and status.tolist() == [41, 3]
        d = clipped(s, hy, 0.5, ranges=ranges, status=status, step=42)
        assert not equal_bits(d, before, ("p", "m", "v", "ea", "eb")) and equal_bits(d, before, ("g",)) and status.tolist() == [41, 3]
        assert equal_bits(d, clipped(s, hy, 0.5, ranges=ranges))


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    """Null pointers, misalignment, n % 4, max_norm <= 0 or NaN, a verdict without a step number: a non-zero status whose message names
    the function; nothing is launched (outputs and status words keep their values)."""
    lib = L()
    s = stress()
    d = device_state(s)
    ptr = [p(d[k]) for k in KEYS]
    g = ptr[1]
    hs = scalars(R.hyper(10, 1e-2, 0.9, 0.99, STDS, 1.0))
    status = torch.tensor([9, 2], dtype=torch.int32, device=DEV)
    partials = torch.full((32,), 3.0, dtype=torch.float64, device=DEV)
    clip = torch.tensor([5.0, 6.0], dtype=torch.float32, device=DEV)
    tab, blk = table([(0, 4096)])
    tail, stp, nan = (B1, B2, EPS), st(), float("nan")
    null_p = [None] + ptr[1:]
    bad = [
        ("grad_sqnorm", (None, 4096, p(partials), stp)), ("grad_sqnorm", (g, 4096, None, stp)), ("grad_sqnorm", (g, 0, p(partials), stp)),
        ("grad_sqnorm", (g, 4098, p(partials), stp)), ("grad_sqnorm", (g + 4, 4096, p(partials), stp)),
        ("grad_sqnorm", (g, 4096, p(partials) + 4, stp)),
        ("grad_sqnorm_ranges", (None, p(tab), 1, blk, p(partials), stp)), ("grad_sqnorm_ranges", (g, None, 1, blk, p(partials), stp)),
        ("grad_sqnorm_ranges", (g, p(tab), 0, blk, p(partials), stp)), ("grad_sqnorm_ranges", (g, p(tab), 1, 0, p(partials), stp)),
        ("grad_sqnorm_ranges", (g, p(tab), 1, blk, None, stp)), ("grad_sqnorm_ranges", (g + 8, p(tab), 1, blk, p(partials), stp)),
        ("grad_sqnorm_sum", (None, 4, p(partials), stp)), ("grad_sqnorm_sum", (p(partials), 4, None, stp)),
        ("grad_sqnorm_sum", (p(partials), 0, p(partials), stp)), ("grad_sqnorm_sum", (p(partials) + 4, 4, p(partials), stp)),
        ("grad_clip_coef", (None, 4, 1.0, 1.0, p(clip), None, 0, stp)), ("grad_clip_coef", (p(partials), 4, 1.0, 1.0, None, None, 0, stp)),
        ("grad_clip_coef", (p(partials), 0, 1.0, 1.0, p(clip), None, 0, stp)), ("grad_clip_coef", (p(partials), 4, 1.0, 0.0, p(clip), None, 0, stp)),
        ("grad_clip_coef", (p(partials), 4, 1.0, -1.0, p(clip), None, 0, stp)), ("grad_clip_coef", (p(partials), 4, 1.0, nan, p(clip), None, 0, stp)),
        ("grad_clip_coef", (p(partials), 4, 1.0, 1.0, p(clip), p(status), 0, stp)),
        ("grad_clip_coef", (p(partials) + 4, 4, 1.0, 1.0, p(clip), None, 0, stp)),
        ("adam_ema_step_clipped", (*null_p, 4096, C.byref(hs), *tail, None, 0, p(clip), stp)),
        ("adam_ema_step_clipped", (*ptr, 4098, C.byref(hs), *tail, None, 0, p(clip), stp)),
        ("adam_ema_step_clipped", (*ptr, 4096, None, *tail, None, 0, p(clip), stp)),
        ("adam_ema_step_clipped", (*ptr, 4096, C.byref(hs), *tail, p(status), 0, p(clip), stp)),
        ("adam_ema_step_clipped", (*ptr, 4096, C.byref(hs), *tail, None, 0, None, stp)),
        ("adam_ema_step_ranges_clipped", (*null_p, p(tab), 1, blk, C.byref(hs), *tail, None, 0, p(clip), stp)),
        ("adam_ema_step_ranges_clipped", (*ptr, None, 1, blk, C.byref(hs), *tail, None, 0, p(clip), stp)),
        ("adam_ema_step_ranges_clipped", (*ptr, p(tab), 0, blk, C.byref(hs), *tail, None, 0, p(clip), stp)),
        ("adam_ema_step_ranges_clipped", (*ptr, p(tab), 1, blk, C.byref(hs), *tail, p(status), 0, p(clip), stp)),
        ("adam_ema_step_ranges_clipped", (*ptr, p(tab), 1, blk, C.byref(hs), *tail, None, 0, None, stp)),
    ]
    for name, args in bad:
        with pytest.raises(lib.MapditError, match=name) as err:
            entry(name)(*args)
        assert f"mapdit_{name} failed (" in str(err.value), str(err.value)
        raw = getattr(lib.lib()._cdll, "mapdit_" + name)(*args)
        assert raw != 0 and lib.lib()._cdll.mapdit_last_error().decode().startswith(name), (name, raw)
    torch.cuda.synchronize()
    assert status.tolist() == [9, 2] and clip.tolist() == [5.0, 6.0] and bool((partials == 3.0).all())
    assert equal_bits(d, device_state(s))
    # max_norm = +inf is legal, and the error text of a failed call does not stick to the next one
    entry("grad_clip_coef")(p(partials), 4, 0.5, math.inf, p(clip), p(status), 5, stp)
    torch.cuda.synchronize()
    assert clip.tolist() == [float(np.float32(0.5 * math.sqrt(12.0))), 1.0] and status.tolist() == [9, 2]      # four partials of 3.0
