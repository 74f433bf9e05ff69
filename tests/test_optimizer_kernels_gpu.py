"""The fused Adam + EMA step and the non-finite gradient guard (csrc/weights.hip: adam_ema_kernel, adam_ema_ranges_kernel,
grad_nonfinite_kernel, grad_nonfinite_ranges_kernel) through the C ABI and through FusedAdamEMA, element by element against the fp64
reference of tests/optimizer_reference.py (checked on the CPU by tests/test_optimizer_reference_cpu.py).

The bound.  With u = 2^-24, ma = |b1 m| + |(1 - b1) g gs|, den = sqrt(v') c + eps and us = |upd| + step_size ma / den, the error scales are
m': u ma, v': u |v'|, p': u (|p'| + us), e': u (|e| + |p'| + us)  (the cancellation of m' is carried through the divide: it is the
conditioning of the update, not an error of its evaluation).  A plain fp32 evaluation in the kernel's operation order stays within 2.6 /
3.9 / 2.2 / 2.2 scales of fp64 on the stress inputs (asserted <= 4 by the CPU test); every GPU result must stay within LIMIT = 8: twice
that, for fused multiply-adds formed in another association and a 1-ulp device sqrtf / divide.  Worst measured on the MI355X over every
case of this file: p' 2.09, m' 1.94, v' 3.09, e' 1.78 / 1.89 scales - the kernel is as good as the plain fp32 evaluation.

Conventions of every case.  The kernels update in place, so every buffer is an input; each carries GUARD = 64 elements of NaN after its
n elements, which must come back with the bits they had, as must every element no range covers and the gradient buffer as a whole.
Every test prints its worst ratios ("ratio ..." lines, pytest -s).  The kernels exist once (fp32), so nothing is run per 16-bit format.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import optimizer_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
LIMIT = 8.0
NAN_BITS = 0x7FC00000
KEYS = ("p", "g", "m", "v", "ea", "eb")
B1, B2, EPS = R.f32(0.9), R.f32(0.99), R.f32(1e-8)
STDS = (0.05, 0.1)
N0 = 65536 + 4
CONTIGUOUS = ("hyper", "scalars", "guarded")


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------
def lib():
    from mapdit_amd import _lib as L
    return L


def entry(name):
    return getattr(lib().lib(), name)


def st():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def nbits(a):
    return np.ascontiguousarray(a).view(np.int32)


def within(got, want, tol):
    """Worst |got - want| / tol over the elements (0 / 0 counts as 0, an error on a zero tolerance as inf); fp64."""
    got, want, tol = (np.asarray(z, dtype=np.float64) for z in (got, want, tol))
    if got.size == 0:
        return 0.0
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(err == 0, 0.0, err / tol)))


@functools.lru_cache(maxsize=None)
def stress(n=N0, seed=3):
    s = R.stress_state(n, np.random.default_rng(seed))
    for z in s.values():
        z.setflags(write=False)
    return s


def plain_state(n, seed):
    """randn parameters, gradients and first moments of 1e-3 randn, second moments of their size, EMA copies within 1 % of p."""
    rng = np.random.default_rng(seed)
    f = np.float32
    s = dict(p=rng.standard_normal(n).astype(f), g=(1e-3 * rng.standard_normal(n)).astype(f), m=(1e-3 * rng.standard_normal(n)).astype(f),
             v=((1e-3 * rng.standard_normal(n)) ** 2).astype(f))
    s["ea"] = (s["p"] * (1 + 0.01 * rng.uniform(-1, 1, n))).astype(f)
    s["eb"] = (s["p"] * (1 + 0.01 * rng.uniform(-1, 1, n))).astype(f)
    return s


def device_state(s):
    """Host fp32 arrays -> device buffers of n + GUARD elements, NaN behind the n."""
    d = {}
    for k in KEYS:
        t = torch.full((len(s[k]) + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        t[:len(s[k])] = torch.from_numpy(np.array(s[k])).to(DEV)
        d[k] = t
    assert int(bits(d["p"])[-1]) == NAN_BITS
    return d


def table(ranges):
    """Device table of mapdit_range_t {lo, hi, first_block} (three longs) -> (tensor, total_blocks).  The documented contract of the range
    forms, asserted as FusedAdamEMA._range_table asserts it: lo and hi multiples of 4."""
    rows, blk = [], 0
    for lo, hi in ranges:
        assert lo % 4 == 0 and hi % 4 == 0 and hi > lo >= 0
        rows.append((lo, hi, blk))
        blk += (hi - lo + 4095) // 4096
    return torch.tensor(rows, dtype=torch.int64, device=DEV), blk


def mask_of(ranges, n):
    m = np.zeros(n, dtype=bool)
    for lo, hi in ranges:
        assert not m[lo:hi].any(), "overlapping ranges"
        m[lo:hi] = True
    return m


def scalars(hy):
    return lib().AdamScalars(*(float(x) for x in hy))


def launch(kind, d, hy, lo, hi, use=("ea", "eb"), status=None, step=0, ranges=None):
    """One optimiser launch over elements [lo, hi) of the buffers `d` through the entry point `kind`; an EMA copy not in `use` goes in as
    NULL.  The contiguous forms get pointers offset by lo * 4 bytes, as optim.py offsets them; "ranges" gets the base pointers and a table."""
    off = 0 if kind == "ranges" else 4 * lo
    ptr = [d[k].data_ptr() + off if (k not in ("ea", "eb") or k in use) else None for k in KEYS]
    hs = scalars(hy)
    if kind == "hyper":
        hd = torch.from_numpy(np.array(hy, dtype=np.float32)).to(DEV)
        entry("adam_ema_step")(*ptr, hi - lo, p(hd), B1, B2, EPS, st())
    elif kind == "scalars":
        entry("adam_ema_step_scalars")(*ptr, hi - lo, C.byref(hs), B1, B2, EPS, st())
    elif kind == "guarded":
        entry("adam_ema_step_guarded")(*ptr, hi - lo, C.byref(hs), B1, B2, EPS, p(status), step, st())
    else:
        assert kind == "ranges"
        tab, blk = table(ranges if ranges is not None else [(lo, hi)])
        entry("adam_ema_step_ranges")(*ptr, p(tab), tab.shape[0], blk, C.byref(hs), B1, B2, EPS, p(status), step, st())
    torch.cuda.synchronize()


def clean_status():
    return torch.zeros(2, dtype=torch.int32, device=DEV)


def run(kind, s, hy, lo=0, hi=None, **kw):
    d = device_state(s)
    status = clean_status() if kind == "guarded" else kw.pop("status", None)
    launch(kind, d, hy, lo, len(s["p"]) if hi is None else hi, status=status, step=kw.pop("step", 3 if kind == "guarded" else 0), **kw)
    if kind == "guarded":
        assert status.tolist() == [0, 0]
    return d


def verify(d, s, hy, what, covered=None, ema=None, quiet=False):
    """The device buffers `d` after ONE step from the host state `s`: inside `covered` (bool mask over the n elements; None = all) p, m, v
    within LIMIT scales of step64; an EMA copy within LIMIT inside ema[key] (default: `covered`; None there = the copy was not passed)
    and bit-identical to its input outside; everything outside `covered`, every guard element and the whole gradient buffer bit-identical
    to what went in.  Returns the worst ratios."""
    n = len(s["p"])
    cov = np.ones(n, dtype=bool) if covered is None else covered
    ema = {} if ema is None else ema
    want, scale = R.step64(*R.args_of(s), np.asarray(hy, dtype=np.float32), B1, B2, EPS)
    worst = {}
    for k in KEYS:
        got = d[k].detach().cpu().numpy()
        assert got.shape[0] in (n, n + GUARD), (what, k)
        assert np.all(nbits(got[n:]) == NAN_BITS), (what, k, "guard elements")
        c = cov
        if k == "g":
            c = np.zeros(n, dtype=bool)
        elif k in ("ea", "eb") and k in ema:
            c = np.zeros(n, dtype=bool) if ema[k] is None else ema[k]
        assert np.array_equal(nbits(got[:n][~c]), nbits(s[k][~c])), (what, k, "an element outside the update changed")
        if k != "g" and c.any():
            worst[k] = within(got[:n][c], want[k][c], scale[k][c])
    if not quiet:
        print(f"ratio {what}: " + ", ".join(f"{k} {x:.3f}" for k, x in worst.items()) + f" (limit {LIMIT:g})")
    assert all(x <= LIMIT for x in worst.values()), (what, worst)
    return worst


def equal_bits(a, b, keys=KEYS):
    return all(same_bits(a[k], b[k]) for k in keys)


# ---- one step, every entry point -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gs", [1.0, 1.0 / 8, 1.0 / 3], ids=["gs1", "gs1_8", "gs1_3"])
@pytest.mark.parametrize("t", [1, 2, 10, 1000, 100000])
def test_one_step_every_entry_point(t, gs):
    """stress_state, n = 65,536 + 4, through adam_ema_step (device hyper), _scalars, _guarded (clean status) and _ranges (one range): all
    five outputs within 8 scales of step64, the four entry points bit-equal, at t = 1 (EMA beta 0) both copies keep their bits, and an
    element with m = v = g = 0 keeps the bits of p (0 / (0 + eps)).
    Worst measured over the fifteen cases (MI355X): p' 1.89, m' 1.94, v' 3.09, e' 1.78 / 1.89 of the limit's 8 scales; the v' figure is the
    same for every t (v' does not depend on it) and comes from grad_scale 1/3."""
    s = stress()
    hy = R.hyper(t, 1e-2, 0.9, 0.99, STDS, gs)
    first = None
    for kind in CONTIGUOUS + ("ranges",):
        d = run(kind, s, hy)
        if first is None:
            first = d
            verify(d, s, hy, f"one step t={t} gs={gs:.4f}")
            host_p = d["p"][:N0].cpu().numpy()
            zero = (s["m"] == 0) & (s["v"] == 0) & (s["g"] == 0)
            assert zero[:4].all() and zero.sum() >= 4
            assert np.array_equal(nbits(host_p[zero]), nbits(s["p"][zero]))
            if t == 1:
                assert hy[2] == 0 and hy[3] == 0
                assert np.array_equal(nbits(d["ea"][:N0].cpu().numpy()), nbits(s["ea"])) and np.array_equal(nbits(d["eb"][:N0].cpu().numpy()), nbits(s["eb"]))
            else:
                assert not same_bits(d["ea"], device_state(s)["ea"])
        else:
            assert equal_bits(first, d), kind


@pytest.mark.parametrize("kind", ["scalars", "ranges"])
def test_ema_pointers_one_at_a_time(kind):
    """(ema_a, NULL), (NULL, ema_b), (NULL, NULL) - optim.py passes both NULL for the segments outside ema_ranges: the copy that is passed
    stays within the bound, the one that is not keeps its bits, and p, m, v are bit-equal to the run with both."""
    s = stress()
    hy = R.hyper(10, 1e-2, 0.9, 0.99, STDS, 1.0 / 3)
    both = run(kind, s, hy)
    verify(both, s, hy, f"ema both {kind}", quiet=True)
    for use in (("ea",), ("eb",), ()):
        d = run(kind, s, hy, use=use)
        verify(d, s, hy, f"ema pointers {use or 'none'} {kind}", ema={k: None for k in ("ea", "eb") if k not in use})
        assert equal_bits(both, d, ("p", "g", "m", "v") + use)


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 1020, 1024, 1028, 4096, 4100, 4096 * 1024 + 1028])
def test_sizes(n):
    """One float4, one block less / exactly / more than a block's 1,024 elements, a range block of 4,096 and four more, and 4,096 * 1,024 +
    1,028: past the contiguous kernel's cap of 4,096 blocks, so its first 1,028 threads' worth runs a second grid pass with a tail.  Full
    element-wise check of the contiguous form; the range form (ceil(n / 4096) blocks) must give the same bits."""
    s = plain_state(n, seed=n)
    hy = R.hyper(7, 1e-2, 0.9, 0.99, STDS, 0.5)
    d = run("scalars", s, hy)
    verify(d, s, hy, f"size n={n}")
    assert equal_bits(d, run("ranges", s, hy))
    if n <= 4100:
        assert equal_bits(d, run("hyper", s, hy)) and equal_bits(d, run("guarded", s, hy))


@pytest.mark.parametrize("lo", [4, 1028])
def test_sub_range_through_offset_pointers(lo):
    """optim.py hands a shard to the contiguous forms as pointers offset by lo * 4 bytes and a count: elements below lo and from hi upward
    keep their bits (verify() checks that for all six buffers), the rest is within the bound; all three contiguous forms, same bits."""
    s = stress()
    hy = R.hyper(10, 1e-2, 0.9, 0.99, STDS, 1.0 / 8)
    hi = N0 - 2052
    cov = mask_of([(lo, hi)], N0)
    first = None
    for kind in CONTIGUOUS:
        d = run(kind, s, hy, lo, hi)
        verify(d, s, hy, f"sub-range [{lo}, {hi}) {kind}", covered=cov, quiet=first is not None)
        first = first or d
        assert equal_bits(first, d)


# ---- range tables ------------------------------------------------------------------------------------------------------------------------
def _mixed85():
    """85 ranges of mixed lengths - one float4, part of a block, one float4 short of a block, exactly one / two blocks (4,096 and 8,192),
    one float4 more, three blocks and a float4 (12,292), ... - separated by gaps of 4 to 5,000 elements."""
    lens = [4, 128, 4092, 4096, 4100, 8192, 12292, 1024, 20, 16388, 4096, 8, 2048, 6000, 4096 * 3, 12, 5000]
    gaps = [4, 5000, 12, 4096, 100, 1024, 8, 2500, 36, 4]
    out, pos = [], 8
    for i in range(85):
        n = lens[i % len(lens)]
        out.append((pos, pos + n))
        pos += n + gaps[i % len(gaps)]
    return out, pos + 40


def _tables():
    m85, n85 = _mixed85()
    return {"one": ([(8, 8 + 4096 * 2 + 12)], 10000), "two": ([(0, 4096), (4100, 9000)], 9000 + 8), "mixed85": (m85, n85),
            "64x4": ([(8 * i + 4, 8 * i + 8) for i in range(64)], 8 * 64 + 4)}


@pytest.mark.parametrize("name", ["one", "two", "mixed85", "64x4"])
def test_range_tables(name):
    """adam_ema_step_ranges and grad_nonfinite_check_ranges over one range, two, the 85 mixed ranges the sharded weight passes use and 64
    one-block ranges of one float4 each (the binary search over first_block with many equal steps): element-wise against step64 on the
    covered elements, bits kept in every gap, before the first and behind the last range, for all six buffers.  The same table through the
    check: clean -> [0, 0]; an inf in a gap, just before a range or just behind one -> still [0, 0]; an inf on the first or last element of
    a range (the first, the last, every range whose length is a multiple of 4,096, and a sample of the others) -> [step, 1]."""
    ranges, n = _tables()[name]
    assert len(ranges) == {"one": 1, "two": 2, "mixed85": 85, "64x4": 64}[name]
    s = stress(n, seed=11)
    hy = R.hyper(10, 1e-2, 0.9, 0.99, STDS, 1.0 / 3)
    cov = mask_of(ranges, n)
    assert not cov.all()
    d = run("ranges", s, hy, ranges=ranges)
    verify(d, s, hy, f"range table {name} ({len(ranges)} ranges, {int(cov.sum())} of {n} elements)", covered=cov)
    # the guarded range form with a clean status: the same bits
    assert equal_bits(d, run("ranges", s, hy, ranges=ranges, status=clean_status(), step=4))
    # the check over the same table
    tab, blk = table(ranges)
    g = device_state(s)["g"]
    gi = bits(g)
    status = clean_status()
    check = entry("grad_nonfinite_check_ranges")
    inf = 0x7F800000

    def verdict(step):
        check(p(g), p(tab), len(ranges), blk, p(status), step, st())
        torch.cuda.synchronize()
        out = status.tolist()
        status.zero_()
        return out

    assert verdict(1) == [0, 0]
    outside = [i for lo, hi in ranges[:6] + ranges[-6:] for i in (lo - 1, hi) if 0 <= i < n and not cov[i]]
    assert outside
    keep = gi.clone()
    gi[torch.tensor(outside, device=DEV)] = inf
    gi[n:] = inf                                                               # (and the guard elements behind the buffer)
    assert verdict(2) == [0, 0]
    gi.copy_(keep)
    picked = [r for j, r in enumerate(ranges) if j in (0, len(ranges) - 1) or (r[1] - r[0]) % 4096 == 0 or j % 9 == 0]
    step = 3
    for lo, hi in picked:
        for i in (lo, hi - 1):
            old = int(gi[i])
            gi[i] = inf
            assert verdict(step) == [step, 1], (lo, hi, i)
            gi[i] = old
            step += 1
    assert verdict(step) == [0, 0]


# ---- the non-finite check --------------------------------------------------------------------------------------------------------------
NF_N = 2048 * 1024 + 4096


def _clean_gradients(n):
    g = torch.randn(n + GUARD, generator=torch.Generator().manual_seed(21)).to(DEV)
    g[n:] = float("nan")                                                       # the guard elements must not be read
    gi = bits(g)
    fmax, one38 = 0x7F7FFFFF, int(np.float32(1e38).view(np.int32))
    sign = -0x80000000
    specials = [fmax, fmax + sign, 1, 1 + sign, sign, one38, one38 + sign, 0]   # +-FLT_MAX, +-smallest denormal, -0, +-1e38, +0
    for base in (0, 4 * 777, 2048 * 1024 - 8, 2048 * 1024, n - 8):             # in both grid passes, several in one float4
        gi[base:base + 8] = torch.tensor(specials, dtype=torch.int32, device=DEV)
    return g, gi


def test_nonfinite_check_by_position_and_value():
    """Contiguous check, n = 2,048 * 1,024 + 4,096 (past the cap of 2,048 blocks: the last 4,096 elements belong to the second grid pass).
    Clean gradients holding +-FLT_MAX, the smallest denormal, -0 and +-1e38 (x - x = 0 for each) leave the status at [0, 0].  One bad
    value - +inf, -inf, the quiet NaN, NaNs with payload bits (a signalling and a negative one), inf beside -inf in one float4 - at index
    0, on each lane of a float4, at n - 1, on the first and on the last element of the second pass: [step, 1] every time."""
    n = NF_N
    g, gi = _clean_gradients(n)
    status = clean_status()
    check = entry("grad_nonfinite_check")

    def verdict(step):
        check(p(g), n, p(status), step, st())
        torch.cuda.synchronize()
        out = status.tolist()
        status.zero_()
        return out

    assert verdict(1) == [0, 0]
    f4 = 4 * 123457
    positions = {"first": 0, "lane x": f4, "lane y": f4 + 1, "lane z": f4 + 2, "lane w": f4 + 3, "n - 1": n - 1,
                 "first of pass 2": 2048 * 1024, "second float4 of pass 2": 2048 * 1024 + 5, "last of pass 2": 2048 * 1024 + 4095}
    assert positions["last of pass 2"] == n - 1
    pinf, ninf = 0x7F800000, 0x7F800000 - 0x80000000
    values = {"+inf": (pinf,), "-inf": (ninf,), "quiet NaN": (NAN_BITS,), "signalling NaN 0x7f800001": (0x7F800001,),
              "negative NaN with payload": (0x7FC12345 - 0x80000000,), "inf beside -inf": (pinf, ninf)}
    step = 2
    for where, i in positions.items():
        for what, vals in values.items():
            idx = [i] if len(vals) == 1 else [i, i ^ 1]                        # the neighbour inside the same float4
            old = gi[idx].clone()
            gi[idx] = torch.tensor(vals, dtype=torch.int32, device=DEV)
            assert verdict(step) == [step, 1], (where, what)
            gi[idx] = old
            step += 1
    assert step == 2 + 9 * 6 and verdict(step) == [0, 0]                       # everything was put back: clean again


def test_nonfinite_count_once_per_step():
    """1,000 bad values, one in every block of a 1,000-block launch, count as ONE refused step; a second launch with the same step number
    over another sub-range (bad again), through either form of the check, still leaves the count at 1; the next step number with a bad
    value makes it 2; a clean launch in between or afterwards leaves both words alone."""
    n1 = 1000 * 1024
    g, gi = _clean_gradients(NF_N)
    status = clean_status()
    check, check_ranges = entry("grad_nonfinite_check"), entry("grad_nonfinite_check_ranges")

    def contiguous(lo, n, step):
        check(g.data_ptr() + 4 * lo, n, p(status), step, st())
        torch.cuda.synchronize()
        return status.tolist()

    gi[torch.arange(1000, device=DEV) * 1024 + (torch.arange(1000, device=DEV) * 7) % 1024] = 0x7F800000
    gi[n1 + 4096 + 17] = NAN_BITS
    gi[n1 + 3 * 4096 + 4095] = 0x7F800000
    assert contiguous(0, n1, 5) == [5, 1]
    assert contiguous(n1 + 4096, 4096, 5) == [5, 1]                            # same step, another sub-range, bad again
    tab, blk = table([(n1 + 2 * 4096, n1 + 3 * 4096), (n1 + 3 * 4096, n1 + 4 * 4096)])
    check_ranges(p(g), p(tab), 2, blk, p(status), 5, st())                     # ... and through the range form (second range bad)
    torch.cuda.synchronize()
    assert status.tolist() == [5, 1]
    assert contiguous(n1, 4096, 6) == [5, 1]                                   # a clean launch of the next step: both words stay
    assert contiguous(n1 + 4096, 4096, 7) == [7, 2]
    check_ranges(p(g), p(tab), 1, 1, p(status), 8, st())                       # the first range alone is clean
    torch.cuda.synchronize()
    assert status.tolist() == [7, 2]
    check_ranges(p(g), p(tab), 2, blk, p(status), 8, st())
    torch.cuda.synchronize()
    assert status.tolist() == [8, 3]


# ---- the guarded step --------------------------------------------------------------------------------------------------------------------
def test_guarded_step_refuses_and_ignores_a_stale_verdict():
    """status[0] == step: all six buffers keep their bits, contiguous and range form.  status[0] == step - 1 (the verdict of the previous
    step) or step + 1: the step is applied, bit-equal to the unguarded one, and the status words are only read."""
    s = stress()
    hy = R.hyper(10, 1e-2, 0.9, 0.99, STDS, 1.0 / 3)
    ranges = [(0, 4096), (8192, N0 - 4)]
    none = mask_of([], N0)
    applied = {"guarded": run("scalars", s, hy), "ranges": run("ranges", s, hy, ranges=ranges)}
    verify(applied["ranges"], s, hy, "guarded reference, range form", covered=mask_of(ranges, N0), quiet=True)
    for kind in ("guarded", "ranges"):
        for word, refused in ((41, True), (40, False), (42, False)):
            status = torch.tensor([word, 3], dtype=torch.int32, device=DEV)
            d = device_state(s)
            launch(kind, d, hy, 0, N0, status=status, step=41, ranges=ranges if kind == "ranges" else None)
            assert status.tolist() == [word, 3]
            if refused:
                verify(d, s, hy, f"refused {kind}", covered=none, quiet=True)  # nothing covered: every element keeps its bits
            else:
                assert equal_bits(d, applied[kind]), (kind, word)


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    """Every MD_CHECK of the six entry points returns a non-zero status and sets last_error (the wrapper raises MapditError with that
    text); nothing is launched, so the buffers and the status words stay as they were.  Argument checks only."""
    L = lib()
    s = stress()
    d = device_state(s)
    ptr = [p(d[k]) for k in KEYS]
    hs = scalars(R.hyper(10, 1e-2, 0.9, 0.99, STDS, 1.0))
    hd = torch.from_numpy(R.hyper(10, 1e-2, 0.9, 0.99, STDS, 1.0)).to(DEV)
    status = torch.tensor([9, 2], dtype=torch.int32, device=DEV)
    tab, blk = table([(0, 4096)])
    tail, stp = (B1, B2, EPS), st()
    null_p = [None] + ptr[1:]
    null_g = ptr[:1] + [None] + ptr[2:]
    null_v = ptr[:3] + [None] + ptr[4:]
    bad = [
        ("adam_ema_step", (*ptr, 4098, p(hd), *tail, stp)), ("adam_ema_step", (*ptr, 0, p(hd), *tail, stp)),
        ("adam_ema_step", (*ptr, -4, p(hd), *tail, stp)), ("adam_ema_step", (*null_p, 4096, p(hd), *tail, stp)),
        ("adam_ema_step", (*ptr, 4096, None, *tail, stp)),
        ("adam_ema_step_scalars", (*ptr, 4097, C.byref(hs), *tail, stp)), ("adam_ema_step_scalars", (*ptr, 0, C.byref(hs), *tail, stp)),
        ("adam_ema_step_scalars", (*null_g, 4096, C.byref(hs), *tail, stp)), ("adam_ema_step_scalars", (*ptr, 4096, None, *tail, stp)),
        ("adam_ema_step_guarded", (*ptr, 4099, C.byref(hs), *tail, p(status), 5, stp)),
        ("adam_ema_step_guarded", (*ptr, -8, C.byref(hs), *tail, p(status), 5, stp)),
        ("adam_ema_step_guarded", (*null_v, 4096, C.byref(hs), *tail, p(status), 5, stp)),
        ("adam_ema_step_guarded", (*ptr, 4096, C.byref(hs), *tail, p(status), 0, stp)),
        ("adam_ema_step_guarded", (*ptr, 4096, C.byref(hs), *tail, p(status), -1, stp)),
        ("adam_ema_step_guarded", (*ptr, 4096, C.byref(hs), *tail, None, 5, stp)),
        ("adam_ema_step_ranges", (*ptr, p(tab), 0, blk, C.byref(hs), *tail, None, 0, stp)),
        ("adam_ema_step_ranges", (*ptr, p(tab), 1, 0, C.byref(hs), *tail, None, 0, stp)),
        ("adam_ema_step_ranges", (*ptr, None, 1, blk, C.byref(hs), *tail, None, 0, stp)),
        ("adam_ema_step_ranges", (*null_p, p(tab), 1, blk, C.byref(hs), *tail, None, 0, stp)),
        ("adam_ema_step_ranges", (*ptr, p(tab), 1, blk, None, *tail, None, 0, stp)),
        ("adam_ema_step_ranges", (*ptr, p(tab), 1, blk, C.byref(hs), *tail, p(status), 0, stp)),
        ("grad_nonfinite_check", (ptr[1], 4098, p(status), 5, stp)), ("grad_nonfinite_check", (ptr[1], 0, p(status), 5, stp)),
        ("grad_nonfinite_check", (None, 4096, p(status), 5, stp)), ("grad_nonfinite_check", (ptr[1], 4096, None, 5, stp)),
        ("grad_nonfinite_check", (ptr[1], 4096, p(status), 0, stp)), ("grad_nonfinite_check", (ptr[1] + 4, 4096, p(status), 5, stp)),
        ("grad_nonfinite_check_ranges", (ptr[1], p(tab), 0, blk, p(status), 5, stp)),
        ("grad_nonfinite_check_ranges", (ptr[1], p(tab), 1, 0, p(status), 5, stp)),
        ("grad_nonfinite_check_ranges", (ptr[1], p(tab), 1, blk, p(status), 0, stp)),
        ("grad_nonfinite_check_ranges", (ptr[1], None, 1, blk, p(status), 5, stp)),
        ("grad_nonfinite_check_ranges", (None, p(tab), 1, blk, p(status), 5, stp)),
        ("grad_nonfinite_check_ranges", (ptr[1], p(tab), 1, blk, None, 5, stp)),
    ]
    for name, args in bad:
        with pytest.raises(L.MapditError, match=name) as err:
            entry(name)(*args)
        assert f"mapdit_{name} failed (" in str(err.value) and not str(err.value).rstrip().endswith(":"), str(err.value)
        raw = getattr(L.lib()._cdll, "mapdit_" + name)(*args)
        assert raw != 0 and L.lib()._cdll.mapdit_last_error().decode().startswith(name), (name, raw)
    torch.cuda.synchronize()
    assert status.tolist() == [9, 2]
    verify(d, s, np.zeros(5, dtype=np.float32), "argument checks", covered=mask_of([], N0), quiet=True)
    # ... and the same entry points with good arguments still run (the error text of a failed call does not stick to the next one)
    entry("grad_nonfinite_check")(ptr[1], 4096, p(status), 5, stp)
    torch.cuda.synchronize()
    assert status.tolist() == [9, 2]


# ---- FusedAdamEMA on the device ----------------------------------------------------------------------------------------------------------
NP = 20480


class StubModel:
    """Exactly what FusedAdamEMA reads of a model: the flat fp32 buffers, three parameter slots over them, the change notification."""
    gemm_precision = "bf16"

    def __init__(self, p0):
        assert p0.shape == (NP,)
        self._pflat = torch.from_numpy(np.array(p0, dtype=np.float32)).to(DEV)
        self._gflat = torch.zeros_like(self._pflat)
        self._poffs = [0, 4096, 12288]
        shapes = [(64, 64), (8192,), (64, 128)]
        self._params = [self._pflat[o:o + int(np.prod(sh))].view(sh) for o, sh in zip(self._poffs, shapes)]
        self.changed = 0

    def parameters(self):
        return iter(self._params)

    def mark_weights_changed(self):
        self.changed += 1


def _nrel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _torch_trajectory(p0, grads, lam, lr):
    """torch.optim.Adam on fp64 CPU tensors under LambdaLR(lam) + the fp64 EMA lerp -> final (p, m, v, ea, eb), the lr of every step and
    the scheduler's last lr."""
    w = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
    opt = torch.optim.Adam([w], lr=lr, betas=(B1, B2), eps=EPS)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lam)
    ema = [w.detach().clone(), w.detach().clone()]
    lrs = []
    for k, g in enumerate(grads):
        lrs.append(sched.get_last_lr()[0])
        w.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
        sched.step()
        for e, std in zip(ema, STDS):
            e.lerp_(w.detach(), float(R.hyper64(k + 1, lr, B1, B2, (std, std), 1.0)[2]))
    stt = opt.state[w]
    out = dict(p=w.detach().numpy(), m=stt["exp_avg"].numpy(), v=stt["exp_avg_sq"].numpy(), ea=ema[0].numpy(), eb=ema[1].numpy())
    return out, lrs, sched.get_last_lr()[0]


def test_fused_adam_ema_follows_lambda_lr():
    """20 steps of FusedAdamEMA with lr_lambda = create_lr_lambda(5, 12) (warm-up, plateau and decay all inside the 20) and fresh random
    gradients against torch.optim.Adam on fp64 CPU tensors driven by torch.optim.lr_scheduler.LambdaLR with the same lambda, plus the
    fp64 EMA lerp.  The reference carries its own fp64 state: the comparison is of the trajectory, as the norm-relative distance of p,
    exp_avg, exp_avg_sq and both copies after the 20 steps.  Limit per quantity: 4 x the distance at which emulate32 - numpy fp32, the
    scalars of optimizer_reference.hyper() - ends up from the same fp64 trajectory; computed here, not a constant.  The schedule shifted by
    one, lambda(k + 1), run through the reference ends up beyond that limit in p and both copies: the off-by-one is visible.
    Measured (MI355X): 0.25 / 0.23 / 0.24 / 0.25 / 0.25 of the limit for p, exp_avg, exp_avg_sq and the copies - the device ends up as far
    from fp64 as the fp32 emulation does; the shifted schedule at 9.6e3 / 9.8e3 / 9.6e3 times the limit."""
    from mapdit_amd.optim import FusedAdamEMA, create_lr_lambda
    lam, lr, steps = create_lr_lambda(5, 12), 1e-2, 20
    rng = np.random.default_rng(31)
    p0 = rng.standard_normal(NP).astype(np.float32)
    grads = [(rng.standard_normal(NP) * 10.0 ** rng.integers(-4, 1, NP)).astype(np.float32) for _ in range(steps)]
    want, lrs, last_lr = _torch_trajectory(p0, grads, lam, lr)
    assert len(set(lrs)) > 8 and lrs[0] == pytest.approx(lr / 5, rel=1e-15) and lrs[4] == lr and lrs[13] < lr      # warm-up, plateau, decay
    shifted, _, _ = _torch_trajectory(p0, grads, lambda k: lam(k + 1), lr)
    # the fp32 emulation of the same 20 steps
    e = dict(p=p0.copy(), m=np.zeros(NP, np.float32), v=np.zeros(NP, np.float32), ea=p0.copy(), eb=p0.copy())
    for k, g in enumerate(grads):
        e = R.emulate32(e["p"], g, e["m"], e["v"], e["ea"], e["eb"], R.hyper(k + 1, lr * lam(k), B1, B2, STDS, 1.0), B1, B2, EPS)
    limit = {k: 4.0 * _nrel(e[k], want[k]) for k in want}
    assert all(0 < x < 1e-5 for x in limit.values()), limit
    # the device
    model = StubModel(p0)
    opt = FusedAdamEMA(model, lr=lr, betas=(B1, B2), eps=EPS, lr_lambda=lam)
    for k, g in enumerate(grads):
        assert opt.current_lr() == lrs[k]
        model._gflat.copy_(torch.from_numpy(g))
        opt.step()
    torch.cuda.synchronize()
    assert opt.current_lr() == last_lr and model.changed == steps
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2] and all(float(sd["state"][i]["step"]) == steps for i in range(3))
    got = dict(p=model._pflat, m=opt.exp_avg, v=opt.exp_avg_sq, ea=opt.ema[0], eb=opt.ema[1])
    got = {k: z.cpu().numpy() for k, z in got.items()}
    for i, (o, sh) in enumerate(zip(model._poffs, [(64, 64), (8192,), (64, 128)])):
        assert torch.equal(sd["state"][i]["exp_avg"].cpu(), torch.from_numpy(got["m"][o:o + int(np.prod(sh))]).view(sh))
    dist = {k: _nrel(got[k], want[k]) for k in want}
    off = {k: _nrel(got[k], shifted[k]) for k in want}
    print("ratio FusedAdamEMA 20 steps under LambdaLR, distance / (4 x emulate32's): " + ", ".join(f"{k} {dist[k] / limit[k]:.3f}" for k in want))
    print("ratio ... the schedule shifted by one step: " + ", ".join(f"{k} {off[k] / limit[k]:.3g}" for k in ("p", "ea", "eb")) + " (must exceed 1)")
    assert all(dist[k] <= limit[k] for k in want), (dist, limit)
    assert all(off[k] > limit[k] for k in ("p", "ea", "eb")), (off, limit)


SHARDS12 = [(1704 * i + 8, 1704 * i + 8 + 1000 + 4 * ((37 * i) % 100)) for i in range(12)]
EMA_RANGES = [(4096, 8192), (16384, 20480)]
LAYOUTS = {"ema_ranges": (None, EMA_RANGES), "12_shards": (SHARDS12, None), "12_shards_ema_ranges": (SHARDS12, EMA_RANGES)}


def _optimizer(s, shards, ema_ranges, guard):
    """FusedAdamEMA over a stub model in the state `s`, nine steps behind it (the next one is t = 10)."""
    from mapdit_amd.optim import FusedAdamEMA
    model = StubModel(s["p"])
    opt = FusedAdamEMA(model, lr=1e-2, betas=(B1, B2), eps=EPS, grad_scale=1.0 / 3, nonfinite_guard=guard)
    for dst, k in ((model._gflat, "g"), (opt.exp_avg, "m"), (opt.exp_avg_sq, "v"), (opt.ema[0], "ea"), (opt.ema[1], "eb")):
        dst.copy_(torch.from_numpy(np.array(s[k])))
    opt.step_count = 9
    if shards is not None:
        opt.shards = list(shards)
    opt.ema_ranges = None if ema_ranges is None else list(ema_ranges)
    return model, opt, dict(p=model._pflat, g=model._gflat, m=opt.exp_avg, v=opt.exp_avg_sq, ea=opt.ema[0], eb=opt.ema[1])


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_fused_adam_ema_shards_and_ema_ranges(layout):
    """ema_ranges with the default shard (four contiguous launches, two of them without EMA pointers), 12 shards (more than 8 segments: ONE
    range launch) and 12 shards with ema_ranges (the per-segment fallback): Adam on every element of the shards within the bound of this
    file, the EMA copies moved only inside ema_ranges (within the bound there, their bits kept outside), everything outside the shards
    with its bits.  With the guard on, an inf inside a shard makes every layout refuse the step (all buffers keep their bits, one refused
    step counted), an inf outside every shard makes none refuse (the two layouts that have an outside)."""
    shards, ema_ranges = LAYOUTS[layout]
    s = stress(NP, seed=41)
    hy = R.hyper(10, 1e-2, B1, B2, STDS, 1.0 / 3)
    cov = mask_of(shards if shards is not None else [(0, NP)], NP)
    ecov = cov if ema_ranges is None else cov & mask_of(ema_ranges, NP)
    assert ecov.any() and (shards is None or not cov.all())
    for guard in (False, True):
        model, opt, d = _optimizer(s, shards, ema_ranges, guard)
        opt.step()
        torch.cuda.synchronize()
        verify(d, s, hy, f"FusedAdamEMA {layout} guard={guard}", covered=cov, ema={"ea": ecov, "eb": ecov}, quiet=guard)
        assert opt.step_count == 10 and model.changed == 1 and (not guard or opt.overflow_steps() == 0)
    # an inf inside a shard: refused
    inside = int(np.flatnonzero(cov)[len(np.flatnonzero(cov)) // 2])
    bad = {k: np.array(z) for k, z in s.items()}
    bad["g"][inside] = np.inf
    model, opt, d = _optimizer(bad, shards, ema_ranges, True)
    opt.step()
    torch.cuda.synchronize()
    for k in KEYS:
        assert np.array_equal(nbits(d[k].cpu().numpy()), nbits(bad[k])), (layout, k)
    assert opt.overflow_steps() == 1 and opt._status.tolist() == [1, 1]
    # an inf outside every shard: applied
    if shards is not None:
        outside = int(np.flatnonzero(~cov)[3])
        ok = {k: np.array(z) for k, z in s.items()}
        ok["g"][outside] = np.inf
        model, opt, d = _optimizer(ok, shards, ema_ranges, True)
        opt.step()
        torch.cuda.synchronize()
        assert opt._status.tolist() == [0, 0]
        got = {k: d[k].cpu().numpy() for k in KEYS}
        assert np.array_equal(nbits(got["g"]), nbits(ok["g"]))
        ref = _optimizer(s, shards, ema_ranges, False)
        ref[1].step()
        torch.cuda.synchronize()
        assert all(same_bits(d[k], ref[2][k]) for k in KEYS if k != "g")
