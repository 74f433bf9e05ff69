"""Counter-based sampler draws on the MI355X: csrc/samplerng.hip against the numpy restatement of its contract
(tests/sample_rng_reference.py), index addressing, the fused steps against today's step kernels fed with mapdit_sample_noise bit for
bit, the eager and captured loops, and sample_fid.py's parts / shards / resume."""
import os

import numpy as np
import pytest
import torch

import sample_rng_reference as S
from test_data_gpu import EPS, NORMAL_BOUND_ULP          # the derived bound of the fp32 normal recipe: the same recipe, the same bound

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SEED = 0x0123456789ABCDEF
INDEX, TS = [0, 7, 2 ** 32 - 1], [0, 1, 999]
SENTINEL = 12345.0


def L():
    from mapdit_amd import _lib
    return _lib


def rng(seed=SEED):
    from mapdit_amd.sample_rng import SampleRNG
    return SampleRNG(seed, DEV)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def dev64(v):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


def plane_buffer(n, per, offset):
    """[n, per] fp32 view with `offset` sentinel elements in front and one behind."""
    full = torch.full((offset + n * per + 1,), SENTINEL, dtype=torch.float32, device=DEV)
    return full, full[offset:offset + n * per].view(n, per)


def check_sentinels(full, offset, what):
    assert float(full[-1]) == SENTINEL and (full[:offset] == SENTINEL).all(), f"{what}: wrote outside its plane"


def raw_draw(index, per, num_classes=10, want_z=True, want_y=True, offset=0, seed=SEED):
    idx = dev64(index)
    full, z = plane_buffer(len(index), per, offset) if want_z else (None, None)
    yfull = torch.full((len(index) + 2,), -77, dtype=torch.int64, device=DEV) if want_y else None
    y = yfull[1:-1] if want_y else None
    L().lib().sample_draw(seed, idx.data_ptr(), len(index), per, num_classes, L().ptr(z), L().ptr(y), L().cur_stream())
    if want_z:
        check_sentinels(full, offset, "z")
    if want_y:
        assert int(yfull[0]) == -77 and int(yfull[-1]) == -77, "y: wrote outside its array"
    return z, y


def raw_noise(index, t, per, offset=0, seed=SEED):
    idx, tt = dev64(index), dev64(t)
    full, nz = plane_buffer(len(index), per, offset)
    L().lib().sample_noise(seed, idx.data_ptr(), tt.data_ptr(), len(index), per, nz.data_ptr(), L().cur_stream())
    check_sentinels(full, offset, "noise")
    return nz


def assert_normals(got, ref, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    err = np.abs(got - ref) / (np.abs(ref) * EPS)
    print(f"{what}: largest error {err.max():.2f} ulp (bound {NORMAL_BOUND_ULP})")
    assert (err <= NORMAL_BOUND_ULP).all(), (what, err.max())


# ---- 1. the contract ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def aligned():
    """The aligned call every ragged / offset call is a prefix of: per = 4100 (a multiple of 4 past the largest ragged size)."""
    z, y = raw_draw(INDEX, 4100)
    assert z.data_ptr() % 16 == 0
    return z, y, raw_noise(INDEX, TS, 4100)


def test_draw_and_noise_are_the_contract(aligned):
    z, y, nz = aligned
    assert_normals(z, np.stack([S.z0(SEED, s, 4100) for s in INDEX]), "z0")
    assert_normals(nz, np.stack([S.noise(SEED, s, t, 4100) for s, t in zip(INDEX, TS)]), "noise")
    for nc in (10, 1000):
        got = raw_draw(INDEX, 1, nc, want_z=False)[1].cpu().numpy()
        ref = S.labels(SEED, INDEX, nc)
        assert (got == ref).all() and (ref < nc).all() and (ref >= 0).all(), nc
    assert (y.cpu().numpy() == S.labels(SEED, INDEX, 10)).all()
    for t in TS + [2, 500]:                                # the initial latent of an index is not its noise at any step
        other = raw_noise(INDEX, [t] * 3, 4100)
        for j in range(3):
            assert not torch.equal(bits(other[j]), bits(z[j])), (t, j)
    assert not same(raw_draw(INDEX, 8, seed=SEED + 1, want_y=False)[0], z[:, :8])
    assert not same(raw_draw(INDEX, 8, seed=SEED + (1 << 32), want_y=False)[0], z[:, :8])      # the key's high word


@pytest.mark.parametrize("per,offset", [(4096, 0), (4, 0), (1, 0), (6, 0), (4097, 0), (4096, 1)])
def test_ragged_and_unaligned_planes_hold_the_aligned_values(aligned, per, offset):
    """per % 4 != 0: the tail path; per = 4: one whole 16-byte group; offset 1: planes 4 bytes off a 16-byte boundary, element-wise
    stores.  An element is a function of (index, t, i) alone, so every call's rows are prefixes of the aligned call's; the raw_*
    helpers check the sentinels on both sides of every plane."""
    z, y = raw_draw(INDEX, per, offset=offset)
    nz = raw_noise(INDEX, TS, per, offset=offset)
    assert z.data_ptr() % 16 == (4 * offset) % 16 and nz.data_ptr() % 16 == (4 * offset) % 16
    assert same(z, aligned[0][:, :per]) and same(nz, aligned[2][:, :per]) and torch.equal(y, aligned[1])


def test_null_outputs_each_work_alone(aligned):
    z, y = raw_draw(INDEX, 4100, want_y=False)
    assert y is None and same(z, aligned[0])
    z, y = raw_draw(INDEX, 4100, want_z=False)
    assert z is None and torch.equal(y, aligned[1])
    idx = dev64(INDEX)
    L().lib().sample_draw(SEED, idx.data_ptr(), 3, 16, 10, None, None, L().cur_stream())          # nothing asked for: nothing done
    with pytest.raises(L().MapditError, match="num_classes"):
        raw_draw(INDEX, 4, num_classes=0)


# ---- 2. index addressing -------------------------------------------------------------------------------------------------------

def test_rows_are_addressed_by_their_index():
    r, shape = rng(), (3, 5, 7)                              # per = 105: ragged
    whole = r.latents([5, 6, 7, 8], shape)
    assert whole.shape == (4, 3, 5, 7) and whole.dtype == torch.float32
    assert same(torch.cat([r.latents([5, 6], shape), r.latents([7, 8], shape)]), whole)
    assert same(r.latents([8, 6, 5, 7], shape), whole[[3, 1, 0, 2]])
    assert same(r.latents([6, 6, 5, 6], shape), whole[[1, 1, 0, 1]])
    assert same(rng().latents(dev64([5, 6, 7, 8]), shape), whole)                    # no state in the object; a device index
    t = dev64([3, 0, 3, 9])
    nz = r.noise([5, 6, 7, 8], t, shape)
    assert same(torch.cat([r.noise([5, 6], t[:2], shape), r.noise([7, 8], t[2:], shape)]), nz)
    assert same(r.noise([7, 5], dev64([3, 3]), shape), nz[[2, 0]])
    assert same(r.noise([5, 5], dev64([3, 3]), shape)[0], nz[0]) and same(r.noise([5, 5], dev64([3, 3]), shape)[1], nz[0])
    assert not same(r.noise([5], dev64([4]), shape)[0], nz[0])                        # another step, other words
    y = r.labels([5, 6, 7, 8], 1000)
    assert y.dtype == torch.int64 and torch.equal(r.labels([8, 5, 5], 1000), y[[3, 0, 0]])
    assert (y.cpu().numpy() == S.labels(SEED, [5, 6, 7, 8], 1000)).all()
    with pytest.raises(ValueError, match=r"does not lie in \[0, 2\^32\)"):
        r.latents([0, 2 ** 32], shape)
    with pytest.raises(ValueError, match=r"does not lie in \[0, 2\^32\)"):
        r.check_index(dev64([-1]))


# ---- 3. fused equals unfused, bit for bit ----------------------------------------------------------------------------------------

N, IDX3 = 3, [11, 2 ** 32 - 1, 5]
EPSILON, START_X = 0, 1
LEARNED_RANGE, FIXED_SMALL, FIXED_LARGE = 0, 1, 2


@pytest.fixture(scope="module")
def sched():
    from mapdit_amd.diffusion import create_diffusion
    d = create_diffusion("8")
    assert d.num_timesteps == 8
    return d, d._tables(DEV), d._obj_tables(DEV), dev64([0, 1, d.num_timesteps - 1]), dev64(IDX3)


def step_inputs(per, channels):
    g = torch.Generator().manual_seed(per * 10 + channels)
    mo = torch.randn(N, channels * per, generator=g).to(DEV)
    x = (1.5 * torch.randn(N, per, generator=g)).to(DEV)
    return mo, x


@pytest.mark.parametrize("per", [256, 6])
@pytest.mark.parametrize("clip", [0, 1])
def test_psample_step_counter_is_psample_step_on_the_materialised_noise(sched, per, clip):
    d, tab, _, t, idx = sched
    lib, st = L().lib(), L().cur_stream()
    mo, x = step_inputs(per, 2)
    nz = raw_noise(IDX3, t.tolist(), per)
    want_s, want_x = torch.empty_like(x), torch.empty_like(x)
    lib.psample_step(mo.data_ptr(), x.data_ptr(), nz.data_ptr(), t.data_ptr(), tab.data_ptr(), 8, clip, want_s.data_ptr(), want_x.data_ptr(), N, per, st)
    got_s, got_x = torch.full_like(x, SENTINEL), torch.full_like(x, SENTINEL)
    lib.psample_step_counter(mo.data_ptr(), x.data_ptr(), SEED, idx.data_ptr(), t.data_ptr(), tab.data_ptr(), 8, clip, got_s.data_ptr(),
                             got_x.data_ptr(), N, per, st)
    assert same(got_s, want_s) and same(got_x, want_x)
    assert not same(want_s[1], torch.zeros_like(want_s[1])) and torch.isfinite(want_s).all()
    only_s = torch.full_like(x, SENTINEL)                                             # without pred_xstart
    lib.psample_step_counter(mo.data_ptr(), x.data_ptr(), SEED, idx.data_ptr(), t.data_ptr(), tab.data_ptr(), 8, clip, only_s.data_ptr(), None, N, per, st)
    assert same(only_s, want_s)
    inplace = x.clone()                                                               # sample aliasing x
    lib.psample_step_counter(mo.data_ptr(), inplace.data_ptr(), SEED, idx.data_ptr(), t.data_ptr(), tab.data_ptr(), 8, clip, inplace.data_ptr(),
                             got_x.data_ptr(), N, per, st)
    assert same(inplace, want_s) and same(got_x, want_x)
    # the row at t = 0 takes no noise: the step kernel gives the same row for any noise tensor
    zero = torch.empty_like(x)
    lib.psample_step(mo.data_ptr(), x.data_ptr(), torch.zeros_like(nz).data_ptr(), t.data_ptr(), tab.data_ptr(), 8, clip, zero.data_ptr(), None, N, per, st)
    assert same(zero[0], want_s[0]) and not same(zero[1], want_s[1])


@pytest.mark.parametrize("per", [256, 6])
@pytest.mark.parametrize("mean_type,var_type,mode,eta", [
    (START_X, LEARNED_RANGE, 0, 0.0), (EPSILON, FIXED_SMALL, 0, 0.0), (EPSILON, FIXED_LARGE, 0, 0.0), (EPSILON, LEARNED_RANGE, 0, 0.0),
    (EPSILON, LEARNED_RANGE, 1, 0.5), (EPSILON, LEARNED_RANGE, 1, 0.0), (START_X, FIXED_SMALL, 1, 0.5)])
def test_obj_step_counter_is_obj_step_on_the_materialised_noise(sched, per, mean_type, var_type, mode, eta):
    d, tab, otab, t, idx = sched
    lib, st = L().lib(), L().cur_stream()
    mo, x = step_inputs(per, 2 if var_type == LEARNED_RANGE else 1)
    nz = raw_noise(IDX3, t.tolist(), per)
    for clip in (0, 1):
        want_s, want_x = torch.empty_like(x), torch.empty_like(x)
        lib.obj_step(mo.data_ptr(), x.data_ptr(), nz.data_ptr(), t.data_ptr(), tab.data_ptr(), otab.data_ptr(), 8, mean_type, var_type, clip, mode,
                     eta, want_s.data_ptr(), want_x.data_ptr(), N, per, st)
        got_s, got_x = torch.full_like(x, SENTINEL), torch.full_like(x, SENTINEL)
        lib.obj_step_counter(mo.data_ptr(), x.data_ptr(), SEED, idx.data_ptr(), t.data_ptr(), tab.data_ptr(), otab.data_ptr(), 8, mean_type,
                             var_type, clip, mode, eta, got_s.data_ptr(), got_x.data_ptr(), N, per, st)
        assert same(got_s, want_s) and same(got_x, want_x), clip
        assert torch.isfinite(want_s).all()
        inplace = x.clone()
        lib.obj_step_counter(mo.data_ptr(), inplace.data_ptr(), SEED, idx.data_ptr(), t.data_ptr(), tab.data_ptr(), otab.data_ptr(), 8, mean_type,
                             var_type, clip, mode, eta, inplace.data_ptr(), None, N, per, st)
        assert same(inplace, want_s), clip


def test_obj_step_counter_refuses_the_reverse_ode(sched):
    d, tab, otab, t, idx = sched
    mo, x = step_inputs(8, 2)
    out = torch.empty_like(x)
    with pytest.raises(L().MapditError, match="reverse ODE"):
        L().lib().obj_step_counter(mo.data_ptr(), x.data_ptr(), SEED, idx.data_ptr(), t.data_ptr(), tab.data_ptr(), otab.data_ptr(), 8, EPSILON,
                                   LEARNED_RANGE, 0, 2, 0.0, out.data_ptr(), None, N, 8, L().cur_stream())
    with pytest.raises(L().MapditError, match="overlaps"):
        L().lib().obj_step_counter(mo.data_ptr(), x.data_ptr(), SEED, idx.data_ptr(), t.data_ptr(), tab.data_ptr(), otab.data_ptr(), 8, EPSILON,
                                   LEARNED_RANGE, 0, 0, 0.0, out.data_ptr(), out.data_ptr(), N, 8, L().cur_stream())


def test_an_out_of_range_timestep_is_clamped_and_recorded(sched):
    d, tab, _, _, idx = sched
    mo, x = step_inputs(8, 2)
    out = torch.empty_like(x)
    L().lib().psample_step_counter(mo.data_ptr(), x.data_ptr(), SEED, idx.data_ptr(), dev64([0, 8, -1]).data_ptr(), tab.data_ptr(), 8, 0,
                                   out.data_ptr(), None, N, 8, L().cur_stream())
    with pytest.raises(L().MapditError, match="timestep"):
        L().lib().device_error_poll(L().cur_stream())
    assert torch.isfinite(out).all()


# ---- 4. the loops ------------------------------------------------------------------------------------------------------------------

SHAPE = (4, 4, 32, 32)                                       # two samples, guidance: four rows


@pytest.fixture(scope="module")
def xs():
    from mapdit_amd.src.models import DIT_MODELS
    torch.manual_seed(0)
    return DIT_MODELS["DiT-XS/2"](in_channels=4, input_size=32, num_classes=10).to(DEV).eval()


@pytest.fixture(scope="module")
def d4():
    from mapdit_amd.diffusion import create_diffusion
    return create_diffusion("4")


@pytest.fixture(scope="module")
def kw():
    return dict(y=torch.tensor([3, 7, 10, 10], device=DEV), cfg_scale=1.5)


@pytest.fixture(scope="module")
def kw_same():
    """A guidance batch whose unconditional half carries the conditional labels: the two halves are then the same computation, and can
    differ only through the noise they are given.  (With the null labels of real guidance the model's variance channels differ between
    the halves - forward_with_cfg mixes eps only, as the reference's does - so the discarded half takes another noise SCALE; the noise
    itself is the same, which is what this isolates.)"""
    return dict(y=torch.tensor([3, 7, 3, 7], device=DEV), cfg_scale=1.5)


@pytest.fixture(scope="module")
def halves39(xs, d4, kw_same):
    with torch.no_grad():
        return d4.p_sample_loop(xs.forward_with_cfg, SHAPE, model_kwargs=kw_same, device=DEV, rng=rng(), index=[3, 9])


@pytest.fixture(scope="module")
def eager39(xs, d4, kw):
    with torch.no_grad():
        return d4.p_sample_loop(xs.forward_with_cfg, SHAPE, model_kwargs=kw, device=DEV, rng=rng(), index=[3, 9])


def test_p_sample_loop_is_a_function_of_the_indices(xs, d4, kw, eager39, halves39):
    assert eager39.shape == SHAPE and torch.isfinite(eager39).all()
    torch.manual_seed(123)                                   # whatever the torch generator holds
    torch.randn(5, device=DEV)
    with torch.no_grad():
        again = d4.p_sample_loop(xs.forward_with_cfg, SHAPE, model_kwargs=kw, device=DEV, rng=rng(), index=[3, 9])
        swapped = d4.p_sample_loop(xs.forward_with_cfg, SHAPE, model_kwargs=dict(y=kw["y"][[1, 0, 3, 2]], cfg_scale=1.5), device=DEV, rng=rng(),
                                   index=[9, 3])
        other = d4.p_sample_loop(xs.forward_with_cfg, SHAPE, model_kwargs=kw, device=DEV, rng=rng(), index=[4, 5])
    assert same(again, eager39)
    assert same(swapped, eager39[[1, 0, 3, 2]])
    assert same(halves39[:2], halves39[2:]) and torch.isfinite(halves39).all()         # the halves carry the same indices: the same noise
    assert not same(other, eager39) and not same(eager39[0], eager39[1])
    before = torch.cuda.get_rng_state(DEV)
    with torch.no_grad():
        d4.p_sample_loop(xs.forward_with_cfg, SHAPE, model_kwargs=kw, device=DEV, rng=rng(), index=[3, 9])
    assert torch.equal(torch.cuda.get_rng_state(DEV), before)                          # the counter path consumes no generator
    with pytest.raises(ValueError, match="3 sample indices for a batch of 4 rows"):
        d4.p_sample_loop(xs.forward_with_cfg, SHAPE, model_kwargs=kw, device=DEV, rng=rng(), index=[3, 9, 4])


def test_captured_sampler_is_the_eager_loop_and_is_re_aimed_without_recapture(xs, d4, kw, kw_same, eager39, halves39):
    from mapdit_amd import sampling as SM
    gs = SM.GraphedSampler(xs, d4, SHAPE, kw["y"], 1.5, clip_denoised=True, rng=rng())
    graph = gs.graph
    assert gs.index.shape == (4,) and gs.index.dtype == torch.int64
    first = gs.sample(index=[3, 9])
    assert same(first, eager39)
    assert gs.index.tolist() == [3, 9, 3, 9]
    other = gs.sample(index=[4, 5])
    assert not same(other, first)
    assert same(gs.sample(index=[3, 9]), first) and gs.graph is graph
    gs.y.copy_(kw_same["y"])                                 # the two halves of the returned state are equal: the same noise reaches both
    both = gs.sample(index=[3, 9])
    assert same(both[:2], both[2:]) and same(both, halves39) and gs.graph is graph
    gs.y.copy_(kw["y"])
    with pytest.raises(ValueError, match="needs index="):
        gs.sample()
    with pytest.raises(ValueError, match=r"does not lie in \[0, 2\^32\)"):
        gs.sample(index=[3, 2 ** 32])
    z = rng().latents([3, 9, 3, 9], SHAPE[1:])
    assert same(gs.sample(z, index=[3, 9]), first)          # a given start is taken as it is


def test_a_sampler_without_an_rng_is_what_it_was(xs, d4, kw):
    from mapdit_amd import sampling as SM
    gs = SM.GraphedSampler(xs, d4, SHAPE, kw["y"], 1.5, clip_denoised=True)
    assert gs.rng is None and gs.index is None
    z = torch.randn(2, *SHAPE[1:], device=DEV)
    z = torch.cat([z, z])
    torch.manual_seed(5)
    a = gs.sample(noise=z)
    torch.manual_seed(5)
    b = gs.sample(z)
    assert a.shape == SHAPE and torch.isfinite(a).all() and same(a, b)                 # the torch generator's noise, as before
    with pytest.raises(ValueError, match="built with rng="):
        gs.sample(z, index=[3, 9])


def test_the_other_loops_run_and_repeat(xs, d4, kw):
    fn = xs.forward_with_cfg
    with torch.no_grad():
        for run in (lambda: d4.ddim_sample_loop(fn, SHAPE, model_kwargs=kw, device=DEV, eta=0.5, rng=rng(), index=[3, 9]),
                    lambda: d4.ddim_sample_loop(fn, SHAPE, model_kwargs=kw, device=DEV, eta=0.0, rng=rng(), index=[3, 9]),
                    lambda: d4.dpm_solver_sample_loop(fn, SHAPE, model_kwargs=kw, device=DEV, num_steps=3, rng=rng(), index=[3, 9]),
                    lambda: d4.p_sample_loop(fn, SHAPE, model_kwargs=kw, device=DEV, denoised_fn=lambda x, *a, **k: x, rng=rng(), index=[3, 9])):
            a = run()
            torch.randn(3, device=DEV)
            b = run()
            assert a.shape == SHAPE and torch.isfinite(a).all() and same(a, b)
    from mapdit_amd.flow import create_flow
    f = create_flow()
    with torch.no_grad():
        a = f.sample_loop(fn, SHAPE, model_kwargs=kw, device=DEV, num_steps=3, rng=rng(), index=[3, 9])
        b = f.sample_loop(fn, SHAPE, model_kwargs=kw, device=DEV, num_steps=3, rng=rng(), index=[3, 9])
    assert same(a, b) and torch.isfinite(a).all()


# ---- 5. sample_fid: parts, shards, resume ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def exp_dir(tmp_path_factory):
    from mapdit_amd import train
    root = tmp_path_factory.mktemp("results")
    return train.main(["--synthetic", "--results-dir", str(root), "--model", "DiT-XS/2", "--num-steps", "8", "--batch-size", "8",
                       "--log-every", "4", "--ckpt-every", "8", "--ema-snapshot-every", "2", "--num-classes", "10",
                       "--num-lin-warmup", "2", "--start-decay", "3", "--verbose", "0"])


def fid_main(exp_dir, *more):
    from mapdit_amd import sample_fid
    return sample_fid.main(["--result-dir", exp_dir, "--use-vae", "false", "--num-sampling-steps", "2", "--batch-size", "4", "--num-samples", "10",
                            *more])


def arr(path):
    with np.load(path) as f:
        return f["arr_0"]


def test_sample_fid_parts_shards_and_resume_give_the_same_bytes(exp_dir, capsys):
    from mapdit_amd.sample_fid import part_path, parts_dir
    ctr = ["--sample-rng", "counter"]
    # (a) one process
    path_a = fid_main(exp_dir, *ctr, "--output-file", "a.npz")
    a = arr(path_a)
    assert a.shape == (10, 32, 32, 4) and a.dtype == np.uint8 and len(np.unique(a)) > 16
    pdir = parts_dir(exp_dir, "a.npz")
    names = ["0-4.npy", "4-8.npy", "8-10.npy"]
    assert sorted(os.listdir(pdir)) == sorted(names + ["manifest.json"])
    assert (np.concatenate([np.load(os.path.join(pdir, n)) for n in names]) == a).all()
    # (b) two shards, one after the other, into another file
    capsys.readouterr()
    got = fid_main(exp_dir, *ctr, "--output-file", "b.npz", "--shard", "0/2")
    said = capsys.readouterr().out
    assert got == parts_dir(exp_dir, "b.npz") and "missing sample ranges: 4-8" in said and "2 of 3 parts" in said
    assert not os.path.exists(os.path.join(exp_dir, "fid_samples", "b.npz"))
    path_b = fid_main(exp_dir, *ctr, "--output-file", "b.npz", "--shard", "1/2")
    assert path_b.endswith("b.npz") and arr(path_b).tobytes() == a.tobytes()
    # (c) the run of (a) again with one part gone: only that batch is made again
    os.remove(part_path(pdir, 4, 8))
    os.remove(path_a)
    kept = {n: os.stat(os.path.join(pdir, n)).st_mtime_ns for n in ("0-4.npy", "8-10.npy", "manifest.json")}
    from mapdit_amd import sampling
    calls, real = [], sampling.GraphedSampler.sample

    def counted(self, *args, **kwargs):
        calls.append(kwargs.get("index"))
        return real(self, *args, **kwargs)
    sampling.GraphedSampler.sample = counted
    try:
        path_c = fid_main(exp_dir, *ctr, "--output-file", "a.npz")
    finally:
        sampling.GraphedSampler.sample = real
    assert calls == [[4, 5, 6, 7]]
    assert {n: os.stat(os.path.join(pdir, n)).st_mtime_ns for n in kept} == kept
    assert path_c == path_a and arr(path_c).tobytes() == a.tobytes()
    # a run that differs in anything the bytes depend on is refused, by name
    with pytest.raises(ValueError, match=r"cfg_scale = 1\.5.*cfg_scale = 1\.0"):
        fid_main(exp_dir, *ctr, "--output-file", "a.npz", "--cfg-scale", "1.0")
    # the eager loop writes the same bytes as the captured one (its manifest says which made them: another file)
    path_e = fid_main(exp_dir, *ctr, "--output-file", "e.npz", "--no-graph")
    assert arr(path_e).tobytes() == a.tobytes()


def test_the_default_rng_writes_no_parts(exp_dir):
    path = fid_main(exp_dir, "--output-file", "t.npz")
    assert arr(path).shape == (10, 32, 32, 4)
    assert sorted(n for n in os.listdir(os.path.join(exp_dir, "fid_samples")) if n.startswith("t.")) == ["t.npz"]
