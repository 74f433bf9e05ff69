"""Device-resident data set on the MI355X: csrc/dataset.hip (Philox normals, the epoch permutation, the one-launch batch) against the
numpy restatement of its contract (tests/data_reference.py) and against torch's own ops on the CPU, data.DeviceLatentDataset's
invariances, and train.py --data-loader."""
import os

import numpy as np
import pytest
import torch

import data_reference as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# ---- the error bound of a normal, derived ---------------------------------------------------------------------------------
# z = r t with r = sqrt(-2 L), L = ln u, t = cos or sin of 2 pi u'.  The kernel hands every library function an EXACT argument
# (include/mapdit.h: u below 1/2 as it is, above 1/2 through 1 - u), so the only errors are the functions' own, in units of
# EPS = 2^-23 >= one ulp relative to the result:
#   logf / log1pf   <= 3 ulp (the larger of the two in the OpenCL accuracy table the device library is built to; HIP's table says 1)
#                   -2 L is exact, and the square root halves a relative error:                                   1.5
#   sqrtf           correctly rounded in this build (0.5); budgeted                                               1
#   sincospif       <= 4 ulp per output (same table; HIP's says 1); cos / sin of pi x are never 0 here: x is an odd
#                   multiple of 2^-24, never a multiple of 1/2, so the bound is relative throughout               4
#   the product r t                                                                                              0.5
# 7 ulp in first order; the cross terms are below 7^2 EPS^2 < 0.01 EPS.  The fp64 restatement's own error (1e-16) does not count.
EPS = 2.0 ** -23
NORMAL_BOUND_ULP = 8


def L():
    from mapdit_amd import _lib
    return _lib


def philox_normal(seed, c1, c2, c3, n):
    out = torch.full((n + 3,), float("nan"), device=DEV)                 # three guard values behind the tail
    L().lib().philox_normal(seed, c1, c2, c3, out.data_ptr(), n, L().cur_stream())
    assert torch.isnan(out[n:]).all()
    return out[:n]


def data_perm(seed, epoch, N, first, count):
    idx = torch.full((count,), -1, dtype=torch.int64, device=DEV)
    L().lib().data_perm(seed, epoch, N, first, count, idx.data_ptr(), L().cur_stream())
    return idx.cpu().numpy()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 4099])
def test_philox_normals_match_the_fp64_restatement_within_the_derived_bound(n):
    seed, c1, c2, c3 = 0x299F31D0A4093822, 0x85A308D3, 0x13198A2E, 0x03707344
    z = philox_normal(seed, c1, c2, c3, n).cpu().numpy().astype(np.float64)
    ref = R.normals(seed, c1, c2, c3, n)
    err = np.abs(z - ref) / (np.abs(ref) * EPS)
    print(f"n={n}: largest error {err.max():.2f} ulp (bound {NORMAL_BOUND_ULP})")
    assert (err <= NORMAL_BOUND_ULP).all(), err.max()


def test_philox_normals_of_the_upper_half_are_as_accurate():
    """Draws whose u lies above 1/2 need 25 bits: the reflected evaluation must not lose them (r would be off by up to 2.4e-4)."""
    n = 1 << 16
    z = philox_normal(1, 2, 3, 4, n).cpu().numpy().astype(np.float64)
    ref = R.normals(1, 2, 3, 4, n)
    u = np.stack([R.uniforms(w) for w in R.philox(np.arange(n // 4, dtype=np.uint64), 2, 3, 4, *R.key(1))], axis=1)
    assert (u[:, 0] > 1 - 2.0 ** -12).any() and (u[:, 1] > 0.5).any()   # the case is in the sample
    err = np.abs(z - ref) / (np.abs(ref) * EPS)
    print(f"n={n}: largest error {err.max():.2f} ulp (bound {NORMAL_BOUND_ULP})")
    assert (err <= NORMAL_BOUND_ULP).all(), err.max()


def test_philox_normal_moments():
    n = 1 << 20
    z = philox_normal(0, 5, 3, R.TAG_NOISE, n).cpu().numpy().astype(np.float64)
    p3 = 0.0026998
    corr = np.corrcoef(z.reshape(-1, 4).T)
    sig = {"mean": abs(z.mean()) * np.sqrt(n), "variance": abs(z.var() - 1.0) / np.sqrt(2.0 / n),
           "share of |z| > 3": abs((np.abs(z) > 3).mean() - p3) / np.sqrt(p3 * (1 - p3) / n),
           "lane correlation": np.abs(corr - np.eye(4)).max() * np.sqrt(n / 4)}
    print(sig)                                                           # the fp64 restatement: 0.47, 0.01, 0.38, 1.93
    assert all(v < 4.0 for v in sig.values()), sig
    assert np.abs(z).max() <= np.sqrt(50 * np.log(2.0)) * (1 + 8 * EPS)


@pytest.mark.parametrize("N", [1, 2, 3, 255, 256, 257, 1000, 65537])
def test_data_perm_is_the_restated_bijection(N):
    whole = data_perm(11, 7, N, 0, N)
    assert (whole == R.perm(11, 7, N, np.arange(N))).all()
    assert (np.sort(whole) == np.arange(N)).all()
    if N > 1:
        h = N // 2
        assert (np.concatenate([data_perm(11, 7, N, 0, h), data_perm(11, 7, N, h, N - h)]) == whole).all()
    if N > 3:
        assert (data_perm(11, 8, N, 0, N) != whole).any()


def make_set(N, C, hw, seed=5):
    g = torch.Generator().manual_seed(seed)
    means = torch.randn(N, C, hw, generator=g)
    stds = torch.rand(N, C, hw, generator=g) * 0.5
    means.view(-1)[::7] = -0.0
    stds.view(-1)[::5] = 0.0
    stds.view(-1)[1::11] = 1e-40                                         # a denormal
    labels = torch.randint(0, 1000, (N,), generator=g)
    m = torch.randn(C, generator=g)
    s = torch.rand(C, generator=g) + 0.5
    return means, stds, labels, m, s


def data_batch(dset, seed, epoch, first, count, eps=None):
    means, stds, labels, m, s = dset
    N, C, hw = means.shape
    x = torch.full((count, C, hw), float("nan"), device=DEV)
    y = torch.full((count,), -1, dtype=torch.int64, device=DEV)
    idx = torch.full((count,), -1, dtype=torch.int64, device=DEV)
    L().lib().data_batch(means.data_ptr(), stds.data_ptr(), labels.data_ptr(), N, C, hw, m.data_ptr(), s.data_ptr(), seed, epoch, first, count,
                         None if eps is None else eps.data_ptr(), x.data_ptr(), y.data_ptr(), idx.data_ptr(), L().cur_stream())
    return x, y, idx


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("count", [1, 5, 64])
@pytest.mark.parametrize("C,hw", [(4, 256), (4, 1024), (3, 15), (1, 1)])
def test_data_batch_with_given_noise_is_bit_equal_to_torch(C, hw, count):
    N, seed, epoch = 257, 0xABCDEF0123, 3
    host = make_set(N, C, hw)
    dset = tuple(t.to(DEV) for t in host)
    first = N - count if count != 5 else 3                               # a window that ends on the last position, and one inside
    eps = torch.randn(count, C, hw, generator=torch.Generator().manual_seed(count))
    x, y, idx = data_batch(dset, seed, epoch, first, count, eps.to(DEV))
    idx = idx.cpu()
    assert (idx.numpy() == R.perm(seed, epoch, N, np.arange(first, first + count))).all()
    means, stds, labels, m, s = host
    ref = ((means[idx] + eps * stds[idx]) - m.view(1, C, 1)) / s.view(1, C, 1)
    assert torch.equal(bits(x), bits(ref))
    assert torch.equal(y.cpu(), labels[idx])


@pytest.mark.parametrize("C,hw,count", [(4, 1024, 5), (3, 15, 5), (1, 1, 1), (4, 256, 64)])
def test_data_batch_draws_the_contracted_noise(C, hw, count):
    N, seed, epoch, first = 257, 77, 9, 100
    dset = tuple(t.to(DEV) for t in make_set(N, C, hw))
    eps = torch.stack([philox_normal(seed, first + j, epoch, R.TAG_NOISE, C * hw) for j in range(count)]).view(count, C, hw)
    x0, y0, i0 = data_batch(dset, seed, epoch, first, count)
    x1, y1, i1 = data_batch(dset, seed, epoch, first, count, eps)
    assert torch.equal(bits(x0), bits(x1)) and torch.equal(y0, y1) and torch.equal(i0, i1)
    assert not torch.isnan(x0).any()


def test_data_batch_on_unaligned_rows_takes_the_scalar_path():
    """per_sample % 4 == 0 but a base 4 bytes off a 16-byte boundary: element-wise path, same bits."""
    N, C, hw, count, seed = 33, 4, 16, 7, 1
    host = make_set(N, C, hw)
    dset = tuple(t.to(DEV) for t in host)
    pad = torch.zeros(N * C * hw + 1, device=DEV)
    pad[1:] = dset[0].view(-1)
    off = (pad[1:].view(N, C, hw),) + dset[1:]
    assert off[0].data_ptr() % 16 == 4
    a, b = data_batch(dset, seed, 0, 2, count), data_batch(off, seed, 0, 2, count)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[1], b[1])


def small_set(N=100, seed=1):
    g = torch.Generator().manual_seed(seed)
    stats = {"mean": torch.randn(4, generator=g), "std": torch.rand(4, generator=g) + 0.5}
    return torch.randn(N, 4, 8, 8, generator=g), torch.rand(N, 4, 8, 8, generator=g), torch.arange(N), stats     # label = index


def test_batches_do_not_depend_on_the_world_size_or_the_object():
    from mapdit_amd.data import DeviceLatentDataset
    B = 16
    ds, twin, other = DeviceLatentDataset(small_set(), DEV, seed=3), DeviceLatentDataset(small_set(), DEV, seed=3), DeviceLatentDataset(small_set(), DEV, seed=4)
    assert (len(ds), ds.channels, ds.data_size) == (100, 4, 8)
    for step in (0, 5, 6, 13):                                           # six steps per epoch: 5 -> 6 crosses into epoch 1
        x, y = ds.batch(step, B)
        assert x.shape == (B, 4, 8, 8) and x.dtype == torch.float32 and y.dtype == torch.int64
        assert ds.position(step, B) == R.position(step, B, 100)
        for world in (2, 4):
            parts = [ds.batch(step, B, r, world) for r in range(world)]
            assert torch.equal(bits(torch.cat([p[0] for p in parts])), bits(x)) and torch.equal(torch.cat([p[1] for p in parts]), y)
        xt, yt = twin.batch(step, B)
        assert torch.equal(bits(xt), bits(x)) and torch.equal(yt, y)
        xo, yo = other.batch(step, B)
        assert not torch.equal(yo, y) and not torch.equal(bits(xo), bits(x))
    seen = [torch.cat([ds.batch(s, B)[1] for s in range(e * 6, e * 6 + 6)]).cpu().tolist() for e in (0, 1)]
    for e in (0, 1):
        assert len(set(seen[e])) == 96                                   # within an epoch no index repeats
        assert seen[e] == R.perm(3, e, 100, np.arange(96)).tolist()
    assert set(range(100)) - set(seen[0]) != set(range(100)) - set(seen[1])      # the dropped tails differ
    # the same sample visited in two epochs draws fresh noise
    k = next(v for v in seen[0] if v in seen[1])
    p0, p1 = seen[0].index(k), seen[1].index(k)
    assert not torch.equal(ds.batch(p0 // B, B)[0][p0 % B], ds.batch(6 + p1 // B, B)[0][p1 % B])


def test_refusals():
    from mapdit_amd._lib import MapditError
    from mapdit_amd.data import DeviceLatentDataset
    dset = tuple(t.to(DEV) for t in make_set(10, 2, 3))
    means, stds, labels, m, s = dset
    x, y = torch.zeros(4, 2, 3, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    lib, st = L().lib(), L().cur_stream()
    good = [means.data_ptr(), stds.data_ptr(), labels.data_ptr(), 10, 2, 3, m.data_ptr(), s.data_ptr(), 0, 0, 0, 4, None, x.data_ptr(), y.data_ptr(), None, st]
    lib.data_batch(*good)
    for pos, val, msg in [(0, None, "null pointer"), (2, None, "null pointer"), (7, None, "null pointer"), (13, None, "null pointer"), (14, None, "null pointer"),
                          (11, 0, "count"), (10, 7, "do not lie in"), (10, -1, "do not lie in"), (4, 0, "channels"), (5, 0, "channels"),
                          (3, 0, "samples"), (3, 1 << 32, "samples")]:
        bad = list(good)
        bad[pos] = val
        with pytest.raises(MapditError, match=msg):
            lib.data_batch(*bad)
    idx = torch.zeros(4, dtype=torch.int64, device=DEV)
    for args, msg in [((0, 0, 10, 7, 4, idx.data_ptr(), st), "do not lie in"), ((0, 0, 10, -1, 4, idx.data_ptr(), st), "do not lie in"),
                      ((0, 0, 10, 0, 0, idx.data_ptr(), st), "do not lie in"), ((0, 0, 1 << 32, 0, 4, idx.data_ptr(), st), "samples"),
                      ((0, 0, 10, 0, 4, None, st), "null")]:
        with pytest.raises(MapditError, match=msg):
            lib.data_perm(*args)
    with pytest.raises(MapditError, match="values"):
        lib.philox_normal(0, 0, 0, 0, x.data_ptr(), 0, st)
    with pytest.raises(MapditError, match="null"):
        lib.philox_normal(0, 0, 0, 0, None, 4, st)
    src = small_set(20)
    with pytest.raises(ValueError, match="std"):
        DeviceLatentDataset(src[:3] + ({"mean": [0.0] * 4, "std": [1.0, 0.0, 1.0, 1.0]},), DEV)
    with pytest.raises(ValueError, match="std"):
        DeviceLatentDataset(src[:3] + ({"mean": [0.0] * 4, "std": [1.0, float("nan"), 1.0, 1.0]},), DEV)
    with pytest.raises(NotImplementedError):
        DeviceLatentDataset(src, torch.device("cpu"))
    with pytest.raises(ValueError, match="fewer than the global batch"):
        DeviceLatentDataset(src, DEV).batch(0, 32)


def test_a_data_set_that_does_not_fit_names_both_figures(monkeypatch):
    from mapdit_amd._lib import MapditError
    from mapdit_amd.data import DeviceLatentDataset
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1000, 2000))
    with pytest.raises(MapditError, match=r"needs 205,600 bytes .* 1,000 are free"):       # 2 x 100 x 256 x 4 + 100 x 8
        DeviceLatentDataset(small_set(), DEV)


def test_data_batch_is_capturable():
    from mapdit_amd.data import DeviceLatentDataset
    ds = DeviceLatentDataset(small_set(), DEV, seed=3)
    want = ds.batch(2, 16)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = ds.batch(2, 16)
    got[0].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(got[1], want[1])


TRAIN = ["--model", "DiT-XS/2", "--num-steps", "4", "--batch-size", "32", "--log-every", "2", "--ckpt-every", "1000", "--ema-snapshot-every", "1000",
         "--num-classes", "10", "--num-lin-warmup", "2", "--start-decay", "3"]


@pytest.fixture(scope="module")
def latent_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("latents")
    g = torch.Generator().manual_seed(0)
    torch.save(torch.randn(512, 4, 32, 32, generator=g), root / "posterior_means.pt")
    torch.save(torch.rand(512, 4, 32, 32, generator=g) * 0.3, root / "posterior_stds.pt")
    torch.save(torch.randint(0, 10, (512,), generator=g), root / "labels.pt")
    torch.save({"mean": torch.randn(4, generator=g) * 0.1, "std": torch.rand(4, generator=g) + 0.5}, root / "stats.pt")
    return str(root)


def run_train(monkeypatch, latent_dir, results, extra):
    """train.main with training_losses recording the batches it is handed."""
    import yaml
    from mapdit_amd import train
    from mapdit_amd.diffusion.respace import SpacedDiffusion
    seen, real = [], SpacedDiffusion.training_losses

    def spy(self, model, x, t, model_kwargs=None, **kw):
        seen.append((x.clone(), model_kwargs["y"].clone()))
        return real(self, model, x, t, model_kwargs, **kw)
    monkeypatch.setattr(SpacedDiffusion, "training_losses", spy)
    exp = train.main(TRAIN + ["--data-path", latent_dir, "--results-dir", str(results)] + extra)
    lines = [ln for ln in open(os.path.join(exp, "log.txt")).read().splitlines() if ln.startswith("(step=")]
    assert len(lines) == 2 and len(seen) == 4 and all(np.isfinite(float(ln.split("train loss: ")[1].split(",")[0])) for ln in lines)
    return yaml.safe_load(open(os.path.join(exp, "config.yaml"))), seen


def test_train_harness_on_the_device_loader(tmp_path, monkeypatch, latent_dir):
    from mapdit_amd.data import DeviceLatentDataset
    cfg, seen = run_train(monkeypatch, latent_dir, tmp_path, ["--data-loader", "device", "--seed", "5"])
    assert cfg["data_loader"] == "device" and cfg["in_channels"] == 4 and cfg["input_size"] == 32
    ds = DeviceLatentDataset(latent_dir, DEV, seed=5)
    for step in (0, 3):
        x, y = ds.batch(step, 32)
        assert torch.equal(bits(seen[step][0]), bits(x)) and torch.equal(seen[step][1], y)


def test_train_harness_on_the_host_loader_still_runs(tmp_path, monkeypatch, latent_dir):
    """The default path (it had no test): in-process loading, so that the test starts no worker processes."""
    cfg, seen = run_train(monkeypatch, latent_dir, tmp_path, ["--num-workers", "0"])
    assert cfg["data_loader"] == "host"
    assert seen[0][0].shape == (32, 4, 32, 32) and seen[0][0].is_cuda and seen[0][1].dtype == torch.int64
