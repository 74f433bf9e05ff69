"""The schedule sampler kernels (csrc/timestep_sampler.hip) and their facade (mapdit_amd.diffusion.timestep_sampler) on the MI355X, against
the fp64 restatement (tests/schedule_sampler_reference.py) and what the reference recorded (tests/golden/schedule_sampler.npz)."""
import os
import re
import socket
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import schedule_sampler_reference as R
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "schedule_sampler_worker.py")
TAGS = ["t37h3", "t1000h10"]


@pytest.fixture(scope="module")
def golden():
    return load_golden("schedule_sampler")


@pytest.fixture(scope="module")
def L():
    import mapdit_amd
    return mapdit_amd._lib


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype=dtype))).to(DEV)


def k_update(L, hist, counts, ts, losses):
    T, H = hist.shape
    L.lib().tsampler_update(L.ptr(hist), L.ptr(counts), T, H, L.ptr(ts), L.ptr(losses), ts.numel(), L.cur_stream())


def k_prepare(L, hist, counts, up):
    T, H = hist.shape
    prob, cdf = (torch.full((T,), float("nan"), dtype=torch.float64, device=DEV) for _ in range(2))
    L.lib().tsampler_prepare(L.ptr(hist), L.ptr(counts), T, H, float(up), L.ptr(prob), L.ptr(cdf), L.cur_stream())
    return prob, cdf


def k_draw(L, prob, cdf, u):
    t = torch.full((u.numel(),), -7, dtype=torch.int64, device=DEV)
    w = torch.full((u.numel(),), float("nan"), dtype=torch.float32, device=DEV)
    L.lib().tsampler_draw(L.ptr(prob), L.ptr(cdf), prob.numel(), L.ptr(u), L.ptr(t), L.ptr(w), u.numel(), L.cur_stream())
    return t, w


def rel_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def bits(t):
    return t.cpu().contiguous().view(torch.int64) if t.dtype == torch.float64 else t.cpu()


def golden_points(g, tag):
    return [(g[f"{tag}_p{k}_hist"].astype(np.float64), g[f"{tag}_p{k}_counts"]) for k in range(3)]


# ---- update ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 7, 64, 65, 1000, 1025])
def test_update_is_bit_equal_to_the_restatement(L, T):
    """hist / counts after two launches (the second shifts rows the first filled) for every H and M of the grid; in each batch with M > H one
    timestep occurs more than H times, so its row fills AND shifts inside one launch."""
    rng = np.random.default_rng(T)
    for H in (1, 3, 10):
        for M in (1, 63, 257, 2048):
            hist, counts = R.new_state(T, H)
            d_hist, d_counts = dev(hist), dev(counts, np.int32)
            for launch in range(2):
                ts = rng.integers(0, T, size=M).astype(np.int64)
                if M > H:
                    hot = int(rng.integers(0, T))
                    ts[rng.choice(M, size=min(M, H + 3), replace=False)] = hot
                    assert (ts == hot).sum() > H
                losses = rng.lognormal(0.0, 2.0, size=M).astype(np.float32)
                assert R.update(hist, counts, ts, losses) == 0
                k_update(L, d_hist, d_counts, dev(ts), dev(losses))
            assert np.array_equal(d_hist.cpu().numpy(), hist), (T, H, M)
            assert np.array_equal(d_counts.cpu().numpy(), counts), (T, H, M)
    L.lib().device_error_poll(L.cur_stream())                                       # nothing was out of range


def test_update_skips_bad_entries_and_reports_the_timestep(L):
    T, H = 65, 3
    rng = np.random.default_rng(3)
    hist, counts = R.new_state(T, H)
    ts0, l0 = rng.integers(0, T, size=300).astype(np.int64), rng.lognormal(size=300).astype(np.float32)
    R.update(hist, counts, ts0, l0)
    d_hist, d_counts = dev(hist), dev(counts, np.int32)
    L.lib().device_error_poll(L.cur_stream())
    ts = np.asarray([-1, T, 5, 6, 7, 2 ** 40, -2 ** 40], dtype=np.int64)
    losses = np.asarray([1.0, 1.0, np.inf, np.nan, -np.inf, 1.0, 1.0], dtype=np.float32)
    k_update(L, d_hist, d_counts, dev(ts), dev(losses))
    assert np.array_equal(d_hist.cpu().numpy(), hist) and np.array_equal(d_counts.cpu().numpy(), counts)      # the state is unchanged
    with pytest.raises(L.MapditError, match="timestep"):
        L.lib().device_error_poll(L.cur_stream())
    L.lib().device_error_poll(L.cur_stream())                                       # reported once, then clear
    # non-finite losses alone are no error, and good entries of the same batch still land
    ts = np.asarray([5, 5, 6], dtype=np.int64)
    losses = np.asarray([np.nan, 2.5, np.inf], dtype=np.float32)
    R.update(hist, counts, ts, losses)
    k_update(L, d_hist, d_counts, dev(ts), dev(losses))
    assert np.array_equal(d_hist.cpu().numpy(), hist) and np.array_equal(d_counts.cpu().numpy(), counts)
    L.lib().device_error_poll(L.cur_stream())


def test_unsupported_sizes_are_refused_by_name(L):
    lib = L.lib()
    x = torch.zeros(64, dtype=torch.float64, device=DEV)
    i32, i64, f32 = (torch.zeros(64, dtype=d, device=DEV) for d in (torch.int32, torch.int64, torch.float32))
    s = L.cur_stream()
    for T in (0, 16385):
        with pytest.raises(L.MapditError, match=r"T="):
            lib.tsampler_update(L.ptr(x), L.ptr(i32), T, 1, L.ptr(i64), L.ptr(f32), 1, s)
        with pytest.raises(L.MapditError, match=r"T="):
            lib.tsampler_prepare(L.ptr(x), L.ptr(i32), T, 1, 0.001, L.ptr(x), L.ptr(x), s)
        with pytest.raises(L.MapditError, match=r"T="):
            lib.tsampler_prepare_weights(L.ptr(x), T, L.ptr(x[32:]), L.ptr(x[48:]), s)
        with pytest.raises(L.MapditError, match=r"T="):
            lib.tsampler_draw(L.ptr(x), L.ptr(x), T, L.ptr(x), L.ptr(i64), L.ptr(f32), 1, s)
    for H in (0, 65):
        with pytest.raises(L.MapditError, match=r"H="):
            lib.tsampler_update(L.ptr(x), L.ptr(i32), 1, H, L.ptr(i64), L.ptr(f32), 1, s)
        with pytest.raises(L.MapditError, match=r"H="):
            lib.tsampler_prepare(L.ptr(x), L.ptr(i32), 1, H, 0.001, L.ptr(x), L.ptr(x), s)
    with pytest.raises(L.MapditError, match=r"M="):
        lib.tsampler_update(L.ptr(x), L.ptr(i32), 1, 1, L.ptr(i64), L.ptr(f32), 0, s)
    with pytest.raises(L.MapditError, match=r"N="):
        lib.tsampler_draw(L.ptr(x), L.ptr(x), 1, L.ptr(x), L.ptr(i64), L.ptr(f32), 0, s)
    with pytest.raises(L.MapditError, match=r"uniform_prob"):
        lib.tsampler_prepare(L.ptr(x), L.ptr(i32), 1, 1, 1.5, L.ptr(x), L.ptr(x), s)


# ---- prepare --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_prepare_matches_the_restatement_and_repeats_its_bits(L, golden, tag):
    up = float(golden[f"{tag}_uniform_prob"])
    for k, (hist, counts) in enumerate(golden_points(golden, tag)):
        T = hist.shape[0]
        want_p, want_c = R.prepare(hist, counts, up)
        d_hist, d_counts = dev(hist), dev(counts, np.int32)
        prob, cdf = k_prepare(L, d_hist, d_counts, up)
        prob2, cdf2 = k_prepare(L, d_hist, d_counts, up)
        assert torch.equal(bits(prob), bits(prob2)) and torch.equal(bits(cdf), bits(cdf2))
        p, c = prob.cpu().numpy(), cdf.cpu().numpy()
        e_p, e_c = rel_max(p, want_p), rel_max(c, want_c)
        print(f"{tag} point {k}: prob rel {e_p:.2e}, cdf rel {e_c:.2e} (bound {R.TABLE_TOL(T):.2e})")
        assert e_p <= R.TABLE_TOL(T) and e_c <= R.TABLE_TOL(T)
        assert c[-1] == 1.0 and np.all(np.diff(c) > 0)
        if k == 0:
            assert np.array_equal(p, np.full(T, 1.0 / T))                           # not warmed up: exactly uniform


@pytest.mark.parametrize("T,H", [(1, 1), (65, 3), (1025, 2), (16384, 64)])
def test_prepare_at_other_sizes(L, T, H):
    """One entry, a wave edge, more than one entry per lane of the 1,024-lane workgroup, and the largest supported table."""
    rng = np.random.default_rng(T + H)
    hist = rng.lognormal(0.0, 2.0, size=(T, H)).astype(np.float32).astype(np.float64)
    counts = np.full(T, H, dtype=np.int64)
    want_p, want_c = R.prepare(hist, counts, 0.01)
    prob, cdf = k_prepare(L, dev(hist), dev(counts, np.int32), 0.01)
    assert rel_max(prob.cpu().numpy(), want_p) <= R.TABLE_TOL(T) and rel_max(cdf.cpu().numpy(), want_c) <= R.TABLE_TOL(T)
    assert float(cdf[-1]) == 1.0 and bool((cdf[1:] >= cdf[:-1]).all())
    counts[T // 2] = H - 1                                                          # one row short of full: uniform
    prob, cdf = k_prepare(L, dev(hist), dev(counts, np.int32), 0.01)
    assert np.array_equal(prob.cpu().numpy(), np.full(T, 1.0 / T)) and float(cdf[-1]) == 1.0


def test_prepare_falls_back_to_uniform_on_a_degenerate_sum(L):
    T, H = 37, 3
    counts = dev(np.full(T, H), np.int32)
    hist = np.zeros((T, H))
    for poison in (None, np.inf, np.nan):
        if poison is not None:
            hist[11, 1] = poison                                                    # (only a loaded state can hold it)
        prob, cdf = k_prepare(L, dev(hist), counts, 0.001)
        assert np.array_equal(prob.cpu().numpy(), np.full(T, 1.0 / T))
        assert rel_max(cdf.cpu().numpy(), R.prepare(hist, np.full(T, H), 0.001)[1]) <= R.TABLE_TOL(T)


def test_prepare_weights(L):
    rng = np.random.default_rng(5)
    for T in (1, 37, 1000, 1025):
        w = rng.lognormal(size=T)
        want_p, want_c, bad = R.prepare_weights(w)
        assert not bad
        prob, cdf = (torch.empty(T, dtype=torch.float64, device=DEV) for _ in range(2))
        L.lib().tsampler_prepare_weights(L.ptr(dev(w)), T, L.ptr(prob), L.ptr(cdf), L.cur_stream())
        assert rel_max(prob.cpu().numpy(), want_p) <= R.TABLE_TOL(T) and rel_max(cdf.cpu().numpy(), want_c) <= R.TABLE_TOL(T)
    L.lib().device_error_poll(L.cur_stream())
    for badv in (0.0, -1.0, np.nan, np.inf):
        w = rng.lognormal(size=37)
        w[20] = badv
        prob, cdf = (torch.empty(37, dtype=torch.float64, device=DEV) for _ in range(2))
        L.lib().tsampler_prepare_weights(L.ptr(dev(w)), 37, L.ptr(prob), L.ptr(cdf), L.cur_stream())
        assert np.array_equal(prob.cpu().numpy(), np.full(37, 1.0 / 37))            # no NaN reaches a draw
        with pytest.raises(L.MapditError, match="weights"):
            L.lib().device_error_poll(L.cur_stream())
        L.lib().device_error_poll(L.cur_stream())


# ---- draw -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_draw_reproduces_the_reference_draws(L, golden, tag):
    g = golden
    up = float(g[f"{tag}_uniform_prob"])
    for k, (hist, counts) in enumerate(golden_points(g, tag)):
        T = hist.shape[0]
        prob, cdf = k_prepare(L, dev(hist), dev(counts, np.int32), up)
        t, w = k_draw(L, prob, cdf, dev(g[f"{tag}_p{k}_u"]))
        assert np.array_equal(t.cpu().numpy(), g[f"{tag}_p{k}_idx"]), k
        e = rel_max(w.cpu().numpy(), g[f"{tag}_p{k}_w"])
        print(f"{tag} point {k}: sample weights rel {e:.2e} (bound {R.W_TOL:.2e})")
        assert e <= R.W_TOL
        edge = dev(np.asarray([0.0, np.nextafter(1.0, 0.0)]))
        t, w = k_draw(L, prob, cdf, edge)
        assert t.tolist() == [0, T - 1]
        p = prob.cpu().numpy()
        assert rel_max(w.cpu().numpy(), 1.0 / (T * p[[0, T - 1]])) <= R.W_TOL


def test_draw_over_several_workgroups_matches_searchsorted(L):
    rng = np.random.default_rng(11)
    T, N = 1025, 3001
    prob_np, cdf_np, _ = R.prepare_weights(rng.lognormal(size=T))
    u = rng.random(N)
    u[:T] = cdf_np                                                                  # exactly on every edge: side="right"
    u[T - 1] = 0.5
    want_t, want_w = R.draw(prob_np, cdf_np, u)
    t, w = k_draw(L, dev(prob_np), dev(cdf_np), dev(u))
    assert np.array_equal(t.cpu().numpy(), want_t) and rel_max(w.cpu().numpy(), want_w) <= R.W_TOL


# ---- the facade -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_facade_reproduces_the_recorded_sequence(golden, tag):
    from mapdit_amd.diffusion.timestep_sampler import LossSecondMomentResampler
    g = golden
    T, H = g[f"{tag}_p0_hist"].shape
    d = types.SimpleNamespace(num_timesteps=T)
    s = LossSecondMomentResampler(d, history_per_term=H, uniform_prob=float(g[f"{tag}_uniform_prob"]))
    points = g[f"{tag}_points"].tolist()
    for i in range(points[-1]):
        ts, losses = g[f"{tag}_batch{i}_ts"].astype(np.int64), g[f"{tag}_batch{i}_losses"]
        if i % 2:
            s.update_with_all_losses(ts.tolist(), losses.tolist())                  # lists are uploaded
        else:
            s.update_with_local_losses(dev(ts), dev(losses))                        # no process group: the same update
        if i + 1 not in points:
            continue
        k = points.index(i + 1)
        t, w = s.sample_from_uniforms(dev(g[f"{tag}_p{k}_u"]))
        assert t.dtype == torch.int64 and w.dtype == torch.float32 and t.is_cuda and w.is_cuda
        assert np.array_equal(t.cpu().numpy(), g[f"{tag}_p{k}_idx"]) and rel_max(w.cpu().numpy(), g[f"{tag}_p{k}_w"]) <= R.W_TOL
        sd = s.state_dict()
        assert sd["loss_history"].dtype == torch.float64 and sd["loss_counts"].dtype == torch.int64
        assert np.array_equal(sd["loss_history"].numpy(), g[f"{tag}_p{k}_hist"].astype(np.float64))
        assert np.array_equal(sd["loss_counts"].numpy(), g[f"{tag}_p{k}_counts"])
        assert rel_max(s.weights(), g[f"{tag}_p{k}_weights"]) <= R.TABLE_TOL(T)
        fresh = LossSecondMomentResampler(d, history_per_term=H, uniform_prob=float(g[f"{tag}_uniform_prob"]))
        fresh.load_state_dict(sd)
        t2, w2 = fresh.sample_from_uniforms(dev(g[f"{tag}_p{k}_u"]))
        assert torch.equal(t2, t) and torch.equal(w2, w)
    with pytest.raises(ValueError):
        LossSecondMomentResampler(d, history_per_term=H + 1).load_state_dict(sd)


def test_uniform_and_subclass_samplers_draw_through_the_weights_path():
    from mapdit_amd.diffusion import create_diffusion
    from mapdit_amd.diffusion.timestep_sampler import ScheduleSampler, create_named_schedule_sampler
    u = create_named_schedule_sampler("uniform", create_diffusion(""))
    gen = torch.Generator(device=DEV).manual_seed(5)
    t, w = u.sample(513, DEV, generator=gen)
    gen.manual_seed(5)
    want = torch.rand(513, dtype=torch.float64, device=DEV, generator=gen)
    assert np.array_equal(t.cpu().numpy(), R.draw(*R.prepare_weights(np.ones(1000))[:2], want.cpu().numpy())[0])      # the caller's RNG
    assert torch.equal(w, torch.ones_like(w)) and int(t.min()) >= 0 and int(t.max()) < 1000

    class Ramp(ScheduleSampler):
        def weights(self):
            return np.arange(1, 38, dtype=np.float64)

    uu = np.random.default_rng(2).random(100)
    t, w = Ramp().sample_from_uniforms(dev(uu))
    want_t, want_w = R.draw(*R.prepare_weights(np.arange(1, 38, dtype=np.float64))[:2], uu)
    assert np.array_equal(t.cpu().numpy(), want_t) and rel_max(w.cpu().numpy(), want_w) <= R.W_TOL


def test_nothing_is_read_back_in_the_step():
    from mapdit_amd.diffusion.timestep_sampler import LossSecondMomentResampler
    s = LossSecondMomentResampler(types.SimpleNamespace(num_timesteps=1000))
    device = torch.device(DEV, torch.cuda.current_device())
    losses = torch.rand(256, device=device)
    s.sample(1, device)                                                             # (loads the library outside the checked region)
    s = LossSecondMomentResampler(types.SimpleNamespace(num_timesteps=1000))
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        t, w = s.sample(256, device)
        s.update_with_local_losses(t, losses)
        t2, w2 = s.sample(256, device)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert int(s.state_dict()["loss_counts"].sum()) == 256 and bool(torch.isfinite(w2).all()) and int(t2.max()) < 1000


# ---- the weights reach the gradients -------------------------------------------------------------------------------------------------------
def test_weighted_loss_gives_the_weighted_sum_of_per_sample_gradients():
    """(losses["loss"] * w).mean().backward() on the fixture tiny_a against sum_i w_i / N * (gradient of sample i's loss), the per-sample
    gradients taken one by one with one-hot g_loss vectors and summed in fp64: nothing between the sampler and the loss kernels drops the
    weights.  bf16x3 (the fp32-accurate engine) at 2e-4, the tolerance tests/test_train_gpu.py holds that precision to."""
    from grad_accum_worker import fixture_model, reset_grads
    from mapdit_amd.diffusion import create_diffusion
    m, _, (x, t, y, noise) = fixture_model("tiny_a", "bf16x3")
    diff = create_diffusion("")
    n = x.shape[0]
    w = dev(np.asarray([0.05, 1.0, 6.5, 0.4][:n] + [1.0] * max(0, n - 4), dtype=np.float32))

    def losses():
        return diff.training_losses(m, x, t, dict(y=y), noise=noise)["loss"]

    reset_grads(m)
    (losses() * w).mean().backward()
    torch.cuda.synchronize()
    got = m._gflat.double().cpu().numpy()
    want = np.zeros_like(got)
    for i in range(n):
        reset_grads(m)
        e = torch.zeros(n, device=DEV)
        e[i] = 1.0
        losses().backward(gradient=e)
        torch.cuda.synchronize()
        want += float(w[i]) / n * m._gflat.double().cpu().numpy()
    reset_grads(m)
    losses().mean().backward()
    torch.cuda.synchronize()
    plain = m._gflat.double().cpu().numpy()
    worst = 0.0
    for (k, p), o in zip(m.named_parameters(), m._poffs):
        sl = slice(o, o + p.numel())
        e = rel_err(got[sl], want[sl])
        worst = max(worst, e)
        assert e < 2e-4, (k, e)
    print(f"weighted loss: worst per-parameter rel err {worst:.2e}; the unweighted gradient is {rel_err(plain, want):.2f} away")
    assert rel_err(plain, want) > 0.1                                               # the weights matter at this tolerance


# ---- two ranks on one GPU over gloo --------------------------------------------------------------------------------------------------------
def test_two_ranks_hold_one_history(tmp_path):
    """Two ranks (gloo, one GPU) feed different entries for three rounds (T = 37, H = 3: warmed up after two): histories and the next
    probability table bit-equal across the ranks, the history equal to the restatement fed rank 0's entries, then rank 1's, per round."""
    import schedule_sampler_worker as W
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), WORKER, str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, MAPDIT_DIST_BACKEND="gloo"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    a, b = (torch.load(tmp_path / f"rank{i}.pt", weights_only=False) for i in range(2))
    assert a["world"] == 2
    assert torch.equal(bits(a["hist"]), bits(b["hist"])) and torch.equal(a["counts"], b["counts"])
    assert torch.equal(bits(a["prob"]), bits(b["prob"])) and torch.equal(bits(a["cdf"]), bits(b["cdf"]))
    hist, counts = R.new_state(W.T, W.H)
    for rnd in range(W.ROUNDS):
        for rank in range(2):
            R.update(hist, counts, *W.rank_batch(rank, rnd))
    assert R.warmed_up(hist, counts)
    assert np.array_equal(a["hist"].numpy(), hist) and np.array_equal(a["counts"].numpy(), counts)
    assert rel_max(a["prob"].numpy(), R.prepare(hist, counts, 0.001)[0]) <= R.TABLE_TOL(W.T)
    assert not torch.equal(a["t"], b["t"])                                          # each rank drew from its own generator


# ---- the harness ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,extra", [("plain", []), ("lsm", ["--schedule-sampler", "loss-second-moment"]),
                                       ("lsm_accum", ["--schedule-sampler", "loss-second-moment", "--grad-accum-steps", "2"])])
def test_train_harness_with_and_without_the_flag(tmp_path, tag, extra):
    from mapdit_amd import train
    args = ["--synthetic", "--model", "DiT-XS/2", "--num-steps", "3", "--batch-size", "4", "--log-every", "1", "--ckpt-every", "3",
            "--ema-snapshot-every", "1000", "--num-classes", "10", "--num-lin-warmup", "1", "--start-decay", "2", "--precision", "bf16"]
    exp = train.main(args + extra + ["--results-dir", str(tmp_path / tag)])
    lines = [ln for ln in open(os.path.join(exp, "log.txt")).read().splitlines() if ln.startswith("(step=")]
    assert len(lines) == 3, lines
    for ln in lines:                                                                # today's format to the byte
        assert re.fullmatch(r"\(step=\d{7}\) train loss: \d+\.\d{4}, train steps/sec: \d+\.\d{2}", ln), (tag, ln)
    ck = torch.load(os.path.join(exp, "checkpoints", "0000003.pt"), weights_only=True)
    if tag == "plain":
        assert set(ck) == {"model", "opt"}
        return
    assert set(ck) == {"model", "opt", "schedule_sampler"}
    sd = ck["schedule_sampler"]
    assert tuple(sd["loss_history"].shape) == (1000, 10) and sd["loss_history"].dtype == torch.float64
    assert int(sd["loss_counts"].sum()) == 12 and (sd["history_per_term"], sd["uniform_prob"]) == (10, 0.001)
    assert int((sd["loss_history"] != 0).sum()) == 12 and bool(torch.isfinite(sd["loss_history"]).all())
