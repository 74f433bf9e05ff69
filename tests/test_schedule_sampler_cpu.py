"""Schedule samplers without a GPU: the fp64 restatement (tests/schedule_sampler_reference.py) against what the reference recorded
(tests/golden/schedule_sampler.npz, written by tests/golden/make_golden_schedule_sampler.py), the restatement's deviations, and the public
surface of mapdit_amd.diffusion.timestep_sampler that needs no device."""
import numpy as np
import pytest

import schedule_sampler_reference as R
from conftest import load_golden

TAGS = ["t37h3", "t1000h10"]


@pytest.fixture(scope="module")
def golden():
    return load_golden("schedule_sampler")


def replay(g, tag):
    """The recorded batches through the restatement: [(hist, counts)] at the three recorded points."""
    T, H = g[f"{tag}_p0_hist"].shape
    hist, counts = R.new_state(T, H)
    out, points = [], g[f"{tag}_points"].tolist()
    for i in range(points[-1]):
        assert R.update(hist, counts, g[f"{tag}_batch{i}_ts"].astype(np.int64), g[f"{tag}_batch{i}_losses"]) == 0
        if i + 1 in points:
            out.append((hist.copy(), counts.copy()))
    return out


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.abs(np.asarray(b, np.float64))))


# ---- the restatement against the reference's recorded results --------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_fixture_covers_what_it_should(golden, tag):
    g = golden
    T, H = g[f"{tag}_p0_hist"].shape
    assert (T, H) == {"t37h3": (37, 3), "t1000h10": (1000, 10)}[tag]
    n = g[f"{tag}_points"][-1]
    repeats = [np.bincount(g[f"{tag}_batch{i}_ts"].astype(np.int64), minlength=T).max() for i in range(n)]
    assert sum(r > 1 for r in repeats) >= 3                                    # several batches repeat a timestep within the batch
    if tag == "t37h3":
        assert max(repeats) > H                                                # a row fills and shifts inside one batch
    assert not (g[f"{tag}_p0_counts"] == H).all() and (g[f"{tag}_p1_counts"] == H).all() and (g[f"{tag}_p2_counts"] == H).all()
    assert np.array_equal(g[f"{tag}_p0_weights"], np.ones(T))
    for k in range(3):                                                         # every uniform clear of every cdf edge: no draw excluded
        assert np.abs(g[f"{tag}_p{k}_u"][:, None] - g[f"{tag}_p{k}_cdf"][None, :]).min() > 1e-9


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_histories_and_counts_exactly(golden, tag):
    for k, (hist, counts) in enumerate(replay(golden, tag)):
        assert np.array_equal(hist, golden[f"{tag}_p{k}_hist"].astype(np.float64)), k
        assert np.array_equal(counts, golden[f"{tag}_p{k}_counts"]), k


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_weights_cdf_and_draws(golden, tag):
    g = golden
    up = float(g[f"{tag}_uniform_prob"])
    for k, (hist, counts) in enumerate(replay(g, tag)):
        T = hist.shape[0]
        w = R.weights(hist, counts, up)
        prob, cdf = R.prepare(hist, counts, up)
        e_w, e_c = rel(w, g[f"{tag}_p{k}_weights"]), rel(cdf, g[f"{tag}_p{k}_cdf"])
        print(f"{tag} point {k}: weights rel {e_w:.2e}, cdf rel {e_c:.2e} (bound {R.TABLE_TOL(T):.2e})")
        assert e_w <= R.TABLE_TOL(T) and e_c <= R.TABLE_TOL(T)
        t, sw = R.draw(prob, cdf, g[f"{tag}_p{k}_u"])
        assert np.array_equal(t, g[f"{tag}_p{k}_idx"])
        assert rel(sw, g[f"{tag}_p{k}_w"]) <= R.W_TOL


# ---- the restatement's deviations ---------------------------------------------------------------------------------------------------------
def test_nonfinite_loss_and_out_of_range_timestep_leave_the_state_untouched():
    hist, counts = R.new_state(5, 2)
    R.update(hist, counts, [0, 1, 1, 1, 4], [1.0, 2.0, 3.0, 4.0, 5.0])
    h0, c0 = hist.copy(), counts.copy()
    assert np.array_equal(h0[1], [3.0, 4.0]) and c0.tolist() == [1, 2, 0, 0, 1]
    bad = R.update(hist, counts, [-1, 5, 2, 3, 0, 10 ** 12], [1.0, 1.0, np.inf, np.nan, -np.inf, 1.0])
    assert bad == 3 and np.array_equal(hist, h0) and np.array_equal(counts, c0)


def test_all_zero_warmed_up_history_gives_the_uniform_table():
    hist, counts = R.new_state(7, 2)
    counts[:] = 2
    prob, cdf = R.prepare(hist, counts, 0.001)
    assert np.array_equal(prob, np.full(7, 1.0 / 7)) and cdf[-1] == 1.0 and np.all(np.diff(cdf) > 0)
    hist[3] = np.inf                                                           # (a loaded state may hold it: the update never stores one)
    assert np.array_equal(R.prepare(hist, counts, 0.001)[0], np.full(7, 1.0 / 7))


def test_prepare_weights_flags_bad_weights():
    p, cdf, bad = R.prepare_weights([1.0, 3.0, 4.0])
    assert not bad and np.allclose(p, [0.125, 0.375, 0.5]) and np.allclose(cdf, [0.125, 0.5, 1.0])
    for w in ([1.0, 0.0], [1.0, -1.0], [1.0, np.nan], [1.0, np.inf]):
        p, cdf, bad = R.prepare_weights(w)
        assert bad and np.array_equal(p, [0.5, 0.5])


def test_draw_edges():
    prob, cdf = R.table(np.asarray([0.25, 0.25, 0.5]))
    t, w = R.draw(prob, cdf, [0.0, 0.25, np.nextafter(0.25, 0), np.nextafter(1.0, 0.0), 1.0])
    assert t.tolist() == [0, 1, 0, 2, 2] and w.dtype == np.float32 and np.allclose(w, [4 / 3, 4 / 3, 4 / 3, 2 / 3, 2 / 3])


# ---- public surface ------------------------------------------------------------------------------------------------------------------------
def test_names_and_factory():
    from mapdit_amd.diffusion import create_diffusion
    from mapdit_amd.diffusion.timestep_sampler import (LossAwareSampler, LossSecondMomentResampler, ScheduleSampler, UniformSampler,
                                                       create_named_schedule_sampler)
    d = create_diffusion("")
    u = create_named_schedule_sampler("uniform", d)
    s = create_named_schedule_sampler("loss-second-moment", d)
    assert isinstance(u, UniformSampler) and isinstance(s, LossSecondMomentResampler) and isinstance(s, LossAwareSampler)
    assert isinstance(u, ScheduleSampler) and (s.history_per_term, s.uniform_prob) == (10, 0.001)
    assert np.array_equal(u.weights(), np.ones(1000)) and np.array_equal(s.weights(), np.ones(1000))
    with pytest.raises(NotImplementedError, match="unknown schedule sampler: lossy"):
        create_named_schedule_sampler("lossy", d)
    with pytest.raises(ValueError):
        LossSecondMomentResampler(d, history_per_term=65)


@pytest.mark.parametrize("name", ["uniform", "loss-second-moment"])
def test_cpu_device_raises(name):
    import torch
    from mapdit_amd.diffusion import create_diffusion
    from mapdit_amd.diffusion.timestep_sampler import create_named_schedule_sampler
    s = create_named_schedule_sampler(name, create_diffusion(""))
    with pytest.raises(NotImplementedError, match="no CPU path"):
        s.sample(4, "cpu")
    with pytest.raises(NotImplementedError, match="no CPU path"):
        s.sample_from_uniforms(torch.rand(4, dtype=torch.float64))


def test_train_parser_knows_the_flag():
    from mapdit_amd import train
    p = train.build_parser()
    assert p.parse_args(["--results-dir", "x"]).schedule_sampler == "uniform"
    assert p.parse_args(["--results-dir", "x", "--schedule-sampler", "loss-second-moment"]).schedule_sampler == "loss-second-moment"
    with pytest.raises(SystemExit):
        p.parse_args(["--results-dir", "x", "--schedule-sampler", "other"])


def test_state_dict_round_trips_on_the_host(golden):
    import types

    import torch
    from mapdit_amd.diffusion.timestep_sampler import LossSecondMomentResampler
    d = types.SimpleNamespace(num_timesteps=37)
    a = LossSecondMomentResampler(d, history_per_term=3)
    sd = a.state_dict()
    assert sd["loss_history"].dtype == torch.float64 and tuple(sd["loss_history"].shape) == (37, 3) and not sd["loss_history"].any()
    assert sd["loss_counts"].dtype == torch.int64 and tuple(sd["loss_counts"].shape) == (37,)
    assert (sd["history_per_term"], sd["uniform_prob"]) == (3, 0.001)
    hist, counts = golden["t37h3_p2_hist"].astype(np.float64), golden["t37h3_p2_counts"]
    a.load_state_dict({"loss_history": hist, "loss_counts": counts, "history_per_term": 3, "uniform_prob": 0.01})
    sd = a.state_dict()
    assert np.array_equal(sd["loss_history"].numpy(), hist) and np.array_equal(sd["loss_counts"].numpy(), counts) and sd["uniform_prob"] == 0.01
    b = LossSecondMomentResampler(d, history_per_term=3)
    b.load_state_dict(sd)                                                      # its own containers (torch tensors) load too
    assert np.array_equal(b.state_dict()["loss_history"].numpy(), hist) and b._warmed_up()
    with pytest.raises(ValueError):
        LossSecondMomentResampler(d, history_per_term=4).load_state_dict(sd)
    with pytest.raises(ValueError):
        LossSecondMomentResampler(types.SimpleNamespace(num_timesteps=36), history_per_term=3).load_state_dict(sd)
    with pytest.raises(ValueError):
        b.load_state_dict({"loss_history": hist, "loss_counts": counts + 1})
