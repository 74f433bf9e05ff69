"""Counter-based sampler draws, the part that needs no GPU: the tags and the ABI, sample_fid's batch plan and manifest, and every refusal
that must come before a model is built."""
import itertools
import re

import pytest

import data_reference as R
import sample_rng_reference as S
import step_rng_reference as STEP

NEW_TAGS = {"MAPDIT_TAG_SMPZ": S.TAG_SMPZ, "MAPDIT_TAG_SMPN": S.TAG_SMPN, "MAPDIT_TAG_SMPY": S.TAG_SMPY}
OLD_TAGS = {"TAG_PERM": R.TAG_PERM, "TAG_NOISE": R.TAG_NOISE, "MAPDIT_TAG_EPS": STEP.TAG_EPS, "MAPDIT_TAG_SYNX": STEP.TAG_SYNX,
            "MAPDIT_TAG_STEP": STEP.TAG_STEP}
FUNCTIONS = ("mapdit_sample_draw", "mapdit_sample_noise", "mapdit_psample_step_counter", "mapdit_obj_step_counter")


def test_tags_are_distinct_and_the_headers():
    from mapdit_amd import _lib
    every = {**NEW_TAGS, **OLD_TAGS}
    assert len(every) == 8 and len(set(every.values())) == 8, every
    assert NEW_TAGS == {"MAPDIT_TAG_SMPZ": 0x534D505A, "MAPDIT_TAG_SMPN": 0x534D504E, "MAPDIT_TAG_SMPY": 0x534D5059}
    for name, value in NEW_TAGS.items():
        assert _lib.ABI.constants[name] == value, name
    for name in ("MAPDIT_TAG_EPS", "MAPDIT_TAG_SYNX", "MAPDIT_TAG_STEP"):              # the five the header had: its defines and its prose
        assert _lib.ABI.constants[name] == OLD_TAGS[name], name
    text = open(_lib.HEADER).read()
    assert int(re.search(r"TAG_PERM = (0x[0-9A-Fa-f]+)", text).group(1), 16) == R.TAG_PERM
    assert int(re.search(r"TAG_NOISE = (0x[0-9A-Fa-f]+)", text).group(1), 16) == R.TAG_NOISE


def test_the_four_entry_points_are_declared_and_bound():
    from mapdit_amd import _lib
    for name in FUNCTIONS:
        ret, params = _lib.ABI.functions[name]
        assert ret == "int" and params[-1] == ("void*", "stream"), name
        assert ("uint64_t", "seed") in params and ("int64_t*", "index") in params, name
    step, ctr = _lib.ABI.functions["mapdit_obj_step"][1], _lib.ABI.functions["mapdit_obj_step_counter"][1]
    i = step.index(("float*", "noise"))
    assert ctr == step[:i] + [("uint64_t", "seed"), ("int64_t*", "index")] + step[i + 1:]      # (seed, index) in place of `noise`
    step, ctr = _lib.ABI.functions["mapdit_psample_step"][1], _lib.ABI.functions["mapdit_psample_step_counter"][1]
    i = step.index(("float*", "noise"))
    assert ctr == step[:i] + [("uint64_t", "seed"), ("int64_t*", "index")] + step[i + 1:]
    lib = _lib.lib()
    for name in FUNCTIONS:
        assert callable(getattr(lib, name[len("mapdit_"):])), name
    assert lib.abi_version() == 5


def plan(*a, **k):
    from mapdit_amd.sample_fid import plan_batches
    return plan_batches(*a, **k)


def test_plan_batches_covers_every_index_once():
    assert plan(10, 4) == plan(10, 4, (0, 1)) == [(0, 0, 4), (1, 4, 8), (2, 8, 10)]          # the last batch is cut at 10
    assert plan(10, 4, (0, 2)) == [(0, 0, 4), (2, 8, 10)] and plan(10, 4, (1, 2)) == [(1, 4, 8)]
    for world in (1, 2, 3, 5):
        got = sorted(i for r in range(world) for _, first, end in plan(10, 4, (r, world)) for i in range(first, end))
        assert got == list(range(10)), world
        assert sorted(itertools.chain(*(plan(10, 4, (r, world)) for r in range(world)))) == plan(10, 4)
    assert plan(8, 4) == [(0, 0, 4), (1, 4, 8)]                                               # no ragged batch
    assert plan(3, 4) == [(0, 0, 3)] and plan(1, 1) == [(0, 0, 1)]
    for b, first, end in plan(1001, 128):
        assert first == b * 128 and 0 < end - first <= 128
    with pytest.raises(ValueError):
        plan(0, 4)
    with pytest.raises(ValueError):
        plan(4, 0)


def fid_args(*more):
    from mapdit_amd import sample_fid
    return sample_fid.build_parser().parse_args(["--result-dir", "x", "--sample-rng", "counter", "--use-vae", "false", "--num-classes", "10",
                                                 *more])


CHANGES = {"seed": ["--seed", "7"], "num_samples": ["--num-samples", "12"], "batch_size": ["--batch-size", "4"],
           "sampler": ["--sampler", "dpm++"], "num_sampling_steps": ["--num-sampling-steps", "3"], "cfg_scale": ["--cfg-scale", "1.0"],
           "precision": ["--precision", "bf16"], "ema_std": ["--ema-std", "0.1"], "ckpt": ["--ckpt", "0000008"],
           "num_classes": ["--num-classes", "11"], "use_vae": ["--use-vae", "true"], "graph": ["--no-graph"]}


def test_manifest_equal_passes_and_every_differing_key_is_named():
    from mapdit_amd.sample_fid import MANIFEST_KEYS, check_manifest, make_manifest
    train_args = {"objective": "diffusion"}
    base = make_manifest(fid_args(), train_args)
    assert set(base) == set(MANIFEST_KEYS)
    check_manifest(base, make_manifest(fid_args(), train_args))
    check_manifest(base, make_manifest(fid_args("--shard", "1/2"), train_args))               # a part is the same whoever makes it
    import json
    check_manifest(json.loads(json.dumps(base)), base)                                         # what a run finds on disk
    for key, flags in CHANGES.items():
        new = make_manifest(fid_args(*flags), train_args)
        differing = [k for k in MANIFEST_KEYS if base[k] != new[k]]
        assert key in differing, (key, differing)
        first = min(differing)                                                                  # keys are compared in sorted order
        with pytest.raises(ValueError, match=rf"\b{first} = ") as e:
            check_manifest(base, new)
        assert f"{first} = {base[first]!r}" in str(e.value) and f"{first} = {new[first]!r}" in str(e.value)
    for key in MANIFEST_KEYS:                                                                  # each key on its own, and a key one side lacks
        with pytest.raises(ValueError, match=rf"\b{key} = "):
            check_manifest(base, {**base, key: "something else"})
        with pytest.raises(ValueError, match=rf"\b{key} = .*<absent>"):
            check_manifest(base, {k: v for k, v in base.items() if k != key})
    flow = make_manifest(fid_args("--sampler", "flow-euler"), {"objective": "flow", "flow_shift": 3.0})
    assert flow["objective"] == "flow" and flow["flow_shift"] == 3.0 and base["flow_shift"] is None
    solver = make_manifest(fid_args("--sampler", "dpm++", "--solver-order", "1"), train_args)
    assert solver["solver_order"] == 1 and base["solver_order"] is None                       # a flag the sampler does not read is no key


@pytest.mark.parametrize("flags,match", [
    (["--shard", "1/2"], "needs --sample-rng counter"),
    (["--shard", "0/2", "--sample-rng", "torch"], "needs --sample-rng counter"),
    (["--shard", "2/2", "--sample-rng", "counter"], "0 <= R < W"),
    (["--shard", "0/0", "--sample-rng", "counter"], "W >= 1"),
    (["--shard=-1/2", "--sample-rng", "counter"], "0 <= R < W"),
    (["--shard", "half", "--sample-rng", "counter"], "expected R/W"),
])
def test_sample_fid_refuses_a_bad_shard_before_any_model_is_built(tmp_path, flags, match):
    from mapdit_amd import sample_fid
    with pytest.raises(ValueError, match=match):                          # before config.yaml of the (missing) run directory is read
        sample_fid.main(["--result-dir", str(tmp_path / "no_such_run")] + flags)


def test_sample_rng_flag_defaults_to_torch_on_the_three_clis():
    from mapdit_amd import sample, sample_ema, sample_fid
    for cli in (sample, sample_ema, sample_fid):
        p = cli.build_parser()
        assert p.parse_args(["--result-dir", "x"]).sample_rng == "torch", cli.__name__
        assert p.parse_args(["--result-dir", "x", "--sample-rng", "counter"]).sample_rng == "counter"
        with pytest.raises(SystemExit):
            p.parse_args(["--result-dir", "x", "--sample-rng", "philox"])
    assert sample_fid.build_parser().parse_args(["--result-dir", "x"]).shard == "0/1"


def test_rng_and_index_go_together_on_every_loop():
    """Refused on the first look at the arguments: no model is called, no device touched."""
    from mapdit_amd.diffusion import create_diffusion
    from mapdit_amd.flow import create_flow
    from mapdit_amd.sampling import run_sampler
    d, f, shape = create_diffusion("4"), create_flow(), (2, 4, 8, 8)
    rng = object()                                                         # (never used: the pairing is checked before the rng is)
    loops = [d.p_sample_loop, d.ddim_sample_loop, d.dpm_solver_sample_loop, f.sample_loop,
             lambda *a, **k: list(d.p_sample_loop_progressive(*a, **k)), lambda *a, **k: list(d.ddim_sample_loop_progressive(*a, **k))]
    for loop in loops:
        with pytest.raises(ValueError, match="go together"):
            loop(None, shape, rng=rng)
        with pytest.raises(ValueError, match="go together"):
            loop(None, shape, index=[0, 1])
    import torch
    x, t = torch.zeros(shape), torch.zeros(2, dtype=torch.int64)
    for step in (d.p_sample, d.ddim_sample):
        with pytest.raises(ValueError, match="go together"):
            step(None, x, t, rng=rng)
        with pytest.raises(ValueError, match="go together"):
            step(None, x, t, index=[0, 1])
    with pytest.raises(ValueError, match="go together"):
        run_sampler(None, d, x, t, None, rng=rng)


@pytest.mark.parametrize("bad", [[-1], [0, 2 ** 32], [3, -1, 5]])
def test_an_index_outside_32_bits_is_refused(bad):
    from mapdit_amd import sample_rng
    from mapdit_amd.diffusion import create_diffusion
    with pytest.raises(ValueError, match=r"does not lie in \[0, 2\^32\)"):
        sample_rng.check_index(bad)
    with pytest.raises(ValueError, match=r"does not lie in \[0, 2\^32\)"):      # on a loop: before the rng or the model is touched
        create_diffusion("4").p_sample_loop(None, (len(bad), 4, 8, 8), rng=object(), index=bad)


def test_index_shapes_and_the_cpu_refusal():
    import torch

    from mapdit_amd import sample_rng
    assert sample_rng.check_index([0, 2 ** 32 - 1]).tolist() == [0, 2 ** 32 - 1]
    for bad in ([], [[0, 1]], [0.5], [True]):
        with pytest.raises(ValueError, match="1-d integer"):
            sample_rng.check_index(bad)
    idx = torch.tensor([3, 9])
    assert sample_rng.rows_index(idx, 2) is idx and sample_rng.rows_index(idx, 4).tolist() == [3, 9, 3, 9]      # both guidance halves
    with pytest.raises(ValueError, match="2 sample indices for a batch of 3 rows"):
        sample_rng.rows_index(idx, 3)
    with pytest.raises(NotImplementedError):
        sample_rng.SampleRNG(0, "cpu")
