"""Counter-based step draws on the MI355X: csrc/steprng.hip against the numpy restatement of its contract (tests/step_rng_reference.py),
its ragged / unaligned store paths, slot independence, null outputs, capture, and DiT.forward's force_drop_ids."""
import copy

import numpy as np
import pytest
import torch

import data_reference as R
import step_rng_reference as S
from test_data_gpu import EPS, NORMAL_BOUND_ULP          # the derived bound of the fp32 normal recipe: the same recipe, the same bound

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SEED, STEP, FIRST, COUNT, PER, T, NC = 0x0123456789ABCDEF, 7, 5, 3, 4096, 1000, 10
SENTINEL = 12345.0
ALL = ("eps", "x_syn", "t", "u", "z", "drop", "y_syn")
DT = {"eps": torch.float32, "x_syn": torch.float32, "t": torch.int64, "u": torch.float64, "z": torch.float64, "drop": torch.int64, "y_syn": torch.int64}


def L():
    from mapdit_amd import _lib
    return _lib


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def same(a, b):
    return all(torch.equal(bits(getattr(a, k)), bits(getattr(b, k))) for k in vars(a)) and set(vars(a)) == set(vars(b))


def raw_draw(count, per, drop_prob=0.1, want=ALL, offset=0, seed=SEED, step=STEP, first=FIRST):
    """mapdit_step_draw into buffers with one sentinel element behind every output (and `offset` elements in front of the planes)."""
    out, full = {}, {}
    for w in want:
        n = count * per if w in ("eps", "x_syn") else count
        off = offset if w in ("eps", "x_syn") else 0
        full[w] = torch.full((off + n + 1,), SENTINEL, dtype=DT[w], device=DEV)
        out[w] = full[w][off:off + n]
    L().lib().step_draw(seed, step, first, count, per, T, NC, drop_prob, *(out[w].data_ptr() if w in out else None for w in ALL), L().cur_stream())
    for w in want:
        assert float(full[w][-1]) == SENTINEL and (full[w][:len(full[w]) - 1 - out[w].numel()] == SENTINEL).all(), f"{w}: wrote outside its plane"
    return {w: (v.view(count, per) if w in ("eps", "x_syn") else v) for w, v in out.items()}


def assert_normals(got, ref, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    err = np.abs(got - ref) / (np.abs(ref) * EPS)
    print(f"{what}: largest error {err.max():.2f} ulp (bound {NORMAL_BOUND_ULP})")
    assert (err <= NORMAL_BOUND_ULP).all(), (what, err.max())


@pytest.mark.parametrize("drop_prob", [0.1, 0.0, 1.0])
def test_step_draw_is_the_contract(drop_prob):
    d = raw_draw(COUNT, PER, drop_prob)
    ref = S.scalars(SEED, STEP, FIRST, COUNT, T, NC, drop_prob)
    for k in ("t", "drop", "y_syn"):
        assert (d[k].cpu().numpy() == ref[k]).all(), k
    assert (d["u"].cpu().numpy().view(np.int64) == ref["u"].view(np.int64)).all()
    assert ((0 <= ref["u"]) & (ref["u"] < 1)).all() and (ref["t"] < T).all() and (ref["y_syn"] < NC).all()
    assert_normals(d["eps"], S.planes(SEED, STEP, FIRST, COUNT, S.TAG_EPS, PER), "eps")
    assert_normals(d["x_syn"], S.planes(SEED, STEP, FIRST, COUNT, S.TAG_SYNX, PER), "x_syn")
    assert_normals(d["z"], ref["z"], "z")
    if drop_prob in (0.0, 1.0):
        assert (d["drop"] == int(drop_prob)).all()


def test_drop_rate_over_many_slots():
    """The integer compare on the device, 4,096 slots: the restatement bit for bit, and both outcomes occur."""
    d = raw_draw(4096, 1, 0.1, want=("drop",), first=0)["drop"].cpu().numpy()
    assert (d == S.scalars(SEED, STEP, 0, 4096, T, NC, 0.1)["drop"]).all() and 0 < d.sum() < 4096


@pytest.fixture(scope="module")
def aligned_planes():
    return raw_draw(COUNT, 4100, want=("eps", "x_syn"))


@pytest.mark.parametrize("per,offset", [(1, 0), (3, 0), (4, 0), (6, 0), (4097, 0), (4096, 1)])
def test_ragged_and_unaligned_planes_hold_the_aligned_values(aligned_planes, per, offset):
    """per % 4 != 0: the tail path; per = 4: one whole 16-byte group; offset 1: planes 4 bytes off a 16-byte boundary, element-wise
    stores.  An element is a function of (slot, i) alone, so every call's rows are prefixes of the aligned call's; raw_draw checks the
    sentinels on both sides of every plane."""
    d = raw_draw(COUNT, per, want=("eps", "x_syn"), offset=offset)
    assert d["eps"].data_ptr() % 16 == (4 * offset) % 16
    for k in ("eps", "x_syn"):
        assert torch.equal(bits(d[k]), bits(aligned_planes[k][:, :per])), k


def rng(seed=SEED):
    from mapdit_amd.step_rng import StepRNG
    return StepRNG(seed, DEV)


KW = dict(per=48, T=T, num_classes=NC, drop_prob=0.1)


def cat(parts):
    from types import SimpleNamespace
    return SimpleNamespace(**{k: torch.cat([getattr(p, k) for p in parts]) for k in vars(parts[0])})


def test_draws_do_not_depend_on_how_the_slots_are_split():
    r = rng()
    whole = r.draw(3, 0, 8, **KW)
    assert set(vars(whole)) == set(ALL) and whole.eps.shape == (8, 48) and whole.t.dtype == torch.int64 and whole.u.dtype == torch.float64
    assert same(cat([r.draw(3, f, 4, **KW) for f in (0, 4)]), whole)
    assert same(cat([r.draw(3, f, 2, **KW) for f in (0, 2, 4, 6)]), whole)          # world = 2, K = 2
    assert same(rng().draw(3, 0, 8, **KW), whole)                                     # no state in the object
    assert not torch.equal(bits(r.draw(4, 0, 8, **KW).eps), bits(whole.eps))          # another step
    assert not torch.equal(bits(rng(SEED + 1).draw(3, 0, 8, **KW).eps), bits(whole.eps))
    assert not torch.equal(bits(rng(SEED + (1 << 32)).draw(3, 0, 8, **KW).eps), bits(whole.eps))      # the key's high word
    assert not torch.equal(bits(whole.eps), bits(whole.x_syn))
    assert not torch.equal(whole.t[:4], whole.t[4:])


def test_the_slot_range_ends_at_two_to_the_32():
    from mapdit_amd._lib import MapditError
    r = rng()
    top = r.draw(0, (1 << 32) - 2, 2, **KW)
    ref = S.scalars(SEED, 0, (1 << 32) - 2, 2, T, NC, 0.1)
    assert (top.t.cpu().numpy() == ref["t"]).all() and (top.y_syn.cpu().numpy() == ref["y_syn"]).all()
    for args, msg in [(((1 << 32) - 2, 3), "do not lie in"), ((-1, 2), "do not lie in"), ((0, 0), "count")]:
        with pytest.raises(MapditError, match=msg):
            r.draw(0, *args, **KW)
    for bad, msg in [(dict(per=0), "per"), (dict(T=0), "timesteps"), (dict(num_classes=0), "num_classes"), (dict(drop_prob=1.5), "drop_prob"),
                     (dict(drop_prob=-0.1), "drop_prob"), (dict(drop_prob=float("nan")), "drop_prob")]:
        with pytest.raises(MapditError, match=msg):
            r.draw(0, 0, 2, **{**KW, **bad})
    with pytest.raises(ValueError, match="needs per"):
        r.draw(0, 0, 2, want=("eps",))
    with pytest.raises(ValueError, match="want names"):
        r.draw(0, 0, 2, want=("noise",))
    with pytest.raises(NotImplementedError):
        from mapdit_amd.step_rng import StepRNG
        StepRNG(0, "cpu")


def test_every_output_alone_and_under_capture():
    r = rng()
    whole = r.draw(9, 16, 5, **KW)
    for k in ALL:
        one = r.draw(9, 16, 5, **KW, want=(k,))
        assert list(vars(one)) == [k] and torch.equal(bits(getattr(one, k)), bits(getattr(whole, k))), k
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                            # one kernel node: draw() is one launch
        got = r.draw(9, 16, 5, **KW)
    for k in ALL:
        getattr(got, k).zero_()
    g.replay()
    torch.cuda.synchronize()
    assert same(got, whole)


def test_force_drop_ids_replaces_the_torch_draw():
    from mapdit_amd.src.models import DIT_MODELS
    torch.manual_seed(0)
    model = DIT_MODELS["DiT-XS/2"](in_channels=4, input_size=32, num_classes=10).to(DEV).train()
    model.gemm_precision = "bf16"
    start = copy.deepcopy(model.state_dict())            # (a training-mode forward rewrites the weights in place: forced weight norm)
    g = torch.Generator().manual_seed(1)
    x, t = torch.randn(4, 4, 32, 32, generator=g).to(DEV), torch.randint(0, 1000, (4,), generator=g).to(DEV)
    y = torch.tensor([3, 7, 1, 9], device=DEV)
    drop = torch.tensor([1, 0, 1, 0], device=DEV)
    before = torch.cuda.get_rng_state(DEV)
    forced = model(x, t, y, force_drop_ids=drop).detach()
    forced_bool = None
    assert torch.equal(torch.cuda.get_rng_state(DEV), before)                      # the keyword consumes no generator
    model.load_state_dict(start)
    forced_bool = model(x, t, y, force_drop_ids=drop.bool()).detach()
    model.load_state_dict(start)
    model.class_dropout_prob = 0.0                       # the same training-mode code with the label drop switched off
    want = model(x, t, torch.tensor([10, 7, 10, 9], device=DEV)).detach()
    assert torch.equal(torch.cuda.get_rng_state(DEV), before)
    model.class_dropout_prob = 0.1
    assert torch.equal(bits(forced), bits(want)) and torch.equal(bits(forced_bool), bits(want))
    model.load_state_dict(start)
    kept = model(x, t, y, force_drop_ids=torch.zeros(4, dtype=torch.int64, device=DEV)).detach()
    assert not torch.equal(bits(kept), bits(want))       # the drop does change the output
    model(x, t, y)
    assert not torch.equal(torch.cuda.get_rng_state(DEV), before)                  # without the keyword token_drop draws as before
    model.eval()
    with torch.no_grad():
        a, b = model(x, t, y), model(x, t, y, force_drop_ids=drop)
    assert torch.equal(bits(a), bits(b))                 # training mode only
    with pytest.raises(ValueError, match="force_drop_ids"):
        model(x, t, y, force_drop_ids=drop[:2])
    with pytest.raises(TypeError):
        model.forward_with_cfg(x, t, y, 1.5, force_drop_ids=drop)
