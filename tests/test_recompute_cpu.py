"""Activation recompute without a device: what mapdit_engine_workspace_bytes answers per level (mapdit_config_t.recompute), the
configurations it refuses, and the facade / CLI switch.

The workspace conditions come from the buffer list of a block (engine.hip, carve()), not from a measurement.  Per token row a plain
training block keeps eight 16-bit [M, D] tensors (xm, qn, kn, v, o, y, xm2, y2), two 16-bit [M, 4D] tensors (hact, hdact) and two fp32
[M, D] residual checkpoints: 16 + 16 + 8 = 40 D bytes, plus two small fp32 vectors per head and token (lse, qks).  Level "mlp" keeps
hact / hdact once: 16 D less per block.  Level "block" keeps the checkpoints, xm and y2 per block (12 D): 28 D less.  With U = M * D
bytes the bounds below leave one U for alignment and the small vectors."""
import copy
import ctypes as C
import pickle

import pytest

from mapdit_amd import _lib as L

B2 = dict(hidden=768, num_heads=12, mlp_hidden=3072, patch=2, input_size=32, in_channels=4, table_rows=1001, max_batch=256)
U = 256 * 256 * 768                       # M * D bytes: 256 samples x 256 tokens x 768
PARENT_WS_DEPTH12_TRAIN = 27303030784     # mapdit_engine_workspace_bytes of this configuration on the commit before the field existed


def ws(depth, recompute, train=1, **over):
    cfg = L.Config(**{**B2, **over}, depth=depth, recompute=recompute)
    return L.lib().engine_workspace_bytes(C.byref(cfg), train)


def inc(recompute):
    return ws(13, recompute) - ws(12, recompute)


def test_workspace_increment_per_block_and_level():
    incs = [inc(r) for r in (0, 1, 2)]
    print("bytes per added block (none, mlp, block):", incs, "in U:", [round(i / U, 3) for i in incs])
    assert incs[0] - incs[1] >= 15 * U            # 16 U expected: the two [M, 4D] 16-bit tensors
    assert incs[0] - incs[2] >= 26 * U            # 28 U expected: y2 stays per block
    assert incs[0] - incs[1] <= 17 * U and incs[0] - incs[2] <= 30 * U      # (and nothing the backward needs per block went missing: >= 10 U stay)
    assert ws(12, 2) < ws(12, 1) < ws(12, 0)


def test_level_none_is_the_parents_workspace():
    assert ws(12, 0) == PARENT_WS_DEPTH12_TRAIN


def test_inference_workspace_ignores_the_field():
    sizes = {ws(12, r, train=0) for r in (0, 1, 2)}
    assert len(sizes) == 1 and 0 not in sizes
    # ... also where a training engine would refuse the combination
    assert ws(12, 2, train=0, precision=L.PRECISIONS["bf16x3"]) == ws(12, 0, train=0, precision=L.PRECISIONS["bf16x3"]) > 0


@pytest.mark.parametrize("recompute,over", [
    (3, {}), (-1, {}),
    (1, dict(precision=L.PRECISIONS["bf16x3"])), (2, dict(precision=L.PRECISIONS["bf16x3"])),
    (1, dict(mp_off=L.MP_OFF["no_layernorm"])), (2, dict(mp_off=L.MP_OFF["no_layernorm"])),
])
def test_refused_configurations(recompute, over):
    assert ws(12, 0, **over) > 0                    # (the combination itself is built: it is the recompute level that is refused)
    assert ws(12, recompute, **over) == 0
    assert "recompute" in L.lib().last_error().decode()


def test_unknown_level_is_refused_for_inference_too():
    assert ws(12, 3, train=0) == 0
    assert "recompute" in L.lib().last_error().decode()


def tiny():
    from mapdit_amd.src.dit import DiT
    return DiT(depth=1, hidden_size=128, patch_size=2, input_size=16, in_channels=4, num_heads=2, num_classes=10)


def test_facade_attribute():
    m = tiny()
    assert m.activation_recompute == "none"
    for v in ("mlp", "block", "none"):
        m.activation_recompute = v
        assert m.activation_recompute == v
    for bad in ("full", "MLP", 1, None, True):
        with pytest.raises(ValueError) as ei:
            m.activation_recompute = bad
        assert all(v in str(ei.value) for v in ("none", "mlp", "block"))
    assert m.activation_recompute == "none"         # a refused value changes nothing
    assert not any("recompute" in k for k in m.state_dict())
    m.activation_recompute = "block"
    m2 = tiny()
    m2.load_state_dict(m.state_dict())
    assert m2.activation_recompute == "none"        # a state dict does not carry the switch


def test_facade_attribute_survives_deepcopy_and_pickle():
    m = tiny()
    m.activation_recompute = "mlp"
    assert copy.deepcopy(m).activation_recompute == "mlp"
    m3 = pickle.loads(pickle.dumps(m))
    assert m3.activation_recompute == "mlp"
    st = m.__getstate__()
    st.pop("_activation_recompute")                 # an object pickled before the attribute existed
    m4 = tiny().__class__.__new__(tiny().__class__)
    m4.__setstate__(st)
    assert m4.activation_recompute == "none"


def test_train_cli_flag():
    from mapdit_amd import train
    p = train.build_parser()
    assert p.parse_args(["--results-dir", "r"]).activation_recompute == "none"
    for v in ("none", "mlp", "block"):
        assert p.parse_args(["--results-dir", "r", "--activation-recompute", v]).activation_recompute == v
    with pytest.raises(SystemExit):
        p.parse_args(["--results-dir", "r", "--activation-recompute", "all"])
