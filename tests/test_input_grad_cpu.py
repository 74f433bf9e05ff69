"""Input-latent gradients, CPU side: the oracle's autograd dL/dx against the reference's own (tests/golden/input_grad.npz, written by
tests/golden/make_golden_input_grad.py), and the facade's refusals where there is no device."""
import pytest
import torch

from conftest import golden_cfg, golden_state_dict, load_golden, rel_err
from oracle import dit_oracle as O

IG = load_golden("input_grad")
FIXTURES = [str(n) for n in IG["fixtures"]]
CFG_FIXTURE, CFG_SCALE = str(IG["cfg_fixture"]), float(IG["cfg_scale"])


def oracle_dx(name):
    """dx of sum(model(x) * w) through the oracle (fp32, CPU); through dit_forward_with_cfg for the CFG fixture."""
    g = load_golden(name)
    cfg = golden_cfg(g)
    sd = golden_state_dict(g, cfg)
    with_cfg = name == CFG_FIXTURE
    xk, tk, yk = ("ps_z", "ps_t", "ps_y") if with_cfg else ("x", "t", "y_eff")
    x, t, y = (torch.from_numpy(g[k]) for k in (xk, tk, yk))
    w = torch.from_numpy(IG[f"{name}/w"])
    x = x.clone().requires_grad_(True)
    out = O.dit_forward_with_cfg(sd, cfg, x, t, y, CFG_SCALE) if with_cfg else O.dit_forward(sd, cfg, x, t, y, train=False)
    (out * w).sum().backward()
    return x.grad


@pytest.mark.parametrize("name", FIXTURES + [CFG_FIXTURE])
def test_oracle_autograd_dx_matches_reference(name):
    dx = oracle_dx(name)
    stride = int(IG["stride"])
    e = rel_err(dx.reshape(-1)[::stride].numpy(), IG[f"{name}/dx"])
    print(f"{name}: oracle dx vs reference rel err {e:.3e}")
    assert e < 1e-5
    assert abs(float(dx.double().norm()) / float(IG[f"{name}/dx_norm"]) - 1) < 1e-5
    if name == CFG_FIXTURE:                     # only the first half of the CFG batch reaches the network
        assert float(dx[dx.shape[0] // 2:].abs().max()) == 0.0


def test_facade_refusals_without_a_device():
    from mapdit_amd import _lib as L
    from mapdit_amd.src.dit import DiT
    m = DiT(depth=1, hidden_size=128, patch_size=2, input_size=16, in_channels=4, num_heads=2, num_classes=10)
    assert m.input_gradients is False
    assert "input_gradients" not in m.state_dict()
    x = torch.randn(2, 4, 16, 16).requires_grad_(True)
    t, y = torch.tensor([1, 2]), torch.tensor([3, 4])
    # off (the default): the refusal the engine has always made, now naming the switch
    with pytest.raises(L.MapditError, match="input latents") as ei:
        m(x, t, y)
    assert "input_gradients" in str(ei.value)
    # on, no device: the ordinary "no CPU path" error and not a new one
    m.input_gradients = True
    with pytest.raises(L.MapditError, match="MI355X only"):
        m(x, t, y)
    # a state dict does not carry the switch
    m2 = DiT(depth=1, hidden_size=128, patch_size=2, input_size=16, in_channels=4, num_heads=2, num_classes=10)
    m2.load_state_dict(m.state_dict())
    assert m2.input_gradients is False
