"""Pins the CPU oracle to the golden vectors of DiT-XL's width on 1,024 tokens per sample (tests/golden/make_golden_xl1024.py:
hidden 1152, 16 heads of 72, patch 2 on 64x64 latents, depth 2).  CPU only; the tolerances are test_oracle_golden.py's."""
import torch

from conftest import golden_cfg, golden_state_dict, load_golden, rel_err, sub
from oracle import dit_oracle as O
from test_oracle_golden import TOL, _train


def test_xl1024_d2_known_answers():
    g = load_golden("xl1024_d2")
    cfg = golden_cfg(g)
    assert (cfg.input_size // cfg.patch_size) ** 2 == 1024 and cfg.hidden_size // cfg.num_heads == 72
    sd = golden_state_dict(g, cfg)
    x, y, t = torch.from_numpy(g["x"]), torch.from_numpy(g["y"]), torch.from_numpy(g["t"])
    with torch.no_grad():
        out = O.dit_forward({k: v.clone() for k, v in sd.items()}, cfg, x, t, y, train=False)
    assert rel_err(out.numpy(), g["eval_out"]) < TOL
    osd, losses = _train(g, cfg, sd)
    for k in ("loss", "mse", "vb"):
        assert rel_err(losses[k].detach().numpy(), g["train_" + k]) < TOL, k
    for k in osd:
        if k in O.BUFFER_KEYS:
            continue
        assert rel_err(sub(osd[k].grad, stride=4099), g["grad/" + k]) < 1e-3, k
        if float(g["gradnorm/" + k]) > 1e-7:
            assert abs(float(osd[k].grad.double().norm()) / float(g["gradnorm/" + k]) - 1) < 1e-3, k
