#!/usr/bin/env python3
"""Golden vectors for the input-latent gradient dL/dx (runs ONLY in the build container, where the reference checkout exists;
see make_golden.py).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_input_grad.py <reference checkout>

Writes input_grad.npz, inputs and expected outputs only (nothing of the reference is copied).  For every fixture in FIXTURES
(weights, x, t, y_eff: the fixture's own .npz, regenerated from its seeds by the tests) a cotangent w ~ N(0, 1) is drawn from
WSEED + the fixture's index, and the REFERENCE model's own autograd gives

    dx = d/dx sum(model(x, t, y_eff) * w)          (eval mode: no label drop, no weight rewrite)

tiny_a (P 16, D 128), tiny_c (P 64), tiny_p8 (P 256, 16 tokens: generic attention), xl_d1 (D 1152, head_dim 72).  For tiny_b the same
through the reference's forward_with_cfg(z, t, yy, 1.5) on the fixture's sampler inputs (ps_z, ps_t, ps_y): only the first half of z
reaches the network, the second half's gradient is zero.  Everything is stored whole (the largest x has 12,288 elements; stride 1 is
recorded so that a later, larger fixture can subsample).  While writing, the oracle's autograd is compared with the reference's
(1e-5): tests/test_input_grad_cpu.py repeats that from the file.
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MAPDIT_REFERENCE", "")
assert os.path.isfile(os.path.join(REF, "src", "dit.py")), "usage: make_golden_input_grad.py <reference checkout> (or MAPDIT_REFERENCE)"
sys.path.insert(0, REF)

import warnings

import numpy as np
import torch

warnings.filterwarnings("ignore")
torch.set_num_threads(8)

from src.dit import DiT as RefDiT                        # noqa: E402  (reference)

from conftest import golden_cfg, golden_state_dict, load_golden   # noqa: E402
from oracle import dit_oracle as O                       # noqa: E402

FIXTURES = ["tiny_a", "tiny_c", "tiny_p8", "xl_d1"]
CFG_FIXTURE, CFG_SCALE = "tiny_b", 1.5
WSEED = 300
STRIDE = 1


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


def build_ref(cfg, sd):
    m = RefDiT(**cfg.to_dict())
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    return m.eval()


if __name__ == "__main__":
    out = {"fixtures": np.array(FIXTURES), "cfg_fixture": np.array(CFG_FIXTURE), "cfg_scale": np.array(CFG_SCALE),
           "wseed": np.array(WSEED), "stride": np.array(STRIDE)}
    for i, name in enumerate(FIXTURES + [CFG_FIXTURE]):
        g = load_golden(name)
        cfg = golden_cfg(g)
        sd = golden_state_dict(g, cfg)
        ref = build_ref(cfg, sd)
        with_cfg = name == CFG_FIXTURE
        xk, tk, yk = ("ps_z", "ps_t", "ps_y") if with_cfg else ("x", "t", "y_eff")
        x, t, y = (torch.from_numpy(g[k]) for k in (xk, tk, yk))
        w = torch.randn(x.shape[0], 2 * cfg.in_channels, cfg.input_size, cfg.input_size, generator=torch.Generator().manual_seed(WSEED + i))
        xr = x.clone().requires_grad_(True)
        o = ref.forward_with_cfg(xr, t, y, CFG_SCALE) if with_cfg else ref(xr, t, y)
        (o * w).sum().backward()
        xo = x.clone().requires_grad_(True)
        sdo = {k: v.clone() for k, v in sd.items()}
        oo = O.dit_forward_with_cfg(sdo, cfg, xo, t, y, CFG_SCALE) if with_cfg else O.dit_forward(sdo, cfg, xo, t, y, train=False)
        (oo * w).sum().backward()
        e = rel(xo.grad, xr.grad)
        print(f"== {name}: |dx| {float(xr.grad.norm()):.4e}  oracle-vs-ref rel {e:.2e}")
        assert e < 1e-5
        out[f"{name}/w"] = w.numpy()
        out[f"{name}/dx"] = xr.grad.reshape(-1)[::STRIDE].numpy().copy()
        out[f"{name}/dx_norm"] = np.array(xr.grad.double().norm().item())
    path = os.path.join(HERE, "input_grad.npz")
    np.savez_compressed(path, **out)
    print(f"== input_grad.npz written ({os.path.getsize(path) / 1e3:.0f} kB)")
