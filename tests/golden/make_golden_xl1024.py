#!/usr/bin/env python3
"""Golden vectors of DiT-XL's width on 1,024 tokens per sample (hidden 1152, 16 heads of 72, patch 2 on 64x64 latents, depth 2):
tests/golden/xl1024_d2.npz.  Same recipe and the same oracle-vs-reference checks as make_golden.py's fixture(); like that script it
runs only where the reference is installed, and writes inputs and expected outputs only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_xl1024.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import O, fixture                     # noqa: E402

if __name__ == "__main__":
    fixture("xl1024_d2", O.DiTConfig(depth=2, hidden_size=1152, patch_size=2, input_size=64, in_channels=4, num_heads=16,
                                     num_classes=10), n=2, wseed=13, dseed=14, gains=0.3, perturb=0.3, full=False, check_tol=5e-5)
