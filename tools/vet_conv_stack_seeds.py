"""CPU: which seeds of the conv-stack update tests (tests/conv_stack_cases.py) leave the REFERENCE arithmetic alone inside the
straggler cap of the encoder parameters?

As tools/vet_mlp_encoder_seeds.py: Adam's first steps move a weight by ~lr * sign(g) whatever |g| is, so a weight whose
gradient is rounding noise can step the other way under another summation order.  case_runner.straggler_check caps how many
elements of a tensor may do that (1 in 10^4, at least one, none over 3e-3, median at most 1e-6).  A seed is usable only if
the oracle itself, run once in fp32 and once with every tensor in fp64, stays inside the cap on every encoder tensor.
Prints one line per (sequence, seed); run with candidate seeds as arguments.

    python tools/vet_conv_stack_seeds.py 3 4 5 6
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ssac_oracle as orc  # noqa: E402
import case_runner  # noqa: E402
import conv_stack_cases as cc  # noqa: E402

# (sequence, mode, update_encoder, with critic_clip / encoder_clip)
RUNS = [("sac", "sac", True, True), ("sac, no clips", "sac", True, False), ("bc", "bc", True, True), ("bc, frozen", "bc", False, True)]


def main(seeds):
    orc.encode = cc.patched_encode(orc)
    clips = (cc.runner.CRITIC_CLIP, cc.runner.ENC_CLIP)
    for label, mode, update_encoder, clipped in RUNS:
        cc.runner.CRITIC_CLIP, cc.runner.ENC_CLIP = clips if clipped else (None, None)
        for seed in seeds or [cc.CONFIGS["minatar"]["seed"]]:
            cfg = dict(cc.CONFIGS["minatar"], seed=seed)
            r32 = cc.run_oracle(orc, cfg, mode, update_encoder=update_encoder)
            torch.set_default_dtype(torch.float64)   # (tensors the oracle makes itself: labels, unit weights)
            try:
                r64 = cc.run_oracle(orc, cfg, mode, dtype=torch.float64, update_encoder=update_encoder)
            finally:
                torch.set_default_dtype(torch.float32)
            verdict, worst, flips = "ok", 0.0, 0
            for key in r32:
                if not (key.startswith("final_") and "encoder" in key):
                    continue
                err = np.abs(r32[key] - r64[key])
                worst = max(worst, float(err.max()))
                try:
                    flips += case_runner.straggler_check(err, 3e-5, 3e-3, "oracle fp32 vs fp64", key)
                    assert float(np.median(err)) <= 1e-6, f"{key}: median {np.median(err):.3e}"
                except AssertionError as e:
                    verdict = f"OUTSIDE THE CAP ({e})"
            print(f"{label:14s} seed {seed}: worst encoder element {worst:.2e}, {flips} counted stragglers: {verdict}")
    cc.runner.CRITIC_CLIP, cc.runner.ENC_CLIP = clips


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]])
