"""CPU, dev container only (skipped where the reference tree is absent): tools/gen_aug_colour_golden.py is deterministic and
the committed colour-augmentation fixtures under tests/golden are what it writes."""
import os
import sys

import numpy as np
import pytest

import aug_colour_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gen():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_harness
    if not os.path.isdir(os.path.join(ref_harness.REFERENCE_ROOT, "super_sac")):
        pytest.skip("reference tree not present")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_aug_colour_golden
    return gen_aug_colour_golden


NAMES = ["aug_jitter_c3", "aug_jitter_odd", "aug_netrand_odd", "aug_colour_mixed", "aug_netrand_mixed", "aug_colour_smaa"]


def test_generator_is_deterministic_and_matches_the_committed_fixtures(gen, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    gen.main(NAMES, str(a))
    gen.main(NAMES, str(b))
    for name in NAMES:
        assert (a / f"{name}.npz").read_bytes() == (b / f"{name}.npz").read_bytes(), name
        with np.load(a / f"{name}.npz") as z:
            fresh = {k: z[k] for k in z.files}
        have = cc.load(name)
        assert sorted(fresh) == sorted(have)
        for k in fresh:
            assert np.array_equal(fresh[k], have[k]), (name, k)
