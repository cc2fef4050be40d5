"""CPU, dev container only (skipped where the reference tree is absent): tools/gen_aug_golden.py is deterministic and the
committed tests/golden/aug_*.npz are what it writes; this package's classes draw like the reference's own."""
import os
import sys

import numpy as np
import pytest
import torch

import aug_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gen():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_harness
    if not os.path.isdir(os.path.join(ref_harness.REFERENCE_ROOT, "super_sac")):
        pytest.skip("reference tree not present")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_aug_golden
    return gen_aug_golden


NAMES = ["aug_RotateAug_c3", "aug_GammaAug_c9", "aug_TranslateAug_c3", "aug_chain_gamma2", "aug_mixed_drqv2", "aug_smaa",
         "aug_critic_update"]


def test_generator_is_deterministic_and_matches_the_committed_fixtures(gen, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    gen.main(NAMES, str(a))
    gen.main(NAMES, str(b))
    for name in NAMES:
        first, second = (a / f"{name}.npz").read_bytes(), (b / f"{name}.npz").read_bytes()
        assert first == second, name
        with np.load(a / f"{name}.npz") as z:
            fresh = {k: z[k] for k in z.files}
        have = aug_cases.load(name)
        assert sorted(fresh) == sorted(have)
        for k in fresh:
            assert np.array_equal(fresh[k], have[k]), (name, k)


@pytest.mark.parametrize("cls", aug_cases.CHAIN_CLASSES)
def test_same_seed_same_parameters_as_the_reference_class(gen, cls):
    import ref_harness
    import super_sac_amd as ssa
    ref = ref_harness.import_reference()
    out = []
    for mod in (ref.augmentations, ssa.augmentations):
        gen.seed_all(17)
        aug = getattr(mod, cls)(7)
        aug.change_randomization_params()
        out.append((aug_cases.snapshot([aug], dict(members=[(cls, {})])), gen.probes(), repr(aug)))
    (p0, q0, r0), (p1, q1, r1) = out
    assert r0 == r1
    for k in p0:
        assert p0[k].dtype == p1[k].dtype and np.array_equal(p0[k], p1[k]), k
    for k in q0:
        assert np.array_equal(q0[k], q1[k]), k
