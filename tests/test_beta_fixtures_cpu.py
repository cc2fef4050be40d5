"""CPU, build container only: tools/gen_beta_golden.py, run again on the unmodified reference, reproduces the committed
Beta fixtures (tests/golden/beta_*.npz) array for array, bit for bit."""
import os

import numpy as np
import pytest

import ref_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(ref_harness.REFERENCE_ROOT, "super_sac")),
                                reason="the reference tree is only present in the build container")


@pytest.mark.parametrize("name", ["beta_redq", "beta_sac", "beta_sunrise"])
def test_generator_reproduces_the_committed_fixture(name, tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_beta_golden", os.path.join(ROOT, "tools", "gen_beta_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    gen.main([name], out=str(tmp_path))
    new = np.load(os.path.join(tmp_path, f"{name}.npz"))
    old = np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))
    assert sorted(new.files) == sorted(old.files)
    for key in old.files:
        assert new[key].dtype == old[key].dtype and np.array_equal(new[key], old[key]), key
