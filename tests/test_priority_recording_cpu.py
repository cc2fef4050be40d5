"""CPU: the two pieces of the recorded priority refresh (critic_update(update_priorities=True)) that can be stated
without a GPU -- which calls may be recorded (learning_utils.priority_recordable, over the full grid of its inputs) and
which noise buffers a recording refills on the host, in which order (learning_utils.recording_noise_buffers)."""
import itertools
import re
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("stochastic", "deterministic", "discrete", "beta")


@pytest.fixture(scope="module")
def lu():
    from super_sac_amd import learning_utils
    return learning_utils


def test_eligibility_over_the_full_grid(lu):
    n_yes = 0
    flags = list(itertools.product([False, True], repeat=6))
    for kind, members, mode, (on_device, identity, per, dr3, sharded, bf16) in itertools.product(
            KINDS, (1, 2, 3), ("list", "graph"), flags):
        got = lu.priority_recordable(kind, on_device, identity, members, per, dr3, sharded, bf16, mode)
        want = (kind != "beta" and members == 1 and mode == "list" and on_device and identity
                and not per and not dr3 and not sharded and not bf16)
        assert got is want, (kind, members, mode, on_device, identity, per, dr3, sharded, bf16)
        n_yes += got
    assert n_yes == 3   # one cell per supported head: everything else keeps the eager path


def test_eligibility_takes_truthy_values_as_the_call_passes_them(lu):
    assert lu.priority_recordable("stochastic", True, True, 1, 0, 0.0, None, False, "list") is True
    assert lu.priority_recordable("stochastic", True, True, 1, False, 0.01, False, False, "list") is False


@pytest.mark.parametrize("kind", KINDS[:3])
@pytest.mark.parametrize("explore", [False, True])
@pytest.mark.parametrize("refresh", [False, True])
def test_draw_order_of_a_recording(lu, kind, explore, refresh):
    from super_sac_amd import adv_estimator
    assert lu.recording_noise_buffers(kind, explore, refresh, True) == ([], [])   # in-kernel noise: nothing on the host
    before, after = lu.recording_noise_buffers(kind, explore, refresh, False)
    # the reference's order on the device generator: head eps, process noise | REDQ subset (Python random) | candidates
    want_before = {"stochastic": ["eps"], "deterministic": [], "discrete": []}[kind]
    if explore and kind != "discrete":
        want_before = want_before + ["proc"]
    want_after = [f"cand{k}" for k in range(adv_estimator.N_SAMPLES)] if (refresh and kind == "stochastic") else []
    assert before == want_before and after == want_after
    assert adv_estimator.N_SAMPLES == 4   # adv_estimator.py:58


def test_the_candidates_key_is_a_site_constant_of_its_own():
    from super_sac_amd import acting, beta
    src = open(os.path.join(ROOT, "super_sac_amd", "csrc", "ssac_adv.hip")).read()
    salt = int(re.search(r"ADV_KEY_SALT\s*=\s*(0x[0-9A-Fa-f]+)ULL", src).group(1), 16)
    header = open(os.path.join(ROOT, "include", "ssac_hip.h")).read()
    assert f"0x{salt:016X}" in header, "the header comment documents another constant"
    taken = {0xE5A1C0DE0D15EA5E, acting._STREAM_SALT, 0x5A17BE7A5A17BE7A, 0} | set(beta.SITE_SALT)
    assert salt not in taken and 0 < salt < 2 ** 64   # (key = seed ^ salt: one seed never gives two sites one key)


def test_the_recording_key_tells_the_two_call_forms_apart():
    src = open(os.path.join(ROOT, "super_sac_amd", "learning.py")).read()
    key = re.search(r"\n    key = \((.*?)\n    cache = ", src, flags=re.S).group(1)
    assert "bool(update_priorities)" in key
