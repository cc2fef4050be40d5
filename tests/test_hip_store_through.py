"""GPU: write-through stores for what the weight-gradient launch hands to the next update (ssac_store_through,
profiles/store_through.md).

The switch changes the cache policy of some 16-byte stores and nothing else, so every comparison here is of BYTES: a launch
with the switch on against the same launch with it off, over everything the launch writes.  Every test asserts through
ssac_store_through_taken() that the form it means to test actually ran.

What writes through: the fc2 tiles' p / m / v / target stores of the fixed-shape form of ssac_mlp_wgrad_all_lossfold.  The
harness is test_hip_wgrad_fixed.FixedLaunch, whose arenas end in sentinel words: a store aimed past a tile's block, or past the
arena, shows there or as a difference from the switch-off launch.  (The same stores were built and measured for h1 / h2 / dz1u
of the chained launch's critic tiles; they were slower and are not in the library, so there is no such form to test.)
"""
import copy
import math
import random
from itertools import chain

import numpy as np
import pytest
import torch

import synth
import wgrad_cases as wc
from test_hip_wgrad_fixed import ADAM, FixedLaunch, _case, _inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
WGRAD_BIT = 1    # ssac_hip_test.h: bit 0 = the optimizer stores of the fixed weight-gradient form's fc2 tiles


@pytest.fixture(scope="module")
def ssa():
    import super_sac_amd
    return super_sac_amd


@pytest.fixture
def lib(ssa):
    """the library with every switch this file turns restored whatever a test does"""
    lib = ssa._lib.lib
    try:
        yield lib
    finally:
        lib.ssac_store_through(-1)
        lib.ssac_fused_tile_rows(0)
        lib.ssac_wgrad_fixed(1)
        lib.ssac_wgrad_variant(0)


# ---- the weight-gradient launch ---------------------------------------------------------------------------------------

WG_BYTES = ("params", "m", "v", "target", "sumsq", "partials", "td_out", "logs", "td_stats", "tick", "done")
# (dz2u rebuilt from h2, late word (None: static tau; 0.0: the bit clear, no target store), target arena, logs)
WG_MODES = [(True, None, 1, "folded"), (False, None, 0, "folded"), (True, 0.0, 1, "folded"), (True, wc.TAU, 1, "deferred")]


def _wgrad_on_off(ssa, lib, L, want_on, want_fixed, what, **opt):
    ssa._lib.check(lib.ssac_store_through(-1))
    on = L.run_fold(True, **opt)
    took_on = lib.ssac_store_through_taken() & WGRAD_BIT
    ssa._lib.check(lib.ssac_store_through(0))
    off = L.run_fold(True, **opt)
    took_off = lib.ssac_store_through_taken() & WGRAD_BIT
    assert on["taken"] == want_fixed and off["taken"] == want_fixed, f"{what}: fixed form {on['taken']} / {off['taken']}"
    assert took_on == want_on and took_off == 0, f"{what}: took {took_on} / {took_off}"
    assert set(on) == set(off)
    for k in WG_BYTES:
        if k in on:
            assert on[k].tobytes() == off[k].tobytes(), f"{what}: {k} differs between write-through and plain stores"
    for k in ("params", "m", "v", "target"):
        if k in on:   # (FixedLaunch hands the arenas back with the TAIL sentinel words that stand behind the last net)
            assert on[k].size == L.case["nets"] * L.stride + wc.TAIL
            assert bool((on[k][-wc.TAIL:] == wc.SENT).all()), f"{what}: {k} written past the arena"
    return on


@pytest.mark.parametrize("n,nets", [(256, 1), (384, 1), (256, 2), (384, 2)])
def test_weight_gradient_launch_writes_the_same_bytes_through(ssa, lib, n, nets):
    """Switch on against off at the smallest row counts that take the fixed form (two and three K iterations), N = 1 and 2:
    Polyak on, no target arena, late-bound tau with the bit clear (the target store is skipped), late-bound tau with deferred
    logs -- p, m, v, target with the sentinels behind the arenas, every gradient-norm slot, the loss partials, td_out and the
    folded log block or the deferred statistics."""
    case = _case(n, nets=nets, dz2="null")
    inp, _ = _inputs(case)
    for null, late, target, logs in WG_MODES:
        L = FixedLaunch(ssa, case, inp, dict(ADAM, target=target, seeded=1, id=case["id"]))
        what = f"{n} rows, {nets} nets [late {late}, target {target}, logs {logs}]"
        got = _wgrad_on_off(ssa, lib, L, WGRAD_BIT, 1, what, dz2_null=null, late=late, logs=logs)
        if late == 0.0:   # the bit clear: the target arena is what it was
            before = wc.adam_state(dict(ADAM, target=1, seeded=1, id=case["id"]), (nets, L.stride))[2]
            live = L.off[5] + case["out"]
            assert np.array_equal(got["target"][:nets * L.stride].reshape(nets, L.stride)[:, :live], before[:, :live]), what


@pytest.mark.parametrize("what,case,opt", [
    ("128 rows (two K-groups: the general kernel)", _case(128), {}),
    ("misaligned arena (the dword epilogue)", _case(256), dict(lead=1)),
])
def test_weight_gradient_launches_outside_the_fixed_form_keep_plain_stores(ssa, lib, what, case, opt):
    """A launch that does not take the fixed-shape form has no write-through stores: it reports so and gives the same bytes."""
    inp, _ = _inputs(case)
    L = FixedLaunch(ssa, case, inp, dict(ADAM, target=1, seeded=1, id=case["id"]))
    _wgrad_on_off(ssa, lib, L, 0, 0, what, logs="folded", **opt)


# ---- whole recorded updates -------------------------------------------------------------------------------------------

def _recorded_updates(ssa, mask, B=256, N=2):
    """critic updates at hidden 256 with 32-row critic tiles and the 64 x 64 weight-gradient form forced, recorded and replayed
    until the input ring has wrapped, Polyak every second update.  After EVERY update: parameters, targets, both moments, the
    TD targets and the logs."""
    L, lib = ssa.learning, ssa._lib.lib
    dev = torch.device("cuda")
    S, A, H = 17, 6, 256
    ssa._lib.check(lib.ssac_store_through(mask))
    ssa._lib.check(lib.ssac_fused_tile_rows(32))
    ssa._lib.check(lib.ssac_wgrad_variant(1))
    assert L.USE_GRAPHS and L.LAUNCH_MODE == "list"
    torch.manual_seed(3); np.random.seed(3); random.seed(3)
    agent = ssa.Agent(act_space_size=A, encoder=ssa.nets.IdentityEncoder(S),
                      actor_network_cls=ssa.nets.ContinuousStochasticActor,
                      critic_network_cls=ssa.nets.ContinuousCritic, ensemble_size=1, num_critics=N,
                      hidden_size=H, auto_rescale_targets=False, log_std_low=-5.0, log_std_high=2.0)
    agent.to(dev)
    target = copy.deepcopy(agent)
    buf = ssa.replay.ReplayBuffer(4096, device=dev)
    buf.load_experience(*synth.synth_transitions(2000, S, A, seed=5))
    copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=3e-4)
    eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
    la = torch.Tensor([math.log(0.1)]).to(dev); la.requires_grad = True
    aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(B)])
    flat = lambda mods: torch.cat([p.detach().flatten() for m in mods for p in m.parameters()]).cpu().numpy()
    ar = agent.critics[0].arena(dev)
    steps, taken = [], []
    for k in range(L.FEED_SLOTS + 3):
        lg, dicts = L.critic_update(
            buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt,
            log_alphas=[la], batch_size=B, gamma=0.99, critic_clip=None, encoder_clip=None,
            target_critic_ensemble_n=2, weighted_bellman_temp=None, weight_type=None, pop=False, augmenter=aug,
            encoder_lambda=0, aug_mix=0.0, discrete=False, random_process=None, noise_clip=None, per=False,
            update_priorities=False, dr3_coeff=0.0)
        taken.append(lib.ssac_store_through_taken())
        td = dicts[0]["td_target"].detach().cpu().numpy().copy()
        logs = np.array([float(v_) for _, v_ in sorted(dict(lg).items())], np.float64)   # (read now: views of a ring slot)
        if k % 2 == 0:
            ssa.learning_utils.soft_update(target.critics[0], agent.critics[0], 0.005)
        m, v = copt._ssac_adam.moments_for(("critic", 0), ar.params)
        steps.append(dict(params=flat(agent.critics), target=flat(target.critics), m=m.detach().cpu().numpy().copy(),
                          v=v.detach().cpu().numpy().copy(), td=td, logs=logs))
    torch.cuda.synchronize()
    return steps, taken


def test_recorded_updates_stay_on_the_same_bits(ssa, lib):
    """FEED_SLOTS + 3 recorded updates at B 256 / N 2 with the switch on, then from the same seeds with it off: after every
    update the parameters, the targets, both moments, the TD targets and the logs as bytes.  A reader of a written-through
    array that still found a stale line would show as a difference that grows from the update it first happens in."""
    on, taken_on = _recorded_updates(ssa, -1)
    off, taken_off = _recorded_updates(ssa, 0)
    # (a replayed update issues no launcher call: it repeats the form of the launch that was recorded)
    assert all(t == WGRAD_BIT for t in taken_on) and all(t == 0 for t in taken_off), f"took {taken_on} / {taken_off}"
    assert len(on) == ssa.learning.FEED_SLOTS + 3 == len(off)
    for k, (a, b) in enumerate(zip(on, off)):
        for name in a:
            assert a[name].tobytes() == b[name].tobytes(), f"update {k}: {name} differs between write-through and plain stores"
    assert np.isfinite(on[-1]["params"]).all() and float(np.abs(on[-1]["m"]).max()) > 0
    assert not np.array_equal(on[0]["params"], on[-1]["params"])
