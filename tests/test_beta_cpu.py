"""CPU: Agent(beta_dist=True) -- the reference's Beta policy option (agent.py:60-81, nets/mlps.py:11-76) -- constructs,
carries the reference's state-dict layout, dispatches as the "beta" kind, and refuses what it does not support.  The
reference-backed checks run only where the reference tree exists (like test_reference_compat.py).  No kernel runs."""
import os

import pytest
import torch

import ref_harness


def _agent(E=2, N=2, A=6, S=17, H=64):
    import super_sac_amd as ssa
    torch.manual_seed(0)
    return ssa.Agent(A, ssa.nets.IdentityEncoder(S), ssa.nets.ContinuousStochasticActor, ssa.nets.ContinuousCritic,
                     ensemble_size=E, num_critics=N, hidden_size=H, beta_dist=True)


def test_beta_agent_constructs_with_beta_heads():
    import super_sac_amd as ssa
    ag = _agent()
    for actor in ag.actors:
        assert actor.dist_impl == "beta" and ssa.learning_utils.actor_kind(actor) == "beta"
        assert actor.fc3.out_features == 2 * 6   # concentrations' pre-softplus, laid out as (mu, log std) would be
    assert ag.inverse_model.dist_impl == "beta"
    assert ssa.adopt.action_size(ag.actors[0]) == 6
    # the tanh-normal default is untouched
    plain = ssa.Agent(6, ssa.nets.IdentityEncoder(17), ssa.nets.ContinuousStochasticActor, ssa.nets.ContinuousCritic)
    assert plain.actors[0].dist_impl == "pyd" and ssa.learning_utils.actor_kind(plain.actors[0]) == "stochastic"


def test_nets_accept_beta_and_reject_unknown_heads():
    import super_sac_amd as ssa
    assert ssa.nets.ContinuousStochasticActor(5, 3, dist_impl="beta").dist_impl == "beta"
    assert ssa.nets.ContinuousInverseModel(5, 3, dist_impl="beta").dist_impl == "beta"
    with pytest.raises(AssertionError):
        ssa.nets.ContinuousStochasticActor(5, 3, dist_impl="gamma")


def test_refusals_name_beta():
    import super_sac_amd as ssa
    ag = _agent()
    with pytest.raises(NotImplementedError, match="Beta"):
        ssa.engine.set_precision(ag, "bf16")
    with pytest.raises(NotImplementedError, match="Beta"):
        ssa.beta.refuse("x")


def test_beta_site_counters_extend_the_checkpointed_noise_list():
    import super_sac_amd as ssa
    ag = _agent()
    ag.__dict__["_ssac_noise"] = [123, 4, 5]   # a list saved before the Beta sites existed
    ns, k = ssa.beta.site_counter(ag, torch.device("cpu"), "alpha")
    assert ns is ag.__dict__["_ssac_noise"] and ns[:3] == [123, 4, 5] and len(ns) == 3 + len(ssa.beta.SITES)
    assert k == 3 + ssa.beta.SITES.index("alpha") and ns[k] == 0


def test_beta_hook_is_stock_until_replaced():
    import super_sac_amd as ssa
    assert ssa.rng.beta_is_stock()
    saved = ssa.rng.draw_beta_into
    ssa.rng.draw_beta_into = lambda dst: dst.fill_(0.5)
    try:
        assert not ssa.rng.beta_is_stock()
    finally:
        ssa.rng.draw_beta_into = saved
    assert ssa.rng.beta_is_stock()


_HAVE_REF = os.path.isdir(os.path.join(ref_harness.REFERENCE_ROOT, "super_sac"))
needs_ref = pytest.mark.skipif(not _HAVE_REF, reason="the reference tree is only present in the build container")


def _ref_beta_agent(ref, E=2, N=2):
    class Enc(ref.nets.Encoder):
        def __init__(self):
            super().__init__()

        @property
        def embedding_dim(self):
            return 17

        def forward(self, obs_dict):
            return obs_dict["obs"]
    torch.manual_seed(0)
    return ref.Agent(act_space_size=6, encoder=Enc(), actor_network_cls=ref.nets.mlps.ContinuousStochasticActor,
                     critic_network_cls=ref.nets.mlps.ContinuousCritic, ensemble_size=E, num_critics=N, hidden_size=64,
                     beta_dist=True)


@needs_ref
def test_state_dicts_match_the_reference_key_for_key():
    ref = ref_harness.import_reference()
    mine, theirs = _agent(), _ref_beta_agent(ref)
    pairs = list(zip(mine.actors, theirs.actors)) + list(zip(mine.critics, theirs.critics)) + [
        (mine.inverse_model, theirs.inverse_model)]
    for a, b in pairs:
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb)
        assert all(sa[k].shape == sb[k].shape for k in sa)
    # a reference Beta checkpoint loads into this package's agent
    for a, b in zip(mine.actors, theirs.actors):
        a.load_state_dict(b.state_dict())
        assert torch.equal(a.fc3.weight, b.fc3.weight)


@needs_ref
def test_adoption_keeps_the_reference_beta_head():
    import super_sac_amd as ssa
    ref = ref_harness.import_reference()
    theirs = _ref_beta_agent(ref)
    ssa.adopt.adopt_agent(theirs, torch.device("cpu"))
    for actor in theirs.actors:
        assert actor.dist_impl == "beta" and ssa.learning_utils.actor_kind(actor) == "beta"
        assert actor.action_size == 6
    assert theirs.act_space_size == 6
