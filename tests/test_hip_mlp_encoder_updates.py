"""GPU: the update functions with a trainable two-layer MLP encoder against the reference's arithmetic
(oracle/ssac_oracle.py on the CPU, its ``encode`` replaced through monkeypatch by one that knows the encoder kind "mlp2";
the oracle module itself is untouched).  Every oracle entry point used here -- critic_update, online_actor_update,
alpha_update, offline_actor_update, markov_state_abstraction_update -- could be driven that way; none is restated.

Host draws (replay indices, policy noise, REDQ subset, permutation, logged-member picks) are injected through the hooks of
super_sac_amd.rng (case_runner.DrawPlayer).  Each configuration runs three consecutive rounds, so Adam state and the target
encoder matter.  Seeds: mlp_encoder_cases.CONFIGS (vetted on the CPU by tools/vet_mlp_encoder_seeds.py: the oracle alone, fp32
against fp64, stays inside the straggler cap on every encoder tensor -- seeds 3, 4, 5 and 6 all did, worst element 1.1e-5).
"""
import copy

import numpy as np
import pytest
import torch

import mlp_encoder_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture
def orc(monkeypatch):
    import ssac_oracle
    monkeypatch.setattr(ssac_oracle, "encode", mc.patched_encode(ssac_oracle))
    return ssac_oracle


_ORACLE = {}


def _reference(orc, name, mode, **kw):
    """the oracle's record of a configuration: computed once, shared, never modified"""
    key = (name, mode, tuple(sorted(kw.items())))
    if key not in _ORACLE:
        _ORACLE[key] = mc.run_oracle(orc, mc.CONFIGS[name], mode, **kw)
    return _ORACLE[key]


def _bound_engine(encoder):
    from super_sac_amd import mlp_encoder as me
    eng = encoder.__dict__.get("_ssac_mlp")
    assert eng is not None and eng.is_bound() and me.is_mlp_encoder(encoder)
    return eng


@pytest.mark.parametrize("own", [False, True], ids=["adopted", "ssa.nets.MlpEncoder"])
@pytest.mark.parametrize("name", ["sac", "ensemble"])
def test_sac_sequence(orc, name, own):
    """critic, actor, alpha, soft_update of critics and encoder, three times (ensemble: one encoder step behind the
    last member, the members' gradients accumulated)"""
    ref = _reference(orc, name, "sac")
    run = mc.EngineRun(orc, mc.CONFIGS[name], "sac", own=own)
    for k in range(mc.STEPS):
        run.step(k)
    rec = run.finish()
    print(mc.compare(rec, ref, f"{name} sequence"))
    # the online and the target encoder each have an engine of their own, bound to their own parameters
    eng, teng = _bound_engine(run.agent.encoder), _bound_engine(run.target.encoder)
    assert eng is not teng and eng.flat.data_ptr() != teng.flat.data_ptr()
    # soft_update moved the target's re-pointed parameters: no longer the initial copy, not yet the online values
    w_on, w_tg = mc.encoder_tensors(run.agent.encoder)["w0"], mc.encoder_tensors(run.target.encoder)["w0"]
    assert not torch.equal(w_on, w_tg)
    run.ssa.learning_utils.hard_update(run.target.encoder, run.agent.encoder)
    assert torch.equal(w_on, w_tg) and teng.is_bound() and eng.is_bound()


@pytest.mark.parametrize("fused", ["all", False], ids=["fused", "layers"])
def test_sac_sequence_in_both_launch_forms(orc, fused):
    from super_sac_amd import mlp_encoder as me
    saved = me.USE_FUSED
    me.USE_FUSED = fused
    try:
        rec = mc.run_engine(orc, mc.CONFIGS["sac"], "sac")
    finally:
        me.USE_FUSED = saved
    mc.compare(rec, _reference(orc, "sac", "sac"), "sac sequence, " + ("fused" if fused else "per layer"))


@pytest.mark.parametrize("update_encoder", [True, False])
def test_bc(orc, update_encoder):
    """offline_actor_update(filter_=False): the BC loss trains the encoder, or only clips and logs"""
    cfg = mc.CONFIGS["sac"]
    run = mc.EngineRun(orc, cfg, "bc", update_encoder=update_encoder)
    before = {k: v.detach().clone() for k, v in mc.encoder_tensors(run.agent.encoder).items()}
    for k in range(mc.STEPS):
        run.step(k)
    rec = run.finish()
    mc.compare(rec, _reference(orc, "sac", "bc", update_encoder=update_encoder), f"bc update_encoder={update_encoder}")
    after = mc.encoder_tensors(run.agent.encoder)
    if update_encoder:
        assert not torch.equal(before["w0"], after["w0"])
    else:
        assert all(torch.equal(before[k], after[k]) for k in before), "update_encoder=False changed the encoder"


def test_visgrid_markov_then_discrete_critic(orc):
    """(18, 18) float32 observations, discrete actions: three Markov updates (stacked 2B pass), then one critic update"""
    rec = mc.run_engine(orc, mc.CONFIGS["visgrid"], "markov")
    print(mc.compare(rec, _reference(orc, "visgrid", "markov"), "visgrid markov"))


def test_continuous_markov(orc):
    rec = mc.run_engine(orc, mc.CONFIGS["sac"], "markov")
    print(mc.compare(rec, _reference(orc, "sac", "markov"), "continuous markov"))


def test_checkpoint_round_trip(orc, tmp_path):
    """two rounds, agent.save, a fresh agent's load (and the optimizers' state), the third round: equal to the
    uninterrupted run under the same bounds, with the engine bound again"""
    import super_sac_amd as ssa
    cfg = mc.CONFIGS["sac"]
    ref = _reference(orc, "sac", "sac")
    first = mc.EngineRun(orc, cfg, "sac")
    for k in range(2):
        first.step(k)
    opts = lambda r: {"critic": r.copt, "actor": r.aopt, "encoder": r.eopt, "alpha": r.lopts}
    ssa.checkpoint.save_training_state(str(tmp_path), first.agent, first.target, opts(first), first.las)
    fresh = mc.EngineRun(orc, cfg, "sac")
    with torch.no_grad():   # other weights than the seed's: everything must come from disk
        for ag in (fresh.agent, fresh.target):
            for mod in ag._modules():
                for p in mod.parameters():
                    p.add_(0.05)
    ssa.checkpoint.load_training_state(str(tmp_path), fresh.agent, fresh.target, opts(fresh), fresh.las)
    for a, b in zip(mc.encoder_tensors(first.agent.encoder).values(), mc.encoder_tensors(fresh.agent.encoder).values()):
        assert torch.equal(a, b)
    fresh.step(2)
    rec = fresh.finish()
    last = {k: v for k, v in ref.items() if k.startswith(("u2_", "a2_", "l2_", "final_"))}
    mc.compare(rec, last, "resumed run")
    _bound_engine(fresh.agent.encoder)
    _bound_engine(fresh.target.encoder)


def test_refusals(orc):
    import super_sac_amd as ssa
    cfg = mc.CONFIGS["sac"]
    run = mc.EngineRun(orc, cfg, "sac")
    run.step(0)   # (the encoder has been recognised)
    kw = dict(buffer=run.buf, agent=run.agent, target_agent=run.target, critic_optimizer=run.copt, encoder_optimizer=run.eopt,
              log_alphas=run.las, batch_size=cfg["B"], gamma=mc.GAMMA, critic_clip=None, encoder_clip=None,
              target_critic_ensemble_n=2, weighted_bellman_temp=None, weight_type=None, pop=False, augmenter=run.aug,
              random_process=None, noise_clip=None, aug_mix=0.0)
    with pytest.raises(NotImplementedError, match="encoder_lambda != 0 .* identity augmentation"):
        ssa.learning.critic_update(encoder_lambda=1.0, **kw)
    with pytest.raises(NotImplementedError, match="actor_lambda != 0 .* identity augmentation"):
        ssa.learning.offline_actor_update(
            buffer=run.buf, agent=run.agent, actor_optimizer=run.aopt, encoder_optimizer=run.eopt, batch_size=cfg["B"],
            actor_clip=None, update_encoder=True, encoder_clip=None, augmenter=run.aug, actor_lambda=1.0, aug_mix=0.0,
            per=False, filter_=False)
    low = mc.EngineRun(orc, cfg, "sac")   # (fresh agents: nothing has been stepped, the first contact recognises the encoder)
    ssa.set_precision(low.agent, "bf16")
    with pytest.raises(NotImplementedError, match="bf16.*MLP encoder"):
        ssa.learning.critic_update(encoder_lambda=0, **dict(kw, agent=low.agent, target_agent=copy.deepcopy(low.agent)))
    sharded = mc.EngineRun(orc, cfg, "sac")
    sharded.agent.ssac_shard = object()   # (what parallel.install leaves on an agent; the refusal comes before it is read)
    with pytest.raises(NotImplementedError, match="sharded agents with the MLP encoder"):
        ssa.learning.critic_update(encoder_lambda=0, **dict(kw, agent=sharded.agent, target_agent=sharded.target))
    # an encoder that is neither an identity, a pixel encoder nor a two-layer MLP is refused as before
    odd = mc.SharedEncoderLike(11, 128)
    odd.fc_extra = torch.nn.Linear(4, 4)
    odd = odd.cuda()
    with pytest.raises(NotImplementedError, match="this encoder has no HIP path"):
        ssa.learning_utils.encode(odd, {"obs": torch.zeros(2, 11, device="cuda")})
