"""GPU: the update functions with a plain conv-stack encoder (MinAtar's: raw 0/1 frames, 16 channels) against the reference's
arithmetic (oracle/ssac_oracle.py on the CPU, its ``encode`` replaced through monkeypatch by one that knows the encoder kind
"convstack"; the oracle module itself is untouched).

Shape: B 8, C 4, 10 x 10 uint8 frames, 6 discrete actions, 2 critics, hidden 64, three rounds (Adam state and the target
encoder matter), IdentityAug -- what ``augmenter = None`` becomes.  Every sequence runs in both launch forms
(conv_encoder.STACK_FUSED "all" / False), for the adopted stand-in and for ssa.nets.ConvStackEncoder.  Host draws are injected
through case_runner.DrawPlayer.  Bounds: TD targets 2e-4 * max(1, |x|), logs 5e-4, parameters 3e-5 with counted sign-flip
stragglers (at most 1 in 10^4).  Seed: conv_stack_cases.CONFIGS (3), vetted on the CPU by tools/vet_conv_stack_seeds.py: the
oracle alone, fp32 against fp64, stays inside the straggler cap on every encoder tensor.
"""
import copy

import pytest
import torch

import conv_stack_cases as cc

pytestmark = pytest.mark.gpu

FORMS = pytest.mark.parametrize("form", ["all", False], ids=["fused", "layers"])
OWN = pytest.mark.parametrize("own", [False, True], ids=["adopted", "ssa.nets.ConvStackEncoder"])
CFG = cc.CONFIGS["minatar"]


@pytest.fixture
def orc(monkeypatch):
    import ssac_oracle
    monkeypatch.setattr(ssac_oracle, "encode", cc.patched_encode(ssac_oracle))
    return ssac_oracle


@pytest.fixture
def launch_form(form):
    from super_sac_amd import conv_encoder as ce
    saved = ce.STACK_FUSED
    ce.STACK_FUSED = form
    yield form
    ce.STACK_FUSED = saved


_ORACLE = {}


def _reference(orc, mode, **kw):
    """the oracle's record: computed once, shared, never modified"""
    key = (mode, tuple(sorted(kw.items())))
    if key not in _ORACLE:
        _ORACLE[key] = cc.run_oracle(orc, CFG, mode, **kw)
    return _ORACLE[key]


def _bound_engine(encoder, form):
    eng = encoder.__dict__.get("_ssac_conv")
    assert eng is not None and eng.is_bound() and (eng.div, eng.shift) == (1.0, 0.0)
    assert eng.stack_fused(CFG["B"], 10, 10, save=True) == (form == "all")
    return eng


@OWN
@FORMS
def test_sac_sequence(orc, launch_form, own):
    """discrete critic_update (with critic_clip and encoder_clip), online_actor_update, alpha_update, soft_update of the
    critics and the encoder, three times"""
    ref = _reference(orc, "sac")
    run = cc.EngineRun(orc, CFG, "sac", own=own)
    for k in range(cc.STEPS):
        run.step(k)
    print(cc.compare(run.finish(), ref, "minatar sequence"))
    eng, teng = _bound_engine(run.agent.encoder, launch_form), _bound_engine(run.target.encoder, launch_form)
    assert eng is not teng and eng.flat.data_ptr() != teng.flat.data_ptr()
    if launch_form == "all":
        assert eng.saved["fused"], "the update did not take the fused launches"
    w_on, w_tg = run.agent.encoder.conv1.weight, run.target.encoder.conv1.weight
    assert not torch.equal(w_on, w_tg)
    run.ssa.learning_utils.hard_update(run.target.encoder, run.agent.encoder)
    assert torch.equal(w_on, w_tg) and teng.is_bound() and eng.is_bound()


@OWN
@FORMS
def test_sac_sequence_without_clips(orc, launch_form, own, monkeypatch):
    monkeypatch.setattr(cc.runner, "CRITIC_CLIP", None)
    monkeypatch.setattr(cc.runner, "ENC_CLIP", None)
    ref = cc.run_oracle(orc, CFG, "sac")
    print(cc.compare(cc.run_engine(orc, CFG, "sac", own=own), ref, "minatar sequence, no clips"))


@pytest.mark.parametrize("update_encoder", [True, False])
@OWN
@FORMS
def test_bc(orc, launch_form, own, update_encoder):
    """offline_actor_update(filter_=False): the BC loss trains the encoder, or only clips and logs"""
    run = cc.EngineRun(orc, CFG, "bc", own=own, update_encoder=update_encoder)
    before = {k: v.detach().clone() for k, v in cc.encoder_tensors(run.agent.encoder).items()}
    for k in range(cc.STEPS):
        run.step(k)
    cc.compare(run.finish(), _reference(orc, "bc", update_encoder=update_encoder), f"bc update_encoder={update_encoder}")
    after = cc.encoder_tensors(run.agent.encoder)
    if update_encoder:
        assert not torch.equal(before["w1"], after["w1"])
    else:
        assert all(torch.equal(before[k], after[k]) for k in before), "update_encoder=False changed the encoder"


@OWN
@FORMS
def test_checkpoint_round_trip(orc, launch_form, own, tmp_path):
    """two rounds, save (agent.save inside save_training_state), a fresh agent's load, the third round: equal to the
    uninterrupted run under the same bounds, with the engine bound again"""
    import super_sac_amd as ssa
    ref = _reference(orc, "sac")
    first = cc.EngineRun(orc, CFG, "sac", own=own)
    for k in range(2):
        first.step(k)
    opts = lambda r: {"critic": r.copt, "actor": r.aopt, "encoder": r.eopt, "alpha": r.lopts}
    ssa.checkpoint.save_training_state(str(tmp_path), first.agent, first.target, opts(first), first.las)
    fresh = cc.EngineRun(orc, CFG, "sac", own=own)
    with torch.no_grad():   # other weights than the seed's: everything must come from disk
        for ag in (fresh.agent, fresh.target):
            for mod in ag._modules():
                for p in mod.parameters():
                    p.add_(0.05)
    ssa.checkpoint.load_training_state(str(tmp_path), fresh.agent, fresh.target, opts(fresh), fresh.las)
    for a, b in zip(cc.encoder_tensors(first.agent.encoder).values(), cc.encoder_tensors(fresh.agent.encoder).values()):
        assert torch.equal(a, b)
    fresh.step(2)
    last = {k: v for k, v in ref.items() if k.startswith(("u2_", "a2_", "l2_", "final_"))}
    cc.compare(fresh.finish(), last, "resumed run")
    _bound_engine(fresh.agent.encoder, launch_form)
    _bound_engine(fresh.target.encoder, launch_form)
    # agent.save / agent.load by themselves
    (tmp_path / "agent").mkdir()
    first.agent.save(str(tmp_path / "agent"))
    fresh.agent.load(str(tmp_path / "agent"))
    for a, b in zip(cc.encoder_tensors(first.agent.encoder).values(), cc.encoder_tensors(fresh.agent.encoder).values()):
        assert torch.equal(a, b)


def _critic_kwargs(run):
    return dict(buffer=run.buf, agent=run.agent, target_agent=run.target, critic_optimizer=run.copt,
                encoder_optimizer=run.eopt, log_alphas=run.las, batch_size=CFG["B"], gamma=0.99, critic_clip=None,
                encoder_clip=None, target_critic_ensemble_n=2, weighted_bellman_temp=None, weight_type=None, pop=False,
                augmenter=run.aug, encoder_lambda=0, random_process=None, noise_clip=None, aug_mix=0.0, discrete=True)


@pytest.mark.parametrize("cls", [cc.SigmoidStackLike, cc.NhwcFlattenLike])
def test_a_stack_that_matches_no_candidate_is_refused(orc, cls, monkeypatch):
    """a module with conv1 and fc used to be taken for a SmallPixelEncoder (and fed x / 255)"""
    import super_sac_amd as ssa
    monkeypatch.setattr(cc.runner, "make_encoder", lambda cfg, own=False: cls(cfg["obs"][0], cfg["obs"][1:], cfg["emb"]))
    run = cc.EngineRun(orc, CFG, "sac")
    with pytest.raises(NotImplementedError, match=f"{cls.__name__}: this encoder has no HIP path"):
        ssa.learning.critic_update(**_critic_kwargs(run))


def test_bf16_and_sharded_agents_are_refused_as_for_pixel_encoders(orc):
    """the refusals an agent with a SmallPixelEncoder meets: the bf16 operand mode covers identity encoders, and a
    trainable encoder is shared by all members, so it is not sharded"""
    import types
    import super_sac_amd as ssa
    low = cc.EngineRun(orc, CFG, "sac")
    ssa.set_precision(low.agent, "bf16")
    low.target = copy.deepcopy(low.agent)
    with pytest.raises(NotImplementedError, match="bf16 mode"):
        ssa.learning.critic_update(**_critic_kwargs(low))
    sharded = cc.EngineRun(orc, CFG, "sac")
    sharded.agent.ssac_member_shard = types.SimpleNamespace(ensemble_size=2, lo=0, hi=1)   # (what parallel.install leaves)
    with pytest.raises(AssertionError, match="a trainable encoder is shared by all members"):
        ssa.learning.critic_update(**_critic_kwargs(sharded))


def test_the_spelling_of_the_device_does_not_repack_the_engine():
    """"cuda" and "cuda:<current>" name one device: one engine, one arena"""
    import super_sac_amd as ssa
    from super_sac_amd import conv_encoder as ce
    enc = ssa.nets.ConvStackEncoder((4, 10, 10)).cuda()
    x = (torch.rand(32, 4, 10, 10, generator=torch.Generator().manual_seed(1)) < 0.3).to(torch.uint8).cuda()
    eng = ce.conv_engine(enc, torch.device("cuda"))
    ptr, out = eng.flat.data_ptr(), enc({"obs": x})
    indexed = ce.conv_engine(enc, torch.device("cuda", torch.cuda.current_device()))
    assert indexed is eng and indexed.flat.data_ptr() == ptr and eng.is_bound()
    assert ce.conv_engine(enc, torch.device("cuda")) is eng and ce.conv_engine(enc, "cuda") is eng
    assert enc.__dict__["_ssac_conv"] is eng and torch.equal(enc({"obs": x}), out)


def test_a_copied_pixel_encoder_forwards_through_an_engine_of_its_own():
    """copy.deepcopy clones the parameters out of the arena and copies the cache slot: the twin's forward re-packs instead
    of running the engine the parameters left"""
    import super_sac_amd as ssa
    conv = ssa.nets.SmallPixelEncoder((4, 36, 36)).cuda()
    x = torch.randint(0, 256, (2, 4, 36, 36), generator=torch.Generator().manual_seed(2)).float().cuda()
    out = conv(x)
    eng = conv.__dict__["_ssac_conv"]
    twin = copy.deepcopy(conv)
    assert torch.equal(twin(x), out)
    teng = twin.__dict__["_ssac_conv"]
    assert teng is not eng and teng.module is twin and teng.is_bound() and eng.is_bound()
    assert teng.flat.data_ptr() != eng.flat.data_ptr()
    with torch.no_grad():
        twin.fc.bias.add_(1.0)
        twin.conv1.weight.mul_(0.5)
    moved = twin(x)
    assert teng.is_bound() and twin.__dict__["_ssac_conv"] is teng
    assert torch.equal(teng._seg(len(teng.plist) - 1), twin.fc.bias.detach()) and not torch.equal(moved, out)
    assert torch.equal(conv(x), out), "the original answers as before"
