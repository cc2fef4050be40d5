"""GPU: Beta-policy update sequences (Agent(beta_dist=True)) against the reference's own numbers (tests/golden/beta_*.npz,
written by tools/gen_beta_golden.py from the unmodified reference): critic updates (TD target through the Beta head's
sample and log-density, REDQ subsets, PopArt, clip, exploration noise), online actor updates, temperature updates and a
plain behavioural-cloning step, with the reference's recorded draws injected (rng.draw_beta_into for the Beta x).
Checked by case_runner.compare at its default tolerances."""
import copy
import math
import types
from itertools import chain

import numpy as np
import pytest
import torch

import case_runner
from beta_cases import BETA_CASES, build_beta_agent

pytestmark = pytest.mark.gpu
DEV = "cuda"


def run_engine_beta(ssa, name, device=DEV):
    cfg = BETA_CASES[name]
    fx = case_runner.load_fixture(name)
    B, E = cfg["B"], cfg["E"]
    device = torch.device(device)
    buf = ssa.replay.ReplayBuffer(cfg["cap"], device=device)
    buf.load_experience(*case_runner._buffers(cfg))
    agent = build_beta_agent(ssa, cfg, device)
    target = copy.deepcopy(agent)
    copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=cfg["lr"], betas=(0.9, 0.999))
    aopt = torch.optim.Adam(chain(*(a.parameters() for a in agent.actors)), lr=cfg["lr"], betas=(0.9, 0.999))
    eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4, betas=(0.9, 0.999))
    las, lopts = [], []
    for _ in range(E):
        la = torch.Tensor([math.log(cfg["init_alpha"])]).to(device)
        la.requires_grad = True
        las.append(la)
        lopts.append(torch.optim.Adam([la], lr=cfg["alpha_lr"], betas=(0.5, 0.999)))
    aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(B)])
    rproc = None
    if cfg["noise"]:
        space = types.SimpleNamespace(low=-np.ones(cfg["act"], np.float32), high=np.ones(cfg["act"], np.float32))
        rproc = ssa.learning_utils.GaussianExplorationNoise(space, start_scale=cfg["noise"]["scale"],
                                                            final_scale=cfg["noise"]["scale"] * 0.1, steps_annealed=1000)
    player = case_runner.DrawPlayer(device)
    player.install(ssa.rng)
    betas = []
    saved_beta = ssa.rng.draw_beta_into
    ssa.rng.draw_beta_into = lambda dst: dst.copy_(torch.from_numpy(betas.pop(0)))
    rec, upd = {}, 0
    try:
        for cyc in range(cfg["cycles"]):
            rp = rproc if cyc in cfg["noise_cycles"] else None
            nclip = cfg["noise"]["clip"] if rp is not None else None
            for k in range(cfg["utd"]):
                for i in range(E):
                    player.idx.append(fx[f"u{upd}_idx{i}"])
                    player.sub.append(fx[f"u{upd}_subset{i}"])
                    betas.append(fx[f"u{upd}_eps{i}"])
                    if rp is not None:
                        player.normal.append(fx[f"u{upd}_noise{i}"])
                player.picks.append(int(fx[f"u{upd}_gpick"]))
                logs, dicts = ssa.learning.critic_update(
                    buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt,
                    log_alphas=las, batch_size=B, gamma=cfg["gamma"], critic_clip=cfg["clip"], encoder_clip=cfg["clip"],
                    target_critic_ensemble_n=cfg["n"], weighted_bellman_temp=cfg["temp"],
                    weight_type=cfg["weight_type"], pop=cfg["pop"], augmenter=aug, encoder_lambda=0, aug_mix=0.0,
                    discrete=False, random_process=rp, noise_clip=nclip, per=False, update_priorities=False,
                    dr3_coeff=0.0)
                for i in range(E):
                    assert np.array_equal(dicts[i]["priority_idxs"], fx[f"u{upd}_idx{i}"])
                    rec[f"u{upd}_td{i}"] = dicts[i]["td_target"].cpu().numpy()
                    if cfg["popart"]:
                        p = agent.popart[i]._read()
                        rec[f"u{upd}_popart{i}"] = np.array([p.mu, p.nu, p.w, p.b, agent.popart[i].sigma, p.t])
                for key, val in logs.items():
                    rec[f"u{upd}_log:{key}"] = np.float64(float(val))
                if int(fx[f"u{upd}_polyak"]):
                    for ac, tc in zip(agent.critics, target.critics):
                        ssa.learning_utils.soft_update(tc, ac, cfg["tau"])
                upd += 1
            for i in range(E):
                betas.append(fx[f"a{cyc}_eps{i}"])
                if rp is not None:
                    player.normal.append(fx[f"a{cyc}_noise{i}"])
            player.picks.append(int(fx[f"a{cyc}_gpick"]))
            alog = ssa.learning.online_actor_update(
                buffer=buf, agent=agent, pop=cfg["pop"], actor_optimizer=aopt, log_alphas=las, batch_size=B,
                aug_mix=0.0, clip=cfg["clip"], augmenter=aug, per=False, discrete=False, random_process=rp,
                noise_clip=nclip, premade_replay_dicts=dicts, use_baseline=False)
            for key, val in alog.items():
                rec[f"a{cyc}_log:{key}"] = np.float64(float(val))
            for i in range(E):
                betas.append(fx[f"l{cyc}_eps{i}"])
            llog = ssa.learning.alpha_update(
                buffer=buf, agent=agent, optimizers=lopts, batch_size=B, log_alphas=las, augmenter=aug, aug_mix=0.0,
                target_entropy=-float(cfg["act"]), premade_replay_dicts=dicts, discrete=False)
            for key, val in llog.items():
                rec[f"l{cyc}_log:{key}"] = np.float64(float(val))
        if cfg["bc"]:
            for i in range(E):
                player.idx.append(fx[f"s0_idx{i}"])
            player.picks.append(int(fx["s0_gpick"]))
            blog = ssa.learning.offline_actor_update(
                buffer=buf, agent=agent, actor_optimizer=aopt, encoder_optimizer=eopt, batch_size=B,
                actor_clip=cfg["clip"], update_encoder=False, encoder_clip=None, augmenter=aug, actor_lambda=0.0,
                aug_mix=0.0, per=False, discrete=False, filter_=False)
            for key, val in blog.items():
                rec[f"s0_log:{key}"] = np.float64(float(val))
        assert not player.idx and not player.sub and not player.normal and not player.picks and not betas, \
            "unconsumed recorded draws"
    finally:
        player.restore()
        ssa.rng.draw_beta_into = saved_beta
    NL = agent.num_critics
    crit = [p for i in range(E) for j in range(NL) for p in agent.critics[i].nets[j].parameters()]
    tcrit = [p for i in range(E) for j in range(NL) for p in target.critics[i].nets[j].parameters()]
    act = [p for i in range(E) for p in agent.actors[i].parameters()]
    grp = copt._ssac_adam
    m_list, v_list = [], []
    for i in range(E):
        ar = agent.critics[i].arena(device)
        m, v = grp.moments_for(("critic", i), ar.params)
        for j in range(NL):
            for seg in ("w1", "b1", "w2", "b2", "w3", "b3"):
                m_list.append(ar.view(j, seg, m))
                v_list.append(ar.view(j, seg, v))
    case_runner._finalise(rec, fx, crit, act, tcrit, m_list, v_list, las)
    return rec, agent


@pytest.mark.parametrize("name", sorted(BETA_CASES))
def test_beta_update_sequences_against_reference_fixtures(name):
    import super_sac_amd as ssa
    rec, agent = run_engine_beta(ssa, name)
    worst = case_runner.compare(rec, case_runner.load_fixture(name), who=f"beta/{name}")
    print(name, worst)
    # the per-layer path ran: nothing was recorded
    assert not agent.__dict__.get("_ssac_graphs") and not agent.__dict__.get("_ssac_actor_rec")
