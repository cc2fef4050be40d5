"""Recorded critic updates that refresh the replay priorities, against the REFERENCE's numbers: oracle/ssac_oracle.py
(pinned to the reference by the fixtures under tests/golden) is driven on the CPU at test time exactly as
case_runner.run_afbc_oracle drives it for a "critic" step -- orc.critic_update, orc.advantage, orc.PerOracle,
orc.soft_update -- for GRAPH_WARMUP + 3 consecutive steps at the awac_offline shape (and the afbc_discrete shape), on
draws generated here.  The engine gets the same draws through a DrawPlayer, so its last three steps are the recording
call and two replays through the C step.  Priorities, refreshed leaves, logs and the final critic parameters are held to
the tolerances of case_runner.compare_afbc (prio_tol 2e-4 / atol 2e-6, log_rtol 5e-4, par_tol 3e-5).  The eager path on
the same draws (USE_GRAPHS off: the launches every update took before recordings carried a refresh) is held to the same
bounds at the same step count."""
import copy
import functools
import math
import random
from itertools import chain

import numpy as np
import pytest
import torch

import case_runner
import synth

orc = case_runner.orc
WARMUP = 3   # learning.GRAPH_WARMUP (asserted on the GPU)
N_STEPS = WARMUP + 3
CASES = {
    "awac_offline": dict(synth.AFBC_CASES["awac_offline"]),
    "afbc_discrete": dict(synth.AFBC_CASES["afbc_discrete"], gamma=0.99, tau=0.005, init_alpha=0.1, clip=None),
}
PRIO_TOL, PRIO_ATOL, LOG_RTOL, PAR_TOL = 2e-4, 2e-6, 5e-4, 3e-5   # case_runner.compare_afbc


@functools.lru_cache(maxsize=None)
def _draws(case):
    cfg = CASES[case]
    g = torch.Generator().manual_seed(cfg["seed"] + 500)
    py = random.Random(cfg["seed"] + 501)
    steps = []
    for _ in range(N_STEPS):
        st = dict(idx=torch.randint(cfg["rows"], (cfg["B"],), generator=g).numpy(),
                  subset=py.sample(range(cfg["N"]), cfg["n"]))
        if not cfg["discrete"]:
            st["ceps"] = torch.randn(cfg["B"], cfg["act"], generator=g).numpy()
            st["prio_eps"] = [torch.randn(cfg["B"], cfg["act"], generator=g).numpy() for _ in range(4)]
        steps.append(st)
    return steps


def _run_oracle(case):
    cfg, B = CASES[case], CASES[case]["B"]
    torch.manual_seed(cfg["seed"]); np.random.seed(cfg["seed"]); random.seed(cfg["seed"])
    obuf = orc.ReplayOracle(cfg["cap"])
    obuf.load_experience(*case_runner._buffers(cfg))
    tree = orc.PerOracle(cfg["cap"], 0.6, 1.0)
    tree.push_rows(np.arange(cfg["rows"]))
    oa = case_runner._oracle_agent(cfg)
    oa.requires_grad_(True)
    ot = oa.clone()
    copt = orc.AdamOracle(oa.critic_params(), lr=cfg["lr"])
    eopt = orc.AdamOracle(oa.encoder_params(), lr=1e-4)
    ola = torch.tensor([math.log(cfg["init_alpha"])], requires_grad=True)
    aug = orc.AugOracle("identity", B)
    rec = {}
    for k, st in enumerate(_draws(case)):
        idx = st["idx"]
        logs, odicts = orc.critic_update(
            obuf, oa, ot, copt, eopt, [ola], B, cfg["gamma"], cfg["clip"], cfg["clip"], cfg["n"], None, None, False, aug,
            aug_mix=0.0, idx_list=[idx], eps_list=None if cfg["discrete"] else [torch.from_numpy(st["ceps"])],
            subset_list=[list(st["subset"])], grad_pick=0)
        rd = odicts[-1]
        adv = orc.advantage(oa, rd["primary_batch"][0], rd["primary_batch"][1], 0,
                            None if cfg["discrete"] else [torch.from_numpy(e) for e in st["prio_eps"]])
        prio = (torch.relu(adv) + 1e-4).squeeze(1).numpy()
        tree.update(idx, prio)
        orc.soft_update(ot.critic_params(), oa.critic_params(), cfg["tau"])
        rec[f"s{k}_prio"], rec[f"s{k}_leaves"] = prio, tree.sum[tree.cap + idx].copy()
        for key, v in logs.items():
            rec[f"s{k}_log:{key}"] = np.float64(v)
    rec["final_critic"] = case_runner._flat(oa.critic_params())
    rec["final_target"] = case_runner._flat(ot.critic_params())
    rec["final_max_priority"] = np.float64(tree.max_priority)
    rec["final_tree_total"] = np.float64(tree.sum[1])
    return rec


@functools.lru_cache(maxsize=None)
def _oracle(case):
    return _run_oracle(case)   # computed once, shared, never modified


def _run_engine(case, recorded):
    import super_sac_amd as ssa
    L = ssa.learning
    assert L.GRAPH_WARMUP == WARMUP
    cfg, B, dev = CASES[case], CASES[case]["B"], torch.device("cuda")
    torch.manual_seed(cfg["seed"]); np.random.seed(cfg["seed"]); random.seed(cfg["seed"])
    buf = ssa.replay.ReplayBuffer(cfg["cap"], device=dev)
    buf.load_experience(*case_runner._buffers(cfg))
    agent = case_runner.build_engine_agent(cfg, dev)
    target = copy.deepcopy(agent)
    copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=cfg["lr"], betas=(0.9, 0.999))
    eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
    la = torch.Tensor([math.log(cfg["init_alpha"])]).to(dev)
    la.requires_grad = True
    aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(B)])
    player = case_runner.DrawPlayer(dev)
    player.install(ssa.rng)
    old = L.USE_GRAPHS
    L.USE_GRAPHS = recorded
    rec = {}
    try:
        for k, st in enumerate(_draws(case)):
            player.idx.append(st["idx"])
            if not cfg["discrete"]:
                player.normal.append(st["ceps"])
            player.sub.append(st["subset"])
            if not cfg["discrete"]:
                player.normal.extend(st["prio_eps"])
            logs, _ = L.critic_update(
                buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt,
                log_alphas=[la], batch_size=B, gamma=cfg["gamma"], critic_clip=cfg["clip"], encoder_clip=cfg["clip"],
                target_critic_ensemble_n=cfg["n"], weighted_bellman_temp=None, weight_type=None, pop=False, augmenter=aug,
                encoder_lambda=0, aug_mix=0.0, discrete=cfg["discrete"], random_process=None, noise_clip=None, per=False,
                update_priorities=True, dr3_coeff=0.0)
            assert not player.normal and not player.idx and not player.sub, "the engine consumed a different number of draws"
            ssa.learning_utils.soft_update(target.critics[0], agent.critics[0], cfg["tau"])
            # (the estimator's priority workspace: where both paths leave this update's priorities)
            prio = agent.__dict__["_ssac_ws"]._bufs[("adv.prio0", (B,), torch.float32)]
            rec[f"s{k}_prio"] = prio.cpu().numpy().astype(np.float64)
            rec[f"s{k}_leaves"] = buf._per.sum_tree[buf._per.cap + st["idx"]].copy()
            for key, v in logs.items():
                rec[f"s{k}_log:{key}"] = np.float64(float(v))
        graphs = agent.__dict__.get("_ssac_graphs") or {}
        if recorded:
            record, = graphs.values()
            assert record.refresh and record.k == N_STEPS - WARMUP and record.path == "fast" and record.fast.calls == 2
        else:
            assert not graphs
    finally:
        L.USE_GRAPHS = old
        player.restore()
    rec["final_critic"] = case_runner._flat([p for c in agent.critics for p in c.parameters()])
    rec["final_target"] = case_runner._flat([p for c in target.critics for p in c.parameters()])
    rec["final_max_priority"] = np.float64(buf._per._max_priority)
    rec["final_tree_total"] = np.float64(buf._per.sum_tree[1])
    return rec


def _compare(rec, ora, who):
    dist = {"prio": 0.0, "leaves": 0.0, "log": 0.0}
    for k in range(N_STEPS):
        for what in ("prio", "leaves"):
            got, want = rec[f"s{k}_{what}"], ora[f"s{k}_{what}"]
            dist[what] = max(dist[what], float(np.max(np.abs(got - want) / (PRIO_ATOL + PRIO_TOL * np.abs(want)))))
        for key in ora:
            if key.startswith(f"s{k}_log:"):
                assert key in rec, (who, key)
                v, r = float(rec[key]), float(ora[key])
                scale = max(1.0, abs(r)) if "gradients/" not in key else max(1e-6, abs(r))   # norms: relative
                dist["log"] = max(dist["log"], abs(v - r) / (LOG_RTOL * scale))
    dist["critic"] = float(np.abs(rec["final_critic"] - ora["final_critic"]).max()) / PAR_TOL
    dist["target"] = float(np.abs(rec["final_target"] - ora["final_target"]).max()) / PAR_TOL
    print(f"{who}: distances in units of their tolerance: " + ", ".join(f"{k_} {v_:.3f}" for k_, v_ in dist.items()))
    for k in range(N_STEPS):
        np.testing.assert_allclose(rec[f"s{k}_prio"], ora[f"s{k}_prio"], rtol=PRIO_TOL, atol=PRIO_ATOL,
                                   err_msg=f"{who} step {k}: priorities after the critic update")
        np.testing.assert_allclose(rec[f"s{k}_leaves"], ora[f"s{k}_leaves"], rtol=PRIO_TOL, atol=PRIO_ATOL,
                                   err_msg=f"{who} step {k}: refreshed leaves")
    assert dist["log"] <= 1.0, (who, "logs", dist)
    assert dist["critic"] <= 1.0 and dist["target"] <= 1.0, (who, "final parameters", dist)
    assert abs(float(rec["final_max_priority"]) - float(ora["final_max_priority"])) < 1e-6
    assert abs(float(rec["final_tree_total"]) - float(ora["final_tree_total"])) <= 1e-5 * float(ora["final_tree_total"])


@pytest.mark.parametrize("case", sorted(CASES))
def test_two_oracle_runs_agree_with_themselves(case):
    """CPU: the oracle is a function of the draws alone (nothing leaks from a global generator into its numbers)"""
    a = _oracle(case)
    random.seed(12345); torch.manual_seed(999); np.random.seed(7)
    b = _run_oracle(case)
    assert sorted(a) == sorted(b)
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    assert all(np.isfinite(np.asarray(v)).all() for v in a.values())
    assert (a[f"s{N_STEPS - 1}_prio"] > 1e-4).any() and (a[f"s{N_STEPS - 1}_prio"] == np.float32(1e-4)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["recorded", "eager"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_priority_refresh_matches_the_oracle(case, path):
    _compare(_run_engine(case, path == "recorded"), _oracle(case), f"{case}/{path}")
