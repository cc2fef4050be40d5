"""Beta-policy update cases (Agent(beta_dist=True)): the configurations tools/gen_beta_golden.py drove the reference with to
write tests/golden/beta_*.npz, and that tests/test_hip_beta_parity.py replays on the engine.  Keys as in synth.CASES;
"actor" names the seeded-weight layout (the Beta head has the tanh-normal head's shapes), "noise_cycles" the cycles that
run with a GaussianExplorationNoise process, "bc" a trailing plain behavioural-cloning step (filter_=False)."""
import torch

import case_runner

BETA_CASES = {
    # E 1, N 2, hidden 256, B 256, PopArt off: 6 critic updates (past the recording warm-up) between actor / alpha updates,
    # then one plain-BC offline actor update
    "beta_sac": dict(obs=17, act=6, hidden=256, N=2, n=2, E=1, B=256, rows=2000, cap=4096,
                     lo=-10.0, hi=2.0, popart=False, pop=False, discrete=False,
                     actor="stochastic", gamma=0.99, lr=3e-4, alpha_lr=1e-4, init_alpha=0.1,
                     clip=None, tau=0.005, weight_type=None, temp=None, noise=None, noise_cycles=(),
                     cycles=3, utd=2, target_delay=1, seed=311, bc=True),
    # REDQ: N 10, n 2, hidden 64, PopArt + pop, critic and actor clip, exploration noise on the second cycle
    "beta_redq": dict(obs=11, act=3, hidden=64, N=10, n=2, E=1, B=64, rows=1000, cap=1024,
                      lo=-10.0, hi=2.0, popart=True, pop=True, discrete=False, popart_min_steps=2,
                      actor="stochastic", gamma=0.99, lr=3e-4, alpha_lr=1e-4, init_alpha=0.1,
                      clip=40.0, tau=0.005, weight_type=None, temp=None, noise=dict(scale=0.5, clip=0.3),
                      noise_cycles=(1,), cycles=2, utd=3, target_delay=1, seed=312, bc=False),
    # SUNRISE: E 3 with the sigmoid-of-std backup weights
    "beta_sunrise": dict(obs=11, act=3, hidden=64, N=2, n=2, E=3, B=64, rows=1000, cap=1024,
                         lo=-10.0, hi=2.0, popart=False, pop=False, discrete=False,
                         actor="stochastic", gamma=0.99, lr=3e-4, alpha_lr=1e-4, init_alpha=0.1,
                         clip=None, tau=0.005, weight_type="sunrise", temp=20.0, noise=None, noise_cycles=(),
                         cycles=2, utd=2, target_delay=1, seed=313, bc=False),
}


def build_beta_agent(ssa, cfg, device):
    """the public constructor, Agent(beta_dist=True), holding the fixtures' seeded weights"""
    oa = case_runner._oracle_agent(cfg)
    ag = ssa.Agent(act_space_size=cfg["act"], encoder=ssa.nets.IdentityEncoder(cfg["obs"]),
                   actor_network_cls=ssa.nets.ContinuousStochasticActor, critic_network_cls=ssa.nets.ContinuousCritic,
                   discrete=False, ensemble_size=cfg["E"], num_critics=cfg["N"], ucb_bonus=0.0,
                   hidden_size=cfg["hidden"], auto_rescale_targets=cfg["popart"], log_std_low=cfg["lo"],
                   log_std_high=cfg["hi"], beta_dist=True)
    assert all(a.dist_impl == "beta" for a in ag.actors) and ag.inverse_model.dist_impl == "beta"

    def load(mod, p, names):
        with torch.no_grad():
            for (wk, bk), nm in zip((("w1", "b1"), ("w2", "b2"), ("w3", "b3")), names):
                getattr(mod, nm).weight.copy_(p[wk])
                getattr(mod, nm).bias.copy_(p[bk])
    for i in range(cfg["E"]):
        load(ag.actors[i], oa.actors[i], ("fc1", "fc2", "fc3"))
        for j in range(cfg["N"]):
            load(ag.critics[i].nets[j], oa.critics[i][j], ("fc1", "fc2", "out"))
    ag.to(device)
    if cfg["popart"]:
        for p in ag.popart:
            p.min_steps = cfg.get("popart_min_steps", 1000)
    ag.train()
    return ag
