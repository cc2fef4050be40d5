"""GPU: the figures of profiles/priority_record.md -- critic updates that refresh the replay priorities
(update_priorities=True: every step of awac.gin / awac_discrete.gin, every config's offline phase), this checkout against
another one (the parent commit: there such updates never leave the eager path).

Shapes (obs 17, act 6, hidden 256, B 256, replay 8 192 rows): awac (tanh-normal actor + process, N 2, n 2),
awac_discrete (categorical actor, 2 SAC-Discrete critics), td3_offline (deterministic actor, no process, N 2, n 2).
One update = critic_update(update_priorities=True) + a Polyak step behind every second one; the process's scale is
annealed before every update as the acting loop does.

Method: that of tools/measure_explore_record.py, whose driver loop this tool runs with its own workers -- one worker
process per checkout, alive for the whole run, the checkouts taking turns window by window, 7 windows each, median and
min .. max in microseconds per update; launches per update counted by recording (ssac_launch_list_size).

    python tools/measure_priority_record.py --trees NAME=PATH [NAME=PATH ...] [--out FILE.json]
    python tools/measure_priority_record.py --worker --tree PATH        (started by the driver)
"""
import argparse
import copy
import json
import math
import os
import sys
import time
from itertools import chain

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measure_explore_record as base  # noqa: E402

# name -> (actor kind, N, n, with an exploration process)
SHAPES = {"awac": ("stochastic", 2, 2, True), "awac_discrete": ("discrete", 2, 2, False),
          "td3_offline": ("deterministic", 2, 2, False)}
OBS, ACT, HIDDEN, B, ROWS = base.OBS, base.ACT, base.HIDDEN, base.B, base.ROWS


def _worker(tree):
    tree = os.path.abspath(tree)
    for p in (os.path.join(tree, "tests"), tree):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import super_sac_amd as ssa
    assert os.path.dirname(os.path.dirname(os.path.abspath(ssa.__file__))) == tree, "imported another checkout"
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda")
    lib = ssa._lib.lib

    def make(kind, N, n, process):
        torch.manual_seed(1); np.random.seed(1)
        rs = np.random.RandomState(0)
        discrete = kind == "discrete"
        act = (rs.randint(0, ACT, size=(ROWS, 1)).astype(np.float32) if discrete
               else rs.uniform(-1, 1, (ROWS, ACT)).astype(np.float32))
        buf = ssa.replay.ReplayBuffer(ROWS, device=dev)
        buf.load_experience({"obs": rs.standard_normal((ROWS, OBS)).astype(np.float32)}, act,
                            rs.standard_normal(ROWS).astype(np.float32),
                            {"obs": rs.standard_normal((ROWS, OBS)).astype(np.float32)}, rs.uniform(size=ROWS) < 0.01)
        actor_cls = {"stochastic": ssa.nets.ContinuousStochasticActor, "deterministic": ssa.nets.ContinuousDeterministicActor,
                     "discrete": ssa.nets.DiscreteActor}[kind]
        ag = ssa.Agent(act_space_size=ACT, encoder=ssa.nets.IdentityEncoder(OBS), actor_network_cls=actor_cls,
                       critic_network_cls=ssa.nets.DiscreteCritic if discrete else ssa.nets.ContinuousCritic,
                       discrete=discrete, ensemble_size=1, num_critics=N, hidden_size=HIDDEN, auto_rescale_targets=False,
                       log_std_low=-5.0, log_std_high=2.0)
        ag.to(dev)
        tg = copy.deepcopy(ag)
        copt = torch.optim.Adam(chain(*(c.parameters() for c in ag.critics)), lr=3e-4)
        eopt = torch.optim.Adam(ag.encoder.parameters(), lr=1e-4)
        la = torch.Tensor([math.log(0.1)]).to(dev); la.requires_grad = True
        aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(B)])
        rp = None
        if process:
            space = type("Space", (), {})()
            space.low, space.high = -np.ones(ACT, np.float32), np.ones(ACT, np.float32)
            rp = ssa.learning_utils.GaussianExplorationNoise(space, start_scale=1.0, final_scale=0.1, steps_annealed=1000000)
        count = [0]

        def update():
            if rp is not None:
                rp.current_scale = max(rp.current_scale - 1e-6, 0.1)
            ssa.learning.critic_update(
                buffer=buf, agent=ag, target_agent=tg, critic_optimizer=copt, encoder_optimizer=eopt, log_alphas=[la],
                batch_size=B, gamma=0.99, critic_clip=None, encoder_clip=None, target_critic_ensemble_n=n,
                weighted_bellman_temp=None, weight_type=None, pop=False, augmenter=aug, encoder_lambda=0, aug_mix=0.0,
                discrete=discrete, random_process=rp, noise_clip=0.3 if process else None, per=False,
                update_priorities=True, dr3_coeff=0.0)
            count[0] += 1
            if count[0] % 2 == 0:
                ssa.learning_utils.soft_update(tg.critics[0], ag.critics[0], 0.005)
        return ag, update

    def window(update, n_upd):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_upd):
            update()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    state = {}
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        name = cmd[1]
        if cmd[0] == "setup":
            ag, update = make(*SHAPES[name])
            for _ in range(base.WARM_UPDATES):
                update()
            n_upd = 200
            while window(update, n_upd) < base.MIN_WINDOW_S:
                n_upd *= 2
            recs = list(ag.__dict__.get("_ssac_graphs", {}).values())
            recorded = bool(recs) and recs[0].graph is not None
            if recorded:
                launches = sum(lib.ssac_launch_list_size(p_) for p_ in recs[0].graph.parts)
            else:
                # (nothing was recorded: count the library launches of one eager update by recording it; the torch
                # kernels of the eager refresh -- copies, randn, the index upload -- are not in this count)
                ssa._lib.check(lib.ssac_record_begin())
                try:
                    update()
                finally:
                    h = lib.ssac_record_end()
                launches = lib.ssac_launch_list_size(h)
                lib.ssac_launch_list_free(h)
            state[name] = (update, n_upd)
            print(json.dumps({"shape": name, "recorded": recorded, "launches": launches, "window_updates": n_upd,
                              "device": torch.cuda.get_device_name(0)}), flush=True)
        elif cmd[0] == "window":
            update, n_upd = state[name]
            print(json.dumps({"shape": name, "us": window(update, n_upd) * 1e6 / n_upd}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--trees", nargs="+", metavar="NAME=PATH", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return _worker(args.tree)
    trees = [tuple(t.split("=", 1)) for t in (args.trees or [f"this={args.tree}"])]
    base._driver(trees, args.out, script=__file__, shapes=SHAPES)


if __name__ == "__main__":
    main()
