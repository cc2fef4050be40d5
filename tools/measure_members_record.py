"""GPU: the figures of profiles/members_record.md -- critic updates of agents with ensemble_size > 1 (SUNRISE), this
checkout against another one (the parent commit: there such updates never leave the eager path).

Shapes (obs 17, hidden 256, B 256, E 5, N 2, n 2, replay 8 192 rows): sunrise_gin (experiments/gym/sunrise.gin: tanh-normal
actors, act 6, "sunrise" weights at temperature 20), sunrise_unweighted (the same, weight_type None), sunrise_discrete
(categorical actors with 2 SAC-Discrete critics per member and 4 actions -- the heads of bench.py's discrete acting row --
on vector observations, "sunrise" weights).  One update = critic_update + a Polyak step of EVERY member behind every
second one.  Stock generators.

Method: that of tools/measure_explore_record.py, whose driver loop this tool runs with its own workers -- one worker
process per column, alive for the whole run, the columns taking turns window by window, 300 warm-up updates, 7 windows of
at least 0.5 s each ending in a device synchronise, median and min .. max in microseconds per update; launches per update
counted with ssac_launch_list_size (the recorded list, or one eager update recorded for the count).  A tree given as
PATH@per-member runs with learning_utils.PACKED_WEIGHTS = False: the column that separates what recording buys from what
the packed weight launch buys.

    python tools/measure_members_record.py --trees parent=<parent checkout> new=. per_member=.@per-member [--out FILE.json]
    python tools/measure_members_record.py --worker --tree PATH[@per-member]        (started by the driver)
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

# name -> (actor kind, action size, weight_type)
SHAPES = {"sunrise_gin": ("stochastic", 6, "sunrise"), "sunrise_unweighted": ("stochastic", 6, None),
          "sunrise_discrete": ("discrete", 4, "sunrise")}
OBS, HIDDEN, B, ROWS = base.OBS, base.HIDDEN, base.B, base.ROWS
E, N, N_SUB, TEMP = 5, 2, 2, 20.0


def _worker(tree):
    tree, _, mode = tree.partition("@")
    tree = os.path.abspath(tree)
    for p in (os.path.join(tree, "tests"), tree):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import super_sac_amd as ssa
    assert os.path.dirname(os.path.dirname(os.path.abspath(ssa.__file__))) == tree, "imported another checkout"
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    if mode == "per-member":
        assert hasattr(ssa.learning_utils, "PACKED_WEIGHTS"), "this checkout has no packed weight form to switch off"
        ssa.learning_utils.PACKED_WEIGHTS = False
    dev = torch.device("cuda")
    lib = ssa._lib.lib

    def make(kind, act_dim, weight_type):
        torch.manual_seed(1); np.random.seed(1)
        rs = np.random.RandomState(0)
        discrete = kind == "discrete"
        act = (rs.randint(0, act_dim, size=(ROWS, 1)).astype(np.float32) if discrete
               else rs.uniform(-1, 1, (ROWS, act_dim)).astype(np.float32))
        buf = ssa.replay.ReplayBuffer(ROWS, device=dev)
        buf.load_experience({"obs": rs.standard_normal((ROWS, OBS)).astype(np.float32)}, act,
                            rs.standard_normal(ROWS).astype(np.float32),
                            {"obs": rs.standard_normal((ROWS, OBS)).astype(np.float32)}, rs.uniform(size=ROWS) < 0.01)
        ag = ssa.Agent(act_space_size=act_dim, encoder=ssa.nets.IdentityEncoder(OBS),
                       actor_network_cls=ssa.nets.DiscreteActor if discrete else ssa.nets.ContinuousStochasticActor,
                       critic_network_cls=ssa.nets.DiscreteCritic if discrete else ssa.nets.ContinuousCritic,
                       discrete=discrete, ensemble_size=E, num_critics=N, hidden_size=HIDDEN, auto_rescale_targets=False,
                       log_std_low=-5.0, log_std_high=2.0)
        ag.to(dev)
        tg = copy.deepcopy(ag)
        copt = torch.optim.Adam(chain(*(c.parameters() for c in ag.critics)), lr=3e-4)
        eopt = torch.optim.Adam(ag.encoder.parameters(), lr=1e-4)
        las = []
        for _ in range(E):
            la = torch.Tensor([math.log(0.1)]).to(dev); la.requires_grad = True
            las.append(la)
        aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(B)])
        count = [0]

        def update():
            ssa.learning.critic_update(
                buffer=buf, agent=ag, target_agent=tg, critic_optimizer=copt, encoder_optimizer=eopt, log_alphas=las,
                batch_size=B, gamma=0.99, critic_clip=None, encoder_clip=None, target_critic_ensemble_n=N_SUB,
                weighted_bellman_temp=TEMP if weight_type else None, weight_type=weight_type, pop=False, augmenter=aug,
                encoder_lambda=0, aug_mix=0.0, discrete=discrete, random_process=None, noise_clip=None, per=False,
                update_priorities=False, dr3_coeff=0.0)
            count[0] += 1
            if count[0] % 2 == 0:
                for i in range(E):
                    ssa.learning_utils.soft_update(tg.critics[i], ag.critics[i], 0.005)
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
            n_upd = 100
            while window(update, n_upd) < base.MIN_WINDOW_S:
                n_upd *= 2
            recs = list(ag.__dict__.get("_ssac_graphs", {}).values())
            recorded = bool(recs) and recs[0].graph is not None
            path = recs[0].path if recorded else "eager"
            if recorded:
                launches = sum(lib.ssac_launch_list_size(p_) for p_ in recs[0].graph.parts)
            else:
                # (nothing was recorded: count the library launches of one eager update by recording it; its torch
                # kernels -- the index uploads, the fresh weight tensors -- are not in this count)
                ssa._lib.check(lib.ssac_record_begin())
                try:
                    update()
                finally:
                    h = lib.ssac_record_end()
                launches = lib.ssac_launch_list_size(h)
                lib.ssac_launch_list_free(h)
            state[name] = (update, n_upd)
            print(json.dumps({"shape": name, "recorded": recorded, "path": path, "launches": launches,
                              "window_updates": n_upd, "device": torch.cuda.get_device_name(0)}), flush=True)
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
