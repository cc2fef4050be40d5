"""GPU: the figures of profiles/concat_encoder.md -- an agent with a concatenating encoder over a three-key dictionary
buffer against its single-key twin, recorded critic update per call and acting per step.

Shapes (obs 17 split (10, 4, 3), act 6, hidden 256, B 256): sac (N 2, n 2: sac.gin's critic count) and redq (N 10, n 2:
redq.gin's).  Columns: the concat agent; the single-key twin with the replay gather folded into the chained launch
(learning_utils.FOLD_GATHER = True, the default) and with the gather as a launch of its own (False) -- the form the concat
agent's update has by construction.  One update = critic_update + a Polyak step behind every second one.  The switch is
read while a call form is being recorded, so each column records under its own setting and the windows then replay.

Method (that of tools/measure_explore_record.py, in one process since every column is this checkout): the columns take
turns window by window, so drift of the machine hits all alike.  A window is a host clock around WINDOW updates
(calibrated per column so that a window takes at least MIN_WINDOW_S) that ends in a device synchronise; per column the
median and min .. max over ROUNDS windows, in microseconds per update.  Launches per update: ssac_launch_list_size of the
recorded list.

Acting: Agent.sample_action and Agent.forward on numpy observations, one environment, per step: the concat agent's
recorded plan, the single-key twin's plan, and the concat agent on the general path (acting.ENABLED = False: torch.cat in
the encoder, per-layer launches, a device -> host copy).  Same alternation, windows of ACT_STEPS steps.

    python tools/measure_concat_encoder.py [--out FILE.json]
"""
import argparse
import copy
import json
import math
import os
import statistics
import sys
import time
from itertools import chain

ROUNDS, MIN_WINDOW_S, WARM_UPDATES, ACT_STEPS = 7, 0.5, 300, 4000
SHAPES = {"sac": (2, 2), "redq": (10, 2)}
WIDTHS = (("observation", 10), ("desired_goal", 4), ("task", 3))
ORDER = ("desired_goal", "observation", "task")   # the encoder's column order (not the storage's)
OBS, ACT, HIDDEN, B, ROWS = 17, 6, 256, 256, 8192


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import super_sac_amd as ssa
    from super_sac_amd import acting
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev, lib, lu = torch.device("cuda"), ssa._lib.lib, ssa.learning_utils

    def split(rows):
        out, c0 = {}, 0
        cols = {}
        for k in ORDER:
            w = dict(WIDTHS)[k]
            cols[k] = (c0, c0 + w)
            c0 += w
        for k, _ in WIDTHS:
            out[k] = np.ascontiguousarray(rows[..., cols[k][0]:cols[k][1]])
        return out

    def make(concat, N, n):
        torch.manual_seed(1); np.random.seed(1)
        rs = np.random.RandomState(0)
        s, s1 = rs.standard_normal((ROWS, OBS)).astype(np.float32), rs.standard_normal((ROWS, OBS)).astype(np.float32)
        buf = ssa.replay.ReplayBuffer(ROWS, device=dev)
        buf.load_experience(split(s) if concat else {"obs": s}, rs.uniform(-1, 1, (ROWS, ACT)).astype(np.float32),
                            rs.standard_normal(ROWS).astype(np.float32), split(s1) if concat else {"obs": s1},
                            rs.uniform(size=ROWS) < 0.01)
        enc = ssa.nets.ConcatEncoder(dict(WIDTHS), order=ORDER) if concat else ssa.nets.IdentityEncoder(OBS)
        ag = ssa.Agent(act_space_size=ACT, encoder=enc, actor_network_cls=ssa.nets.ContinuousStochasticActor,
                       critic_network_cls=ssa.nets.ContinuousCritic, ensemble_size=1, num_critics=N, hidden_size=HIDDEN,
                       auto_rescale_targets=False, log_std_low=-5.0, log_std_high=2.0)
        ag.to(dev)
        tg = copy.deepcopy(ag)
        copt = torch.optim.Adam(chain(*(c.parameters() for c in ag.critics)), lr=3e-4)
        eopt = torch.optim.Adam(ag.encoder.parameters(), lr=1e-4)
        la = torch.Tensor([math.log(0.1)]).to(dev); la.requires_grad = True
        aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(B)])
        count = [0]

        def update():
            ssa.learning.critic_update(
                buffer=buf, agent=ag, target_agent=tg, critic_optimizer=copt, encoder_optimizer=eopt, log_alphas=[la],
                batch_size=B, gamma=0.99, critic_clip=None, encoder_clip=None, target_critic_ensemble_n=n,
                weighted_bellman_temp=None, weight_type=None, pop=False, augmenter=aug, encoder_lambda=0, aug_mix=0.0,
                discrete=False, random_process=None, noise_clip=None, per=False, update_priorities=False, dr3_coeff=0.0)
            count[0] += 1
            if count[0] % 2 == 0:
                lu.soft_update(tg.critics[0], ag.critics[0], 0.005)
        return ag, update

    def window(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def summary(us):
        return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}

    result = {"device": torch.cuda.get_device_name(0), "updates": {}, "acting": {}}
    agents = {}
    for shape, (N, n) in SHAPES.items():
        cols = {}
        for col, concat, fold in (("concat", True, True), ("twin_fold_on", False, True), ("twin_fold_off", False, False)):
            old = lu.FOLD_GATHER
            lu.FOLD_GATHER = fold
            try:
                ag, update = make(concat, N, n)
                for _ in range(WARM_UPDATES):
                    update()
            finally:
                lu.FOLD_GATHER = old
            n_upd = 200
            while window(update, n_upd) < MIN_WINDOW_S:
                n_upd *= 2
            rec, = ag.__dict__["_ssac_graphs"].values()
            assert rec.path == "fast", (shape, col, rec.path)
            cols[col] = dict(update=update, n=n_upd, us=[], launches=sum(lib.ssac_launch_list_size(p_) for p_ in rec.graph.parts))
            agents[(shape, col)] = ag
        for _ in range(ROUNDS):
            for col, c in cols.items():
                c["us"].append(window(c["update"], c["n"]) * 1e6 / c["n"])
        result["updates"][shape] = {col: dict(summary(c["us"]), launches=c["launches"], window_updates=c["n"])
                                    for col, c in cols.items()}
        print(json.dumps({shape: result["updates"][shape]}), flush=True)

    # ---- acting, one environment
    rs = np.random.RandomState(3)
    obs = rs.standard_normal((64, OBS)).astype(np.float32)
    one = [{"obs": o} for o in obs]
    three = [split(o) for o in obs]
    cag, iag = agents[("sac", "concat")], agents[("sac", "twin_fold_on")]
    for rule in ("sample_action", "forward"):
        def stepper(ag, seq, enabled):
            k = [0]

            def step():
                acting.ENABLED = enabled
                getattr(ag, rule)(seq[k[0] & 63], num_envs=1)
                k[0] += 1
            return step
        cols = {"concat_plan": stepper(cag, three, True), "twin_plan": stepper(iag, one, True),
                "concat_general_path": stepper(cag, three, False)}
        us = {col: [] for col in cols}
        try:
            for fn in cols.values():
                window(fn, 200)
            for _ in range(ROUNDS):
                for col, fn in cols.items():
                    us[col].append(window(fn, ACT_STEPS) * 1e6 / ACT_STEPS)
        finally:
            acting.ENABLED = True
        assert (acting._PLANS.get(cag) or {}) and not acting._FAILED.get(cag)
        result["acting"][rule] = {col: summary(v) for col, v in us.items()}
        print(json.dumps({rule: result["acting"][rule]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
