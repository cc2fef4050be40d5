"""GPU: the figures of profiles/explore_record.md -- critic updates that carry an exploration process, this checkout
against another one (the parent commit: there such updates never leave the eager path).

Shapes (obs 17, act 6, hidden 256, B 256): td3 (deterministic actor, N 2, n 2), ddpg (deterministic, N 1, n 1), awac
(tanh-normal actor + process, N 2, n 2).  One update = critic_update + a Polyak step behind every second one, the
process's scale annealed before every update as the acting loop does.

Method: one worker process per checkout (its own super_sac_amd and its own libssac_hip.so, built beforehand with that
checkout's build.sh), both alive for the whole run; the driver makes them take turns, shape by shape and round by round,
so drift of the machine hits both columns alike.  A window is a host clock around WINDOW_UPDATES updates (calibrated per
shape and checkout so that a window takes at least MIN_WINDOW_S) that ends in a device synchronise; per (checkout, shape)
the median and min .. max over ROUNDS windows are reported, in microseconds per update.  Clocks are whatever the device
runs at under this load.  Launches per update: the library launches of one update, counted by recording it
(ssac_launch_list_size) -- the recorded list where the update was recorded, one eager update inside
ssac_record_begin / ssac_record_end where it was not.

    python tools/measure_explore_record.py --trees NAME=PATH [NAME=PATH ...] [--out FILE.json]
    python tools/measure_explore_record.py --worker --tree PATH        (started by the driver)
"""
import argparse
import copy
import json
import math
import os
import subprocess
import sys
import time
from itertools import chain

ROUNDS, MIN_WINDOW_S, WARM_UPDATES = 7, 0.5, 300
SHAPES = {"td3": ("deterministic", 2, 2), "ddpg": ("deterministic", 1, 1), "awac": ("stochastic", 2, 2)}
OBS, ACT, HIDDEN, B, ROWS = 17, 6, 256, 256, 8192


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

    def make(kind, N, n):
        torch.manual_seed(1); np.random.seed(1)
        rs = np.random.RandomState(0)
        buf = ssa.replay.ReplayBuffer(ROWS, device=dev)
        buf.load_experience({"obs": rs.standard_normal((ROWS, OBS)).astype(np.float32)},
                            rs.uniform(-1, 1, (ROWS, ACT)).astype(np.float32), rs.standard_normal(ROWS).astype(np.float32),
                            {"obs": rs.standard_normal((ROWS, OBS)).astype(np.float32)}, rs.uniform(size=ROWS) < 0.01)
        actor_cls = ssa.nets.ContinuousStochasticActor if kind == "stochastic" else ssa.nets.ContinuousDeterministicActor
        ag = ssa.Agent(act_space_size=ACT, encoder=ssa.nets.IdentityEncoder(OBS), actor_network_cls=actor_cls,
                       critic_network_cls=ssa.nets.ContinuousCritic, ensemble_size=1, num_critics=N, hidden_size=HIDDEN,
                       auto_rescale_targets=False, log_std_low=-5.0, log_std_high=2.0)
        ag.to(dev)
        tg = copy.deepcopy(ag)
        copt = torch.optim.Adam(chain(*(c.parameters() for c in ag.critics)), lr=3e-4)
        eopt = torch.optim.Adam(ag.encoder.parameters(), lr=1e-4)
        la = torch.Tensor([math.log(0.1)]).to(dev); la.requires_grad = True
        aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(B)])
        space = type("Space", (), {})()
        space.low, space.high = -np.ones(ACT, np.float32), np.ones(ACT, np.float32)
        rp = ssa.learning_utils.GaussianExplorationNoise(space, start_scale=1.0, final_scale=0.1, steps_annealed=1000000)
        count = [0]

        def update():
            rp.current_scale = max(rp.current_scale - 1e-6, 0.1)
            ssa.learning.critic_update(
                buffer=buf, agent=ag, target_agent=tg, critic_optimizer=copt, encoder_optimizer=eopt, log_alphas=[la],
                batch_size=B, gamma=0.99, critic_clip=None, encoder_clip=None, target_critic_ensemble_n=n,
                weighted_bellman_temp=None, weight_type=None, pop=False, augmenter=aug, encoder_lambda=0, aug_mix=0.0,
                discrete=False, random_process=rp, noise_clip=0.3, per=False, update_priorities=False, dr3_coeff=0.0)
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
            for _ in range(WARM_UPDATES):
                update()
            n_upd = 200
            while window(update, n_upd) < MIN_WINDOW_S:
                n_upd *= 2
            recs = list(ag.__dict__.get("_ssac_graphs", {}).values())
            recorded = bool(recs) and recs[0].graph is not None
            if recorded:
                launches = sum(lib.ssac_launch_list_size(p_) for p_ in recs[0].graph.parts)
            else:
                # (nothing was recorded: count the library launches of one eager update by recording it)
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


def _driver(trees, out_path, script=None, shapes=None):
    """script, shapes: the worker script and its shape names (tools/measure_priority_record.py drives its own workers
    through this loop)"""
    import statistics
    here = os.path.abspath(script or __file__)
    shapes = list(shapes or SHAPES)
    procs = {}
    for name, path in trees:
        procs[name] = subprocess.Popen([sys.executable, here, "--worker", "--tree", path], stdin=subprocess.PIPE,
                                       stdout=subprocess.PIPE, text=True, bufsize=1)

    def ask(name, line):
        p = procs[name]
        p.stdin.write(line + "\n")
        p.stdin.flush()
        while True:
            reply = p.stdout.readline()
            if not reply:
                raise RuntimeError(f"the worker of {name} ended (exit status {p.wait()})")
            if reply.startswith("{"):   # (anything else is chatter of a library on the worker's stdout)
                return json.loads(reply)
    result = {"rounds": ROUNDS, "min_window_s": MIN_WINDOW_S, "shapes": {}}
    try:
        for shape in shapes:
            info = {name: ask(name, f"setup {shape}") for name, _ in trees}
            got = {name: [] for name, _ in trees}
            for _ in range(ROUNDS):
                for name, _ in trees:   # the checkouts take turns inside every round
                    got[name].append(ask(name, f"window {shape}")["us"])
            result["shapes"][shape] = {
                name: dict(info[name], median_us=statistics.median(v), min_us=min(v), max_us=max(v), windows_us=v)
                for name, v in got.items()}
            for name, r in result["shapes"][shape].items():
                print(f"{shape:13s} {name:8s} {r['median_us']:8.2f} us/update [{r['min_us']:.2f} .. {r['max_us']:.2f}]  "
                      f"recorded {r['recorded']}  launches/update {r['launches']}  window {r['window_updates']} updates",
                      flush=True)
            if out_path:
                with open(out_path, "w") as f:
                    json.dump(result, f, indent=1)
    finally:
        for p in procs.values():
            try:
                p.stdin.write("quit\n")
                p.stdin.close()
            except Exception:
                pass
        for p in procs.values():
            try:
                p.wait(timeout=60)
            except subprocess.TimeoutExpired:
                p.kill()


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
    _driver(trees, args.out)


if __name__ == "__main__":
    main()
