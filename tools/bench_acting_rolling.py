"""Time the acting calls of pixel agents as the training loop makes them (profiles/acting_rolling.md) on the MI355X.

    python tools/bench_acting_rolling.py [--general] [--package-root DIR] [--calls 1000] [--repeats 7] [--warmup 300]

Four rows, one environment each, host to host (frames in, action out):
    atari_sample_rolling      sample_action(uint8 4 x 84 x 84, rolling=True): SmallPixelEncoder (emb 128), discrete actor, 6 actions
    dmc_sample_rolling        sample_action(uint8 9 x 84 x 84, rolling=True): BigPixelEncoder (emb 50), deterministic actor, hidden 1024
    atari_forward_rolling     forward(..., rolling=True) of the first agent (what evaluation.run_env calls)
    atari_sample_float32      the first row with the frames handed over as float32 (acting.FLOAT32_FRAMES = True)
Method (the one of profiles/acting_rules.md): `warmup` calls, then `repeats` repeats of `calls` calls, wall clock per repeat over
the calls; median, min and max of the repeats.  One process per column: --general switches the recorded path off
(acting.ENABLED = False); --package-root imports super_sac_amd from another checkout (the parent commit's build).  Every row
says whether a plan of the agent was present in acting._PLANS afterwards.  One JSON line on stdout.
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--general", action="store_true")
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=300)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import numpy as np
    import torch
    import super_sac_amd as ssa
    from super_sac_amd import acting
    assert torch.cuda.is_available(), "needs the MI355X"
    assert os.path.abspath(ssa.__file__).startswith(os.path.abspath(args.package_root))
    acting.ENABLED = not args.general
    acting.FLOAT32_FRAMES = True          # (the last row's switch; a checkout from before it existed ignores the name)
    dev = torch.device("cuda")
    torch.manual_seed(0)
    N = ssa.nets

    def agent(conv, actor_cls, critic_cls, discrete, hidden, act):
        a = ssa.Agent(act_space_size=act, encoder=N.PixelEncoder(conv), actor_network_cls=actor_cls, critic_network_cls=critic_cls,
                      discrete=discrete, ensemble_size=1, num_critics=2, hidden_size=hidden, auto_rescale_targets=False)
        a.to(dev)
        return a
    atari = agent(N.SmallPixelEncoder((4, 84, 84), 128), N.DiscreteActor, N.DiscreteCritic, True, 256, 6)
    dmc = agent(N.BigPixelEncoder((9, 84, 84), 50), N.ContinuousDeterministicActor, N.ContinuousCritic, False, 1024, 6)
    rs = np.random.RandomState(0)
    f_atari = rs.randint(0, 256, (4, 84, 84)).astype(np.uint8)
    f_dmc = rs.randint(0, 256, (9, 84, 84)).astype(np.uint8)
    f_float = f_atari.astype(np.float32)
    rows = {
        "atari_sample_rolling": (atari, lambda: atari.sample_action({"obs": f_atari}, rolling=True)),
        "dmc_sample_rolling": (dmc, lambda: dmc.sample_action({"obs": f_dmc}, rolling=True)),
        "atari_forward_rolling": (atari, lambda: atari.forward({"obs": f_atari}, rolling=True)),
        "atari_sample_float32": (atari, lambda: atari.sample_action({"obs": f_float}, rolling=True)),
    }
    res = {"general": bool(args.general), "package": os.path.abspath(ssa.__file__), "calls": args.calls, "repeats": args.repeats,
           "warmup": args.warmup, "rows": {}}
    for name, (ag, fn) in rows.items():
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()                      # (host to host: the action is a numpy array when the call returns)
            ts.append((time.perf_counter() - t0) * 1e6 / args.calls)
        res["rows"][name] = {"median_us": round(statistics.median(ts), 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1),
                             "plans": sorted(str(k) for k in acting._PLANS.get(ag, {}))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
