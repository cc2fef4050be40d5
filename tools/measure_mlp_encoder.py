"""GPU: the figures of profiles/mlp_encoder.md.

  1. the fused MLP-encoder launches (ssac_enc_mlp2_fwd / _bwd) against the per-layer launches they replace, and against
     the same encoder as torch modules on the GPU (the reference's way), at B 256 and 512 for 17->128->17, 376->128->376
     and 324->256->2;
  2. one eager critic_update at the SAC shape (obs 17, A 6, hidden 256, 2 critics, B 256) with a SharedEncoder-shaped
     encoder beside the same call with an identity encoder: the fixed cost the encoder adds.

  3. acting (--acting): the three forward forms at 1 and 4 rows (per layer, the fused tile launch, the few-row launch
     ssac_enc_mlp2_fwd_rows), and the wall time per environment step of agent.sample_action / agent.forward with the
     recorded plan (acting.ENABLED) on and off, for a SharedEncoder-shaped SAC agent (obs 17, A 6, hidden 256) and a
     visgrid-shaped discrete agent, beside the identity-encoder plan at the same actor shape (the floor).  --steps-only
     skips the launches (the part a checkout without the few-row launch can run: its "off" row is that commit's path).

Method: device events around windows of REPS back-to-back launches after a warm-up, ROUNDS windows per form with the forms
alternating inside every round; reported per launch: median over the rounds and their min .. max (the spread a difference
has to exceed).  Clocks are whatever the device runs at under this load (not pinned); nothing else is measured in the
same process.

Steps: wall-clock windows of 200 calls with the result consumed, otherwise the same scheme.

    python tools/measure_mlp_encoder.py [out.txt] [--acting [--steps-only]]
"""
import copy
import os
import sys
import time
from itertools import chain

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

REPS, ROUNDS, WARM = 200, 9, 50
SHAPES = [(17, 128, 17, "relu"), (376, 128, 376, "relu"), (324, 256, 2, "tanh")]
ACT = {"none": 0, "relu": 1, "tanh": 2}


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps   # us per call


def compare(forms, reps=REPS):
    """{name: (median, min, max)} us per call; the forms alternate inside every round"""
    for fn in forms.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in forms}
    for _ in range(ROUNDS):
        for k, fn in forms.items():
            got[k].append(window(fn, reps))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in got.items()}


def fmt(r):
    return "  ".join(f"{k} {m:7.2f} us [{lo:.2f} .. {hi:.2f}]" for k, (m, lo, hi) in r.items())


def kernels(out):
    from super_sac_amd import engine
    from super_sac_amd._lib import check, lib
    import mlp_encoder_cases as mc
    st = engine.stream()
    for K, H, N, act in SHAPES:
        for B in (256, 512):
            g = torch.Generator().manual_seed(1)
            dev = lambda *s: torch.randn(*s, generator=g).cuda()
            X, W0, b0, W1, b1, dY = dev(B, K), dev(H, K) / K ** 0.5, dev(H), dev(N, H) / H ** 0.5, dev(N), dev(B, N)
            Hs, Y = torch.empty(B, H, device="cuda"), torch.empty(B, N, device="cuda")
            dZ1, dZ0 = torch.empty(B, N, device="cuda"), torch.empty(B, H, device="cuda")
            a = ACT[act]

            def fused_fwd():
                check(lib.ssac_enc_mlp2_fwd(X.data_ptr(), K, W0.data_ptr(), b0.data_ptr(), W1.data_ptr(), b1.data_ptr(), B, K,
                                            H, N, a, Hs.data_ptr(), Y.data_ptr(), N, st))

            def layers_fwd():
                check(lib.ssac_linear_fwd(X.data_ptr(), K, W0.data_ptr(), K, b0.data_ptr(), Hs.data_ptr(), H, B, H, K, 1, st))
                check(lib.ssac_linear_fwd(Hs.data_ptr(), H, W1.data_ptr(), H, b1.data_ptr(), Y.data_ptr(), N, B, N, H,
                                          1 if a == 1 else 0, st))
                if a == 2:
                    check(lib.ssac_enc_act_fwd(Y.data_ptr(), N, B, N, a, st))

            def fused_bwd():
                check(lib.ssac_enc_mlp2_bwd(dY.data_ptr(), N, Y.data_ptr(), N, Hs.data_ptr(), W1.data_ptr(), B, H, N, a,
                                            dZ1.data_ptr(), dZ0.data_ptr(), st))

            def layers_bwd():
                check(lib.ssac_enc_act_bwd(dY.data_ptr(), N, Y.data_ptr(), N, B, N, a, dZ1.data_ptr(), st))
                check(lib.ssac_linear_dgrad_masked(dZ1.data_ptr(), N, W1.data_ptr(), H, Hs.data_ptr(), H, dZ0.data_ptr(), H,
                                                   B, H, N, st))
            lin0, lin1 = torch.nn.Linear(K, H).cuda(), torch.nn.Linear(H, N).cuda()

            def torch_fwd():
                with torch.no_grad():
                    mc.mlp2_act(act, lin1(torch.relu(lin0(X))))

            def torch_fwd_bwd():
                y = mc.mlp2_act(act, lin1(torch.relu(lin0(X))))
                y.backward(dY)
            fused_fwd()
            out(f"{K}->{H}->{N} {act} B {B}")
            out("   forward : " + fmt(compare({"fused": fused_fwd, "per-layer": layers_fwd, "torch": torch_fwd})))
            out("   backward (no weight gradients): " + fmt(compare({"fused": fused_bwd, "per-layer": layers_bwd})))
            out("   torch forward + autograd backward (with weight gradients): " + fmt(compare({"torch": torch_fwd_bwd})))


def critic(out):
    import super_sac_amd as ssa
    import mlp_encoder_cases as mc
    ssa.learning.USE_GRAPHS = False   # the eager path on both sides (a trainable encoder never reaches the recording)
    obs, A, hidden, N, B, rows = 17, 6, 256, 2, 256, 4096
    dev = torch.device("cuda")
    rng = np.random.RandomState(0)
    data = ({"obs": rng.standard_normal((rows, obs)).astype(np.float32)}, rng.uniform(-1, 1, (rows, A)).astype(np.float32),
            rng.standard_normal(rows).astype(np.float32), {"obs": rng.standard_normal((rows, obs)).astype(np.float32)},
            rng.uniform(size=rows) < 0.01)
    calls = {}
    for name, enc in (("identity encoder", ssa.nets.IdentityEncoder(obs)), ("MLP encoder", mc.SharedEncoderLike(obs, 128))):
        buf = ssa.replay.ReplayBuffer(rows, device=dev)
        buf.load_experience(*data)
        ag = ssa.Agent(act_space_size=A, encoder=enc, actor_network_cls=ssa.nets.ContinuousStochasticActor,
                       critic_network_cls=ssa.nets.ContinuousCritic, ensemble_size=1, num_critics=N, hidden_size=hidden,
                       auto_rescale_targets=False)
        ag.to(dev)
        tg = copy.deepcopy(ag)
        copt = torch.optim.Adam(chain(*(c.parameters() for c in ag.critics)), lr=3e-4)
        eopt = torch.optim.Adam(ag.encoder.parameters(), lr=1e-4)
        la = torch.zeros(1, device=dev, requires_grad=True)
        aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(B)])

        def call(buf=buf, ag=ag, tg=tg, copt=copt, eopt=eopt, la=la, aug=aug):
            ssa.learning.critic_update(
                buffer=buf, agent=ag, target_agent=tg, critic_optimizer=copt, encoder_optimizer=eopt, log_alphas=[la],
                batch_size=B, gamma=0.99, critic_clip=10.0, encoder_clip=40.0, target_critic_ensemble_n=N,
                weighted_bellman_temp=None, weight_type=None, pop=False, augmenter=aug, encoder_lambda=0,
                random_process=None, noise_clip=None, aug_mix=0.0)
        calls[name] = call
    out(f"eager critic_update, obs {obs}, A {A}, hidden {hidden}, {N} critics, B {B} (host-bound: wall time per call)")
    out("   " + fmt(compare(calls, reps=50)))


def wall_window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e6 / reps   # us per call


def compare_wall(forms, reps=REPS):
    for fn in forms.values():
        for _ in range(WARM):
            fn()
    got = {k: [] for k in forms}
    for _ in range(ROUNDS):
        for k, fn in forms.items():
            got[k].append(wall_window(fn, reps))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in got.items()}


def acting_launches(out):
    """the three forward forms on a few rows, as a plan would record them (no H_save)"""
    from super_sac_amd import engine
    from super_sac_amd._lib import check, lib
    st = engine.stream()
    for K, H, N, act in SHAPES:
        for B in (1, 4):
            g = torch.Generator().manual_seed(1)
            dev = lambda *s: torch.randn(*s, generator=g).cuda()
            X, W0, b0, W1, b1 = dev(B, K), dev(H, K) / K ** 0.5, dev(H), dev(N, H) / H ** 0.5, dev(N)
            Hs, Y = torch.empty(B, H, device="cuda"), torch.empty(B, N, device="cuda")
            scratch = torch.zeros(4 + 16 * 256, device="cuda")
            a = ACT[act]

            def fused():
                check(lib.ssac_enc_mlp2_fwd(X.data_ptr(), K, W0.data_ptr(), b0.data_ptr(), W1.data_ptr(), b1.data_ptr(), B, K,
                                            H, N, a, 0, Y.data_ptr(), N, st))

            def layers():
                check(lib.ssac_linear_fwd(X.data_ptr(), K, W0.data_ptr(), K, b0.data_ptr(), Hs.data_ptr(), H, B, H, K, 1, st))
                check(lib.ssac_linear_fwd(Hs.data_ptr(), H, W1.data_ptr(), H, b1.data_ptr(), Y.data_ptr(), N, B, N, H,
                                          1 if a == 1 else 0, st))
                if a == 2:
                    check(lib.ssac_enc_act_fwd(Y.data_ptr(), N, B, N, a, st))

            def rows():
                check(lib.ssac_enc_mlp2_fwd_rows(X.data_ptr(), K, W0.data_ptr(), b0.data_ptr(), W1.data_ptr(), b1.data_ptr(), B,
                                                 K, H, N, a, Y.data_ptr(), N, scratch.data_ptr(), st))
            out(f"{K}->{H}->{N} {act} rows {B}")
            out("   forward : " + fmt(compare({"fused": fused, "per-layer": layers, "few-row": rows})))


def acting_steps(out):
    import super_sac_amd as ssa
    import mlp_encoder_cases as mc
    from super_sac_amd import acting
    from super_sac_amd import mlp_encoder as me
    dev = torch.device("cuda")
    has_rows = hasattr(me, "USE_ROWS")

    def agent(enc, A, discrete):
        ag = ssa.Agent(act_space_size=A, encoder=enc, discrete=discrete, ensemble_size=1, num_critics=2, hidden_size=256,
                       actor_network_cls=ssa.nets.DiscreteActor if discrete else ssa.nets.ContinuousStochasticActor,
                       critic_network_cls=ssa.nets.DiscreteCritic if discrete else ssa.nets.ContinuousCritic,
                       auto_rescale_targets=False)
        ag.to(dev)
        return ag
    kinds = [("SharedEncoder-shaped SAC agent (obs 17 -> 128 -> 17 relu, A 6, hidden 256)", (17,), 6, False,
              lambda: mc.SharedEncoderLike(17, 128), lambda: ssa.nets.IdentityEncoder(17)),
             ("visgrid-shaped discrete agent (18 x 18 -> 256 -> 2 tanh, A 4, hidden 256)", (18, 18), 4, True,
              lambda: mc.VisgridEncoderLike(18, 256, 2), lambda: ssa.nets.IdentityEncoder(2))]
    for title, shape, A, discrete, make_enc, make_id in kinds:
        for n in (1, 4):
            rs = np.random.RandomState(n)
            obs = rs.standard_normal(shape if n == 1 else (n,) + shape).astype(np.float32)
            emb = 17 if not discrete else 2
            flat = rs.standard_normal((emb,) if n == 1 else (n, emb)).astype(np.float32)
            torch.manual_seed(0)
            plain, forced, ident = agent(make_enc(), A, discrete), agent(make_enc(), A, discrete), agent(make_id(), A, discrete)

            def general(fn):
                def call():
                    acting.ENABLED = False
                    try:
                        return fn()
                    finally:
                        acting.ENABLED = True
                return call

            def with_rows(fn):
                def call():   # (the form is settled when the plan is recorded: the switch matters in the first call only)
                    saved = me.USE_ROWS
                    me.USE_ROWS = "all"
                    try:
                        return fn()
                    finally:
                        me.USE_ROWS = saved
                return call
            for rule in ("sample_action", "forward"):
                forms = {"plan": lambda: getattr(plain, rule)({"obs": obs}, num_envs=n),
                         "off": general(lambda: getattr(plain, rule)({"obs": obs}, num_envs=n)),
                         "identity plan": lambda: getattr(ident, rule)({"obs": flat}, num_envs=n)}
                if has_rows:
                    forms["plan, few-row"] = with_rows(lambda: getattr(forced, rule)({"obs": obs}, num_envs=n))
                res = compare_wall(forms)
                taken = (rule.split("_")[0], n, 0.0) in (acting._PLANS.get(plain) or {})
                out(f"{title}, num_envs {n}, {rule} (plan taken: {taken})")
                out("   " + fmt(res))


def main():
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else None
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
        if path:
            with open(path, "w") as f:
                f.write("\n".join(lines) + "\n")
    out(f"device: {torch.cuda.get_device_name(0)}; REPS {REPS}, ROUNDS {ROUNDS}, warm-up {WARM}")
    if "--acting" in sys.argv:
        if "--steps-only" not in sys.argv:
            acting_launches(out)
        acting_steps(out)
        return
    kernels(out)
    critic(out)


if __name__ == "__main__":
    main()
