"""Write tests/golden/beta_*.npz by driving the UNMODIFIED reference's Beta agent (Agent(beta_dist=True)); dev container only.

    python tools/gen_beta_golden.py            # writes tests/golden/beta_{sac,redq,sunrise}.npz

The cases are tests/beta_cases.py.  Seeded weights and buffers come from the same generators as the other fixtures
(case_runner._oracle_agent / _buffers).  Beta draws consume torch's CPU generator inside torch._sample_dirichlet, so
oracle/gen_golden.py's "replicate the draws, then rewind" does not work for them: they are RECORDED in call order by a spy
on torch._sample_dirichlet (x = component 0 of each Dirichlet sample), the exploration normals by a spy on torch.randn, the
replay indices from the replay dicts the reference returns; only the Python `random` draws (REDQ subsets, logged-net
picks) are replicated and rewound.  The record layout is oracle/gen_golden.py's: the draw keys are inputs of
case_runner.compare, everything else an output.  Running the script twice writes identical files.
"""
import copy
import math
import os
import random
import sys
import types
from itertools import chain

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_harness  # noqa: E402
import synth  # noqa: E402
import case_runner  # noqa: E402
from beta_cases import BETA_CASES  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


class _Spies:
    """records torch._sample_dirichlet outputs (component 0) and torch.randn outputs while installed"""

    def __init__(self):
        self.dir, self.randn = [], []

    def __enter__(self):
        self._d, self._r = torch._sample_dirichlet, torch.randn

        def dirichlet(*a, **k):
            out = self._d(*a, **k)
            self.dir.append(out[..., 0].detach().clone().numpy())
            return out

        def randn(*a, **k):
            out = self._r(*a, **k)
            self.randn.append(out.detach().clone().numpy())
            return out
        torch._sample_dirichlet, torch.randn = dirichlet, randn
        return self

    def __exit__(self, *exc):
        torch._sample_dirichlet, torch.randn = self._d, self._r

    def take(self):
        d, r = self.dir, self.randn
        self.dir, self.randn = [], []
        return d, r


def _ref_agent(ref, cfg):
    class Enc(ref.nets.Encoder):
        @property
        def embedding_dim(self):
            return cfg["obs"]

        def forward(self, obs_dict):
            return obs_dict["obs"]
    oa = case_runner._oracle_agent(cfg)
    ra = ref.Agent(act_space_size=cfg["act"], encoder=Enc(), actor_network_cls=ref.nets.mlps.ContinuousStochasticActor,
                   critic_network_cls=ref.nets.mlps.ContinuousCritic, discrete=False, ensemble_size=cfg["E"],
                   num_critics=cfg["N"], ucb_bonus=0.0, hidden_size=cfg["hidden"], auto_rescale_targets=cfg["popart"],
                   log_std_low=cfg["lo"], log_std_high=cfg["hi"], beta_dist=True)
    assert all(a.dist_impl == "beta" for a in ra.actors)

    def load(mod, p, names):
        with torch.no_grad():
            for (wk, bk), nm in zip((("w1", "b1"), ("w2", "b2"), ("w3", "b3")), names):
                getattr(mod, nm).weight.copy_(p[wk])
                getattr(mod, nm).bias.copy_(p[bk])
    for i in range(cfg["E"]):
        load(ra.actors[i], oa.actors[i], ("fc1", "fc2", "fc3"))
        for j in range(cfg["N"]):
            load(ra.critics[i].nets[j], oa.critics[i][j], ("fc1", "fc2", "out"))
        if cfg["popart"]:
            ra.popart[i].min_steps = cfg.get("popart_min_steps", 1000)
    ra.train()
    return ra


def _params(ra, E, N):
    crit = [p for i in range(E) for j in range(N) for p in ra.critics[i].nets[j].parameters()]
    act = [p for i in range(E) for p in ra.actors[i].parameters()]
    return crit, act


def run_case(ref, name, cfg):
    print(f"== {name}")
    rl, rlu = ref.learning, ref.learning_utils
    torch.manual_seed(cfg["seed"]); np.random.seed(cfg["seed"]); random.seed(cfg["seed"])
    B, E, N = cfg["B"], cfg["E"], cfg["N"]
    rbuf = ref.replay.ReplayBuffer(cfg["cap"])
    rbuf.load_experience(*case_runner._buffers(cfg))
    ra = _ref_agent(ref, cfg)
    rt = copy.deepcopy(ra)
    copt = torch.optim.Adam(chain(*(c.parameters() for c in ra.critics)), lr=cfg["lr"], betas=(0.9, 0.999))
    aopt = torch.optim.Adam(chain(*(a.parameters() for a in ra.actors)), lr=cfg["lr"], betas=(0.9, 0.999))
    eopt = torch.optim.Adam(ra.encoder.parameters(), lr=1e-4, betas=(0.9, 0.999))
    las, lopts = [], []
    for _ in range(E):
        la = torch.Tensor([math.log(cfg["init_alpha"])])
        la.requires_grad = True
        las.append(la)
        lopts.append(torch.optim.Adam([la], lr=cfg["alpha_lr"], betas=(0.5, 0.999)))
    aug = ref.augmentations.AugmentationSequence([ref.augmentations.IdentityAug(B)])
    rproc = None
    if cfg["noise"]:
        space = types.SimpleNamespace(low=-np.ones(cfg["act"], np.float32), high=np.ones(cfg["act"], np.float32))
        rproc = rlu.GaussianExplorationNoise(space, start_scale=cfg["noise"]["scale"],
                                             final_scale=cfg["noise"]["scale"] * 0.1, steps_annealed=1000)
    captured = []
    orig_td = rlu.compute_td_targets

    def td_spy(*a, **k):
        out = orig_td(*a, **k)
        captured.append(out[0].detach().clone())
        return out
    rlu.compute_td_targets = td_spy
    rec, upd = {}, 0
    spies = _Spies()
    try:
        with spies:
            for cyc in range(cfg["cycles"]):
                rp = rproc if cyc in cfg["noise_cycles"] else None
                nclip = cfg["noise"]["clip"] if rp is not None else None
                for k in range(cfg["utd"]):
                    pst = random.getstate()
                    subsets = [random.sample(range(N), k=cfg["n"]) for _ in range(E)]
                    gpick = random.choice(range(E))
                    random.setstate(pst)
                    captured.clear()
                    logs, dicts = rl.critic_update(
                        buffer=rbuf, agent=ra, target_agent=rt, critic_optimizer=copt, encoder_optimizer=eopt,
                        log_alphas=las, batch_size=B, gamma=cfg["gamma"], critic_clip=cfg["clip"],
                        encoder_clip=cfg["clip"], target_critic_ensemble_n=cfg["n"],
                        weighted_bellman_temp=cfg["temp"], weight_type=cfg["weight_type"], pop=cfg["pop"],
                        augmenter=aug, encoder_lambda=0, aug_mix=0.0, discrete=False, random_process=rp,
                        noise_clip=nclip, per=False, update_priorities=False, dr3_coeff=0.0)
                    xs, nz = spies.take()
                    assert len(xs) == E and len(nz) == (E if rp is not None else 0)
                    rec[f"u{upd}_gpick"] = np.int64(gpick)
                    for i in range(E):
                        rec[f"u{upd}_idx{i}"] = np.asarray(dicts[i]["priority_idxs"]).astype(np.int64)
                        rec[f"u{upd}_subset{i}"] = np.array(subsets[i], np.int64)
                        rec[f"u{upd}_eps{i}"] = xs[i]
                        if rp is not None:
                            rec[f"u{upd}_noise{i}"] = nz[i]
                        rec[f"u{upd}_td{i}"] = captured[i].numpy()
                        if cfg["popart"]:
                            pr = ra.popart[i]
                            rec[f"u{upd}_popart{i}"] = np.array([float(pr.mu), float(pr.nu), float(pr.w), float(pr.b),
                                                                 float(pr.sigma), pr._t], np.float64)
                    for key, val in logs.items():
                        rec[f"u{upd}_log:{key}"] = np.float64(float(val))
                    if (k + cyc) % cfg["target_delay"] == 0:
                        for ac, tc in zip(ra.critics, rt.critics):
                            rlu.soft_update(tc, ac, cfg["tau"])
                        rec[f"u{upd}_polyak"] = np.int64(1)
                    else:
                        rec[f"u{upd}_polyak"] = np.int64(0)
                    upd += 1
                pst = random.getstate()
                apick = random.choice(range(E))
                random.setstate(pst)
                alogs = rl.online_actor_update(
                    buffer=rbuf, agent=ra, pop=cfg["pop"], actor_optimizer=aopt, log_alphas=las, batch_size=B,
                    aug_mix=0.0, clip=cfg["clip"], augmenter=aug, per=False, discrete=False, random_process=rp,
                    noise_clip=nclip, premade_replay_dicts=dicts, use_baseline=False)
                xs, nz = spies.take()
                assert len(xs) == E and len(nz) == (E if rp is not None else 0)
                rec[f"a{cyc}_gpick"] = np.int64(apick)
                for i in range(E):
                    rec[f"a{cyc}_eps{i}"] = xs[i]
                    if rp is not None:
                        rec[f"a{cyc}_noise{i}"] = nz[i]
                for key, val in alogs.items():
                    rec[f"a{cyc}_log:{key}"] = np.float64(float(val))
                llogs = rl.alpha_update(buffer=rbuf, agent=ra, optimizers=lopts, batch_size=B, log_alphas=las,
                                        augmenter=aug, aug_mix=0.0, target_entropy=-float(cfg["act"]),
                                        premade_replay_dicts=dicts, discrete=False)
                xs, nz = spies.take()
                assert len(xs) == E and not nz
                for i in range(E):
                    rec[f"l{cyc}_eps{i}"] = xs[i]
                for key, val in llogs.items():
                    rec[f"l{cyc}_log:{key}"] = np.float64(float(val))
            if cfg["bc"]:
                # plain behavioural cloning (learning.py:144-219, filter_=False): the batch indices come from the spy
                idx = []
                orig_smaa = rlu.sample_move_and_augment

                def smaa(*a, **k):
                    out = orig_smaa(*a, **k)
                    idx.append(np.asarray(out["priority_idxs"]).astype(np.int64))
                    return out
                rlu.sample_move_and_augment = smaa
                pst = random.getstate()
                spick = random.choice(range(E))
                random.setstate(pst)
                try:
                    blogs = rl.offline_actor_update(
                        buffer=rbuf, agent=ra, actor_optimizer=aopt, encoder_optimizer=eopt, batch_size=B,
                        actor_clip=cfg["clip"], update_encoder=False, encoder_clip=None, augmenter=aug, actor_lambda=0.0,
                        aug_mix=0.0, per=False, discrete=False, filter_=False)
                finally:
                    rlu.sample_move_and_augment = orig_smaa
                xs, nz = spies.take()
                assert not xs and not nz and len(idx) == E
                rec["s0_gpick"] = np.int64(spick)
                for i in range(E):
                    rec[f"s0_idx{i}"] = idx[i]
                for key, val in blogs.items():
                    rec[f"s0_log:{key}"] = np.float64(float(val))
    finally:
        rlu.compute_td_targets = orig_td
    crit, act = _params(ra, E, N)
    tcrit, _ = _params(rt, E, N)
    small = sum(p.numel() for p in crit) < 40000
    for tag, plist in (("critic", crit), ("actor", act), ("target_critic", tcrit)):
        if small:
            rec[f"final_{tag}"] = case_runner._flat(plist)
        else:
            rec[f"finalfp_{tag}"] = case_runner._fingerprint(plist)
    ms, vs = [], []
    for p in crit:
        stt = copt.state[p]
        fi = synth.fingerprint_indices(p.numel())
        ms.append(stt["exp_avg"].numpy().ravel()[fi])
        vs.append(stt["exp_avg_sq"].numpy().ravel()[fi])
    rec["finalfp_critic_m"] = np.concatenate(ms)
    rec["finalfp_critic_v"] = np.concatenate(vs)
    rec["final_log_alpha"] = np.array([float(x) for x in las], np.float64)
    rec["n_updates"] = np.int64(upd)
    return rec


def main(names=None, out=OUT):
    ref = ref_harness.import_reference()
    torch.set_num_threads(4)
    os.makedirs(out, exist_ok=True)
    for name in names or sorted(BETA_CASES):
        rec = run_case(ref, name, BETA_CASES[name])
        path = os.path.join(out, f"{name}.npz")
        np.savez_compressed(path, **rec)
        print(f"   {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1:] or None)
