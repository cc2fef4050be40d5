"""Shared by the MLP-encoder tests: encoder stand-ins that carry the attribute names of the reference's experiment
scripts (``--shared_encoder`` of experiments/gym/train_gym.py; experiments/visgrid/train.py) and nothing of their text,
the matching encoder ``kind`` for the CPU oracle (oracle/ssac_oracle.py is not edited: the tests replace ``orc.encode``
through monkeypatch), and the measured-tolerance rule of the kernel tests."""
import numpy as np
import torch
from torch import nn
import torch.nn.functional as F


class SharedEncoderLike(nn.Module):
    """obs -> Linear(dim, hidden) -> ReLU -> Linear(hidden, dim) -> ReLU"""

    def __init__(self, dim, hidden=128):
        super().__init__()
        self.have_at_least_one_param = nn.Linear(1, 1)
        self.fc0 = nn.Linear(dim, hidden)
        self.fc1 = nn.Linear(hidden, dim)
        self._dim = dim

    @property
    def embedding_dim(self):
        return self._dim

    def forward_rolling(self, obs):
        return self.forward(obs)

    def reset_rolling(self):
        pass

    def forward(self, obs_dict):
        x = F.relu(self.fc0(obs_dict["obs"]))
        return F.relu(self.fc1(x))


class VisgridEncoderLike(nn.Module):
    """(18, 18) grid -> flatten -> Linear(324, hidden) -> ReLU -> Linear(hidden, 2) -> tanh"""

    def __init__(self, hw=18, hidden=256, out=2):
        super().__init__()
        self.have_at_least_one_param = nn.Linear(1, 1)
        self.fc1 = nn.Linear(hw * hw, hidden)
        self.fc2 = nn.Linear(hidden, out)
        self._dim = out

    @property
    def embedding_dim(self):
        return self._dim

    def forward_rolling(self, obs):
        return self.forward(obs)

    def reset_rolling(self):
        pass

    def forward(self, obs_dict):
        x = obs_dict["obs"].flatten(1)
        return torch.tanh(self.fc2(F.relu(self.fc1(x))))


def mlp2_act(name, z):
    return torch.relu(z) if name == "relu" else torch.tanh(z) if name == "tanh" else z


def oracle_encoder(seed, in_dim, hidden, out_dim, act, dtype=torch.float32):
    """encoder dict of the oracle's shape with the new kind "mlp2" (seeded weights, scaled like orc.make_mlp)"""
    rng = np.random.RandomState(seed)

    def lin(o, i):
        w = (rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32)
        b = (rng.standard_normal((o,)) * 0.05).astype(np.float32)
        return torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype)
    w0, b0 = lin(hidden, in_dim)
    w1, b1 = lin(out_dim, hidden)
    return {"kind": "mlp2", "key": "obs", "act": act, "p": {"w0": w0, "b0": b0, "w1": w1, "b1": b1}}


def patched_encode(orc):
    """orc.encode with the kind "mlp2" added; every other kind goes to the oracle's own function"""
    stock = orc.encode

    def encode(enc, obs_dict):
        if enc["kind"] != "mlp2":
            return stock(enc, obs_dict)
        p = enc["p"]
        x = obs_dict[enc["key"]].flatten(1).to(p["w0"].dtype)
        return mlp2_act(enc["act"], F.linear(F.relu(F.linear(x, p["w0"], p["b0"])), p["w1"], p["b1"]))
    return encode


def load_encoder(module, enc):
    """the oracle encoder's weights into a stand-in (or nets.MlpEncoder): its two Linears in registration order"""
    lins = [m for m in module.modules() if isinstance(m, nn.Linear) and m is not module.have_at_least_one_param]
    with torch.no_grad():
        lins[0].weight.copy_(enc["p"]["w0"]); lins[0].bias.copy_(enc["p"]["b0"])
        lins[1].weight.copy_(enc["p"]["w1"]); lins[1].bias.copy_(enc["p"]["b1"])
    return lins


def measured_bound(ref32, ref64, *magnitudes):
    """the ``ref_dev64`` rule: 4 x the largest distance between torch's own fp32 CPU result and the fp64 result on the
    same inputs, never below one fp32 ulp of the largest magnitude involved"""
    dev = float((ref32.double() - ref64).abs().max()) if ref32.numel() else 0.0
    big = max([float(ref64.abs().max()) if ref64.numel() else 0.0] + [float(m) for m in magnitudes] + [1e-30])
    return max(4.0 * dev, float(np.spacing(np.float32(big))))


# ---------------------------------------------------------------------------------------------------------------------
# update sequences: the oracle on the CPU and the engine on the GPU, fed the same host draws
# ---------------------------------------------------------------------------------------------------------------------
# seed: the straggler allowance of the encoder parameters (case_runner.straggler_check) is a cap, not a measurement.  The
# seeds below are ones for which the oracle ALONE -- run in fp32 and again with every tensor in fp64, i.e. under another
# rounding of every sum -- stays inside the cap on every encoder tensor (tools/vet_mlp_encoder_seeds.py prints the table).
CONFIGS = {
    "sac": dict(obs=(11,), emb=11, act=3, hidden=64, N=2, E=1, B=32, enc_hidden=128, enc_act="relu", discrete=False, seed=3),
    "ensemble": dict(obs=(11,), emb=11, act=3, hidden=64, N=2, E=2, B=32, enc_hidden=128, enc_act="relu", discrete=False,
                     seed=4),
    "visgrid": dict(obs=(18, 18), emb=2, act=4, hidden=64, N=2, E=1, B=32, enc_hidden=64, enc_act="tanh", discrete=True,
                    seed=5),
}
ROWS, CAP = 96, 128
GAMMA, TAU, ENC_TAU, LR, ENC_LR, ALPHA_LR = 0.99, 0.005, 0.01, 3e-4, 1e-3, 1e-3
CRITIC_CLIP, ENC_CLIP, ACTOR_CLIP = 10.0, 40.0, 10.0
STEPS = 3


def transitions(cfg):
    rng = np.random.RandomState(cfg["seed"] + 100)
    s = rng.standard_normal((ROWS,) + cfg["obs"]).astype(np.float32)
    s1 = rng.standard_normal((ROWS,) + cfg["obs"]).astype(np.float32)
    if cfg["discrete"]:
        a = rng.randint(0, cfg["act"], size=(ROWS, 1)).astype(np.float32)
    else:
        a = rng.uniform(-1.0, 1.0, size=(ROWS, cfg["act"])).astype(np.float32)
    r = rng.standard_normal((ROWS,)).astype(np.float32)
    d = rng.uniform(size=(ROWS,)) < 0.05
    return {"obs": s}, a, r, {"obs": s1}, d


def draws(cfg):
    """the host draws of STEPS rounds of (critic, actor, alpha [, bc, markov]) for every member"""
    rng = np.random.RandomState(cfg["seed"] + 200)
    B, A, E, N = cfg["B"], cfg["act"], cfg["E"], cfg["N"]
    out = []
    for _ in range(STEPS):
        out.append(dict(idx=[rng.randint(0, ROWS, size=B) for _ in range(E)],
                        eps=[rng.standard_normal((B, A)).astype(np.float32) for _ in range(E)],
                        subset=[[int(v) for v in rng.permutation(N)] for _ in range(E)],
                        aeps=[rng.standard_normal((B, A)).astype(np.float32) for _ in range(E)],
                        leps=[rng.standard_normal((B, A)).astype(np.float32) for _ in range(E)],
                        perm=rng.permutation(B).astype(np.int64), gpick=int(rng.randint(0, E)), apick=int(rng.randint(0, E))))
    return out


def oracle_agent(orc, cfg, dtype=torch.float32):
    in_dim = int(np.prod(cfg["obs"]))
    enc = oracle_encoder(cfg["seed"] + 7, in_dim, cfg["enc_hidden"], cfg["emb"], cfg["enc_act"])
    oa = orc.AgentOracle(state_dim=cfg["emb"], act_dim=cfg["act"], hidden=cfg["hidden"], num_critics=cfg["N"],
                         ensemble_size=cfg["E"], discrete=cfg["discrete"],
                         actor_kind="discrete" if cfg["discrete"] else "stochastic", popart=False, encoder=enc,
                         seed=cfg["seed"])
    if dtype != torch.float32:
        cast = lambda d: {k: v.to(dtype) for k, v in d.items()}
        oa.actors = [cast(a) for a in oa.actors]
        oa.critics = [[cast(c) for c in ens] for ens in oa.critics]
        oa.encoder = dict(oa.encoder, p=cast(oa.encoder["p"]))
    return oa


def markov_models(orc, cfg, dtype=torch.float32):
    rng = np.random.RandomState(cfg["seed"] + 11)
    inv_out = cfg["act"] if cfg["discrete"] else 2 * cfg["act"]
    inv, con = orc.make_mlp(rng, 2 * cfg["emb"], cfg["hidden"], inv_out), orc.make_mlp(rng, 2 * cfg["emb"], cfg["hidden"], 1)
    return {k: v.to(dtype) for k, v in inv.items()}, {k: v.to(dtype) for k, v in con.items()}


def _np(t):
    return t.detach().cpu().double().numpy()


def _flat(ts):
    return np.concatenate([_np(t).ravel() for t in ts])


def target_entropy(cfg):
    return (-np.log(1.0 / cfg["act"]) * 0.98) if cfg["discrete"] else -float(cfg["act"])


def run_oracle(orc, cfg, mode, dtype=torch.float32, update_encoder=True):
    """mode "sac": STEPS x (critic, actor, alpha, Polyak); "bc": STEPS x offline_actor_update(filter_=False);
    "markov": STEPS x markov update (+ one critic update when the configuration is discrete).  orc.encode must be patched."""
    import math
    obuf = orc.ReplayOracle(CAP)
    obuf.load_experience(*transitions(cfg))
    oa = oracle_agent(orc, cfg, dtype).requires_grad_(True)
    ot = oa.clone()
    E, B = cfg["E"], cfg["B"]
    T = lambda a: torch.from_numpy(a).to(dtype)
    copt = orc.AdamOracle(oa.critic_params(), lr=LR)
    aopt = orc.AdamOracle(oa.actor_params(), lr=LR)
    eopt = orc.AdamOracle(oa.encoder_params(), lr=ENC_LR)
    las = [torch.tensor([math.log(0.1)], dtype=dtype, requires_grad=True) for _ in range(E)]
    lopts = [orc.AdamOracle([la], lr=ALPHA_LR, betas=(0.5, 0.999)) for la in las]
    aug = orc.AugOracle("identity", B)
    rec = {}
    if mode == "markov":
        inv_p, con_p = markov_models(orc, cfg, dtype)
        for t in list(inv_p.values()) + list(con_p.values()):
            t.requires_grad_(True)
        mopt = orc.AdamOracle(oa.encoder_params() + [inv_p[k] for k in orc.MLP_KEYS] + [con_p[k] for k in orc.MLP_KEYS], lr=LR)
    for k, dr in enumerate(draws(cfg)):
        if mode == "sac":
            logs, dicts = orc.critic_update(
                obuf, oa, ot, copt, eopt, las, B, GAMMA, CRITIC_CLIP, ENC_CLIP, cfg["N"], None, None, False, aug, aug_mix=0.0,
                idx_list=dr["idx"], eps_list=None if cfg["discrete"] else [T(e) for e in dr["eps"]],
                subset_list=dr["subset"], grad_pick=dr["gpick"])
            for i in range(E):
                rec[f"u{k}_td{i}"] = _np(dicts[i]["td_target"])
            rec.update({f"u{k}_log:{n}": float(v) for n, v in logs.items()})
            alog = orc.online_actor_update(oa, aopt, las, dicts, False, ACTOR_CLIP,
                                           eps_list=None if cfg["discrete"] else [T(e) for e in dr["aeps"]],
                                           grad_pick=dr["apick"])
            rec.update({f"a{k}_log:{n}": float(v) for n, v in alog.items()})
            llog = orc.alpha_update(oa, lopts, las, dicts, target_entropy(cfg),
                                    eps_list=None if cfg["discrete"] else [T(e) for e in dr["leps"]])
            rec.update({f"l{k}_log:{n}": float(v) for n, v in llog.items()})
            orc.soft_update(ot.critic_params(), oa.critic_params(), TAU)
            orc.soft_update(ot.encoder_params(), oa.encoder_params(), ENC_TAU)
        elif mode == "bc":
            logs, _, _, _ = orc.offline_actor_update(
                obuf, None, oa, aopt, B, ACTOR_CLIP, aug, 0.0, per=False, filter_=False, idx_list=dr["idx"],
                update_encoder=update_encoder, encoder_opt=eopt, encoder_clip=ENC_CLIP, grad_pick=dr["apick"])
            rec.update({f"b{k}_log:{n}": float(v) for n, v in logs.items()})
        else:
            logs, _ = orc.markov_state_abstraction_update(
                obuf, oa, inv_p, con_p, mopt, B, aug, 0.0, 1.0, 1.0, 1.0, 0.5, 5.0, idx=dr["idx"][0],
                perm=torch.from_numpy(dr["perm"]))
            rec.update({f"m{k}_log:{n}": float(v) for n, v in logs.items()})
    if mode == "markov":
        rec["final_inverse"] = _flat([inv_p[k] for k in orc.MLP_KEYS])
        rec["final_contrastive"] = _flat([con_p[k] for k in orc.MLP_KEYS])
        if cfg["discrete"]:
            dr = draws(cfg)[0]
            logs, dicts = orc.critic_update(obuf, oa, ot, copt, eopt, las, B, GAMMA, CRITIC_CLIP, ENC_CLIP, cfg["N"], None,
                                            None, False, aug, aug_mix=0.0, idx_list=dr["idx"], eps_list=None,
                                            subset_list=dr["subset"], grad_pick=dr["gpick"])
            rec["u0_td0"] = _np(dicts[0]["td_target"])
            rec.update({f"u0_log:{n}": float(v) for n, v in logs.items()})
    rec["final_critic"] = _flat(oa.critic_params())
    rec["final_actor"] = _flat(oa.actor_params())
    rec["final_target_critic"] = _flat(ot.critic_params())
    rec["final_log_alpha"] = np.array([float(x) for x in las])
    for nm, t in oa.encoder["p"].items():
        rec[f"final_encoder_{nm}"] = _np(t).ravel()
    for nm, t in ot.encoder["p"].items():
        rec[f"final_target_encoder_{nm}"] = _np(t).ravel()
    return rec


def make_encoder(cfg, own=False):
    """the encoder module of a configuration: a stand-in in the reference's shape, or (own) ssa.nets.MlpEncoder"""
    in_dim = int(np.prod(cfg["obs"]))
    if own:
        import super_sac_amd as ssa
        return ssa.nets.MlpEncoder(cfg["obs"], cfg["enc_hidden"], cfg["emb"], out_act=cfg["enc_act"])
    if len(cfg["obs"]) == 1:
        assert cfg["enc_act"] == "relu" and cfg["emb"] == in_dim
        return SharedEncoderLike(in_dim, cfg["enc_hidden"])
    return VisgridEncoderLike(cfg["obs"][0], cfg["enc_hidden"], cfg["emb"])


def engine_agent(orc, cfg, device, own=False):
    import super_sac_amd as ssa
    oa = oracle_agent(orc, cfg)
    enc = make_encoder(cfg, own)
    load_encoder(enc, oa.encoder)
    actor_cls = ssa.nets.DiscreteActor if cfg["discrete"] else ssa.nets.ContinuousStochasticActor
    critic_cls = ssa.nets.DiscreteCritic if cfg["discrete"] else ssa.nets.ContinuousCritic
    ag = ssa.Agent(act_space_size=cfg["act"], encoder=enc, actor_network_cls=actor_cls, critic_network_cls=critic_cls,
                   discrete=cfg["discrete"], ensemble_size=cfg["E"], num_critics=cfg["N"], ucb_bonus=0.0,
                   hidden_size=cfg["hidden"], auto_rescale_targets=False)
    head = "act_p" if cfg["discrete"] else "fc3"

    def load(mod, p, names):
        with torch.no_grad():
            for (wk, bk), nm in zip((("w1", "b1"), ("w2", "b2"), ("w3", "b3")), names):
                getattr(mod, nm).weight.copy_(p[wk])
                getattr(mod, nm).bias.copy_(p[bk])
    for i in range(cfg["E"]):
        load(ag.actors[i], oa.actors[i], ("fc1", "fc2", head))
        for j in range(cfg["N"]):
            load(ag.critics[i].nets[j], oa.critics[i][j], ("fc1", "fc2", "out"))
    ag.to(device)
    ag.train()
    return ag


def encoder_tensors(enc):
    lins = [m for m in enc.modules() if isinstance(m, nn.Linear) and m is not enc.have_at_least_one_param]
    return {"w0": lins[0].weight, "b0": lins[0].bias, "w1": lins[1].weight, "b1": lins[1].bias}


class EngineRun:
    """the engine side of run_oracle: built once, stepped round by round (the checkpoint test stops in the middle)"""

    def __init__(self, orc, cfg, mode, device="cuda", own=False, update_encoder=True):
        import copy
        import math
        from itertools import chain
        import super_sac_amd as ssa
        import case_runner
        self.ssa, self.cfg, self.mode, self.update_encoder, self.orc = ssa, cfg, mode, update_encoder, orc
        self.device = device = torch.device(device)
        self.buf = ssa.replay.ReplayBuffer(CAP, device=device)
        self.buf.load_experience(*transitions(cfg))
        self.agent = ag = engine_agent(orc, cfg, device, own)
        self.target = copy.deepcopy(ag)
        E, B = cfg["E"], cfg["B"]
        adam = lambda ps, lr, betas=(0.9, 0.999): torch.optim.Adam(ps, lr=lr, betas=betas)
        self.copt = adam(chain(*(c.parameters() for c in ag.critics)), LR)
        self.aopt = adam(chain(*(a.parameters() for a in ag.actors)), LR)
        self.eopt = adam(ag.encoder.parameters(), ENC_LR)
        self.las, self.lopts = [], []
        for _ in range(E):
            la = torch.Tensor([math.log(0.1)]).to(device)
            la.requires_grad = True
            self.las.append(la)
            self.lopts.append(adam([la], ALPHA_LR, (0.5, 0.999)))
        self.aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(B)])
        if mode == "markov":
            inv_p, con_p = markov_models(orc, cfg)
            with torch.no_grad():
                for mod, p, names in ((ag.inverse_model, inv_p, ("fc1", "fc2", "act_p" if cfg["discrete"] else "fc3")),
                                      (ag.contrastive_model, con_p, ("fc1", "fc2", "out"))):
                    for (wk, bk), nm in zip((("w1", "b1"), ("w2", "b2"), ("w3", "b3")), names):
                        getattr(mod, nm).weight.copy_(p[wk])
                        getattr(mod, nm).bias.copy_(p[bk])
            self.mopt = adam(chain(ag.encoder.parameters(), ag.inverse_model.parameters(),
                                   ag.contrastive_model.parameters()), LR)
        self.player = case_runner.DrawPlayer(device)
        self.rec = {}
        self.draws = draws(cfg)

    def _critic(self, k, dr):
        ssa, cfg, p = self.ssa, self.cfg, self.player
        for i in range(cfg["E"]):
            p.idx.append(dr["idx"][i])
            if not cfg["discrete"]:
                p.normal.append(dr["eps"][i])
            p.sub.append(dr["subset"][i])
        p.picks.append(dr["gpick"])
        logs, dicts = ssa.learning.critic_update(
            buffer=self.buf, agent=self.agent, target_agent=self.target, critic_optimizer=self.copt,
            encoder_optimizer=self.eopt, log_alphas=self.las, batch_size=cfg["B"], gamma=GAMMA, critic_clip=CRITIC_CLIP,
            encoder_clip=ENC_CLIP, target_critic_ensemble_n=cfg["N"], weighted_bellman_temp=None, weight_type=None,
            pop=False, augmenter=self.aug, encoder_lambda=0, aug_mix=0.0, discrete=cfg["discrete"], random_process=None,
            noise_clip=None, per=False, update_priorities=False, dr3_coeff=0.0)
        for i in range(cfg["E"]):
            assert np.array_equal(dicts[i]["priority_idxs"], dr["idx"][i])
            self.rec[f"u{k}_td{i}"] = _np(dicts[i]["td_target"])
        self.rec.update({f"u{k}_log:{n}": float(v) for n, v in logs.items()})
        return dicts

    def step(self, k):
        ssa, cfg, p, dr = self.ssa, self.cfg, self.player, self.draws[k]
        E, B = cfg["E"], cfg["B"]
        saved_perm = ssa.rng.draw_permutation
        p.install(ssa.rng)
        try:
            if self.mode == "sac":
                dicts = self._critic(k, dr)
                if not cfg["discrete"]:
                    p.normal.extend(dr["aeps"])
                p.picks.append(dr["apick"])
                alog = ssa.learning.online_actor_update(
                    buffer=self.buf, agent=self.agent, pop=False, actor_optimizer=self.aopt, log_alphas=self.las,
                    batch_size=B, aug_mix=0.0, clip=ACTOR_CLIP, augmenter=self.aug, per=False, discrete=cfg["discrete"],
                    random_process=None, noise_clip=None, premade_replay_dicts=dicts)
                self.rec.update({f"a{k}_log:{n}": float(v) for n, v in alog.items()})
                if not cfg["discrete"]:
                    p.normal.extend(dr["leps"])
                llog = ssa.learning.alpha_update(
                    buffer=self.buf, agent=self.agent, optimizers=self.lopts, batch_size=B, log_alphas=self.las,
                    augmenter=self.aug, aug_mix=0.0, target_entropy=target_entropy(cfg), premade_replay_dicts=dicts,
                    discrete=cfg["discrete"])
                self.rec.update({f"l{k}_log:{n}": float(v) for n, v in llog.items()})
                for ac, tc in zip(self.agent.critics, self.target.critics):
                    ssa.learning_utils.soft_update(tc, ac, TAU)
                ssa.learning_utils.soft_update(self.target.encoder, self.agent.encoder, ENC_TAU)
            elif self.mode == "bc":
                p.idx.extend(dr["idx"])
                p.picks.append(dr["apick"])
                logs = ssa.learning.offline_actor_update(
                    buffer=self.buf, agent=self.agent, actor_optimizer=self.aopt, encoder_optimizer=self.eopt, batch_size=B,
                    actor_clip=ACTOR_CLIP, update_encoder=self.update_encoder, encoder_clip=ENC_CLIP, augmenter=self.aug,
                    actor_lambda=0.0, aug_mix=0.0, per=False, discrete=cfg["discrete"], filter_=False)
                self.rec.update({f"b{k}_log:{n}": float(v) for n, v in logs.items()})
            else:
                p.idx.append(dr["idx"][0])
                perms = [dr["perm"]]
                ssa.rng.draw_permutation = lambda n: torch.from_numpy(perms.pop(0))
                logs = ssa.learning.markov_state_abstraction_update(
                    buffer=self.buf, agent=self.agent, optimizer=self.mopt, batch_size=B, augmenter=self.aug, aug_mix=0.0,
                    discrete=cfg["discrete"], inverse_coeff=1.0, contrastive_coeff=1.0, smoothness_coeff=1.0,
                    smoothness_max_dist=0.5, grad_clip=5.0)
                self.rec.update({f"m{k}_log:{n}": float(v) for n, v in logs.items()})
                assert not perms
            assert not p.idx and not p.sub and not p.normal and not p.picks, "unconsumed injected draws"
        finally:
            p.restore()
            ssa.rng.draw_permutation = saved_perm

    def finish(self):
        ag, cfg = self.agent, self.cfg
        if self.mode == "markov":
            self.rec["final_inverse"] = _flat(list(ag.inverse_model.parameters()))
            self.rec["final_contrastive"] = _flat(list(ag.contrastive_model.parameters()))
            if cfg["discrete"]:
                self.player.install(self.ssa.rng)
                try:
                    self._critic(0, self.draws[0])
                finally:
                    self.player.restore()
        E, N = cfg["E"], cfg["N"]
        rec = self.rec
        rec["final_critic"] = _flat([p for i in range(E) for j in range(N) for p in ag.critics[i].nets[j].parameters()])
        rec["final_target_critic"] = _flat([p for i in range(E) for j in range(N)
                                            for p in self.target.critics[i].nets[j].parameters()])
        rec["final_actor"] = _flat([p for i in range(E) for p in ag.actors[i].parameters()])
        rec["final_log_alpha"] = np.array([float(x.detach()) for x in self.las])
        for nm, t in encoder_tensors(ag.encoder).items():
            rec[f"final_encoder_{nm}"] = _np(t).ravel()
        for nm, t in encoder_tensors(self.target.encoder).items():
            rec[f"final_target_encoder_{nm}"] = _np(t).ravel()
        return rec


def run_engine(orc, cfg, mode, **kw):
    run = EngineRun(orc, cfg, mode, **kw)
    for k in range(STEPS):
        run.step(k)
    return run.finish()


def compare(rec, ref, who, markov=False):
    """the project's tolerances (case_runner.compare / compare_markov): TD targets 2e-4, logs 5e-4 with gradient norms
    relative (Markov gradient norms 2e-3), parameters 3e-5, encoder parameters under straggler_check"""
    import case_runner
    worst = {"td": 0.0, "log": 0.0, "param": 0.0, "stragglers": 0}
    for key, want in ref.items():
        assert key in rec, f"{who}: the record lacks {key}"
        got, want = np.asarray(rec[key], np.float64), np.asarray(want, np.float64)
        if "_td" in key:
            dv = float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
            worst["td"] = max(worst["td"], dv)
            assert dv <= 2e-4, f"{who}: {key} deviates {dv:.3e}"
        elif "_log:" in key:
            if key.startswith("m"):
                dv = float(abs(got - want) / max(1.0, abs(want)))
                tol = 2e-3 if "gradients/" in key else 5e-4
            else:
                dv = float(abs(got - want) / (max(1.0, abs(want)) if "gradients/" not in key else max(1e-6, abs(want))))
                if "gradients/" in key and abs(want) < 1e-12:
                    dv = float(abs(got))
                tol = 5e-4
            worst["log"] = max(worst["log"], dv)
            assert dv <= tol, f"{who}: {key} = {got} vs {want}"
        elif "encoder" in key:
            err = np.abs(got - want)
            worst["stragglers"] += case_runner.straggler_check(err, 3e-5, 3e-3, who, key)
            assert float(np.median(err)) <= 1e-6, f"{who}: {key} median {np.median(err):.3e}"
        elif key == "final_log_alpha":
            assert np.max(np.abs(got - want)) <= 1e-6, f"{who}: log_alpha {got} vs {want}"
        else:
            dv = float(np.max(np.abs(got - want)))
            worst["param"] = max(worst["param"], dv)
            assert dv <= 3e-5, f"{who}: {key} deviates {dv:.3e}"
    return worst
