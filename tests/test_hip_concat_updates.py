"""GPU: an agent with a concatenating encoder over a three-key dictionary buffer against its single-key twin.

Two agents from the same seeds with the same initial weights:
  (a) a buffer with one key of 11 columns, IdentityEncoder, learning_utils.FOLD_GATHER = False (the replay gather is a
      launch of its own);
  (b) a buffer with the keys pos (5), goal (2), vel (4), a concatenating encoder whose order -- goal, vel, pos -- is not
      the storage's.
The columns of (a) are (b)'s keys side by side in the encoder's order, and the host generators start both runs from one
state.  Both twins then issue the same launches on buffers with the same contents -- (b)'s gather is ssac_gather_concat
where (a)'s is ssac_gather_transition, the same copies -- so the expected difference is zero: every comparison is bit for
bit (parameters, target parameters, optimizer moments, log values, TD targets, priorities, actions, generator states).

Shape: obs 11, act 3, hidden 64, N 2, n 2, B 64, 600 rows in a capacity of 1 024."""
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

pytestmark = pytest.mark.gpu
_BASE = dict(synth.AFBC_CASES["awac_offline"])        # obs 11, act 3, hidden 64, N 2, n 2, B 64, 600 rows in 1 024
CASES = {
    "stochastic": dict(_BASE),
    "refresh": dict(_BASE, update_priorities=True, seed=41),
    "deterministic+process": dict(_BASE, actor="deterministic", process=True, noise_clip=0.3, seed=42),
    "discrete": dict(_BASE, actor="discrete", discrete=True, seed=43),
    "bf16": dict(_BASE, precision="bf16", seed=44),
}
SEED = 0x5EED5EED
STORED = (("pos", 5), ("goal", 2), ("vel", 4))        # the storage's key order
ORDER = ("goal", "vel", "pos")                        # the encoder's
COLS = {"goal": (0, 2), "vel": (2, 6), "pos": (6, 11)}   # where the encoder's order puts each key in the twin's row


class UserEncoder(torch.nn.Module):
    """a user's concatenating encoder: nothing of this package but what the reference's Encoder base has"""

    def __init__(self):
        super().__init__()
        self.have_at_least_one_param = torch.nn.Linear(1, 1)
        self.embedding_dim = 11

    def forward_rolling(self, obs):
        return self.forward(obs)

    def reset_rolling(self):
        pass

    def forward(self, o):
        return torch.cat([o["goal"], o["vel"], o["pos"]], 1)


class ReferenceIdentity(UserEncoder):
    """the reference scripts' identity encoder (experiments/gym/train_gym.py:18-28): its one key, handed back"""

    def forward(self, o):
        return o["obs"]


def _split(obs):
    """the twin's {"obs": (..., 11)} as the three-key dictionary, keys in the storage's order"""
    return {k: np.ascontiguousarray(obs["obs"][..., COLS[k][0]:COLS[k][1]]) for k, _ in STORED}


def _seed_all(seed):
    torch.manual_seed(seed); np.random.seed(seed); random.seed(seed); torch.cuda.manual_seed(seed)


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a)


def _opt_moments(opt, out, name):
    grp = getattr(opt, "_ssac_adam", None)
    if grp is None:
        return
    out[f"{name}.ctl"] = _bits(grp.ctl.dev)
    for k_, (m, v) in grp.moments.items():
        out[f"{name}.m.{k_}"], out[f"{name}.v.{k_}"] = _bits(m), _bits(v)


def _state(out, agent, target, opts, las, buf):
    for i, (a_, c_) in enumerate(zip(agent.actors, agent.critics)):
        out[f"actor{i}"] = _bits(torch.cat([p.detach().flatten() for p in a_.parameters()]))
        out[f"critic{i}"] = _bits(torch.cat([p.detach().flatten() for p in c_.parameters()]))
        out[f"target_critic{i}"] = _bits(torch.cat([p.detach().flatten() for p in target.critics[i].parameters()]))
        out[f"target_actor{i}"] = _bits(torch.cat([p.detach().flatten() for p in target.actors[i].parameters()]))
    for name, opt in opts.items():
        for j, o in enumerate(opt if isinstance(opt, list) else [opt]):
            _opt_moments(o, out, f"{name}{j}")
    out["log_alphas"] = _bits(torch.cat([la.detach() for la in las]))
    out["sum_tree"], out["min_tree"], out["max_prio"] = _bits(buf._per.sum_dev), _bits(buf._per.min_dev), _bits(buf._per.max_dev)
    torch.cuda.synchronize()
    assert int(buf._per.err[0]) == 0
    out["py_random"] = np.frombuffer(repr(random.getstate()).encode(), np.uint8).copy()
    out["np_random"] = np.random.get_state()[1].copy()
    out["torch_rng"], out["cuda_rng"] = _bits(torch.get_rng_state()), _bits(torch.cuda.get_rng_state())
    return out


def _logs(out, tag, logs):
    out[f"logs:{tag}"] = {k_: float(v) for k_, v in logs.items()}


@functools.lru_cache(maxsize=None)
def _run(case, twin, fold=False, full=False):
    """twin "a" (one key, identity encoder, FOLD_GATHER = fold) or "b" (three keys, the package's ConcatEncoder) or "u" (three
    keys, a user's encoder recognised by the probe) or "r" (one key, the reference's identity encoder, acting before the
    first update).  full: behind the critic updates also the actor, temperature and
    filtered-BC updates, acting, and a checkpoint round trip with one more update.  Returns host arrays."""
    import super_sac_amd as ssa
    from super_sac_amd import acting
    L, lu = ssa.learning, ssa.learning_utils
    cfg, dev = CASES[case], torch.device("cuda")
    B, n_upd = cfg["B"], L.GRAPH_WARMUP + 3
    old_fold, old_serial = lu.FOLD_GATHER, acting._SERIAL[0]
    if twin == "a":
        lu.FOLD_GATHER = fold
    try:
        _seed_all(cfg["seed"])
        s, a, r, s1, d = case_runner._buffers(cfg)
        buf = ssa.replay.ReplayBuffer(cfg["cap"], device=dev)
        agent = case_runner.build_engine_agent(cfg, dev)
        if twin in ("a", "r"):
            buf.load_experience(s, a, r, s1, d)
            if twin == "r":
                agent.encoder = ReferenceIdentity().to(dev)
        else:
            buf.load_experience(_split(s), a, r, _split(s1), d)
            enc = ssa.nets.ConcatEncoder(dict(STORED), order=ORDER) if twin == "b" else UserEncoder()
            agent.encoder = enc.to(dev)
        if cfg.get("precision"):
            ssa.set_precision(agent, cfg["precision"])
        target = copy.deepcopy(agent)
        copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=cfg["lr"], betas=(0.9, 0.999))
        aopt = torch.optim.Adam(chain(*(a_.parameters() for a_ in agent.actors)), lr=cfg["lr"], betas=(0.9, 0.999))
        eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
        las, lopts = [], []
        for _ in range(agent.ensemble_size):
            la = torch.Tensor([math.log(cfg["init_alpha"])]).to(dev)
            la.requires_grad = True
            las.append(la)
            lopts.append(torch.optim.Adam([la], lr=1e-4, betas=(0.5, 0.999)))
        opts = {"critic": copt, "actor": aopt, "alpha": lopts}
        aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(B)])
        rp = None
        if cfg.get("process"):
            space = type("Space", (), {})()
            space.low, space.high = -np.ones(cfg["act"], np.float32), np.ones(cfg["act"], np.float32)
            rp = lu.GaussianExplorationNoise(space, start_scale=1.0, final_scale=0.1, steps_annealed=1000)
        agent.__dict__["_ssac_noise"] = [SEED, 0, 0]
        disc = bool(cfg["discrete"])

        def critic(k):
            if rp is not None:
                rp.current_scale = 0.7 - 0.05 * k
            return L.critic_update(
                buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt, log_alphas=las,
                batch_size=B, gamma=cfg["gamma"], critic_clip=cfg["clip"], encoder_clip=cfg["clip"],
                target_critic_ensemble_n=cfg["n"], weighted_bellman_temp=None, weight_type=None, pop=False, augmenter=aug,
                encoder_lambda=0, aug_mix=0.0, discrete=disc, random_process=rp, noise_clip=cfg.get("noise_clip"),
                per=False, update_priorities=bool(cfg.get("update_priorities")), dr3_coeff=0.0)

        if twin == "r":
            # the reference loop acts before its first update (main.py:342, 380): nobody has looked at the encoder yet, the
            # calls take the general path and leave it alone
            g = np.random.RandomState(8)
            for n_env in (1, 3):
                ob = {"obs": g.standard_normal((11,) if n_env == 1 else (n_env, 11)).astype(np.float32)}
                assert np.array(agent.sample_action(ob, num_envs=n_env)).shape == ((3,) if n_env == 1 else (3, 3))
                assert np.array(agent.forward(ob, num_envs=n_env)).shape == ((3,) if n_env == 1 else (3, 3))
            assert not lu.is_identity(agent.encoder) and not acting._PLANS.get(agent)
        # the host generators: one state before each twin's run
        _seed_all(cfg["seed"] + 1)
        out = {}
        n_first = 1 if cfg.get("precision") else n_upd      # (bf16: one update)
        for k in range(n_first):
            logs, dicts = critic(k)
            out[f"td{k}"], out[f"idx{k}"] = _bits(dicts[0]["td_target"]), np.array(dicts[0]["priority_idxs"])
            _logs(out, f"critic{k}", logs)
            if k % 2 == 1:
                lu.soft_update(target.critics[0], agent.critics[0], cfg["tau"])
        graphs = agent.__dict__.get("_ssac_graphs") or {}
        if not cfg.get("precision"):
            # (on the code before this feature (b) fails long before: encode() has no HIP path for its encoder)
            assert len(graphs) == 1, "the call form was not recorded"
            record, = graphs.values()
            assert record.path == "fast" and record.fast is not None, record.path
            out["list_size"] = np.array([sum(ssa._lib.lib.ssac_launch_list_size(p_) for p_ in record.graph.parts)])
        o, _, _, o1, _ = dicts[0]["primary_batch"]
        out["batch_s"] = _bits(lu.encode(agent.encoder, o))
        out["batch_s1"] = _bits(lu.encode(target.encoder, o1))
        if twin == "r":
            for enc in (agent.encoder, target.encoder):
                assert enc.ssac_identity_key == "obs" and getattr(enc, "ssac_concat_keys", None) is None
            assert lu.concat_order(buf._storage) is None
        elif twin != "a":
            # the replay dict still carries every key, each a column view of ONE allocation
            for od, row in ((o, dicts[0]["_ssac"].xsa), (o1, dicts[0]["_ssac"].x1sa)):
                assert sorted(od) == sorted(k_ for k_, _ in STORED)
                assert {t.untyped_storage().data_ptr() for t in od.values()} == {row.untyped_storage().data_ptr()}
                for k_, (c0, c1) in COLS.items():
                    assert od[k_].data_ptr() == row.data_ptr() + 4 * c0 and od[k_].shape == (B, c1 - c0)
                    assert od[k_].stride() == (row.stride(0), 1)
            assert lu.encode(agent.encoder, o).data_ptr() == dicts[0]["_ssac"].xsa.data_ptr()
            assert lu.concat_order(buf._storage) == (("goal", 2), ("vel", 4), ("pos", 5))
            assert agent.encoder.ssac_concat_keys == (("goal", 2), ("vel", 4), ("pos", 5))
        if full:
            for rep in range(3):   # (the third call of this form replays its recording)
                _logs(out, f"actor{rep}", L.online_actor_update(
                    buffer=buf, agent=agent, pop=False, actor_optimizer=aopt, log_alphas=las, batch_size=B, aug_mix=0.0,
                    clip=cfg["clip"], augmenter=aug, per=False, discrete=disc, random_process=rp,
                    noise_clip=cfg.get("noise_clip"), premade_replay_dicts=dicts))
            _logs(out, "alpha", L.alpha_update(
                buffer=buf, agent=agent, optimizers=lopts, batch_size=B, log_alphas=las, augmenter=aug, aug_mix=0.0,
                target_entropy=-float(cfg["act"]), premade_replay_dicts=dicts, discrete=disc))
            _logs(out, "actor_fresh", L.online_actor_update(
                buffer=buf, agent=agent, pop=False, actor_optimizer=aopt, log_alphas=las, batch_size=B, aug_mix=0.0,
                clip=cfg["clip"], augmenter=aug, per=False, discrete=disc, random_process=rp,
                noise_clip=cfg.get("noise_clip"), premade_replay_dicts=None))
            for filt, per in ((False, False), (True, False), (True, True)):
                _logs(out, f"bc{int(filt)}{int(per)}", L.offline_actor_update(
                    buffer=buf, agent=agent, actor_optimizer=aopt, encoder_optimizer=eopt, batch_size=B, actor_clip=cfg["clip"],
                    update_encoder=False, encoder_clip=cfg["clip"], augmenter=aug, actor_lambda=0.0, aug_mix=0.0,
                    premade_replay_dicts=None, per=per, discrete=disc, filter_=filt))
            out.update({f"updates:{k_}": v for k_, v in _state({}, agent, target, opts, las, buf).items()})
            # ---- acting on numpy observations: one C call per step for both twins
            # (the plans' serial number keys their noise stream: the same for both twins)
            acting._SERIAL[0] = 9000
            g = np.random.RandomState(7)
            for n_env in (1, 3):
                for step in range(3):
                    ob = {"obs": g.standard_normal((11,) if n_env == 1 else (n_env, 11)).astype(np.float32)}
                    if step == 2:
                        ob = {"obs": ob["obs"].astype(np.float64)}   # (converted as the identity plan converts)
                    ob = ob if twin == "a" else _split(ob)
                    out[f"sample{n_env}.{step}"] = np.array(agent.sample_action(ob, num_envs=n_env))
                    out[f"greedy{n_env}.{step}"] = np.array(agent.forward(ob, num_envs=n_env))
            plans = acting._PLANS.get(agent) or {}
            assert sorted(plans) == sorted((rule, n_env, 0.0) for rule in ("sample", "forward") for n_env in (1, 3)), \
                "an acting call went down the general path"
            assert not acting._FAILED.get(agent)
            out["py_random_acting"] = np.frombuffer(repr(random.getstate()).encode(), np.uint8).copy()
            # ---- a checkpoint round trip, then one more update
            import tempfile
            with tempfile.TemporaryDirectory() as path:
                ssa.checkpoint.save_training_state(path, agent, target, opts, las, buf)
                _logs(out, "critic_scratch", critic(n_upd)[0])      # (moves everything on; the load puts it back)
                ssa.checkpoint.load_training_state(path, agent, target, opts, las, buf)
            logs, dicts = critic(n_upd)
            out["td_after_load"] = _bits(dicts[0]["td_target"])
            _logs(out, "critic_after_load", logs)
            _state(out, agent, target, opts, las, buf)
        else:
            _state(out, agent, target, opts, las, buf)
        return out
    finally:
        lu.FOLD_GATHER = old_fold
        acting._SERIAL[0] = max(old_serial, acting._SERIAL[0])


def _assert_same(a, b, what):
    assert sorted(a) == sorted(b), (what, sorted(set(a) ^ set(b)))
    for k_ in a:
        if k_.startswith("logs:"):
            assert a[k_] == b[k_], (what, k_, a[k_], b[k_])
            assert all(np.isfinite(v) for v in a[k_].values()), (what, k_)
        else:
            assert a[k_].dtype == b[k_].dtype and a[k_].shape == b[k_].shape, (what, k_)
            assert np.array_equal(a[k_].view(np.uint8), b[k_].view(np.uint8)), (what, k_)


@pytest.mark.parametrize("case", sorted(CASES))
def test_concat_agent_equals_its_single_key_twin(case):
    """GRAPH_WARMUP + 3 critic updates (bf16: one), recorded on both sides with launch lists of one size: plain, with a
    priority refresh on the device trees, with an exploration process on a deterministic head, with a discrete head, and
    one update in the bf16 operand mode"""
    a, b = _run(case, "a"), _run(case, "b")
    _assert_same(b, a, case)
    if case != "bf16":
        assert int(b["list_size"][0]) == int(a["list_size"][0]) > 0
        assert not np.array_equal(a["td3"], a["td4"])   # (the updates are not copies of each other)
    if case == "refresh":
        fresh = np.isfinite(a["sum_tree"]) & (a["sum_tree"] != 1.0) & (a["sum_tree"] != 0.0)
        assert fresh[1024:].sum() >= 64, "the refresh wrote no leaves"


def test_actor_updates_acting_and_checkpoints_equal_the_twin():
    """behind the critic updates: online_actor_update (on the recorded batch three times, then on a fresh one),
    alpha_update, offline_actor_update without / with the filter and on a prioritised batch, Agent.sample_action and
    Agent.forward on numpy observations for 1 and 3 environments (a plan for each, float64 input included),
    checkpoint.save_training_state, a load, and one more update"""
    a, b = _run("stochastic", "a", full=True), _run("stochastic", "b", full=True)
    _assert_same(b, a, "full")
    assert not np.array_equal(a["sample1.0"], a["sample1.1"]) and a["sample3.0"].shape == (3, 3)


def test_a_users_encoder_is_recognised_at_first_contact():
    """the same run with an encoder written like a user's (torch.cat in forward, no attribute of this package): the probe of
    the first update finds the order, and everything after it is the package class's run"""
    u, b = _run("stochastic", "u"), _run("stochastic", "b")
    _assert_same(u, b, "user encoder")


def test_a_reference_identity_encoder_that_acts_first_keeps_the_folded_gather():
    """a single-key agent with the reference's own identity encoder, acting on numpy observations BEFORE its first update:
    the encoder ends as an identity encoder (ssac_identity_key, no column order on the buffer), and its recorded update is
    the default one -- the gather folded into the chained launch, the launch list of the package's IdentityEncoder agent
    and one launch shorter than the concat agent's -- with the same bits"""
    r, a, b = _run("stochastic", "r"), _run("stochastic", "a", fold=True), _run("stochastic", "b")
    _assert_same(r, a, "reference identity encoder, acting first")
    assert int(r["list_size"][0]) == int(a["list_size"][0]) == int(b["list_size"][0]) - 1


def test_against_the_twin_with_the_folded_gather():
    """(b) against (a) as it runs by default, its replay gather folded into the chained launch.  The chained launch's
    workgroups then fetch the rows themselves instead of reading what a gather launch wrote: tests/test_hip_cases.py holds
    that switch to equal bits in the producer / consumer form and compares launch forms at atol 2e-6, the bound used
    here.  Whether the bits are equal is printed (profiles/concat_encoder.md records it)."""
    a, b = _run("stochastic", "a", fold=True), _run("stochastic", "b")
    equal = all(np.array_equal(a[k_], b[k_]) for k_ in ("critic0", "target_critic0"))
    print(f"concat agent vs single-key twin with FOLD_GATHER = True: bits {'equal' if equal else 'differ'}; "
          f"max |d critic| = {np.abs(a['critic0'] - b['critic0']).max():.3e}")
    for k_ in ("critic0", "target_critic0"):
        assert np.allclose(a[k_], b[k_], atol=2e-6), k_
    for k in range(6):
        assert np.array_equal(a[f"idx{k}"], b[f"idx{k}"])
        assert np.allclose(a[f"td{k}"], b[f"td{k}"], atol=2e-6)


def test_a_second_order_on_the_same_buffer_is_refused():
    import super_sac_amd as ssa
    dev = torch.device("cuda")
    cfg = CASES["stochastic"]
    s, a, r, s1, d = case_runner._buffers(cfg)
    buf = ssa.replay.ReplayBuffer(cfg["cap"], device=dev)
    buf.load_experience(_split(s), a, r, _split(s1), d)
    first = case_runner.build_engine_agent(cfg, dev)
    first.encoder = ssa.nets.ConcatEncoder(dict(STORED), order=ORDER).to(dev)
    second = case_runner.build_engine_agent(cfg, dev)
    second.encoder = ssa.nets.ConcatEncoder(dict(STORED)).to(dev)
    ssa.learning_utils.ensure_adopted(first, buf)
    with pytest.raises(NotImplementedError, match="already laid out as"):
        ssa.learning_utils.ensure_adopted(second, buf)
    rd = ssa.learning_utils.sample_move_and_augment(
        buf, 8, ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(8)]), 0.0, per=False)
    o = rd["primary_batch"][0]
    idx = np.asarray(rd["priority_idxs"])
    for k_, (c0, c1) in COLS.items():
        assert np.array_equal(o[k_].cpu().numpy(), s["obs"][idx, c0:c1])
