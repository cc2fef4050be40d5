"""GPU: the acting rules that joined the ONE-CALL path (super_sac_amd/acting.py + csrc/ssac_act.hip) -- SUNRISE's UCB rule for
DISCRETE agents (agent.py:259-304, the `if self.discrete:` branch: ssac_act_ucb_discrete behind the packed forwards) and
ensembles above 8 members (reductions up to 32 members, packs above SSAC_MAX_NETS split into several packed launches) -- and
the fallback of a recording that fails.  Method of tests/test_hip_acting_fast.py: the kernel's Philox uniforms regenerated on
the host with _philox4x32_10, agent.py:259-304 restated in float64 numpy."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import case_runner
import ssac_oracle as orc
import synth
from test_hip_bench_bridge import _philox4x32_10

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = 2.0 ** -24            # unit roundoff of fp32
NOISE_SEED = 0x2545F4914F6CDD1D >> 2   # the agents' engine noise seed in these tests (pinned: the draws are the same on every run)
STREAM_SALT = 0x41C7A11D5EEDB00C


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement (pure numpy / float64: runs without a GPU)
def _w64(p):
    return {k: v.detach().numpy().astype(np.float64) for k, v in p.items()}


def _mlp64(p, x):
    """(y, bound): the MLP of mlps.py:32-35 in float64, and a bound of |fp32 result - y| from the magnitudes involved: a K-term
    fp32 dot product is off by at most (K + 1) u sum |w| |x| (u = 2^-24, whatever the summation order), and an error in a
    layer's input reaches the output through the later layers' |W| (ReLU is 1-Lipschitz)"""
    err = np.zeros(x.shape[0])
    h = x
    for k, relu in (("1", True), ("2", True), ("3", False)):
        w, b = p["w" + k], p["b" + k]
        mag = (np.abs(h) @ np.abs(w).T + np.abs(b)).max(-1)              # per row: the largest sum |w| |x| + |b| of the layer
        err = err * np.abs(w).sum(-1).max() + (w.shape[1] + 1) * U24 * mag
        h = h @ w.T + b
        if relu:
            h = np.maximum(h, 0.0)
    return h, err


def _uniforms(seed, draw, n):
    """the uniform of (row b, draw): first word of Philox4x32-10 at counter (b, 0, draw), as discrete_act_kernel forms it"""
    cnt = np.stack([np.arange(n), np.zeros(n, np.int64), np.full(n, draw & 0xFFFFFFFF), np.full(n, draw >> 32)], 1)
    return _philox4x32_10(cnt, (seed & 0xFFFFFFFF, seed >> 32))[:, 0].astype(np.float32) * np.float32(2.3283064365386963e-10)


def restate_discrete_ucb(actors, critics, s, bonus, seed, offsets, call_no):
    """agent.py:259-304 for a discrete agent.  actors[e], critics[m][j]: float64 parameter dicts; s (n x S) float64;
    offsets[e]: member e's stream offset.  Returns (action (n,), skip (n,), candidates (E, n), mean (E, n)).
    skip[b]: the top two UCB values of two DIFFERENT actions lie closer than the fp32 rounding of the sum --
      tol = 2 (1 + bonus sqrt(E / (E - 1))) dq + (E + 6) u (1 + bonus) max |q|:
    dq bounds the fp32 forward's error of a critic value (_mlp64; the min over a member's nets is 1-Lipschitz), the unbiased
    std of E values moves by at most sqrt(E / (E - 1)) times the largest move of a value, both UCB values move (factor 2),
    and the E-term sum, the division, the squares, the square root and the final multiply-add round (E + 6) times at
    the size of the values."""
    E, n = len(actors), s.shape[0]
    cands = np.zeros((E, n), np.int64)
    for e in range(E):
        logits = _mlp64(actors[e], s)[0]
        pr = np.exp(logits - logits.max(-1, keepdims=True))
        pr /= pr.sum(-1, keepdims=True)
        u = _uniforms(seed, offsets[e] + call_no, n)
        for b in range(n):
            cands[e, b] = min(int(np.searchsorted(np.cumsum(pr[b]), float(u[b]) * pr[b].sum(), side="right")), pr.shape[1] - 1)
    q, dq = [], 0.0
    for nets in critics:                                     # Critic.forward: default subset, min over the member's nets
        ys = [_mlp64(p, s) for p in nets]
        q.append(np.min(np.stack([y for y, _ in ys], 0), 0))
        dq = max(dq, max(float(err.max()) for _, err in ys))
    q = np.stack(q, 0)                                       # (members, n, A)
    qa = np.stack([q[:, np.arange(n), cands[e]] for e in range(E)], 1)          # (members, candidates, n)
    mean = qa.mean(0)
    ucb = mean + bonus * qa.std(0, ddof=1)
    best = ucb.argmax(0)                                     # (first maximum, as torch.argmax on the CPU)
    act = cands[best, np.arange(n)]
    tol = 2.0 * (1.0 + bonus * np.sqrt(E / (E - 1.0))) * dq + (E + 6) * U24 * (1.0 + bonus) * float(np.abs(q).max())
    skip = np.zeros(n, bool)
    for b in range(n):
        other = ucb[cands[:, b] != act[b], b]
        skip[b] = other.size > 0 and ucb[best[b], b] - other.max() < tol
    return act, skip, cands, mean


# ---------------------------------------------------------------------------------------------------------------------------
def _pair(cfg, ucb=0.0):
    agent = case_runner.build_engine_agent(cfg, torch.device(DEV))
    agent.ucb_bonus = ucb
    agent.__dict__["_ssac_noise"] = [NOISE_SEED, 0, 0]
    return agent, case_runner._oracle_agent(cfg)


def _calls(plan):
    from super_sac_amd._lib import lib
    return int(lib.ssac_act_calls(plan.handle))


def _oracle64(oa):
    return [_w64(a) for a in oa.actors], [[_w64(p) for p in nets] for nets in oa.critics]


def _check_discrete_ucb(agent, oa, obs, n, bonus, state=None):
    """one call of the fast path against the restatement; returns (action, restated action, skip, candidates, means)"""
    from super_sac_amd import acting
    act = agent.sample_action({"obs": obs}, num_envs=n)
    assert ("sample", n, float(bonus)) in acting._PLANS.get(agent, {}), "the call did not take the recorded path"
    plan = acting._PLANS[agent][("sample", n, float(bonus))]
    assert act.dtype == np.int64 and act.shape == ((n, 1) if n > 1 else (1,))
    E = len(agent.actors)
    seed = plan.rng_for(agent, 0).seed
    assert seed == (NOISE_SEED ^ STREAM_SALT) & (2 ** 64 - 1)
    offsets = [plan.rng_for(agent, e).offset for e in range(E)]
    assert all(offsets[e] - offsets[0] == e << 40 for e in range(E))          # every member on a stream of its own
    s = (obs.reshape(n, -1) if state is None else state).astype(np.float64)
    actors, critics = _oracle64(oa)
    want, skip, cands, mean = restate_discrete_ucb(actors, critics, s, bonus, seed, offsets, _calls(plan) - 1)
    return act.reshape(n), want, skip, cands, mean


SUNRISE_DISCRETE = synth.CASES["sunrise_discrete"]
ATARI_SUNRISE = dict(synth.CASES["atari_pixels"], E=3, weight_type="sunrise", temp=20.0)


@pytest.mark.parametrize("n", [1, 5, 16])
def test_discrete_ucb_equals_the_restated_reference(n, monkeypatch):
    """1. the `sunrise_discrete` shape (3 members x 2 critics, 8 -> 64 -> 64 -> 4).  The seeds (observations 41 + n, the pinned
    noise seed, plan serial 7000 + n) were checked on the CPU: the float64 restatement alone skips no environment of these
    calls (cap: 2 %)."""
    from super_sac_amd import acting
    monkeypatch.setattr(acting, "_SERIAL", [7000 + n])
    cfg = SUNRISE_DISCRETE
    agent, oa = _pair(cfg, ucb=0.7)
    rs = np.random.RandomState(41 + n)
    envs = skipped = 0
    for rep in range(6):   # (the first call records, the others replay)
        obs = rs.standard_normal((n, cfg["obs"]) if n > 1 else (cfg["obs"],)).astype(np.float32)
        got, want, skip, _, _ = _check_discrete_ucb(agent, oa, obs, n, 0.7)
        print(f"n={n} rep={rep}: action {got.tolist()} restated {want.tolist()} skipped {int(skip.sum())}")
        assert np.array_equal(got[~skip], want[~skip])
        envs, skipped = envs + n, skipped + int(skip.sum())
    assert skipped <= 0.02 * envs


def test_discrete_ucb_on_atari_frames(monkeypatch):
    """1. a SUNRISE agent on 4 x 84 x 84 uint8 frames, n = 1: the recorded encoder in front of the rule.  agent.py:259-304
    starts from the state representation: the restatement takes it from the encoder's own forward (lines 254-257)."""
    from super_sac_amd import acting
    monkeypatch.setattr(acting, "_SERIAL", [7100])
    cfg = ATARI_SUNRISE
    agent, oa = _pair(cfg, ucb=0.7)
    rs = np.random.RandomState(61)
    skipped = 0
    for rep in range(6):
        obs = rs.randint(0, 256, (4, 84, 84)).astype(np.uint8)
        with torch.no_grad():
            state = agent._state_rep(agent._process_obs({"obs": obs}, 1), False).cpu().numpy()
        got, want, skip, _, _ = _check_discrete_ucb(agent, oa, obs, 1, 0.7, state=state)
        print(f"atari rep={rep}: action {got.tolist()} restated {want.tolist()} skipped {int(skip.sum())}")
        assert np.array_equal(got[~skip], want[~skip])
        skipped += int(skip.sum())
    assert skipped <= 0.02 * 6
    assert acting._PLANS[agent][("sample", 1, 0.7)].pixel_shape == (4, 84, 84)


def test_discrete_ucb_is_really_ucb(monkeypatch):
    """2. member 1's critics (both nets: the member's value is their min) get -3 on action 2: the mean of that action drops by 1,
    its std over the 3 members rises by ~1.73.  With a large bonus the std term dominates and action 2 wins wherever an actor
    proposes it; with bonus -> 0 the rule is the arg-max of the mean over the candidates."""
    from super_sac_amd import acting
    monkeypatch.setattr(acting, "_SERIAL", [7200])
    cfg = SUNRISE_DISCRETE
    agent, oa = _pair(cfg)
    with torch.no_grad():
        for j in range(cfg["N"]):
            agent.critics[1].nets[j].out.bias[2] -= 3.0
            oa.critics[1][j]["b3"][2] -= 3.0
    n = 16
    obs = np.random.RandomState(77).standard_normal((n, cfg["obs"])).astype(np.float32)
    chosen = {}
    for bonus in (2.0, 1e-6):
        agent.ucb_bonus = bonus
        got, want, skip, cands, mean = _check_discrete_ucb(agent, oa, obs, n, bonus)
        assert not skip.any() and np.array_equal(got, want)
        chosen[bonus] = (got, cands, mean)
    got, cands, mean = chosen[1e-6]
    assert np.array_equal(got, cands[mean.argmax(0), np.arange(n)])            # bonus -> 0: the arg-max of the mean
    got, cands, mean = chosen[2.0]
    proposed = (cands == 2).any(0)
    assert proposed.sum() >= 4 and np.all(got[proposed] == 2)                   # the std term dominates
    assert np.any(got != cands[mean.argmax(0), np.arange(n)])                   # ... and changes the choice


def test_discrete_ucb_call_counter_advances(monkeypatch):
    """3. two consecutive calls on the SAME observation: the uniforms of call k are those of draw (offset + k), different from
    call k + 1's, and each call's action is the restatement's at its own draw number"""
    from super_sac_amd import acting
    monkeypatch.setattr(acting, "_SERIAL", [7300])
    cfg = SUNRISE_DISCRETE
    agent, oa = _pair(cfg, ucb=0.7)
    n = 16
    obs = np.random.RandomState(78).standard_normal((n, cfg["obs"])).astype(np.float32)
    seen = []
    for rep in range(3):
        got, want, skip, cands, _ = _check_discrete_ucb(agent, oa, obs, n, 0.7)
        plan = acting._PLANS[agent][("sample", n, 0.7)]
        assert not skip.any() and np.array_equal(got, want)   # (pinned seeds: checked on the CPU, no near tie)
        seen.append((_calls(plan), _uniforms(plan.rng_for(agent, 0).seed, plan.rng_for(agent, 0).offset + _calls(plan) - 1, n), cands))
    assert [c for c, _, _ in seen] == [seen[0][0], seen[0][0] + 1, seen[0][0] + 2]
    assert not np.array_equal(seen[0][1], seen[1][1]) and not np.array_equal(seen[1][1], seen[2][1])
    assert not np.array_equal(seen[0][2], seen[1][2])   # (the candidates of the two calls differ: the draws did move)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. large ensembles
def _eps_of_call(agent, plan, member, call_no, n, A):
    from super_sac_amd import _lib
    from super_sac_amd._lib import check, lib
    r = plan.rng_for(agent, member)
    r = _lib.Rng(r.seed, None, r.offset + call_no)
    out = torch.empty(n, A, device=DEV)
    check(lib.ssac_philox_normal(out.data_ptr(), n, A, C.byref(r), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("n", [1, 5])
def test_twelve_member_forward_and_sample_match_the_oracle(n):
    """E = 12 REDQ-shaped agent (17 -> 64 -> 64 -> 12, 4 critics per member): as test_fast_forward_and_sample_match_the_oracle"""
    from super_sac_amd import acting
    cfg = dict(synth.CASES["redq_small"], E=12)
    agent, oa = _pair(cfg)
    rs = np.random.RandomState(20 + n)
    A = cfg["act"]
    for rep in range(3):
        obs = rs.standard_normal((n, cfg["obs"]) if n > 1 else (cfg["obs"],)).astype(np.float32)
        s = torch.from_numpy(obs.reshape(n, -1))
        act = agent.forward({"obs": obs}, num_envs=n)
        assert ("forward", n, 0.0) in acting._PLANS.get(agent, {})
        want = torch.stack([torch.tanh(orc.mlp3(a, s)[0][:, :A]) for a in oa.actors], 0).mean(0).clamp(-1, 1).numpy()
        assert act.dtype == np.float32 and act.shape == ((n, A) if n > 1 else (A,))
        np.testing.assert_allclose(act.reshape(n, A), want, atol=2e-6)
        random.seed(200 + rep)
        k = random.choice(range(cfg["E"]))
        random.seed(200 + rep)
        act, dist = agent.sample_action({"obs": obs}, num_envs=n, return_dist=True)
        assert ("sample", n, 0.0) in acting._PLANS.get(agent, {})
        plan = acting._PLANS[agent][("sample", n, 0.0)]
        eps = _eps_of_call(agent, plan, k, _calls(plan) - 1, n, A)
        out = orc.mlp3(oa.actors[k], s)[0]
        want = orc.tanh_normal_sample(out, oa.lo, oa.hi, eps)[0].clamp(-1, 1).numpy()
        np.testing.assert_allclose(act.reshape(n, A), want, atol=3e-6)
        np.testing.assert_allclose(dist.cpu().numpy(), out.numpy(), atol=3e-6)


def _check_continuous_ucb(cfg, n, reps, seed):
    """as test_fast_ucb_picks_the_argmax_candidate_and_equals_the_general_path, for any ensemble"""
    from super_sac_amd import acting
    agent, oa = _pair(cfg, ucb=0.7)
    rs = np.random.RandomState(seed)
    E, A = cfg["E"], cfg["act"]
    for rep in range(reps):
        obs = rs.standard_normal((n, cfg["obs"])).astype(np.float32)
        act = agent.sample_action({"obs": obs}, num_envs=n)
        assert ("ucb", n, 0.7) in acting._PLANS.get(agent, {}), "the call did not take the recorded path"
        plan = acting._PLANS[agent][("ucb", n, 0.7)]
        call_no = _calls(plan) - 1
        eps = [_eps_of_call(agent, plan, a, call_no, n, A) for a in range(E)]
        s = torch.from_numpy(obs)
        cands = torch.stack([orc.tanh_normal_sample(orc.mlp3(oa.actors[a], s)[0], oa.lo, oa.hi, eps[a])[0] for a in range(E)], 0)
        q = torch.stack([torch.stack([orc.ensemble_q(oa.critics[c], s, cands[a]).squeeze(-1) for a in range(E)], 0)
                         for c in range(E)], 0)                         # (members, candidates, envs)
        ucb = q.mean(0) + 0.7 * q.std(0)
        want = cands[ucb.argmax(0), torch.arange(n)].clamp(-1, 1)
        top2 = ucb.topk(2, dim=0).values
        clear = ((top2[0] - top2[1]) > 1e-4).numpy()   # (a near-tie may flip under fp32 reordering)
        assert clear.sum() >= n - 1
        np.testing.assert_allclose(act[clear], want.numpy()[clear], atol=3e-6)
    return agent


def test_twelve_member_continuous_ucb_matches_the_oracle():
    _check_continuous_ucb(dict(synth.CASES["sunrise"], E=12), n=6, reps=3, seed=31)


def test_eight_members_of_ten_critics_act_on_a_split_pack(monkeypatch):
    """8 x 10 = 80 critics: above SSAC_MAX_NETS (64) -- two packed critic launches in one recorded list, never a refusal"""
    from super_sac_amd import acting
    fused, real = [], acting.lib.ssac_mlp3_fwd_fused

    def counted(*args):
        fused.append(int(args[2]))
        return real(*args)
    monkeypatch.setattr(acting.lib, "ssac_mlp3_fwd_fused", counted, raising=False)
    agent = _check_continuous_ucb(dict(synth.CASES["sunrise"], E=8, N=10), n=4, reps=3, seed=32)
    assert fused == [8, 64, 16], "one recording: the packed actors, then the 80 critics as packed launches of 64 and 16 nets"
    assert acting._PLANS[agent][("ucb", 4, 0.7)].lists == {None: 0} and agent not in acting._FAILED


@pytest.mark.parametrize("E", [12, 32])
def test_discrete_large_ensembles_match_the_restatement(E, monkeypatch):
    """the wide (32-pointer) categorical / greedy reductions and the discrete UCB kernel above 8 lanes: E = 12 and the
    E = 32 boundary at the `sunrise_discrete` shape.  greedy = arg-max of the mean softmax, sample = the drawn actor's
    categorical inversion, UCB = the restatement; seeds checked on the CPU (no near tie in the UCB calls)."""
    from super_sac_amd import acting
    monkeypatch.setattr(acting, "_SERIAL", [7500 + E])
    cfg = dict(SUNRISE_DISCRETE, E=E)
    agent, oa = _pair(cfg)
    actors, _ = _oracle64(oa)
    n, A = 16, cfg["act"]
    rs = np.random.RandomState(54 + E)
    for rep in range(3):
        obs = rs.standard_normal((n, cfg["obs"])).astype(np.float32)
        s = obs.astype(np.float64)
        probs = []
        for a in actors:
            lg = _mlp64(a, s)[0]
            pr = np.exp(lg - lg.max(-1, keepdims=True))
            probs.append(pr / pr.sum(-1, keepdims=True))
        mean_p = np.mean(probs, 0)
        greedy = agent.forward({"obs": obs}, num_envs=n)
        assert ("forward", n, 0.0) in acting._PLANS.get(agent, {})
        top2 = np.sort(mean_p, -1)[:, -2:]
        clear = top2[:, 1] - top2[:, 0] > 1e-5      # (fp32 softmax of O(1) logits errs by a few ulp of 1: far below)
        assert clear.sum() >= n - 1 and np.array_equal(greedy[clear, 0], mean_p.argmax(-1)[clear])
        agent.ucb_bonus = 0.0
        random.seed(300 + rep)
        k = random.choice(range(E))
        random.seed(300 + rep)
        got = agent.sample_action({"obs": obs}, num_envs=n)
        plan = acting._PLANS[agent][("sample", n, 0.0)]
        r = plan.rng_for(agent, k)
        u = _uniforms(r.seed, r.offset + _calls(plan) - 1, n)
        cum = np.cumsum(probs[k], -1)
        want = np.array([min(int(np.searchsorted(cum[b], float(u[b]) * cum[b, -1], side="right")), A - 1) for b in range(n)])
        edge = np.array([np.min(np.abs(cum[b] - float(u[b]) * cum[b, -1])) < 1e-5 for b in range(n)])   # (a draw on a boundary)
        assert edge.sum() <= 1 and np.array_equal(got[~edge, 0], want[~edge])
        agent.ucb_bonus = 0.7
        got, want, skip, _, _ = _check_discrete_ucb(agent, oa, obs, n, 0.7)
        assert not skip.any() and np.array_equal(got, want)


def test_forty_members_take_the_general_path():
    from super_sac_amd import acting
    cfg = dict(synth.CASES["redq_small"], E=40, N=2)
    agent, oa = _pair(cfg)
    n, A = 3, cfg["act"]
    obs = np.random.RandomState(33).standard_normal((n, cfg["obs"])).astype(np.float32)
    s = torch.from_numpy(obs)
    act = agent.forward({"obs": obs}, num_envs=n)
    want = torch.stack([torch.tanh(orc.mlp3(a, s)[0][:, :A]) for a in oa.actors], 0).mean(0).clamp(-1, 1).numpy()
    np.testing.assert_allclose(act, want, atol=3e-6)
    # the sample: the general path's own answer under the same seeds (host draw of the actor, device noise)
    torch.manual_seed(600); random.seed(600)
    smp = agent.sample_action({"obs": obs}, num_envs=n)
    assert agent not in acting._PLANS
    acting.ENABLED = False
    try:
        torch.manual_seed(600); random.seed(600)
        ref = agent.sample_action({"obs": obs}, num_envs=n)
    finally:
        acting.ENABLED = True
    assert smp.shape == (n, A) and np.array_equal(smp, ref)
    # ... which is the oracle's tanh-normal sample of the drawn actor on the noise the device generator gave
    torch.manual_seed(600); random.seed(600)
    k = random.choice(range(cfg["E"]))
    eps = torch.randn(n, A, device=DEV).cpu()
    want = orc.tanh_normal_sample(orc.mlp3(oa.actors[k], s)[0], oa.lo, oa.hi, eps)[0].clamp(-1, 1).numpy()
    np.testing.assert_allclose(smp, want, atol=3e-6)


# ---------------------------------------------------------------------------------------------------------------------------
def test_a_failed_recording_falls_back_to_the_general_path(monkeypatch, recwarn):
    """5. the rule's launch answers with an error code while the plan is recorded (a patched entry of the binding table: nothing
    is launched, nothing faults): the call is served by the general path -- the same action and the same host draws as with
    the fast path switched off --, no half-built plan stays behind, and the second call does not record again"""
    from super_sac_amd import acting
    cfg = SUNRISE_DISCRETE
    agent, _ = _pair(cfg, ucb=0.7)
    n = 5
    obs = np.random.RandomState(90).standard_normal((n, cfg["obs"])).astype(np.float32)
    tried = []

    def refuse(*args):
        tried.append(len(args))
        return 1
    monkeypatch.setattr(acting.lib, "ssac_act_ucb_discrete", refuse, raising=False)
    for call in range(2):
        torch.manual_seed(500 + call); random.seed(500 + call)
        got = agent.sample_action({"obs": obs}, num_envs=n)
        after = random.getstate()
        assert agent not in acting._PLANS and ("sample", n, 0.7) in acting._FAILED[agent]
        assert len(tried) == 1, "the recording was tried again"
        acting.ENABLED = False
        try:
            torch.manual_seed(500 + call); random.seed(500 + call)
            want = agent.sample_action({"obs": obs}, num_envs=n)
        finally:
            acting.ENABLED = True
        assert np.array_equal(got, want) and random.getstate() == after
    told = [w for w in recwarn.list if issubclass(w.category, RuntimeWarning) and "super_sac_amd.acting" in str(w.message)]
    assert len(told) == 1, "a key that leaves the recorded path says so, once"
    # the other rules of the same agent are not affected
    agent.forward({"obs": obs}, num_envs=n)
    assert ("forward", n, 0.0) in acting._PLANS[agent]


def test_discrete_ucb_reads_the_weights_of_the_moment(monkeypatch):
    """6. the packs are refilled from the members' arenas at the head of every call: an optimizer step on the critics is seen
    by the next call"""
    from super_sac_amd import acting
    monkeypatch.setattr(acting, "_SERIAL", [7400])
    cfg = SUNRISE_DISCRETE
    agent, oa = _pair(cfg, ucb=1e-6)
    n = 16
    obs = np.random.RandomState(79).standard_normal((n, cfg["obs"])).astype(np.float32)
    got, want, skip, cands, _ = _check_discrete_ucb(agent, oa, obs, n, 1e-6)
    assert np.array_equal(got[~skip], want[~skip])
    # one SGD step (lr 1) on a gradient of -5 at the bias of action 3, every critic: q(., 3) rises by 5 everywhere
    params = [net.out.bias for c in agent.critics for net in c.nets]
    opt = torch.optim.SGD(params, lr=1.0)
    for p in params:
        p.grad = torch.zeros_like(p)
        p.grad[3] = -5.0
    opt.step()
    for nets in oa.critics:
        for p in nets:
            with torch.no_grad():
                p["b3"][3] += 5.0
    plan = acting._PLANS[agent][("sample", n, 1e-6)]
    got, want, skip, cands, _ = _check_discrete_ucb(agent, oa, obs, n, 1e-6)
    assert acting._PLANS[agent][("sample", n, 1e-6)] is plan, "an in-place step must not invalidate the plan"
    assert np.array_equal(got[~skip], want[~skip])
    proposed = (cands == 3).any(0)
    assert proposed.sum() >= 4 and np.all(got[proposed] == 3)
