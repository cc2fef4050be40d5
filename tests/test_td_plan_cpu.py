"""CPU: learning_utils.td_member_plan -- the ONE decision "which head produces a' of a member's TD target, in which launch,
with noise from where, consuming which host draws" -- against a verbatim restatement of the expressions it replaced (commit
58224a5: compute_td_targets' fuse_sample / chain / explore_launch / in-kernel clause / use_entropy assignments with the
branches of _explore_action and _actor_sample, skip_td_draws, learning._in_kernel_noise, recording_noise_buffers), over the
full cross product of their inputs.  No kernel runs and no generator is consumed: the draw sites are wrapped."""
import itertools
import types

import pytest

KINDS = ("stochastic", "deterministic", "discrete", "beta")
FLAGS = (False, True)


@pytest.fixture
def mods():
    import super_sac_amd as ssa
    return ssa, ssa.learning, ssa.learning_utils


def _set_switches(mp, ssa, lu, chain_launch, in_kernel, stock):
    mp.setattr(lu, "CHAIN_LAUNCH", chain_launch)
    mp.setattr(lu, "IN_KERNEL_NOISE", in_kernel)
    if not stock:
        mp.setattr(ssa.rng, "draw_normal", lambda shape, device: None)
    assert ssa.rng.normal_is_stock() == stock


# ---- the parent's rules, restated (sw = CHAIN_LAUNCH, IN_KERNEL_NOISE, the generator is the stock one; random_process and
# ---- co_fwd are an object or None, as there)
def _p_fuse_sample(kind, a_fused, random_process):
    return kind == "stochastic" and a_fused and random_process is None


def _p_chain(sw, fuse_sample, co_fwd, want_bwd, target_sharded, capture, fused_dbuf, out_dim):
    return bool(sw[0] and fuse_sample and co_fwd is not None and want_bwd
                and (not target_sharded or capture)
                and fused_dbuf
                and out_dim == 1)


def _p_explore_launch(sw, explore, random_process, kind, capture):
    return bool(explore and random_process is not None and kind in ("stochastic", "deterministic")
                and (capture or (sw[1] and sw[2])))


def _p_actor_sample(m, chain):
    """_actor_sample's three exits"""
    if m is not None and chain:
        return "chain"
    if m is not None:
        return "dual"
    return "fused"


def _p_member(sw, kind, random_process, explore, a_fused, capture, want_fwd, want_bwd, fused_dbuf, out_dim, target_sharded):
    """compute_td_targets' branches as the parent wrote them, noting instead of launching:
    (head, launch, noise, draws, use_entropy)"""
    co_fwd = object() if want_fwd else None
    fuse_sample = _p_fuse_sample(kind, a_fused, random_process)
    chain = _p_chain(sw, fuse_sample, co_fwd, want_bwd, target_sharded, capture, fused_dbuf, out_dim)
    launch = "layers" if not fuse_sample else None     # `if not fuse_sample: engine.mlp_forward(a_arena, ...)`
    draws = []
    use_entropy = 0
    explore_launch = _p_explore_launch(sw, explore, random_process, kind, capture)
    if kind == "discrete":
        head = "discrete"
    elif kind == "beta":
        head = "beta"
        use_entropy = 1
        if random_process is not None:
            draws.append("proc")
            use_entropy = 0
    elif explore_launch:
        head = "explore"                               # _explore_action
        if sw[1] and sw[2]:
            draws.append("tick")
        else:
            assert capture
            if kind == "stochastic":
                draws.append("eps")
            draws.append("proc")
    elif kind == "stochastic":
        head = "tanh_normal"
        if fuse_sample and sw[1] and sw[2]:
            draws.append("tick")
            launch = _p_actor_sample(co_fwd, chain)
            eps = None
        else:
            draws.append("eps")
            eps = True
        if eps is not None and fuse_sample:
            launch = _p_actor_sample(co_fwd, chain)
        use_entropy = 1
        if random_process is not None:
            draws.append("proc")
            use_entropy = 0
    else:
        head = "deterministic"
        if random_process is not None:
            draws.append("proc")
        else:
            use_entropy = 1
    return head, launch, "kernel" if "tick" in draws else "buffer", tuple(draws), use_entropy


def test_the_plan_is_the_parents_expressions(mods, monkeypatch):
    ssa, L, lu = mods
    process = object()
    n, seen = 0, {"head": set(), "launch": set(), "noise": set()}
    for sw in itertools.product(FLAGS, repeat=3):
        with monkeypatch.context() as mp:
            _set_switches(mp, ssa, lu, *sw)
            for kind, rp, explore, a_fused, capture, want_fwd, want_bwd, dbuf, out_dim, sharded in itertools.product(
                    KINDS, (None, process), FLAGS, FLAGS, FLAGS, FLAGS, FLAGS, FLAGS, (1, 3), FLAGS):
                plan = lu.td_member_plan(kind, rp is not None, explore, a_fused, capture, want_fwd, want_bwd, dbuf,
                                         out_dim == 1, sharded)
                want = _p_member(sw, kind, rp, explore, a_fused, capture, want_fwd, want_bwd, dbuf, out_dim, sharded)
                assert tuple(plan) == want, (sw, kind, rp is not None, explore, a_fused, capture, want_fwd, want_bwd, dbuf,
                                             out_dim, sharded)
                # the parent's remaining readers of the same expressions
                fuse_sample = _p_fuse_sample(kind, a_fused, rp)
                assert (plan.launch in ("fused", "layers")) == (not (fuse_sample and want_fwd))     # ensure_gathered up front
                assert (plan.launch == "chain") == _p_chain(sw, fuse_sample, object() if want_fwd else None, want_bwd, sharded,
                                                            capture, dbuf, out_dim)
                for field in seen:
                    seen[field].add(getattr(plan, field))
                n += 1
    assert n == 4 * 2 ** 12 == 16384
    assert seen == {"head": {"discrete", "beta", "explore", "tanh_normal", "deterministic"},
                    "launch": {"chain", "dual", "fused", "layers"}, "noise": {"kernel", "buffer"}}


def _p_skip_td_draws(sw, kind, a_fused, random_process):
    """the parent's skip_td_draws, noting instead of drawing"""
    events = []
    if kind != "discrete":
        if kind == "stochastic":
            fused = a_fused and random_process is None
            events.append("tick" if fused and sw[1] and sw[2] else "normal")
        if random_process is not None:
            events.append("normal")
    return events + ["subset"]


def _actor(kind, A=3):
    a = types.SimpleNamespace(action_size=A, dist_impl={"deterministic": "deterministic", "beta": "beta"}.get(kind, "tanh_normal"))
    if kind == "discrete":
        a.act_p = None
    return a


class _Stream(list):
    """an agent's _ssac_noise whose tick is seen"""

    def __init__(self, events):
        super().__init__([7, 0, 0])
        self.events = events

    def __setitem__(self, k, v):
        assert k == 1 and v == self[1] + 1
        self.events.append("tick")
        super().__setitem__(k, v)


@pytest.mark.parametrize("kind", KINDS)
def test_the_skipper_consumes_what_the_owners_plan_lists(mods, monkeypatch, kind):
    ssa, L, lu = mods
    assert lu.actor_kind(_actor(kind)) == kind
    B, process, n = 32, object(), 0
    for rp, a_fused, in_kernel, stock in itertools.product((None, process), FLAGS, FLAGS, FLAGS):
        with monkeypatch.context() as mp:
            sw = (True, in_kernel, stock)
            _set_switches(mp, ssa, lu, *sw)
            events = []
            # (the two draw sites of learning_utils, not rng.draw_normal: replacing that is what normal_is_stock() sees)
            mp.setattr(lu, "draw_normal", lambda shape, device: events.append("normal") or shape == (B, 3) or pytest.fail(str(shape)))
            mp.setattr(lu, "draw_subset", lambda num, k: events.append("subset") or (num, k) == (5, 2) or pytest.fail("subset"))
            mp.setattr(lu.engine, "bind_arena", lambda *a: types.SimpleNamespace(fused=a_fused))
            agent = types.SimpleNamespace(_ssac_noise=_Stream(events))
            lu.skip_td_draws(agent, _actor(kind), B, "cpu", 5, 2, rp)
            owner = lu.td_member_plan(kind, rp is not None, False, a_fused, False)
            assert events == [{"tick": "tick", "eps": "normal", "proc": "normal"}[d] for d in owner.draws] + ["subset"]
            assert events == _p_skip_td_draws(sw, kind, a_fused, rp)      # ... which is what the parent's skipper consumed
            assert agent._ssac_noise[1] == owner.draws.count("tick") and (owner.noise == "kernel") == ("tick" in events)
            n += 1
    assert n == 16


def _p_in_kernel_noise(sw, proc_dev, kind, a_fused):
    """the parent's learning._in_kernel_noise"""
    if not (sw[1] and sw[2]):
        return False
    return proc_dev is not None or (kind == "stochastic" and a_fused)


@pytest.mark.parametrize("kind", KINDS[:3])
@pytest.mark.parametrize("explore", FLAGS)
@pytest.mark.parametrize("refresh", FLAGS)
def test_a_recordings_noise_source_and_buffers_are_the_plans(mods, monkeypatch, kind, explore, refresh):
    """the grid of tests/test_priority_recording_cpu.py (which pins the buffer lists themselves) x the switches x the
    actor's arena.  One cell leaves the parent: a DISCRETE head with verdict.explore -- a discrete agent called with
    discrete=False and a process, which no update can carry out (its critics take s, the call feeds them [s | a]).  The
    parent called that recording's noise in-kernel although it draws none; the plan says what the head does: no noise."""
    ssa, L, lu = mods
    for in_kernel, stock, a_fused in itertools.product(FLAGS, FLAGS, FLAGS):
        with monkeypatch.context() as mp:
            sw = (True, in_kernel, stock)
            _set_switches(mp, ssa, lu, *sw)
            mp.setattr(L.engine, "bind_arena", lambda *a: types.SimpleNamespace(fused=a_fused))
            gs = types.SimpleNamespace(proc_dev=object() if explore else None, dev="cpu")
            got = L._in_kernel_noise(gs, types.SimpleNamespace(actors=[_actor(kind)]))
            # the plan of the recording call: capture open, a process exactly when the verdict said explore
            plan = lu.td_member_plan(kind, explore, explore, a_fused, True)
            assert got == (plan.noise == "kernel")
            if not (kind == "discrete" and explore):
                assert got == _p_in_kernel_noise(sw, gs.proc_dev, kind, a_fused)
            else:
                assert got is False and plan.draws == ()
            # what the recording refills on the host is what that plan draws from buffers
            before, after = lu.recording_noise_buffers(kind, explore, refresh, got)
            assert before == [d for d in plan.draws if d != "tick"] and set(before) <= {"eps", "proc"}
            # ... and prepare()'s list (made before the noise source is known) is the buffer-noise plan's, whatever the arena
            hook_before, hook_after = lu.recording_noise_buffers(kind, explore, refresh, False)
            assert hook_before == list(lu.td_member_plan(kind, explore, explore, a_fused, True, in_kernel=False).draws)
            assert after == ([] if got else hook_after)
