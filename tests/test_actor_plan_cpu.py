"""CPU: learning._actor_member_plan -- the ONE decision "which launch form does this member's online actor update take, and
where does its noise come from" -- against a verbatim restatement of the five predicates it replaced (commit 65950e7:
_actor_fused_member, _actor_chain_form's condition, _member_noise_in_kernel, the arena clause of `recordable`, and
owner_in_kernel of a member another rank owns), over the full cross product of their inputs.  No kernel runs: the arenas are
stand-ins and ssac_fused_row_tiles reads dimensions only."""
import ctypes as C
import itertools

import pytest

KINDS = ("stochastic", "deterministic", "discrete", "beta")
OBS = 17
# (B, A, hidden, n_nets)
SHAPES = ((128, 6, 64, 4), (2048, 6, 256, 2), (2064, 6, 256, 2), (512, 32, 256, 2), (512, 33, 256, 2), (128, 17, 256, 16),
          (256, 17, 256, 16))


class _Arena:
    def __init__(self, fused, fused_dbuf, in_dim, hidden, out_dim, n_nets):
        self.fused, self.fused_dbuf, self.in_dim, self.hidden, self.out_dim, self.n_nets = fused, fused_dbuf, in_dim, hidden, out_dim, n_nets

    def desc(self):
        from super_sac_amd import _lib
        return _lib.MlpDesc(0, 0, self.n_nets, self.in_dim, self.hidden, self.out_dim)


def _workgroups(c_arena, B):
    from super_sac_amd import _lib
    return (B + 15) // 16 + int(_lib.lib.ssac_fused_row_tiles(C.byref(c_arena.desc()), B, c_arena.n_nets)) * c_arena.n_nets


# ---- the parent's rules, restated (sw = FUSED_ACTOR, ACTOR_CHAIN, IN_KERNEL_NOISE, the generator is the stock one)
def _p_fused_member(sw, kind, random_process, use_baseline, clip, a_arena, c_arena):
    return bool(sw[0] and kind == "stochastic" and random_process is None and not use_baseline and not clip
                and a_arena.fused and c_arena.fused_dbuf and c_arena.out_dim == 1)


def _p_chain_form(sw, a_arena, A, B, c_arena):
    if not (sw[1] and a_arena.fused and A <= 32 and a_arena.hidden * A <= 512 * 9 and B <= 2048 and c_arena.fused_dbuf
            and c_arena.out_dim == 1):
        return False
    return _workgroups(c_arena, B) <= 256


def _p_noise_in_kernel(sw, chain, rec_eps):
    return bool(chain and sw[2] and sw[3] and rec_eps is None)


def _p_recordable_arenas(sw, kind, random_process, use_baseline, clip, a_arena, c_arena, sharded):
    return bool(sw[0] and not clip and random_process is None and not use_baseline and not sharded
                and kind == "stochastic" and a_arena.fused and c_arena.fused_dbuf and c_arena.out_dim == 1)


def _p_owner_in_kernel(sw, kind, random_process, use_baseline, clip, a_arena, c_arena, A, B, sharded, rec_eps):
    return bool(_p_fused_member(sw, kind, random_process, use_baseline, clip, a_arena, c_arena) and not sharded
                and _p_noise_in_kernel(sw, _p_chain_form(sw, a_arena, A, B, c_arena), rec_eps))


def _p_launch_site(sw, kind, random_process, use_baseline, clip, a_arena, c_arena, A, B, sharded, rec_eps):
    """the three per-member branches of the parent's loop body and the noise pointer of the second"""
    if not _p_fused_member(sw, kind, random_process, use_baseline, clip, a_arena, c_arena):
        return "layers", "draw"
    if sharded:
        return "fused", "draw"
    chain = _p_chain_form(sw, a_arena, A, B, c_arena)
    if _p_noise_in_kernel(sw, chain, rec_eps):
        noise = "kernel"
    else:
        noise = "recording" if rec_eps is not None else "draw"
    return ("chain" if chain else "fused"), noise


def test_the_shapes_straddle_one_resident_round():
    """what ssac_fused_row_tiles says about the shapes: both sides of the chained launch's one-resident-round limit are
    in the product.  (B 128 with 16 critics, hidden 256, is 8 + 16 x 8 = 136 workgroups: INSIDE one round; B 256 of the
    same networks and the two-critic shape at B 2048 are past it.)"""
    wg = {s: _workgroups(_Arena(True, True, OBS + s[1], s[2], 1, s[3]), s[0]) for s in SHAPES}
    assert wg[(128, 17, 256, 16)] == 136
    assert wg[(256, 17, 256, 16)] > 256 and wg[(2048, 6, 256, 2)] > 256
    assert wg[(128, 6, 64, 4)] <= 256 and wg[(512, 32, 256, 2)] <= 256 and wg[(512, 33, 256, 2)] <= 256


@pytest.mark.parametrize("switches", list(itertools.product((True, False), repeat=4)),
                         ids=lambda s: "".join("ft"[v] for v in s))
def test_the_plan_is_the_parents_predicates(switches, monkeypatch):
    import super_sac_amd as ssa
    L, lu = ssa.learning, ssa.learning_utils
    monkeypatch.setattr(L, "FUSED_ACTOR", switches[0])
    monkeypatch.setattr(L, "ACTOR_CHAIN", switches[1])
    monkeypatch.setattr(lu, "IN_KERNEL_NOISE", switches[2])
    if not switches[3]:
        monkeypatch.setattr(ssa.rng, "draw_normal", lambda shape, device: None)
    assert ssa.rng.normal_is_stock() == switches[3]
    process, rec_eps = object(), [object()]
    n = 0
    for B, A, H, N in SHAPES:
        for a_fused, c_dbuf, out_dim in itertools.product((True, False), (True, False), (1, 3)):
            a_arena = _Arena(a_fused, a_fused, OBS, H, 2 * A, 1)
            c_arena = _Arena(True, c_dbuf, OBS + A, H, out_dim, N)
            for kind, rp, ub, clip, sharded, eps in itertools.product(KINDS, (None, process), (False, True), (None, 1.0),
                                                                      (False, True), (None, rec_eps)):
                args = (kind, rp, ub, clip, a_arena, c_arena, A, B, sharded)
                plan = L._actor_member_plan(*args, eps is not None)
                what = (switches, args[:4], a_fused, c_dbuf, out_dim, (B, A, H, N), sharded, eps is not None)
                # the launch site: branch taken, chained or three launches, and the noise pointer
                assert plan == _p_launch_site(switches, *args, eps), what
                assert (plan[0] == "chain") == (_p_fused_member(switches, *args[:6]) and not sharded
                                                and L._actor_chain_form(a_arena, A, B, c_arena)), what
                # a member another rank owns: host draws are skipped exactly when its owner's noise is in-kernel
                assert (plan[1] == "kernel") == _p_owner_in_kernel(switches, *args, eps), what
                # `recordable`: every member on a fused form (asked without recording buffers, off a sharded rank)
                ask = L._actor_member_plan(*args[:8], False, False)
                rec_ok = _p_recordable_arenas(switches, kind, rp, ub, clip, a_arena, c_arena, sharded)
                if not sharded:
                    assert (ask[0] != "layers") == rec_ok, what
                # the recording's noise source (_actor_noise_in_kernel, one member): in-kernel iff chained + stock generator
                if rec_ok:
                    assert (ask[1] == "kernel") == bool(switches[2] and switches[3]
                                                        and _p_chain_form(switches, a_arena, A, B, c_arena)), what
                n += 1
    assert n == len(SHAPES) * 8 * 4 * 8 * 4
    assert L._actor_chain_form(_Arena(True, True, OBS, 64, 12, 1), 6, 128, _Arena(True, True, OBS + 6, 64, 1, 4)) == switches[1]
