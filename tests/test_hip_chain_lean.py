"""GPU: the chained update launch's critic tile -- its lean instantiation against the general one, and the general one
(whose template gained the flag) against the launches the chained one replaces.

The lean tile leaves every floating-point operation and its order alone, so every comparison of the chained launch with
itself (lean against general) is bit for bit.  Against the separate launches the existing rules hold
(test_hip_kernels.py::test_chain_launch_equals_the_separate_launches): everything bit for bit, but the target Q of the
producer / consumer form, whose fc1 adds the action columns after the state columns' sum (2e-5).

The automatic tile choice gives 16-row tiles at every shape small enough for a test, so the 32-row tiles -- the only
ones with a lean form -- are forced (ssac_fused_tile_rows(32)), as the existing tests of the tile sizes do.
"""
import copy
import ctypes as C
import math
import random
from itertools import chain

import numpy as np
import pytest
import torch

import ssac_oracle as orc
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ssa():
    import super_sac_amd
    return super_sac_amd


@pytest.fixture
def forms(ssa):
    """the two switches this file turns, restored whatever a test does"""
    lib = ssa._lib.lib
    yield lib
    lib.ssac_chain_lean(1)
    lib.ssac_fused_tile_rows(0)


def _arena_from(ssa, mlps):
    in_dim, hidden, out = mlps[0]["w1"].shape[1], mlps[0]["w1"].shape[0], mlps[0]["w3"].shape[0]
    ar = ssa.engine.MlpArena(len(mlps), in_dim, hidden, out, torch.device(DEV))
    for j, p in enumerate(mlps):
        for seg in ssa.engine.SEGS:
            ar.view(j, seg).copy_(p[seg])
    return ar


class _Problem:
    """one actor, N critics, N target critics and a batch: the operands of ssac_chain_update"""

    def __init__(self, ssa, B, N, S, A, H):
        rng = np.random.RandomState(1000 * B + 10 * N + S)
        self.ssa, self.B, self.N, self.S, self.A, self.H = ssa, B, N, S, A, H
        self.aa = _arena_from(ssa, [orc.make_mlp(rng, S, H, 2 * A)])
        self.ca = _arena_from(ssa, [orc.make_mlp(rng, S + A, H, 1) for _ in range(N)])
        self.ta = _arena_from(ssa, [orc.make_mlp(rng, S + A, H, 1) for _ in range(N)])
        t = lambda a: torch.from_numpy(a.astype(np.float32)).to(DEV)
        self.x1, self.xc = t(rng.standard_normal((B, S + A))), t(rng.standard_normal((B, S + A)))
        self.eps = t(rng.standard_normal((B, A)))
        self.n_sel = 2 if N > 1 else 1
        self.ids = torch.tensor([N - 1, 0][:self.n_sel], dtype=torch.int32, device=DEV)

    def separate(self, rows=0):
        """actor sample, critic forward, target forward + unscaled backward as three launches; rows: the tile size forced
        for the critics' two (the actor's tiles are 16 rows in every chained launch, so its stand-alone launch gets 16)"""
        ssa, lib, st = self.ssa, self.ssa._lib.lib, self.ssa.engine.stream()
        B, S, A = self.B, self.S, self.A
        ws = ssa.engine.Workspace(torch.device(DEV))
        xa, lp = self.x1.clone(), torch.zeros(B, device=DEV)
        ssa._lib.check(lib.ssac_fused_tile_rows(16))
        ssa._lib.check(lib.ssac_actor_sample_fused(C.byref(self.aa.desc()), xa.data_ptr(), S + A, B, self.eps.data_ptr(),
                                                   -5.0, 2.0, xa.data_ptr(), S + A, S, lp.data_ptr(), 0, 0, 0, 0, st))
        ssa._lib.check(lib.ssac_fused_tile_rows(rows))
        h1, h2, q = (t.clone() for t in ssa.engine.mlp_forward(self.ca, self.xc, S + A, 0, B, ws, "sep"))
        qt, dz2, dz1 = torch.zeros(self.n_sel, B, 1, device=DEV), torch.zeros_like(h1), torch.zeros_like(h1)
        ssa._lib.check(lib.ssac_target_fwd_critic_bwdu(
            C.byref(self.ta.desc()), self.ids.data_ptr(), self.n_sel, xa.data_ptr(), S + A, B, qt.data_ptr(),
            C.byref(self.ca.desc()), h1.data_ptr(), h2.data_ptr(), 0, 0, dz2.data_ptr(), dz1.data_ptr(), st))
        torch.cuda.synchronize()
        return dict(a=xa, logp=lp, h1=h1, h2=h2, q=q, qt=qt, dz2u=dz2, dz1u=dz1)

    def chained(self, handoff=True, dz2_out=True):
        """ssac_chain_update; handoff: the producer / consumer form; dz2_out False: the W3 snapshot instead of dz2u"""
        ssa, lib, st = self.ssa, self.ssa._lib.lib, self.ssa.engine.stream()
        B, S, A, N, H = self.B, self.S, self.A, self.N, self.H
        xa, lp = self.x1.clone(), torch.zeros(B, device=DEV)
        h1, h2, q = torch.zeros(N, B, H, device=DEV), torch.zeros(N, B, H, device=DEV), torch.zeros(N, B, 1, device=DEV)
        qt = torch.full((self.n_sel, B, 1), float("nan"), device=DEV)
        dz2, dz1, w3s = torch.zeros_like(h1), torch.zeros_like(h1), torch.zeros(N, H, device=DEV)
        ho = torch.zeros(B * A, dtype=torch.int64, device=DEV)
        ssa._lib.check(lib.ssac_chain_update(
            C.byref(self.aa.desc()), xa.data_ptr(), S + A, B, self.eps.data_ptr(), -5.0, 2.0, xa.data_ptr(), S + A, S,
            lp.data_ptr(), 0, C.byref(self.ta.desc()), self.ids.data_ptr(), self.n_sel, qt.data_ptr(),
            C.byref(self.ca.desc()), self.xc.data_ptr(), S + A, h1.data_ptr(), h2.data_ptr(), q.data_ptr(),
            dz2.data_ptr() if dz2_out else 0, dz1.data_ptr(), 0 if dz2_out else w3s.data_ptr(), 0, 0,
            ho.data_ptr() if handoff else 0, 1, 0, st))
        torch.cuda.synchronize()
        return dict(a=xa, logp=lp, h1=h1, h2=h2, q=q, qt=qt, dz2u=dz2, dz1u=dz1, w3s=w3s)


def _same(got, want, who, keys=None, qt_atol=None):
    for k in keys or want:
        if k == "qt" and qt_atol is not None:
            d = float((got[k] - want[k]).abs().max())
            assert torch.isfinite(got[k]).all() and d <= qt_atol, f"{who}: target q off by {d}"
        else:
            assert torch.equal(got[k], want[k]), f"{who}: {k} differs"


@pytest.mark.parametrize("S,A", [(3, 1), (17, 6), (26, 6)])   # IN = 4, 23 (padded chunk), 32 (exactly full)
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("B", [32, 33, 96])                     # a full tile, a ragged last tile, three tiles
def test_lean_critic_tile_gives_the_general_tiles_bits(ssa, forms, B, N, S, A):
    """The same chained launch with ssac_chain_lean(1) and (0): h1, h2, q, dz1u and the target Q (and everything else the
    launch writes) bit for bit, with dz2u written out and with the W3 snapshot in its place."""
    p = _Problem(ssa, B, N, S, A, 256)
    ssa._lib.check(forms.ssac_fused_tile_rows(32))
    for dz2_out in (True, False):
        ssa._lib.check(forms.ssac_chain_lean(1))
        lean = p.chained(dz2_out=dz2_out)
        assert forms.ssac_chain_lean_taken() == 1
        ssa._lib.check(forms.ssac_chain_lean(0))
        gen = p.chained(dz2_out=dz2_out)
        assert forms.ssac_chain_lean_taken() == 0
        _same(lean, gen, f"lean vs general (dz2u written: {dz2_out})")
        assert bool(torch.isfinite(lean["qt"]).all()) and float(lean["h2"].abs().max()) > 0


@pytest.mark.parametrize("what,B,N,S,A,H,rows", [
    ("hidden 128", 96, 3, 17, 6, 128, 32),
    ("input of 33 columns", 96, 3, 27, 6, 256, 32),
    ("16-row tiles", 96, 3, 17, 6, 256, 16),
    ("qualifies", 96, 3, 17, 6, 256, 32),        # (the control: this one IS lean)
])
def test_launcher_takes_the_lean_tile_only_where_it_applies(ssa, forms, what, B, N, S, A, H, rows):
    """Shapes outside the lean instantiation's constants take the general one (ssac_chain_lean_taken) and match the
    separate launches as before; so does the one-workgroup form (no hand-off buffer), which has no lean kernel."""
    p = _Problem(ssa, B, N, S, A, H)
    want = p.separate(rows)     # (leaves the tile size forced)
    got = p.chained()
    assert forms.ssac_chain_lean_taken() == (1 if what == "qualifies" else 0), what
    _same(got, want, what, keys=want.keys(), qt_atol=2e-5)
    got = p.chained(handoff=False)
    assert forms.ssac_chain_lean_taken() == 0
    # (the stand-alone target forward follows the forced tile size, the chained launch's target chains are always 16 rows:
    #  with 32 rows forced the K sums of the target Q associate differently)
    _same(got, want, what + ", one-workgroup target chains", keys=want.keys(), qt_atol=2e-5 if rows == 32 else None)


def test_discrete_critics_never_reach_the_chained_launch(ssa, forms):
    """A critic with more than one head output is refused by ssac_chain_update (its update takes the per-role launches with
    the matrix-core head and the action selector, covered by the existing suite), so it cannot take the lean tile."""
    p = _Problem(ssa, 32, 2, 17, 6, 256)
    rng = np.random.RandomState(2)
    p.ca = _arena_from(ssa, [orc.make_mlp(rng, 23, 256, 4) for _ in range(2)])
    before = forms.ssac_chain_lean_taken()
    with pytest.raises(RuntimeError, match="single-output critics only"):
        p.chained()
    assert forms.ssac_chain_lean_taken() == before


@pytest.mark.parametrize("handoff", [False, True])
def test_general_16_row_tiles_of_a_wide_input_match_the_separate_launches(ssa, forms, handoff):
    """The general instantiation where the lean one never applies: 16-row critic tiles -- the direct backward-data loop --
    of a critic whose input is wider than one K chunk (IN = 46), B 32 / N 2, against the separate launches, bit for bit."""
    p = _Problem(ssa, 32, 2, 40, 6, 256)
    want = p.separate()      # (automatic tile choice: 16 rows at this size, for both)
    got = p.chained(handoff=handoff)
    assert forms.ssac_chain_lean_taken() == 0
    _same(got, want, "16-row tiles", keys=want.keys(), qt_atol=2e-5 if handoff else None)


def test_chained_actor_update_at_one_tile_matches_the_three_launches():
    """The actor update's chained launch at B 32 / N 2: its critic tiles (the general instantiation as a hand-off consumer)
    publish Q and dQ/da as granules from the head sum and the dQ/da tail, and the actor's workgroups poll for them --
    against the three launches, with the existing comparison's bounds (the critics' fc1 sums state and action columns
    separately: fp32 association, 3e-5 of the largest value)."""
    from test_hip_cases import _actor_update_run
    shape = (32, 17, 6, 2, 64)
    f3, l3, _, _, _ = _actor_update_run(False, n_upd=2, shape=shape)
    fc, lc, _, _, _ = _actor_update_run(True, n_upd=2, shape=shape)
    for n_ in f3:
        scale = max(1.0, float(np.abs(f3[n_]).max()))
        np.testing.assert_allclose(fc[n_], f3[n_], rtol=0, atol=3e-5 * scale, err_msg=n_)
    np.testing.assert_allclose(np.array(lc), np.array(l3), rtol=2e-4, atol=1e-6)


def _recorded_updates(ssa, lean, B=64, N=2, pop=False, weights=False, n_upd=6):
    """critic updates at hidden 256 with 32-row tiles forced -- eager, then recorded and replayed (the library's launch
    list): chained launch, weight-gradient launch with Adam, Polyak.  Returns the parameters, the targets, Adam's moments
    and the form every chained launch took."""
    L, lib = ssa.learning, ssa._lib.lib
    dev = torch.device("cuda")
    S, A, H = 17, 6, 256
    ssa._lib.check(lib.ssac_chain_lean(1 if lean else 0))
    ssa._lib.check(lib.ssac_fused_tile_rows(32))
    assert L.USE_GRAPHS and L.LAUNCH_MODE == "list"
    torch.manual_seed(3); np.random.seed(3); random.seed(3)
    agent = ssa.Agent(act_space_size=A, encoder=ssa.nets.IdentityEncoder(S),
                      actor_network_cls=ssa.nets.ContinuousStochasticActor,
                      critic_network_cls=ssa.nets.ContinuousCritic, ensemble_size=1, num_critics=N,
                      hidden_size=H, auto_rescale_targets=pop, log_std_low=-5.0, log_std_high=2.0)
    agent.to(dev)
    target = copy.deepcopy(agent)
    buf = ssa.replay.ReplayBuffer(4096, device=dev)
    buf.load_experience(*synth.synth_transitions(2000, S, A, seed=5))
    copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=3e-4)
    eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
    la = torch.Tensor([math.log(0.1)]).to(dev); la.requires_grad = True
    aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(B)])
    taken = []
    for k in range(n_upd):
        L.critic_update(
            buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt,
            log_alphas=[la], batch_size=B, gamma=0.99, critic_clip=None, encoder_clip=None,
            target_critic_ensemble_n=2, weighted_bellman_temp=10.0 if weights else None,
            weight_type="sunrise" if weights else None, pop=pop, augmenter=aug, encoder_lambda=0, aug_mix=0.0,
            discrete=False, random_process=None, noise_clip=None, per=False, update_priorities=False, dr3_coeff=0.0)
        taken.append(lib.ssac_chain_lean_taken())
        if k % 2 == 0:
            ssa.learning_utils.soft_update(target.critics[0], agent.critics[0], 0.005)
    torch.cuda.synchronize()
    flat = lambda mods: torch.cat([p.detach().flatten() for m in mods for p in m.parameters()]).cpu().numpy()
    ar = agent.critics[0].arena(dev)
    m, v = copt._ssac_adam.moments_for(("critic", 0), ar.params)
    return dict(params=flat(agent.critics), target=flat(target.critics), m=m.detach().cpu().numpy().copy(),
                v=v.detach().cpu().numpy().copy()), taken


@pytest.mark.parametrize("setting", ["plain", "popart", "per-row weights"])
def test_recorded_update_ends_on_the_same_bits_with_either_tile(ssa, forms, setting):
    """Whole updates -- chained launch, weight-gradient launch, Adam, Polyak; eager, recorded and replayed -- with the
    switch on and off, at B 64 / N 2: parameters, moments and targets bit for bit.

    PopArt and per-row weights: the chained launch carries neither (ssac_chain_update has no such operand -- its backward
    half is the UNSCALED one, and both terms enter the weight-gradient launch as row scales), so such an update has nothing
    the lean tile lacks and takes it like the plain one; what is pinned here is that its results do not depend on it."""
    kw = dict(pop=setting == "popart", weights=setting == "per-row weights")
    if setting == "popart":   # (with PopArt the engine wants the target Q in one part: a launch too large for column-split
        kw.update(B=512, N=10)   #  target critics -- the benchmark's shape)
    a, taken_a = _recorded_updates(ssa, True, **kw)
    b, taken_b = _recorded_updates(ssa, False, **kw)
    print(setting, "chained launches took (lean on):", taken_a, "(lean off):", taken_b)
    # (a replayed update issues no ssac_chain_update: its entry repeats the form of the launch that was recorded)
    assert all(t == 1 for t in taken_a) and all(t == 0 for t in taken_b)
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{setting}: {k} differs between the lean and the general critic tile"
    assert np.isfinite(a["params"]).all() and float(np.abs(a["m"]).max()) > 0
