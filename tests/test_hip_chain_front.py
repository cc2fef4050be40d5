"""GPU: the front of the chained update launch's lean critic tile, whose operands are read from a compact argument block
(CriticLeanArgs, the kernel's last parameter) instead of the critic role's FusedArgs.

That touches no floating-point operation or its order, so every comparison is between the lean and the general tile
(ssac_chain_lean(1 / 0)) as bytes: the general tile keeps the full argument struct.  One test pins h1 of the lean launch
to a float64 reference as well -- a weight chunk that landed in the staging buffer while fc1 still read W1's image there
(W2's first chunk is requested while fc1 runs) would be a wrong fc1, which a comparison of two forms could only see if
one of them were right.

The automatic tile choice gives 16-row tiles at every shape small enough for a test, so the 32-row tiles -- the only
ones with a lean form -- are forced (ssac_fused_tile_rows(32)), as tests/test_hip_chain_lean.py does.
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
    """the switches this file turns, restored whatever a test does"""
    lib = ssa._lib.lib
    yield lib
    lib.ssac_chain_lean(1)
    lib.ssac_fused_tile_rows(0)
    lib.ssac_slot_by_value(1)


def _arena_from(ssa, mlps):
    in_dim, hidden, out = mlps[0]["w1"].shape[1], mlps[0]["w1"].shape[0], mlps[0]["w3"].shape[0]
    ar = ssa.engine.MlpArena(len(mlps), in_dim, hidden, out, torch.device(DEV))
    for j, p in enumerate(mlps):
        for seg in ssa.engine.SEGS:
            ar.view(j, seg).copy_(p[seg])
    return ar


class _Problem:
    """one actor, N critics, N target critics, a batch and a 256-row replay: the operands of ssac_chain_update"""
    R = 256

    def __init__(self, ssa, B, N, S, A, H=256):
        rng = np.random.RandomState(1000 * B + 10 * N + S)
        self.ssa, self.B, self.N, self.S, self.A, self.H = ssa, B, N, S, A, H
        self.critics = [orc.make_mlp(rng, S + A, H, 1) for _ in range(N)]
        self.aa = _arena_from(ssa, [orc.make_mlp(rng, S, H, 2 * A)])
        self.ca = _arena_from(ssa, self.critics)
        self.ta = _arena_from(ssa, [orc.make_mlp(rng, S + A, H, 1) for _ in range(N)])
        t = lambda a: torch.from_numpy(a.astype(np.float32)).to(DEV)
        self.x1, self.xc = t(rng.standard_normal((B, S + A))), t(rng.standard_normal((B, S + A)))
        self.eps = t(rng.standard_normal((B, A)))
        self.n_sel = 2 if N > 1 else 1
        self.ids = torch.tensor([N - 1, 0][:self.n_sel], dtype=torch.int32, device=DEV)
        R = self.R
        self.rs, self.rs1 = t(rng.standard_normal((R, S))), t(rng.standard_normal((R, S)))
        self.ra, self.rr = t(rng.uniform(-1, 1, (R, A))), t(rng.standard_normal(R))
        self.rdn = torch.from_numpy((rng.uniform(size=R) < 0.3).astype(np.uint8)).to(DEV)
        self.idx = torch.from_numpy(rng.permutation(R)[:B].astype(np.int64)).to(DEV)   # distinct rows

    def chained(self, dz2_out=True, gather=False):
        """ssac_chain_update, producer / consumer form; dz2_out False: the W3 snapshot instead of dz2u; gather: the rows
        come from the replay arrays through the index vector (and [s|a], r, d are written out)"""
        ssa, lib, st = self.ssa, self.ssa._lib.lib, self.ssa.engine.stream()
        B, S, A, N, H = self.B, self.S, self.A, self.N, self.H
        xa = torch.zeros(B, S + A, device=DEV) if gather else self.x1.clone()
        lp = torch.zeros(B, device=DEV)
        h1, h2, q = torch.zeros(N, B, H, device=DEV), torch.zeros(N, B, H, device=DEV), torch.zeros(N, B, 1, device=DEV)
        qt = torch.full((self.n_sel, B, 1), float("nan"), device=DEV)
        dz2, dz1, w3s = torch.zeros_like(h1), torch.zeros_like(h1), torch.zeros(N, H, device=DEV)
        ho = torch.zeros(B * A, dtype=torch.int64, device=DEV)
        xsa = torch.full((B, S + A), 7.0, device=DEV)
        rew, done = torch.zeros(B, device=DEV), torch.zeros(B, device=DEV)
        gt = ssa._lib.Gather(self.rs.data_ptr(), self.rs1.data_ptr(), self.ra.data_ptr(), self.rr.data_ptr(),
                             self.rdn.data_ptr(), S, A, self.idx.data_ptr(), 0, xsa.data_ptr(), S + A, xa.data_ptr(), S + A,
                             rew.data_ptr(), done.data_ptr(), 0, 0, -1, 0)
        ssa._lib.check(lib.ssac_chain_update(
            C.byref(self.aa.desc()), 0 if gather else xa.data_ptr(), 0 if gather else S + A, B, self.eps.data_ptr(), -5.0,
            2.0, xa.data_ptr(), S + A, S, lp.data_ptr(), 0, C.byref(self.ta.desc()), self.ids.data_ptr(), self.n_sel,
            qt.data_ptr(), C.byref(self.ca.desc()), 0 if gather else self.xc.data_ptr(), 0 if gather else S + A,
            h1.data_ptr(), h2.data_ptr(), q.data_ptr(), dz2.data_ptr() if dz2_out else 0, dz1.data_ptr(),
            0 if dz2_out else w3s.data_ptr(), C.byref(gt) if gather else 0, 0, ho.data_ptr(), 1, 0, st))
        torch.cuda.synchronize()
        out = dict(a=xa, logp=lp, h1=h1, h2=h2, q=q, qt=qt, dz2u=dz2, dz1u=dz1, w3s=w3s)
        if gather:
            out.update(xsa=xsa, rew=rew, done=done)
        return out


def _lean_and_general(p, forms, **kw):
    ssa = p.ssa
    ssa._lib.check(forms.ssac_fused_tile_rows(32))
    ssa._lib.check(forms.ssac_chain_lean(1))
    lean = p.chained(**kw)
    assert forms.ssac_chain_lean_taken() == 1
    ssa._lib.check(forms.ssac_chain_lean(0))
    gen = p.chained(**kw)
    assert forms.ssac_chain_lean_taken() == 0
    return lean, gen


def _same_bytes(lean, gen, who):
    for k in gen:
        assert torch.equal(lean[k], gen[k]), f"{who}: {k} differs between the lean and the general critic tile"
    assert bool(torch.isfinite(lean["qt"]).all()) and float(lean["h2"].abs().max()) > 0 and float(lean["dz1u"].abs().max()) > 0


CASES = [
    ("one full tile", 32, 1, 17, 6),
    ("a ragged second tile of 8 rows", 40, 1, 17, 6),
    ("two full tiles", 64, 1, 17, 6),
    ("subset ids [N-1, 0]", 40, 3, 17, 6),
    ("in = 32: a full chunk, no zero padding", 40, 3, 26, 6),
    ("in = 4", 40, 3, 3, 1),
]


@pytest.mark.parametrize("what,B,N,S,A", CASES, ids=[c[0] for c in CASES])
def test_launch_outputs_are_the_general_tiles_bytes(ssa, forms, what, B, N, S, A):
    """Everything ssac_chain_update writes in its producer / consumer form -- a', log pi, h1, h2, q, q_t, dz1u, and dz2u or
    the W3 snapshot in its place -- lean against general, as bytes."""
    p = _Problem(ssa, B, N, S, A)
    for dz2_out in (True, False):
        lean, gen = _lean_and_general(p, forms, dz2_out=dz2_out)
        _same_bytes(lean, gen, f"{what} (dz2u written: {dz2_out})")


@pytest.mark.parametrize("what,B,N,S,A", CASES, ids=[c[0] for c in CASES])
def test_launch_outputs_with_the_replay_gather_folded_in(ssa, forms, what, B, N, S, A):
    """The same with the rows fetched from a 256-row replay through distinct random indices: the lean tile takes the
    gather's operands (s, act, their widths, the [s|a] rows it writes out) from its compact block.  The [s|a] rows are
    compared with the gather done by hand as well."""
    p = _Problem(ssa, B, N, S, A)
    for dz2_out in (True, False):
        lean, gen = _lean_and_general(p, forms, dz2_out=dz2_out, gather=True)
        _same_bytes(lean, gen, f"{what}, gathered (dz2u written: {dz2_out})")
        assert torch.equal(lean["xsa"], torch.cat([p.rs[p.idx], p.ra[p.idx]], 1)), "[s|a] rows"
        assert torch.equal(lean["rew"], p.rr[p.idx]) and torch.equal(lean["done"], p.rdn[p.idx].float())


@pytest.mark.parametrize("gather", [False, True], ids=["rows from X", "gathered rows"])
def test_lean_fc1_against_float64(ssa, forms, gather):
    """h1 of the lean launch per element against relu(x W1^T + b1) in float64 from the arena's weights, B 40 / N 3 / 17 + 6
    columns.  The bound is the fp32 forward's for h1 in tests/test_hip_kernels.py (1e-5 + 1e-5 |ref|): 23 products of O(1)
    inputs with weights of O(1 / sqrt(23)), fp32 rounding of each at 6e-8 relative -- two orders of magnitude inside it,
    while a weight image overwritten by another layer's chunk is wrong by O(1)."""
    p = _Problem(ssa, 40, 3, 17, 6)
    ssa._lib.check(forms.ssac_fused_tile_rows(32))
    ssa._lib.check(forms.ssac_chain_lean(1))
    got = p.chained(gather=gather)
    assert forms.ssac_chain_lean_taken() == 1
    x = (torch.cat([p.rs[p.idx], p.ra[p.idx]], 1) if gather else p.xc).cpu().double()
    worst = 0.0
    for j, m in enumerate(p.critics):
        ref = torch.relu(x @ m["w1"].double().T + m["b1"].double())
        err = (got["h1"][j].cpu().double() - ref).abs()
        worst = max(worst, float(err.max()))
        assert bool((err <= 1e-5 + 1e-5 * ref.abs()).all()), f"h1[{j}]: max err {float(err.max()):.3e}"
        assert float(ref.abs().max()) > 0.5
    print("lean h1 vs float64: max abs err", worst)


def _recorded_updates(ssa, lean, by_value=True, B=64, N=3):
    """critic updates at hidden 256 with 32-row tiles forced, recorded and replayed through the input ring for
    FEED_SLOTS + 3 updates (the ring wraps), a fresh index draw each: every update's TD targets, and the parameters, the
    targets and Adam's moments at the end"""
    L, lib = ssa.learning, ssa._lib.lib
    dev = torch.device("cuda")
    S, A, H = 17, 6, 256
    ssa._lib.check(lib.ssac_chain_lean(1 if lean else 0))
    ssa._lib.check(lib.ssac_fused_tile_rows(32))
    ssa._lib.check(lib.ssac_slot_by_value(1 if by_value else 0))
    assert L.USE_GRAPHS and L.LAUNCH_MODE == "list"
    torch.manual_seed(3); np.random.seed(3); random.seed(3)
    agent = ssa.Agent(act_space_size=A, encoder=ssa.nets.IdentityEncoder(S),
                      actor_network_cls=ssa.nets.ContinuousStochasticActor,
                      critic_network_cls=ssa.nets.ContinuousCritic, ensemble_size=1, num_critics=N,
                      hidden_size=H, auto_rescale_targets=False, log_std_low=-5.0, log_std_high=2.0)
    agent.to(dev)
    target = copy.deepcopy(agent)
    buf = ssa.replay.ReplayBuffer(4096, device=dev)
    buf.load_experience(*synth.synth_transitions(2000, S, A, seed=5))
    copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=3e-4)
    eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
    la = torch.Tensor([math.log(0.1)]).to(dev); la.requires_grad = True
    aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(B)])
    tds, idxs, taken = [], [], []
    for k in range(L.FEED_SLOTS + 3):
        _, dicts = L.critic_update(
            buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt,
            log_alphas=[la], batch_size=B, gamma=0.99, critic_clip=None, encoder_clip=None,
            target_critic_ensemble_n=2, weighted_bellman_temp=None, weight_type=None, pop=False, augmenter=aug,
            encoder_lambda=0, aug_mix=0.0, discrete=False, random_process=None, noise_clip=None, per=False,
            update_priorities=False, dr3_coeff=0.0)
        taken.append(lib.ssac_chain_lean_taken())
        tds.append(dicts[0]["td_target"].detach().cpu().numpy().copy())
        idxs.append(np.array(dicts[0]["priority_idxs"]).copy())
        if k % 2 == 0:
            ssa.learning_utils.soft_update(target.critics[0], agent.critics[0], 0.005)
    torch.cuda.synchronize()
    flat = lambda mods: torch.cat([p.detach().flatten() for m in mods for p in m.parameters()]).cpu().numpy()
    ar = agent.critics[0].arena(dev)
    m, v = copt._ssac_adam.moments_for(("critic", 0), ar.params)
    return dict(params=flat(agent.critics), target=flat(target.critics), m=m.detach().cpu().numpy().copy(),
                v=v.detach().cpu().numpy().copy()), tds, idxs, taken


def test_recorded_updates_follow_the_input_ring(ssa, forms):
    """A critic update at B 64 / N 3 / hidden 256, recorded, then replayed until the input ring has wrapped, each update
    with its own index draw: lean, general, and lean with the slot found through the feed block instead of handed over by
    value.  Every update's TD targets and the final critic, target and Adam-moment arrays, as bytes.  (The compact block
    carries its own copy of the slot pointer, which the replay must fill in like the three FusedArgs'.)"""
    a, td_a, idx_a, taken_a = _recorded_updates(ssa, True)
    b, td_b, idx_b, taken_b = _recorded_updates(ssa, False)
    c, td_c, idx_c, taken_c = _recorded_updates(ssa, True, by_value=False)
    assert all(t == 1 for t in taken_a) and all(t == 0 for t in taken_b) and all(t == 1 for t in taken_c)
    n = len(td_a)
    assert n == ssa.learning.FEED_SLOTS + 3
    assert any(not np.array_equal(idx_a[0], idx_a[k]) for k in range(1, n)), "every update draws its own rows"
    for k in range(n):
        assert np.array_equal(idx_a[k], idx_b[k]) and np.array_equal(idx_a[k], idx_c[k]), f"update {k}: the draws differ"
        assert np.array_equal(td_a[k], td_b[k]), f"update {k}: TD targets differ between the lean and the general tile"
        assert np.array_equal(td_a[k], td_c[k]), f"update {k}: TD targets differ with the slot by value and through the feed"
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{k} differs between the lean and the general critic tile"
        assert np.array_equal(a[k], c[k]), f"{k} differs with the slot by value and through the feed block"
    assert np.isfinite(a["params"]).all() and float(np.abs(a["m"]).max()) > 0
