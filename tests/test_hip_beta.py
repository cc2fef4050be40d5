"""GPU: the Beta policy head (Agent(beta_dist=True); csrc/ssac_beta.hip) per element against float64 torch, the sampler's
statistics, and a Beta agent through the update / acting entry points it supports and the ones it refuses."""
import copy
import ctypes as C
import math
import random
from itertools import chain

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import case_runner
import synth
from beta_cases import build_beta_agent

pytestmark = pytest.mark.gpu
DEV = "cuda"
SAMPLE, MEAN, GIVEN = 0, 1, 2


@pytest.fixture(scope="module")
def ssa():
    import super_sac_amd
    return super_sac_amd


def _grid():
    """(vec, x): every (v_alpha, v_beta) of a [-30, 30] grid at every x of a grid reaching 1e-6 from both ends; A = 3"""
    v = torch.linspace(-30.0, 30.0, 13)
    xs = torch.tensor([1e-6, 1e-4, 0.01, 0.3, 0.5, 0.7, 0.99, 1 - 1e-4, 1 - 1e-6], dtype=torch.float32)
    va, vb, xx = torch.meshgrid(v, v, xs, indexing="ij")
    A = 3
    n = va.numel() // A
    vec = torch.cat([va.reshape(n, A), vb.reshape(n, A)], 1).contiguous()
    return vec, xx.reshape(n, A).contiguous(), n, A


def _conc(vec, A):
    """alpha, beta exactly as the reference computes them (fp32, F.softplus threshold 20)"""
    c = 1.0 + F.softplus(vec)
    return c[:, :A], c[:, A:]


def _logp64(vec, x, A):
    """float64 restatement of BetaDist.log_prob(a).sum(-1) at the cached x; alpha - 1 and 1 - x in fp32 as torch has them"""
    al, be = _conc(vec, A)
    am1, bm1, omx = (al - 1.0).double(), (be - 1.0).double(), (1.0 - x).double()
    al, be, x = al.double(), be.double(), x.double()
    lp = (torch.xlogy(am1, x) + torch.xlogy(bm1, omx) + torch.lgamma(al + be) - torch.lgamma(al) - torch.lgamma(be)
          - math.log(2.0))
    return lp.sum(-1)


def _fwd(ssa, vec, n, A, mode, xin=None, ld_x=None, rng=None):
    act = torch.full((n, A), float("nan"), device=DEV)
    logp = torch.full((n,), float("nan"), device=DEV)
    xs = torch.full((n, A), float("nan"), device=DEV)
    v = vec.to(DEV)
    xi = (xin if xin.is_cuda else xin.to(DEV)) if xin is not None else None
    ssa._lib.check(ssa._lib.lib.ssac_beta_fwd(
        v.data_ptr(), 2 * A, n, A, mode, xi.data_ptr() if xi is not None else 0, ld_x or A,
        C.addressof(rng) if rng is not None else 0, act.data_ptr(), A, 0,
        0 if mode == MEAN else logp.data_ptr(), 0 if mode == MEAN else xs.data_ptr(), ssa.engine.stream()))
    torch.cuda.synchronize()
    return act.cpu(), logp.cpu(), xs.cpu()


def test_forward_injected_sample_mode(ssa):
    vec, x, n, A = _grid()
    act, logp, xs = _fwd(ssa, vec, n, A, SAMPLE, x)
    assert torch.equal(act, 2.0 * x - 1.0)   # the action is bit-equal to 2x - 1 in fp32
    assert torch.equal(xs, x)
    want = _logp64(vec, x, A)
    err = (logp.double() - want).abs()
    assert bool((err <= 1e-4 * want.abs().clamp(min=1.0)).all()), float((err / want.abs().clamp(min=1.0)).max())


def test_forward_mean_mode(ssa):
    vec, _, n, A = _grid()
    act, _, _ = _fwd(ssa, vec, n, A, MEAN)
    al, be = _conc(vec, A)
    want = 2.0 * (al / (al + be)) - 1.0
    assert torch.allclose(act, want, atol=1e-6, rtol=0)


def test_forward_given_action_mode(ssa):
    vec, x, n, A = _grid()
    a = (2.0 * x - 1.0) * 1.05          # some beyond the +-0.99 clamp
    wide = torch.zeros(n, A + 5, device=DEV)
    wide[:, 2:2 + A] = a.to(DEV)        # a strided action buffer
    _, logp, xs = _fwd(ssa, vec, n, A, GIVEN, wide[:, 2:], ld_x=A + 5)
    xg = (a.clamp(-0.99, 0.99) + 1.0) / 2.0
    assert torch.equal(xs, xg)
    want = _logp64(vec, xg, A)
    err = (logp.double() - want).abs()
    assert bool((err <= 1e-4 * want.abs().clamp(min=1.0)).all())


class _DirichletRsample(torch.autograd.Function):
    """the injected Dirichlet sample [x, 1 - x] with torch's _Dirichlet_backward (torch/distributions/dirichlet.py)"""

    @staticmethod
    def forward(ctx, conc, x2):
        ctx.save_for_backward(x2, conc)
        return x2.clone()

    @staticmethod
    def backward(ctx, g):
        x2, conc = ctx.saved_tensors
        total = conc.sum(-1, True).expand_as(conc)
        grad = torch._dirichlet_grad(x2, conc, total)
        return grad * (g - (x2 * g).sum(-1, True)), None


def _bwd_ref(vec, x, G, c, data_action):
    """float64 autograd of L = sum(G * a) + c * sum_b log pi_b  (data_action: x fixed, only the log-density term)"""
    A = x.shape[1]
    v = vec.double().requires_grad_(True)
    conc = 1.0 + F.softplus(v)
    al, be = conc[:, :A], conc[:, A:]
    x2 = torch.stack([x.double(), (1.0 - x).double()], -1)
    if data_action:
        x0, x1 = x2[..., 0], x2[..., 1]
    else:
        x0 = _DirichletRsample.apply(torch.stack([al, be], -1), x2)[..., 0]
        x1 = 1.0 - x0   # Beta.log_prob recomputes 1 - value from the cached x
    lp = (torch.xlogy(al - 1.0, x0) + torch.xlogy(be - 1.0, x1) + torch.lgamma(al + be) - torch.lgamma(al)
          - torch.lgamma(be) - math.log(2.0)).sum(-1)
    L = c * lp.sum()
    if not data_action:
        L = L + (G.double() * (2.0 * x0 - 1.0)).sum()
    L.backward()
    return v.grad


@pytest.mark.parametrize("data_action", [0, 1])
def test_backward_against_float64_autograd(ssa, data_action):
    vec, x, n, A = _grid()
    g = torch.Generator().manual_seed(5)
    G = torch.randn(n, A, generator=g) * 0.01
    la, inv_e = math.log(0.3), 0.5
    c = (math.exp(la) * inv_e / n) if not data_action else (-inv_e / n)
    dX = G.reshape(1, n, A).to(DEV)
    d_vec = torch.full((n, 2 * A), float("nan"), device=DEV)
    log_alpha = torch.tensor([la], device=DEV)
    v, xs = vec.to(DEV), x.to(DEV)
    ssa._lib.check(ssa._lib.lib.ssac_beta_bwd(
        dX.data_ptr(), 1, A, n * A, 0, v.data_ptr(), 2 * A, xs.data_ptr(), n, A, log_alpha.data_ptr(), 1,
        -inv_e if data_action else inv_e, data_action, d_vec.data_ptr(), 2 * A, ssa.engine.stream()))
    torch.cuda.synchronize()
    got = d_vec.cpu().double()
    want = _bwd_ref(vec, x, G, c, data_action)
    both_bad = ~torch.isfinite(want) & ~torch.isfinite(got)
    err = (got - want).abs()
    ok = (err <= 1e-4 * want.abs()) | (err <= 1e-6) | both_bad
    assert bool(ok.all()), f"{int((~ok).sum())} elements off; worst {float(err[~ok].max()) if (~ok).any() else 0:.3e}"


def _beta_cdf_grid(a, b):
    """numerically integrated Beta(a, b) CDF on a grid covering its mass (numpy only: scipy may be absent)"""
    m = a / (a + b)
    s = math.sqrt(a * b / ((a + b) ** 2 * (a + b + 1)))
    lo, hi = max(0.0, m - 14 * s), min(1.0, m + 14 * s)
    xg = np.linspace(lo, hi, 400001)
    with np.errstate(divide="ignore"):
        lpdf = ((a - 1) * np.log(xg) + (b - 1) * np.log1p(-xg) + math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b))
    pdf = np.exp(lpdf)
    pdf[~np.isfinite(pdf)] = 0.0
    cdf = np.concatenate([[0.0], np.cumsum(0.5 * (pdf[1:] + pdf[:-1]) * np.diff(xg))])
    return xg, cdf / cdf[-1], m, s


def _vec_for(alpha, beta, n, A):
    inv = lambda c: -200.0 if c == 1.0 else (c - 1.0 if c - 1.0 > 20 else math.log(math.expm1(c - 1.0)))
    vec = torch.empty(n, 2 * A)
    vec[:, :A], vec[:, A:] = inv(alpha), inv(beta)
    return vec


@pytest.mark.parametrize("alpha,beta", [(1.0, 1.0), (1.001, 5.0), (2.0, 2.0), (5.0, 1.5), (30.0, 30.0), (1000.0, 2.0)])
def test_sampler_statistics(ssa, alpha, beta):
    A, n = 4, 1 << 18                # 2^20 draws
    vec = _vec_for(alpha, beta, n, A)
    al, be = (float(t[0, 0]) for t in _conc(vec[:1], A))   # the concentrations the kernel sees (fp32)
    cnt = torch.tensor([7], dtype=torch.int64, device=DEV)
    rs = ssa._lib.Rng(0x1234ABCD5678, cnt.data_ptr(), 3)
    act, logp, x = _fwd(ssa, vec, n, A, SAMPLE, rng=rs)
    xf = x.double().numpy().reshape(-1)
    assert np.all(np.isfinite(xf)) and np.all(xf > 0.0) and np.all(xf < 1.0)
    assert torch.equal(act, 2.0 * x - 1.0) and bool(torch.isfinite(logp).all())
    N = xf.size
    xg, cdf, m, s = _beta_cdf_grid(al, be)
    assert abs(xf.mean() - m) <= 6 * s / math.sqrt(N)
    xs = np.sort(xf)
    F_ = np.interp(xs, xg, cdf)
    emp_hi = np.arange(1, N + 1) / N
    ks = max(np.max(emp_hi - F_), np.max(F_ - (emp_hi - 1.0 / N)))
    assert ks <= 2.5 / math.sqrt(N), ks
    xm = x.double().numpy()
    r = np.corrcoef(xm[:, 0], xm[:, 1])[0, 1]
    assert abs(r) < 5 / math.sqrt(n), r
    # counter-based: the same (seed, draw number) repeats, the next draw number differs
    _, _, x_again = _fwd(ssa, vec[:4096], 4096, A, SAMPLE, rng=rs)
    assert torch.equal(x_again, x[:4096])
    cnt.add_(1)
    _, _, x_next = _fwd(ssa, vec[:4096], 4096, A, SAMPLE, rng=rs)
    assert not torch.equal(x_next, x[:4096])


# ------------------------------------------------------------------------------------------ the agent
def _beta_case(ssa, name="redq_small"):
    cfg = synth.CASES[name]
    torch.manual_seed(cfg["seed"]); np.random.seed(cfg["seed"]); random.seed(cfg["seed"])
    dev = torch.device(DEV)
    buf = ssa.replay.ReplayBuffer(cfg["cap"], device=dev)
    buf.load_experience(*case_runner._buffers(cfg))
    agent = build_beta_agent(ssa, cfg, dev)   # Agent(beta_dist=True) holding the case's seeded weights
    target = copy.deepcopy(agent)
    copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=cfg["lr"])
    aopt = torch.optim.Adam(chain(*(a.parameters() for a in agent.actors)), lr=cfg["lr"])
    eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
    las, lopts = [], []
    for _ in range(agent.ensemble_size):
        la = torch.tensor([math.log(cfg["init_alpha"])], device=dev, requires_grad=True)
        las.append(la)
        lopts.append(torch.optim.Adam([la], lr=cfg["alpha_lr"], betas=(0.5, 0.999)))
    aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(cfg["B"])])
    return dict(cfg=cfg, buf=buf, agent=agent, target=target, copt=copt, aopt=aopt, eopt=eopt, las=las, lopts=lopts,
                aug=aug)


def _critic(ssa, k, random_process=None):
    cfg = k["cfg"]
    return ssa.learning.critic_update(
        buffer=k["buf"], agent=k["agent"], target_agent=k["target"], critic_optimizer=k["copt"],
        encoder_optimizer=k["eopt"], log_alphas=k["las"], batch_size=cfg["B"], gamma=cfg["gamma"],
        critic_clip=cfg["clip"], encoder_clip=cfg["clip"], target_critic_ensemble_n=cfg["n"],
        weighted_bellman_temp=cfg["temp"], weight_type=cfg["weight_type"], pop=cfg["pop"], augmenter=k["aug"],
        encoder_lambda=0, aug_mix=0.0, discrete=False, random_process=random_process, noise_clip=None, per=False,
        update_priorities=False, dr3_coeff=0.0)


def _actor(ssa, k, dicts, **kw):
    cfg = k["cfg"]
    args = dict(buffer=k["buf"], agent=k["agent"], pop=cfg["pop"], actor_optimizer=k["aopt"], log_alphas=k["las"],
                batch_size=cfg["B"], aug_mix=0.0, clip=cfg["clip"], augmenter=k["aug"], per=False, discrete=False,
                random_process=None, noise_clip=None, premade_replay_dicts=dicts)
    args.update(kw)
    return ssa.learning.online_actor_update(**args)


def _alpha(ssa, k, dicts):
    cfg = k["cfg"]
    return ssa.learning.alpha_update(buffer=k["buf"], agent=k["agent"], optimizers=k["lopts"], batch_size=cfg["B"],
                                     log_alphas=k["las"], augmenter=k["aug"], aug_mix=0.0, target_entropy=-cfg["act"],
                                     premade_replay_dicts=dicts, discrete=False)


def _params(k):
    ag = k["agent"]
    return torch.cat([p.detach().reshape(-1) for p in chain(*(a.parameters() for a in ag.actors),
                                                            *(c.parameters() for c in ag.critics))] +
                     [la.detach() for la in k["las"]]).cpu()


def _run(ssa, k, cycles):
    for _ in range(cycles):
        for _ in range(k["cfg"]["utd"]):
            _, dicts = _critic(ssa, k)
        _actor(ssa, k, dicts)
        _alpha(ssa, k, dicts)
    torch.cuda.synchronize()


def test_beta_sac_updates_run_on_the_per_layer_path_and_are_replayable(ssa):
    k = _beta_case(ssa)
    before = _params(k)
    _run(ssa, k, 3)       # past GRAPH_WARMUP critic updates
    after = _params(k)
    assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)
    ag = k["agent"]
    # the recorded critic update, the recorded actor update and the fused launches were declined
    assert not ag.__dict__.get("_ssac_graphs") and not ag.__dict__.get("_ssac_fast")
    assert not ag.__dict__.get("_ssac_actor_rec")
    ns = ag.__dict__["_ssac_noise"]
    i = {s: 3 + j for j, s in enumerate(ssa.beta.SITES)}
    E, utd = k["cfg"]["E"], k["cfg"]["utd"]
    assert ns[i["td"]] == 3 * utd * E and ns[i["actor"]] == 3 * E and ns[i["alpha"]] == 3 * E
    # stock-stream determinism: the same seeds give bit-identical parameters
    k2 = _beta_case(ssa)
    _run(ssa, k2, 3)
    assert torch.equal(_params(k2), after)


def test_beta_resume_continues_the_stream(ssa, tmp_path):
    """K updates, save_training_state, load into a fresh agent, K more == the same 2K updates uninterrupted (bit for bit,
    the agent's Beta draw counters included); the acting draws continue too"""
    def opts(k):
        return {"critic": k["copt"], "actor": k["aopt"], "alpha": k["lopts"]}
    kb = _beta_case(ssa)
    _run(ssa, kb, 2)
    ssa.checkpoint.save_training_state(str(tmp_path), kb["agent"], kb["target"], opts(kb), kb["las"], kb["buf"])
    noise = list(kb["agent"].__dict__["_ssac_noise"])
    kc = _beta_case(ssa)
    ssa.checkpoint.load_training_state(str(tmp_path), kc["agent"], kc["target"], opts(kc), kc["las"], kc["buf"])
    assert kc["agent"].__dict__["_ssac_noise"] == noise
    obs = _obs(kb["cfg"], 3, 4)
    torch.manual_seed(99); random.seed(99)
    _run(ssa, kb, 2)
    act_b = kb["agent"].sample_action(obs, num_envs=3)
    torch.manual_seed(99); random.seed(99)
    _run(ssa, kc, 2)
    act_c = kc["agent"].sample_action(obs, num_envs=3)
    assert kb["agent"].__dict__["_ssac_noise"] == kc["agent"].__dict__["_ssac_noise"]
    assert torch.equal(_params(kb), _params(kc))
    assert np.array_equal(act_b, act_c)
    # the continuation is not a replay of the first half
    assert kb["agent"].__dict__["_ssac_noise"][3] > noise[3]


def test_beta_exploration_noise_process_and_backup_weights(ssa):
    k = _beta_case(ssa, "sunrise")
    rp = ssa.learning_utils.GaussianExplorationNoise(k["cfg"]["act"])
    _, dicts = _critic(ssa, k, random_process=rp)
    _actor(ssa, k, dicts, random_process=rp, noise_clip=0.3)
    cfg = k["cfg"]
    for wt in ("sunrise", "softmax"):
        rd = ssa.learning_utils.sample_move_and_augment(buffer=k["buf"], batch_size=cfg["B"], augmenter=k["aug"],
                                                        aug_mix=0.0, per=False)
        w = ssa.learning_utils.compute_backup_weights({}, rd, k["agent"], k["target"], wt, 5.0, cfg["B"])
        torch.cuda.synchronize()
        assert bool(torch.isfinite(w).all())
    assert bool(torch.isfinite(_params(k)).all())


def _obs(cfg, n, seed):
    return {"obs": np.random.RandomState(seed).standard_normal((n, cfg["obs"])).astype(np.float32)}


def test_beta_forward_is_the_ensemble_mean_of_the_means(ssa):
    k = _beta_case(ssa, "sunrise")
    ag, cfg = k["agent"], k["cfg"]
    obs = _obs(cfg, 5, 0)
    act = ag.forward(obs, num_envs=5)
    s = torch.from_numpy(obs["obs"]).to(DEV)
    A = cfg["act"]
    means = []
    for a in ag.actors:
        al, be = _conc(a.raw_forward(s).cpu(), A)
        means.append(2.0 * (al / (al + be)) - 1.0)
    want = torch.stack(means, 0).mean(0).clamp(-1, 1)
    np.testing.assert_allclose(act, want.numpy(), atol=2e-6)


def test_beta_sample_action_with_injected_x(ssa):
    k = _beta_case(ssa, "sunrise")
    ag, cfg = k["agent"], k["cfg"]
    n, A = 4, cfg["act"]
    x = torch.rand(n, A, generator=torch.Generator().manual_seed(3)).clamp(1e-3, 1 - 1e-3)
    saved = ssa.rng.draw_beta_into
    ssa.rng.draw_beta_into = lambda dst: dst.copy_(x)
    try:
        act = ag.sample_action(_obs(cfg, n, 1), num_envs=n)
    finally:
        ssa.rng.draw_beta_into = saved
    assert np.array_equal(act, (2.0 * x - 1.0).numpy())


def test_beta_ucb_picks_the_argmax_candidate(ssa):
    k = _beta_case(ssa, "sunrise")
    ag, cfg = k["agent"], k["cfg"]
    ag.ucb_bonus = 0.7
    n, A, E = 6, cfg["act"], cfg["E"]
    xs = [torch.rand(n, A, generator=torch.Generator().manual_seed(10 + e)).clamp(1e-3, 1 - 1e-3) for e in range(E)]
    queue = list(xs)
    saved = ssa.rng.draw_beta_into
    ssa.rng.draw_beta_into = lambda dst: dst.copy_(queue.pop(0))
    try:
        obs = _obs(cfg, n, 2)
        act = ag.sample_action(obs, num_envs=n)
    finally:
        ssa.rng.draw_beta_into = saved
    s = torch.from_numpy(obs["obs"]).to(DEV)
    cands = torch.stack([2.0 * x - 1.0 for x in xs], 0).to(DEV)                # (E, n, A)
    q = torch.stack([torch.stack([c(s, cands[a]).view(n) for a in range(E)], 0) for c in ag.critics], 0)
    ucb = q.mean(0) + 0.7 * q.std(0)
    top2 = ucb.topk(2, dim=0).values
    clear = ((top2[0] - top2[1]) > 1e-4).cpu()
    assert clear.sum() >= n - 1
    want = cands[ucb.argmax(0), torch.arange(n, device=DEV)].cpu()
    np.testing.assert_array_equal(act[clear.numpy()], want.numpy()[clear.numpy()])


def test_beta_plain_behavioural_cloning(ssa):
    k = _beta_case(ssa)
    cfg = k["cfg"]
    before = _params(k)
    logs = ssa.learning.offline_actor_update(
        buffer=k["buf"], agent=k["agent"], actor_optimizer=k["aopt"], encoder_optimizer=k["eopt"],
        batch_size=cfg["B"], actor_clip=cfg["clip"], update_encoder=False, encoder_clip=None, augmenter=k["aug"],
        actor_lambda=0.0, aug_mix=0.0, per=False, discrete=False, filter_=False)
    torch.cuda.synchronize()
    assert math.isfinite(float(logs["losses/filtered_bc_overall_loss"]))
    assert not torch.equal(before, _params(k))


def test_beta_refusals(ssa):
    k = _beta_case(ssa)
    cfg = k["cfg"]
    _, dicts = _critic(ssa, k)
    with pytest.raises(NotImplementedError, match="Beta"):
        _actor(ssa, k, dicts, use_baseline=True)
    with pytest.raises(NotImplementedError, match="Beta"):
        ssa.learning.offline_actor_update(
            buffer=k["buf"], agent=k["agent"], actor_optimizer=k["aopt"], encoder_optimizer=k["eopt"],
            batch_size=cfg["B"], actor_clip=None, update_encoder=False, encoder_clip=None, augmenter=k["aug"],
            actor_lambda=0.0, aug_mix=0.0, per=False, discrete=False, filter_=True)
    with pytest.raises(NotImplementedError, match="Beta"):
        ssa.engine.set_precision(k["agent"], "bf16")
    # the acting fast path declines Beta actors
    assert not ssa.acting._eligible(k["agent"], _obs(cfg, 1, 0), 1, True, False)
    assert not ssa.acting._eligible(k["agent"], _obs(cfg, 1, 0), 1, False, False)


def test_beta_draw_sites_are_independent_streams(ssa):
    """draw k of one site and draw k of another (each site's counter starts at 0) use different Philox keys"""
    k = _beta_case(ssa)
    ag, cfg = k["agent"], k["cfg"]
    n, A = 256, cfg["act"]
    vec = torch.zeros(n, 2 * A, device=DEV)
    xs = {}
    for site in ssa.beta.SITES:
        ns, idx = ssa.beta.site_counter(ag, torch.device(DEV), site)
        assert ns[idx] == 0
        xs[site] = ssa.beta.sample(ag, vec, n, A, site, torch.empty(n, A, device=DEV)).cpu()
        assert ns[idx] == 1
    sites = list(xs)
    for a_ in range(len(sites)):
        for b_ in range(a_ + 1, len(sites)):
            assert not torch.equal(xs[sites[a_]], xs[sites[b_]]), (sites[a_], sites[b_])
            assert bool((xs[sites[a_]] != xs[sites[b_]]).float().mean() > 0.99)


def test_beta_refusals_of_the_other_entry_points(ssa, monkeypatch):
    k = _beta_case(ssa)
    cfg = k["cfg"]
    with pytest.raises(NotImplementedError, match="Beta"):   # action invariance
        ssa.learning.offline_actor_update(
            buffer=k["buf"], agent=k["agent"], actor_optimizer=k["aopt"], encoder_optimizer=k["eopt"],
            batch_size=cfg["B"], actor_clip=None, update_encoder=False, encoder_clip=None, augmenter=k["aug"],
            actor_lambda=0.5, aug_mix=0.0, per=False, discrete=False, filter_=False)
    with pytest.raises(NotImplementedError, match="Beta"):   # PER refresh through the advantage estimator
        ssa.learning.offline_actor_update(
            buffer=k["buf"], agent=k["agent"], actor_optimizer=k["aopt"], encoder_optimizer=k["eopt"],
            batch_size=cfg["B"], actor_clip=None, update_encoder=False, encoder_clip=None, augmenter=k["aug"],
            actor_lambda=0.0, aug_mix=0.0, per=True, discrete=False, filter_=False)
    mopt = torch.optim.Adam(chain(k["agent"].encoder.parameters(), k["agent"].inverse_model.parameters(),
                                  k["agent"].contrastive_model.parameters()), lr=1e-4)
    with pytest.raises(NotImplementedError, match="Beta"):   # Markov update with the Beta inverse model
        ssa.learning.markov_state_abstraction_update(
            buffer=k["buf"], agent=k["agent"], optimizer=mopt, batch_size=cfg["B"], augmenter=k["aug"], aug_mix=0.0,
            discrete=False, inverse_coeff=1.0, contrastive_coeff=1.0, smoothness_coeff=1.0, smoothness_max_dist=0.5,
            grad_clip=None)
    # critic- and member-sharded agents: every entry point refuses before touching a shard
    _, dicts = _critic(ssa, k)
    for attr in ("shard_of", "member_shard_of"):
        with monkeypatch.context() as mp:
            mp.setattr(ssa.parallel, attr, lambda agent: object())
            with pytest.raises(NotImplementedError, match="Beta"):
                _critic(ssa, k)
            with pytest.raises(NotImplementedError, match="Beta"):
                _actor(ssa, k, dicts)
            if attr == "member_shard_of":
                with pytest.raises(NotImplementedError, match="Beta"):
                    _alpha(ssa, k, dicts)
