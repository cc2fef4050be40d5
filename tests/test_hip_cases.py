"""GPU: multi-step update sequences (critic updates + Polyak + actor + temperature) through the
reference-shaped API of super_sac_amd, against the outputs the REFERENCE produced for the same
replay batches, subsets and noise (tests/golden/<case>.npz), and against the CPU oracle.

Stated tolerances (fp32): TD targets 2e-4 relative-to-max(1,|x|); scalar logs 5e-4; parameters,
Polyak targets and Adam first moments 3e-5 absolute after the whole sequence; replay indices
bit-exact.
"""
import numpy as np
import pytest

import case_runner
import synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("wgrad", [1, 2], ids=["wgrad-64x64", "wgrad-32x32"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per-layer"])
@pytest.mark.parametrize("name", [n_ for n_ in synth.CASES if n_ not in synth.FULL_SIZE])
def test_engine_matches_reference(name, fused, wgrad):
    """both kernel families: the one-launch fused MLP kernels and the per-layer GEMM path -- and both forms of the merged
    weight-gradient launch under each: 64 x 64 tiles with an LDS-staged K loop, and the latency form (32 x 32 tiles, K
    split over the waves, operands straight from memory) that launches take automatically while all of their
    workgroups are resident at once."""
    import super_sac_amd as ssa
    old = ssa.engine.USE_FUSED
    ssa.engine.USE_FUSED = fused
    ssa.engine.set_wgrad_variant(wgrad)
    try:
        rec = case_runner.run_engine(name)
    finally:
        ssa.engine.USE_FUSED = old
        ssa.engine.set_wgrad_variant(0)
    fx = case_runner.load_fixture(name)
    worst = case_runner.compare(rec, fx, who=f"hip[{name},{'fused' if fused else 'per-layer'},wgrad {wgrad}]")
    print(f"{name}: worst deviations vs reference {worst}")


@pytest.mark.parametrize("name", synth.FULL_SIZE)
def test_full_size_pixel_updates_match_the_reference(name):
    """BASELINE configs 3 and 4 at their FULL sizes against the REFERENCE (round-4 review, weak 1d: the pixel fixtures were
    B 8, the full-size tests compared the implicit-GEMM path with the im2col path): DrQv2 on 9 x 84 x 84 observations, B 512,
    hidden 1024 (`drqv2_pixels_full`) and SAC-Discrete on 4 x 84 x 84, B 1024, clip 40 (`atari_pixels_full`) -- one
    environment step each (two critic updates, Polyak, actor [, temperature] update) through the implicit-GEMM convolutions
    the benchmark runs, fixtures written by oracle/gen_golden.py from the unmodified reference.  Tolerances: see
    case_runner.compare_full_size (update 0 at the fp32 tolerances of every other fixture; parameters with counted, bounded
    sign-flip stragglers; what sits behind an optimizer step at 3e-3 / 1e-2)."""
    cfg = synth.CASES[name]
    rec = case_runner.run_engine(name)
    worst = case_runner.compare_full_size(rec, case_runner.load_fixture(name), cfg, who=f"hip[{name}]")
    print(f"{name}: worst deviations vs reference {worst}")


@pytest.mark.parametrize("name", ["redq_small", "pendulum_sac", "redq_M", "redq_S", "redq_c2"])
def test_chained_launch_forms_match_reference_and_each_other(name):
    """the chained launch (everything of a critic update that does not need the TD target) in its two forms: ONE
    workgroup per target chain (actor pass, then the target-critic pass, the actor repeated per subset slot) and the
    PRODUCER / CONSUMER form (the actor once per 16-row tile; the tile's target-critic workgroups gather their own s'
    rows, run fc1 on the state columns, poll the tagged a' granules and add a' W1[:, S:]^T).  Both land on the reference
    fixture; their TD targets agree to fp32 association of fc1's sum."""
    import super_sac_amd as ssa
    recs = {}
    for pc in (False, True):
        old = ssa.learning_utils.CHAIN_PC
        ssa.learning_utils.CHAIN_PC = pc
        try:
            recs[pc] = case_runner.run_engine(name)
        finally:
            ssa.learning_utils.CHAIN_PC = old
        case_runner.compare(recs[pc], case_runner.load_fixture(name), who=f"hip[{name}, chain {'producer/consumer' if pc else 'one workgroup'}]")
    for key in recs[True]:
        if "_td" in key:
            assert np.max(np.abs(recs[True][key] - recs[False][key])) <= 2e-5, key


@pytest.mark.parametrize("name", ["redq_small", "sac_popart", "sac_discrete", "td3_noise"])
def test_update_functions_adopt_a_foreign_agent(name):
    """an agent that carries ONLY the reference classes' attributes (tests/foreign_agent.py: no arena(), no
    action_size, plain-tensor PopArt, an identity encoder the engine has to recognise by probing) goes through the
    same update sequence and lands on the reference's outputs (the engine adopts `agent.*` in place)."""
    rec = case_runner.run_engine(name, foreign=True)
    case_runner.compare(rec, case_runner.load_fixture(name), who=f"hip[{name},foreign agent]")


@pytest.mark.parametrize("name", ["redq_small", "drqv2_pixels", "atari_pixels"])
def test_update_functions_adopt_a_foreign_buffer_and_augmenter(name):
    """a numpy replay buffer and an augmentation sequence that carry ONLY the reference classes' attributes
    (tests/foreign_agent.py; what experiments/gym/train_gym.py:84 and dmc/train_dmc_from_pixels.py:62,88 build before
    main.super_sac runs) are adopted in place by the first update -- storage moved to HBM, classes swapped, the
    randomisation kept -- and the sequence lands on the reference's outputs."""
    import super_sac_amd as ssa
    rec = case_runner.run_engine(name, foreign_io=True)
    case_runner.compare(rec, case_runner.load_fixture(name), who=f"hip[{name},foreign buffer + augmenter]")


def test_adopted_buffer_keeps_collecting_on_the_device():
    """after adoption the collection loop's buffer.push (main.py:365) lands in the HBM ring and the PER trees carry on"""
    import torch
    import foreign_agent
    import super_sac_amd as ssa
    s, a, r, s1, d = synth.synth_transitions(300, 5, 2, seed=3)
    buf = foreign_agent.ForeignReplayBuffer(512, s, a, r, s1, d)
    ssa.adopt_buffer(buf, torch.device("cuda"))
    assert type(buf) is ssa.replay.ReplayBuffer and len(buf) == 300 and buf._storage.s_stack["obs"].is_cuda
    assert np.array_equal(buf._storage.s_stack["obs"][:300].cpu().numpy(), s["obs"].astype(np.float32))
    assert np.array_equal(buf._storage.done_stack[:300, 0].cpu().numpy(), np.asarray(d).reshape(-1).astype(np.uint8))
    s2, a2, r2, s12, d2 = synth.synth_transitions(300, 5, 2, seed=4)
    buf.push(s2, a2, r2.reshape(-1, 1), s12, d2.reshape(-1, 1))   # wraps around the ring
    torch.cuda.synchronize()
    assert len(buf) == 512 and buf._storage._next_idx == (600 % 512)
    assert np.array_equal(buf._storage.action_stack[300:512].cpu().numpy(), a2[:212].astype(np.float32))
    assert np.array_equal(buf._storage.action_stack[:88].cpu().numpy(), a2[212:].astype(np.float32))
    assert buf._per.sum_tree[1] == 512.0
    with pytest.raises(TypeError, match="install"):
        ssa.adopt_buffer(object())


@pytest.mark.parametrize("seed", [0, 7, 123])
@pytest.mark.parametrize("n", [1000, 100_000, 1_000_000])
def test_product_index_draw_is_bit_exact_on_the_gpu_box(seed, n):
    """super_sac_amd.rng.draw_indices (what critic_update calls) under torch.manual_seed, on this machine, against
    the reference's replay.sample_uniform index stream (replay.py:121-126) recorded in replay_indices.npz; and the
    product replay buffer's sample_uniform returns those very rows."""
    import torch
    import super_sac_amd as ssa
    ref = case_runner.load_fixture("replay_indices")[f"s{seed}_n{n}"]
    torch.manual_seed(seed)
    got = np.stack([ssa.rng.draw_indices(n, 512).numpy() for _ in range(3)])
    assert got.dtype == np.int64 and np.array_equal(got, ref)
    if n == 1000:
        buf = ssa.replay.ReplayBuffer(2048, device=torch.device("cuda"))
        s, a, r, s1, d = synth.synth_transitions(n, 5, 2, seed=3)
        buf.load_experience(s, a, r, s1, d)
        torch.manual_seed(seed)
        (o, act, rew, o1, done), idx = buf.sample_uniform(512)
        assert np.array_equal(idx, ref[0])
        assert np.array_equal(o["obs"].cpu().numpy(), s["obs"][ref[0]])
        assert np.array_equal(act.cpu().numpy(), a[ref[0]])


def test_deferred_log_blocks_read_late_or_at_once():
    """recorded updates leave their log block to the NEXT update's first launch (or a flush when somebody looks
    first): values read long after the fact, values read at once and the eager path's values are the same numbers."""
    import copy
    import math
    import random
    from itertools import chain

    import torch
    import super_sac_amd as ssa

    def run(use_lists, read_now):
        old = ssa.learning.USE_GRAPHS
        ssa.learning.USE_GRAPHS = use_lists
        try:
            torch.manual_seed(4); np.random.seed(4); random.seed(4)
            dev = torch.device("cuda")
            agent = ssa.Agent(act_space_size=6, encoder=ssa.nets.IdentityEncoder(17),
                              actor_network_cls=ssa.nets.ContinuousStochasticActor,
                              critic_network_cls=ssa.nets.ContinuousCritic, ensemble_size=1, num_critics=4,
                              hidden_size=64, auto_rescale_targets=False, log_std_low=-5.0, log_std_high=2.0)
            agent.to(dev)
            target = copy.deepcopy(agent)
            buf = ssa.replay.ReplayBuffer(4096, device=dev)
            buf.load_experience(*synth.synth_transitions(2000, 17, 6, seed=5))
            copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=3e-4)
            eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
            la = torch.Tensor([math.log(0.1)]).to(dev); la.requires_grad = True
            aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(128)])
            kept, vals = [], []
            for k in range(14):
                logs, _ = ssa.learning.critic_update(
                    buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt,
                    log_alphas=[la], batch_size=128, gamma=0.99, critic_clip=None, encoder_clip=None,
                    target_critic_ensemble_n=2, weighted_bellman_temp=None, weight_type=None, pop=False,
                    augmenter=aug, encoder_lambda=0, aug_mix=0.0, discrete=False, random_process=None,
                    noise_clip=None, per=False, update_priorities=False, dr3_coeff=0.0)
                if k % 2 == 0:
                    ssa.learning_utils.soft_update(target.critics[0], agent.critics[0], 0.005)
                if read_now or k % 5 == 3:   # (some values are looked at straight away, most long afterwards)
                    vals.append({k_: float(v) for k_, v in logs.items()})
                    kept.append(None)
                else:
                    vals.append(None)
                    kept.append(logs)
            for k, lg in enumerate(kept):
                if lg is not None:
                    vals[k] = {k_: float(v) for k_, v in lg.items()}
            return vals
        finally:
            ssa.learning.USE_GRAPHS = old

    eager = run(False, True)
    late = run(True, False)
    now = run(True, True)
    assert all(np.isfinite(list(v.values())).all() and v["gradients/critic_random_grad"] > 0 for v in eager)
    for k in range(14):
        assert late[k] == eager[k] == now[k], (k, late[k], eager[k], now[k])


def test_engine_matches_oracle_on_metric_shape():
    """engine vs oracle directly (not via the fixture) at obs 17 / act 6 / B 512 / N 10."""
    rec_o = case_runner.run_oracle("redq_M")
    rec_e = case_runner.run_engine("redq_M")
    for key, val in rec_o.items():
        if "_td" in key:
            assert np.allclose(rec_e[key], val, atol=3e-4, rtol=1e-4), key
        if key.startswith("finalfp_") and not key.endswith("_v"):
            assert np.max(np.abs(rec_e[key] - val)) <= 3e-5, key


def test_grad_norm_log_and_lazy_logs():
    """logs are device scalars: readable, finite, and the grad-norm log is positive."""
    import torch
    rec = case_runner.run_engine("redq_small")
    assert all(np.isfinite(v) for k, v in rec.items() if "_log:" in k)
    assert rec["u0_log:gradients/critic_random_grad"] > 0
    assert rec["u0_log:gradients/encoder_criticloss_grad_norm"] == 0.0
    assert torch.cuda.is_available()


def test_graph_replay_equals_eager_launches():
    """20 critic updates (+Polyak) with the captured HIP graph vs. plain launches: same parameters."""
    import copy
    import math
    import random
    from itertools import chain

    import torch
    import super_sac_amd as ssa

    def run(use_graphs, split, mode="list", dual=True, rank1=True, fold=True, chained=True, gather=True, pc=True):
        L = ssa.learning
        old = (L.USE_GRAPHS, L.SPLIT_FORWARD, L.LAUNCH_MODE, L.DUAL_LAUNCH, L.RANK1_BWD, L.FOLD_LOSS)
        old_lu = (ssa.learning_utils.CHAIN_LAUNCH, ssa.learning_utils.FOLD_GATHER, ssa.learning_utils.CHAIN_PC)
        (L.USE_GRAPHS, L.SPLIT_FORWARD, L.LAUNCH_MODE, L.DUAL_LAUNCH, L.RANK1_BWD,
         L.FOLD_LOSS) = use_graphs, split, mode, dual, rank1, fold
        ssa.learning_utils.CHAIN_LAUNCH, ssa.learning_utils.FOLD_GATHER, ssa.learning_utils.CHAIN_PC = chained, gather, pc
        try:
            torch.manual_seed(3); np.random.seed(3); random.seed(3)
            dev = torch.device("cuda")
            agent = ssa.Agent(act_space_size=6, encoder=ssa.nets.IdentityEncoder(17),
                              actor_network_cls=ssa.nets.ContinuousStochasticActor,
                              critic_network_cls=ssa.nets.ContinuousCritic, ensemble_size=1, num_critics=4,
                              hidden_size=64, auto_rescale_targets=False, log_std_low=-5.0, log_std_high=2.0)
            agent.to(dev)
            target = copy.deepcopy(agent)
            buf = ssa.replay.ReplayBuffer(4096, device=dev)
            buf.load_experience(*synth.synth_transitions(2000, 17, 6, seed=5))
            copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=3e-4)
            eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
            la = torch.Tensor([math.log(0.1)]).to(dev); la.requires_grad = True
            aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(128)])
            last = None
            for k in range(20):
                logs, dicts = ssa.learning.critic_update(
                    buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt,
                    log_alphas=[la], batch_size=128, gamma=0.99, critic_clip=None, encoder_clip=None,
                    target_critic_ensemble_n=2, weighted_bellman_temp=None, weight_type=None, pop=False,
                    augmenter=aug, encoder_lambda=0, aug_mix=0.0, discrete=False, random_process=None,
                    noise_clip=None, per=False, update_priorities=False, dr3_coeff=0.0)
                if k % 2 == 0:
                    ssa.learning_utils.soft_update(target.critics[0], agent.critics[0], 0.005)
                last = (float(logs["losses/critic_overall_loss"]), float(logs["td_targets/mean_td_target_0"]),
                        dicts[0]["priority_idxs"].copy())
            params = torch.cat([p.detach().flatten() for p in agent.critics[0].parameters()]).cpu().numpy()
            tparams = torch.cat([p.detach().flatten() for p in target.critics[0].parameters()]).cpu().numpy()
            return params, tparams, last, buf.total_sample_calls
        finally:
            L.USE_GRAPHS, L.SPLIT_FORWARD, L.LAUNCH_MODE, L.DUAL_LAUNCH, L.RANK1_BWD, L.FOLD_LOSS = old
            ssa.learning_utils.CHAIN_LAUNCH, ssa.learning_utils.FOLD_GATHER, ssa.learning_utils.CHAIN_PC = old_lu

    # default configuration (merged launches, rank-1 backward): the three launch mechanisms agree bit for bit
    pe, te, le, ce = run(False, split=False)
    pg, tg, lg, cg = run(True, split=False, mode="list")     # the library's recorded launch list
    ph, th, lh, ch = run(True, split=False, mode="graph")    # a hipGraph captured through torch
    assert np.array_equal(pg, ph) and np.array_equal(tg, th) and lg[:2] == lh[:2] and ch == 20
    # ssac_step_run hands the replayed launches their input slot by value (include/ssac_hip.h: ssac_slot_by_value); the
    # hipGraph above found it through the feed block, and so does the list with the switch off: the same bits
    ssa._lib.lib.ssac_slot_by_value(0)
    try:
        pv, tv, lv, _ = run(True, split=False, mode="list")
    finally:
        ssa._lib.lib.ssac_slot_by_value(1)
    assert np.array_equal(pg, pv) and np.array_equal(tg, tv) and lg[:2] == lv[:2]
    # the one-launch critic kernel, the forward riding in the actor launch + backward-only launch, and the critic
    # forward as a parallel branch are the same arithmetic in the same order: bit-identical to each other
    # (the rank-1 backward reorders the scaling by dL/dq and is only tolerance-equal: covered by the fixtures)
    p0, t0, l0, _ = run(False, split=False, dual=False, rank1=False)
    pd, td_, ld_, _ = run(False, split=False, dual=True, rank1=False)
    p1, t1, l1, _ = run(False, split=True, dual=False, rank1=False)
    p2, t2, l2, _ = run(True, split=True, dual=False, rank1=False)
    assert np.array_equal(p1, p2) and np.array_equal(t1, t2)
    assert np.array_equal(p0, pd) and np.array_equal(t0, td_) and l0[0] == ld_[0], "merged actor + critic-forward launch"
    assert np.array_equal(p0, p1) and np.array_equal(t0, t1) and l0[0] == l1[0], \
        "split forward/backward launches must be bit-identical to the one-launch critic kernel"
    assert np.allclose(pe, p0, atol=2e-6) and np.allclose(te, t0, atol=2e-6), "rank-1 backward vs fused backward"
    # dL/dq evaluated inside the weight-gradient launch vs written by the separate loss launch: the same products
    # (the scale multiplies the rows when they are stored to LDS instead of when they are loaded)
    # the chained launch in its ONE-WORKGROUP form, the two merged launches and the replay gather as its own launch: same
    # bits, eager or replayed.  (The producer / consumer form of the chained launch -- today's default, `pe` above -- adds
    # the action columns of the target critics' fc1 AFTER the state columns' sum: equal to rounding, and bit-identical
    # across its own launch mechanisms and with or without the folded gather.)
    po, to, lo, _ = run(False, split=False, pc=False)
    assert np.allclose(pe, po, atol=2e-6) and np.allclose(te, to, atol=2e-6), "producer/consumer vs one-workgroup chained launch"
    for kw in (dict(chained=False), dict(chained=False, gather=False), dict(gather=False, pc=False)):
        for graphs in (False, True):
            pc, tc_, lc, _ = run(graphs, split=False, **kw)
            assert np.array_equal(po, pc) and np.array_equal(to, tc_) and lo[:2] == lc[:2], (kw, graphs)
    for graphs in (False, True):
        pc, tc_, lc, _ = run(graphs, split=False, gather=False)
        assert np.array_equal(pe, pc) and np.array_equal(te, tc_) and le[:2] == lc[:2], ("producer/consumer, gather launch", graphs)
    pf, tf, lf, _ = run(False, split=False, fold=False)
    assert np.array_equal(pe, pf) and np.array_equal(te, tf), "folded loss gradient vs loss launch"
    assert abs(le[0] - lf[0]) <= 1e-5 * max(1.0, abs(lf[0])) and abs(le[1] - lf[1]) <= 1e-5 * max(1.0, abs(lf[1]))
    assert ce == cg == 20
    assert np.array_equal(le[2], lg[2]), "replay indices must not depend on the launch mechanism"
    assert np.array_equal(pe, pg) and np.array_equal(te, tg), "graph replay must be bit-identical to eager launches"
    assert le[0] == lg[0] and le[1] == lg[1]


@pytest.mark.parametrize("setting", ["eager", "no-dual-launch", "no-rank1-backward", "no-loss-fold", "recorded-list"])
def test_critic_update_hands_back_no_private_launch_state(setting):
    """which launch did which part of a member's update travels in the member's record, not in what the caller gets
    back: the replay dicts hold no private key but "_ssac", "_subset", "_x1", and the TD target is a plain tensor.
    (obs 17 / act 6 / hidden 64 / 4 critics / subset 2 / B 128: the smallest shape at which every merged launch
    form is still eligible; recorded-list runs 5 calls past the warm-up, so the fast C step hands back the dicts too)"""
    import copy
    import math
    import random
    from itertools import chain

    import torch
    import super_sac_amd as ssa

    L = ssa.learning
    knob = {"no-dual-launch": "DUAL_LAUNCH", "no-rank1-backward": "RANK1_BWD", "no-loss-fold": "FOLD_LOSS"}.get(setting)
    recorded = setting == "recorded-list"
    old = (L.USE_GRAPHS, L.LAUNCH_MODE, L.DUAL_LAUNCH, L.RANK1_BWD, L.FOLD_LOSS)
    L.USE_GRAPHS, L.LAUNCH_MODE = recorded, "list"
    if knob is not None:
        setattr(L, knob, False)
    try:
        torch.manual_seed(3); np.random.seed(3); random.seed(3)
        dev = torch.device("cuda")
        agent = ssa.Agent(act_space_size=6, encoder=ssa.nets.IdentityEncoder(17),
                          actor_network_cls=ssa.nets.ContinuousStochasticActor,
                          critic_network_cls=ssa.nets.ContinuousCritic, ensemble_size=1, num_critics=4,
                          hidden_size=64, auto_rescale_targets=False, log_std_low=-5.0, log_std_high=2.0)
        agent.to(dev)
        target = copy.deepcopy(agent)
        buf = ssa.replay.ReplayBuffer(4096, device=dev)
        buf.load_experience(*synth.synth_transitions(2000, 17, 6, seed=5))
        copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=3e-4)
        eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
        la = torch.Tensor([math.log(0.1)]).to(dev); la.requires_grad = True
        aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(128)])
        for k in range(L.GRAPH_WARMUP + 1 + 5 if recorded else 2):
            _, dicts = L.critic_update(
                buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt,
                log_alphas=[la], batch_size=128, gamma=0.99, critic_clip=None, encoder_clip=None,
                target_critic_ensemble_n=2, weighted_bellman_temp=None, weight_type=None, pop=False,
                augmenter=aug, encoder_lambda=0, aug_mix=0.0, discrete=False, random_process=None,
                noise_clip=None, per=False, update_priorities=False, dr3_coeff=0.0)
            for rd in dicts:
                private = sorted(k_ for k_ in rd if isinstance(k_, str) and k_.startswith("_"))
                assert set(private) <= {"_ssac", "_subset", "_x1"}, (setting, k, private)
                hung = [n_ for n_ in vars(rd["td_target"]) if n_.startswith("_ssac")]
                assert not hung, (setting, k, hung)
        if recorded:
            assert agent.__dict__.get("_ssac_fast"), "the fast C step was never reached"
    finally:
        L.USE_GRAPHS, L.LAUNCH_MODE, L.DUAL_LAUNCH, L.RANK1_BWD, L.FOLD_LOSS = old


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_late_bound_polyak_equals_the_polyak_launch(precision):
    """soft_update right behind a recorded critic update leaves a request in the input ring's tail and the update's own
    weight-gradient launch applies the target update (ssac_late_polyak): bit-identical to the Polyak launch -- whether
    the request is served (host ahead of the device), found too late (device already past the update: the fallback
    launches the kernel) or the mechanism is switched off."""
    import copy
    import math
    import random
    from itertools import chain

    import torch
    import super_sac_amd as ssa
    lu = ssa.learning_utils

    def run(late, sync_before, tau_seq):
        old = lu.LATE_POLYAK
        lu.LATE_POLYAK = late
        served = [0, 0]
        real_polyak = ssa._lib.lib.ssac_step_polyak

        def counting(handle, tau):   # (ctypes function objects are replaceable attributes of the CDLL)
            rc = real_polyak(handle, tau)
            served[0 if rc == 1 else 1] += 1
            return rc
        try:
            torch.manual_seed(3); np.random.seed(3); random.seed(3)
            dev = torch.device("cuda")
            agent = ssa.Agent(act_space_size=6, encoder=ssa.nets.IdentityEncoder(17),
                              actor_network_cls=ssa.nets.ContinuousStochasticActor,
                              critic_network_cls=ssa.nets.ContinuousCritic, ensemble_size=1, num_critics=4,
                              hidden_size=64, auto_rescale_targets=False, log_std_low=-5.0, log_std_high=2.0)
            agent.to(dev)
            ssa.set_precision(agent, precision)
            target = copy.deepcopy(agent)
            buf = ssa.replay.ReplayBuffer(4096, device=dev)
            buf.load_experience(*synth.synth_transitions(2000, 17, 6, seed=5))
            copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=3e-4)
            eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
            la = torch.Tensor([math.log(0.1)]).to(dev); la.requires_grad = True
            aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(128)])
            ssa._lib.lib.ssac_step_polyak = counting
            for k in range(48):   # (more than one trip around the 32-slot input ring)
                if k == 8 and not sync_before:
                    # park the device for a few milliseconds so that the host runs ahead of it, as it does in a
                    # GPU-bound training loop (this tiny network alone keeps up with the host)
                    torch.cuda._sleep(20_000_000)
                ssa.learning.critic_update(
                    buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt,
                    log_alphas=[la], batch_size=128, gamma=0.99, critic_clip=None, encoder_clip=None,
                    target_critic_ensemble_n=2, weighted_bellman_temp=None, weight_type=None, pop=False,
                    augmenter=aug, encoder_lambda=0, aug_mix=0.0, discrete=False, random_process=None,
                    noise_clip=None, per=False, update_priorities=False, dr3_coeff=0.0)
                if tau_seq[k % len(tau_seq)]:
                    if sync_before:
                        torch.cuda.synchronize()
                    lu.soft_update(target.critics[0], agent.critics[0], tau_seq[k % len(tau_seq)])
            params = torch.cat([p.detach().flatten() for p in agent.critics[0].parameters()]).cpu().numpy()
            tparams = torch.cat([p.detach().flatten() for p in target.critics[0].parameters()]).cpu().numpy()
            return params, tparams, served
        finally:
            lu.LATE_POLYAK = old
            ssa._lib.lib.ssac_step_polyak = real_polyak

    taus = (0.005, 0.0, 0.01, 0.0, 0.0)   # irregular pattern, two different step sizes
    p0, t0, s0 = run(False, False, taus)
    p1, t1, s1 = run(True, False, taus)
    p2, t2, s2 = run(True, True, taus)
    assert s0 == [0, 0], "switched off: no request is ever made"
    assert s1[0] > 0, "requests are served by the weight-gradient launch (ahead of it, or decided while the host waits)"
    assert s2[0] == 0 and s2[1] > 0, "device idle before every soft_update: every request comes too late"
    assert np.array_equal(p0, p1) and np.array_equal(t0, t1), "served requests vs Polyak launches"
    assert np.array_equal(p0, p2) and np.array_equal(t0, t2), "late requests must fall back to the Polyak launch"


def test_late_bound_polyak_under_random_timing():
    """the host / device race of the late-bound Polyak request, exercised instead of staged: 1500 recorded updates, a
    soft_update behind every second one, with random host delays (0-150 us busy wait) in front of the request and
    random device stalls (0-40 us) in front of the updates, so requests arrive before the update's first launch has
    begun, while it runs, and after it -- in one run.  Online and target parameters must equal, bit for bit, those of
    the same run with the mechanism switched off (a Polyak launch per soft_update)."""
    import copy
    import math
    import random
    import time
    from itertools import chain

    import torch
    import super_sac_amd as ssa
    lu = ssa.learning_utils

    def run(late):
        old = lu.LATE_POLYAK
        lu.LATE_POLYAK = late
        served = [0, 0]
        real_polyak = ssa._lib.lib.ssac_step_polyak

        def counting(handle, tau):
            rc = real_polyak(handle, tau)
            served[0 if rc == 1 else 1] += 1
            return rc
        try:
            torch.manual_seed(4); np.random.seed(4); random.seed(4)
            jitter = np.random.RandomState(99)
            dev = torch.device("cuda")
            agent = ssa.Agent(act_space_size=6, encoder=ssa.nets.IdentityEncoder(17),
                              actor_network_cls=ssa.nets.ContinuousStochasticActor,
                              critic_network_cls=ssa.nets.ContinuousCritic, ensemble_size=1, num_critics=10,
                              hidden_size=256, auto_rescale_targets=False, log_std_low=-5.0, log_std_high=2.0)
            agent.to(dev)
            target = copy.deepcopy(agent)
            buf = ssa.replay.ReplayBuffer(8192, device=dev)
            buf.load_experience(*synth.synth_transitions(4000, 17, 6, seed=6))
            copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=3e-4)
            eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
            la = torch.Tensor([math.log(0.1)]).to(dev); la.requires_grad = True
            aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(512)])
            ssa._lib.lib.ssac_step_polyak = counting
            for k in range(1500):
                stall = int(jitter.randint(0, 4)) * 25_000       # 0 / ~13 / ~27 / ~40 us of device stall
                if stall:
                    torch.cuda._sleep(stall)
                ssa.learning.critic_update(
                    buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt,
                    log_alphas=[la], batch_size=512, gamma=0.99, critic_clip=None, encoder_clip=None,
                    target_critic_ensemble_n=2, weighted_bellman_temp=None, weight_type=None, pop=False,
                    augmenter=aug, encoder_lambda=0, aug_mix=0.0, discrete=False, random_process=None,
                    noise_clip=None, per=False, update_priorities=False, dr3_coeff=0.0)
                if k % 2:
                    t_end = time.perf_counter() + float(jitter.randint(0, 150)) * 1e-6
                    while time.perf_counter() < t_end:
                        pass
                    lu.soft_update(target.critics[0], agent.critics[0], 0.005)
                if k % 400 == 399:
                    torch.cuda.synchronize()   # (drain now and then: the host is not always far ahead)
            params = torch.cat([p.detach().flatten() for p in agent.critics[0].parameters()]).cpu().numpy()
            tparams = torch.cat([p.detach().flatten() for p in target.critics[0].parameters()]).cpu().numpy()
            return params, tparams, served
        finally:
            lu.LATE_POLYAK = old
            ssa._lib.lib.ssac_step_polyak = real_polyak

    p0, t0, s0 = run(False)
    p1, t1, s1 = run(True)
    assert s0 == [0, 0] and 700 <= sum(s1) <= 750   # (the first updates run eagerly: their soft_update is a launch)
    assert s1[0] > 0, f"no request was ever served by the weight-gradient launch: {s1}"
    assert np.array_equal(t0, t1), f"target parameters differ (served / fell back: {s1})"
    assert np.array_equal(p0, p1), f"online parameters differ (served / fell back: {s1})"
    print(f"late-bound Polyak under random timing: {s1[0]} served in the weight-gradient launch, {s1[1]} fell back")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per-layer"])
@pytest.mark.parametrize("name", sorted(synth.AFBC_CASES))
def test_afbc_and_per_match_reference(name, fused):
    """learning.offline_actor_update (advantage filter from one stacked ensemble-Q launch,
    filtered BC gradient, Adam) with prioritised sampling and the advantage-based priority refresh.  Prioritised
    indices and importance weights must equal the reference's (float64 trees on the host, numpy global stream);
    priorities within 2e-4, logs 5e-4, final actor parameters 3e-5."""
    import super_sac_amd as ssa
    old = ssa.engine.USE_FUSED
    ssa.engine.USE_FUSED = fused
    try:
        rec = case_runner.run_afbc_engine(name)
    finally:
        ssa.engine.USE_FUSED = old
    case_runner.compare_afbc(rec, case_runner.load_fixture(name))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per-layer"])
@pytest.mark.parametrize("name", sorted(synth.MARKOV_CASES))
def test_markov_state_abstraction_update_matches_reference(name, fused):
    """learning.markov_state_abstraction_update (learning.py:266-341) -- inverse model (tanh-normal
    / categorical log-probability of the data action), contrastive model on [real | shuffled] transitions with BCE,
    smoothness hinge, joint clip over encoder + both models, one Adam step -- on vector observations and through
    both pixel encoders (s and s' as one stacked pass).  Logs within 5e-4 (gradient norms 2e-3), parameters 3e-5."""
    import super_sac_amd as ssa
    old = ssa.engine.USE_FUSED
    ssa.engine.USE_FUSED = fused
    try:
        rec = case_runner.run_markov_engine(name)
    finally:
        ssa.engine.USE_FUSED = old
    cfg = synth.MARKOV_CASES[name]
    case_runner.compare_markov(rec, case_runner.load_fixture(name), f"hip[{name}]",
                               max_step=2.2 * cfg["lr"] * cfg["markov"]["steps"] if "pixels" in name else 0.0)


@pytest.mark.parametrize("name", sorted(synth.BC_PIXEL_CASES))
def test_bc_warmup_trains_the_pixel_encoder_through_the_bc_loss(name):
    """main.py:292-312 (dmc/bc_from_pixels.gin): learning.offline_actor_update(update_encoder=True, filter_=False,
    per=False) -- the actor's input gradient runs back through the conv engine, encoder clip and optimizer step
    included.  Logs within 5e-4 (gradient norms 2e-3), actor and encoder parameters 3e-5."""
    cfg = synth.BC_PIXEL_CASES[name]
    rec = case_runner.run_bc_pixels_engine(name)
    case_runner.compare_markov(rec, case_runner.load_fixture(name), f"hip[{name}]",
                               max_step=2.2 * max(cfg["lr"], cfg["pixels"]["enc_lr"]) * len(cfg["steps"]))


@pytest.mark.parametrize("name", sorted(synth.ACTOR_INV_CASES))
def test_action_invariance_constraint_matches_reference(name):
    """learning.offline_actor_update(actor_lambda > 0) (learning_utils.py:272-285): an action sampled at the original
    observation must be as likely at the augmented one.  The BC rows and the augmented rows run through the actor (and
    a pixel encoder) as ONE stacked pass; the encoder is clipped and logged always, stepped only with update_encoder.
    Logs within 5e-4 (gradient norms 2e-3), parameters 3e-5."""
    cfg = synth.ACTOR_INV_CASES[name]
    rec = case_runner.run_actor_inv_engine(name)
    px = cfg.get("pixels")
    case_runner.compare_markov(rec, case_runner.load_fixture(name), f"hip[{name}]",
                               max_step=2.2 * max(cfg["lr"], px["enc_lr"]) * len(cfg["steps"]) if px else 0.0)


@pytest.mark.parametrize("name", ["drqv2_pixels", "atari_pixels"])
def test_pixel_cases_with_implicit_gemm_convolutions(name):
    """the pixel fixtures again with the implicit-GEMM kernels forced on for every eligible layer (the
    automatic choice keeps maps this small on im2col)."""
    import super_sac_amd as ssa
    old = ssa.conv_encoder.IMPLICIT_MIN_ROWS, ssa.conv_encoder.FIRST_MIN_ROWS
    ssa.conv_encoder.IMPLICIT_MIN_ROWS = ssa.conv_encoder.FIRST_MIN_ROWS = 0
    try:
        rec = case_runner.run_engine(name)
    finally:
        ssa.conv_encoder.IMPLICIT_MIN_ROWS, ssa.conv_encoder.FIRST_MIN_ROWS = old
    case_runner.compare(rec, case_runner.load_fixture(name), who=f"hip[{name},implicit-conv]")


def test_recorded_updates_with_a_wide_action_head():
    """9-dimensional actions: the actor's 18 outputs take two 16-column passes of the fused kernels' head (an
    earlier version sent such actors to the per-layer kernels with torch's generator for the noise, and that
    combination once crashed the recording).  Recorded replay must equal eager launches bit for bit."""
    import copy
    import math
    import random
    from itertools import chain

    import torch
    import super_sac_amd as ssa

    def run(use_lists):
        old = ssa.learning.USE_GRAPHS
        ssa.learning.USE_GRAPHS = use_lists
        try:
            torch.manual_seed(5); np.random.seed(5); random.seed(5)
            dev = torch.device("cuda")
            agent = ssa.Agent(act_space_size=9, encoder=ssa.nets.IdentityEncoder(20),
                              actor_network_cls=ssa.nets.ContinuousStochasticActor,
                              critic_network_cls=ssa.nets.ContinuousCritic, ensemble_size=1, num_critics=2,
                              hidden_size=64, auto_rescale_targets=False, log_std_low=-5.0, log_std_high=2.0)
            agent.to(dev)
            target = copy.deepcopy(agent)
            buf = ssa.replay.ReplayBuffer(2048, device=dev)
            buf.load_experience(*synth.synth_transitions(1000, 20, 9, seed=7))
            copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=3e-4)
            eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
            la = torch.Tensor([math.log(0.1)]).to(dev); la.requires_grad = True
            aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(64)])
            for _ in range(8):
                ssa.learning.critic_update(
                    buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt,
                    log_alphas=[la], batch_size=64, gamma=0.99, critic_clip=None, encoder_clip=None,
                    target_critic_ensemble_n=2, weighted_bellman_temp=None, weight_type=None, pop=False,
                    augmenter=aug, encoder_lambda=0, aug_mix=0.0, discrete=False, random_process=None,
                    noise_clip=None, per=False, update_priorities=False, dr3_coeff=0.0)
            return torch.cat([p.detach().flatten() for p in agent.critics[0].parameters()]).cpu().numpy()
        finally:
            ssa.learning.USE_GRAPHS = old

    assert np.array_equal(run(False), run(True))


def test_recorded_updates_wrap_the_input_ring():
    """100 recorded updates (the 32-slot input ring wraps three times, slot reuse is guarded by one stream event per 8
    updates) against 100 eager updates: same parameters, same last logs, same replay indices."""
    import copy
    import math
    import random
    from itertools import chain

    import torch
    import super_sac_amd as ssa

    def run(recorded):
        old = ssa.learning.USE_GRAPHS
        ssa.learning.USE_GRAPHS = recorded
        try:
            torch.manual_seed(11); np.random.seed(11); random.seed(11)
            dev = torch.device("cuda")
            agent = ssa.Agent(act_space_size=3, encoder=ssa.nets.IdentityEncoder(11),
                              actor_network_cls=ssa.nets.ContinuousStochasticActor,
                              critic_network_cls=ssa.nets.ContinuousCritic, ensemble_size=1, num_critics=3,
                              hidden_size=64, auto_rescale_targets=False, log_std_low=-5.0, log_std_high=2.0)
            agent.to(dev)
            target = copy.deepcopy(agent)
            buf = ssa.replay.ReplayBuffer(4096, device=dev)
            buf.load_experience(*synth.synth_transitions(1500, 11, 3, seed=9))
            copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=3e-4)
            eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
            la = torch.Tensor([math.log(0.2)]).to(dev); la.requires_grad = True
            aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(96)])
            seen = []
            for k in range(100):
                logs, dicts = ssa.learning.critic_update(
                    buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt,
                    log_alphas=[la], batch_size=96, gamma=0.99, critic_clip=None, encoder_clip=None,
                    target_critic_ensemble_n=2, weighted_bellman_temp=None, weight_type=None, pop=False,
                    augmenter=aug, encoder_lambda=0, aug_mix=0.0, discrete=False, random_process=None,
                    noise_clip=None, per=False, update_priorities=False, dr3_coeff=0.0)
                if k % 2 == 1:
                    ssa.learning_utils.soft_update(target.critics[0], agent.critics[0], 0.01)
                if k in (40, 99):  # (reading a log in the middle drains the queue: the ring must cope with that too)
                    seen.append((float(logs["losses/critic_overall_loss"]), float(logs["td_targets/mean_td_target_0"]),
                                 dicts[0]["priority_idxs"].copy()))
            params = torch.cat([p.detach().flatten() for p in agent.critics[0].parameters()]).cpu().numpy()
            tparams = torch.cat([p.detach().flatten() for p in target.critics[0].parameters()]).cpu().numpy()
            return params, tparams, seen
        finally:
            ssa.learning.USE_GRAPHS = old

    pe, te, se = run(False)
    pr, tr, sr = run(True)
    assert np.array_equal(pe, pr) and np.array_equal(te, tr)
    for a, b in zip(se, sr):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])


def test_recorded_updates_change_replayer_in_the_middle_of_a_run():
    """The shapes of test_recorded_updates_wrap_the_input_ring, but for calls 45-52 and 77-78 the C step
    (ssac_step_run) is out of reach, so those calls replay through the Python path on the same record and hand back
    to the C step afterwards.  The first window starts off an EVENT_EVERY boundary, crosses one and comes after the
    input ring has wrapped once; the second is shorter than an event group.  Against 100 eager updates: same
    parameters, same target parameters, same logs and replay indices at calls 40, 60 and 99, bit for bit."""
    import copy
    import math
    import random
    from itertools import chain

    import torch
    import super_sac_amd as ssa

    n_upd, windows = 100, ((45, 52), (77, 78))

    def run(recorded):
        old = ssa.learning.USE_GRAPHS
        ssa.learning.USE_GRAPHS = recorded
        try:
            torch.manual_seed(11); np.random.seed(11); random.seed(11)
            dev = torch.device("cuda")
            agent = ssa.Agent(act_space_size=3, encoder=ssa.nets.IdentityEncoder(11),
                              actor_network_cls=ssa.nets.ContinuousStochasticActor,
                              critic_network_cls=ssa.nets.ContinuousCritic, ensemble_size=1, num_critics=3,
                              hidden_size=64, auto_rescale_targets=False, log_std_low=-5.0, log_std_high=2.0)
            agent.to(dev)
            target = copy.deepcopy(agent)
            buf = ssa.replay.ReplayBuffer(4096, device=dev)
            buf.load_experience(*synth.synth_transitions(1500, 11, 3, seed=9))
            copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=3e-4)
            eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
            la = torch.Tensor([math.log(0.2)]).to(dev); la.requires_grad = True
            aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(96)])
            seen, taken = [], {}
            for k in range(n_upd):
                if recorded and any(k == first for first, _ in windows):
                    fast = agent.__dict__["_ssac_fast"]
                    taken = dict(fast)
                    assert taken, "the fast C step was never reached"
                    fast.clear()
                logs, dicts = ssa.learning.critic_update(
                    buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt,
                    log_alphas=[la], batch_size=96, gamma=0.99, critic_clip=None, encoder_clip=None,
                    target_critic_ensemble_n=2, weighted_bellman_temp=None, weight_type=None, pop=False,
                    augmenter=aug, encoder_lambda=0, aug_mix=0.0, discrete=False, random_process=None,
                    noise_clip=None, per=False, update_priorities=False, dr3_coeff=0.0)
                if recorded and any(k == last for _, last in windows):
                    assert not agent.__dict__["_ssac_fast"], "a second C step was built inside the window"
                    agent.__dict__["_ssac_fast"].update(taken)   # the same objects
                if k % 2 == 1:
                    ssa.learning_utils.soft_update(target.critics[0], agent.critics[0], 0.01)
                if k in (40, 60, 99):
                    seen.append((float(logs["losses/critic_overall_loss"]), float(logs["td_targets/mean_td_target_0"]),
                                 dicts[0]["priority_idxs"].copy()))
            params = torch.cat([p.detach().flatten() for p in agent.critics[0].parameters()]).cpu().numpy()
            tparams = torch.cat([p.detach().flatten() for p in target.critics[0].parameters()]).cpu().numpy()
            if recorded:
                record, = agent.__dict__["_ssac_graphs"].values()
                step, = agent.__dict__["_ssac_fast"].values()
                assert step is record.fast and step.gs is record
                assert record.path == "fast"
                assert record.k == n_upd - ssa.learning.GRAPH_WARMUP
                # every call but the warm-up, the recording call and the two windows went through the C step
                assert step.calls == n_upd - ssa.learning.GRAPH_WARMUP - 1 - sum(b - a + 1 for a, b in windows)
            return params, tparams, seen
        finally:
            ssa.learning.USE_GRAPHS = old

    pe, te, se = run(False)
    pr, tr, sr = run(True)
    assert np.array_equal(pe, pr) and np.array_equal(te, tr)
    assert len(se) == len(sr) == 3
    for a, b in zip(se, sr):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])


def test_recorded_updates_record_again_when_a_noise_hook_comes_and_goes():
    """The shapes of test_recorded_updates_wrap_the_input_ring with a noise hook (a private generator behind rng.draw_normal /
    rng.draw_normal_into) installed before call 43 and removed before call 59.  Each change makes the recorded run drop
    its recording and record again -- at ring updates 40 and 56, both past FEED_SLOTS and on an EVENT_EVERY boundary, on
    the same input ring -- and retires the C step built over the dropped launch lists; a new one serves the calls after.
    Against eager updates under the same hook schedule: same parameters, target parameters, logs and replay indices."""
    import copy
    import math
    import random
    from itertools import chain

    import torch
    import super_sac_amd as ssa

    n_upd, hook_on, hook_off = 100, 43, 59

    def run(recorded):
        old = ssa.learning.USE_GRAPHS, ssa.rng.draw_normal, ssa.rng.draw_normal_into
        ssa.learning.USE_GRAPHS = recorded
        try:
            torch.manual_seed(11); np.random.seed(11); random.seed(11)
            dev = torch.device("cuda")
            gen = torch.Generator(device=dev)
            gen.manual_seed(77)
            agent = ssa.Agent(act_space_size=3, encoder=ssa.nets.IdentityEncoder(11),
                              actor_network_cls=ssa.nets.ContinuousStochasticActor,
                              critic_network_cls=ssa.nets.ContinuousCritic, ensemble_size=1, num_critics=3,
                              hidden_size=64, auto_rescale_targets=False, log_std_low=-5.0, log_std_high=2.0)
            agent.to(dev)
            target = copy.deepcopy(agent)
            buf = ssa.replay.ReplayBuffer(4096, device=dev)
            buf.load_experience(*synth.synth_transitions(1500, 11, 3, seed=9))
            copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=3e-4)
            eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
            la = torch.Tensor([math.log(0.2)]).to(dev); la.requires_grad = True
            aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(96)])
            seen, steps = [], []
            for k in range(n_upd):
                if k == hook_on:
                    ssa.rng.draw_normal = lambda shape, device: torch.randn(*shape, device=device, generator=gen)
                    ssa.rng.draw_normal_into = lambda dst: dst.normal_(generator=gen)
                if k == hook_off:
                    ssa.rng.draw_normal, ssa.rng.draw_normal_into = old[1:]
                logs, dicts = ssa.learning.critic_update(
                    buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt,
                    log_alphas=[la], batch_size=96, gamma=0.99, critic_clip=None, encoder_clip=None,
                    target_critic_ensemble_n=2, weighted_bellman_temp=None, weight_type=None, pop=False,
                    augmenter=aug, encoder_lambda=0, aug_mix=0.0, discrete=False, random_process=None,
                    noise_clip=None, per=False, update_priorities=False, dr3_coeff=0.0)
                if k % 2 == 1:
                    ssa.learning_utils.soft_update(target.critics[0], agent.critics[0], 0.01)
                if k in (40, 43, 50, 59, 99):
                    seen.append((float(logs["losses/critic_overall_loss"]), float(logs["td_targets/mean_td_target_0"]),
                                 dicts[0]["priority_idxs"].copy()))
                if recorded and k in (hook_on - 1, hook_on, hook_off - 1, hook_off, n_upd - 1):
                    record, = agent.__dict__["_ssac_graphs"].values()
                    steps.append((record.fast, record.in_kernel_noise, record.k))
            params = torch.cat([p.detach().flatten() for p in agent.critics[0].parameters()]).cpu().numpy()
            tparams = torch.cat([p.detach().flatten() for p in target.critics[0].parameters()]).cpu().numpy()
            if recorded:
                warm = ssa.learning.GRAPH_WARMUP
                # the ring goes on counting over both re-recordings: no update starts again from slot 0
                assert [s_[2] for s_ in steps] == [hook_on - warm, hook_on - warm + 1, hook_off - warm, hook_off - warm + 1,
                                                  n_upd - warm]
                assert [s_[1] for s_ in steps] == [True, False, False, True, True]
                # three C steps, one per recording; each is retired with its recording and serves only its own calls
                first, second, third = steps[0][0], steps[1][0], steps[3][0]
                assert steps[2][0] is second and steps[4][0] is third and len({id(first), id(second), id(third)}) == 3
                assert first.calls == hook_on - warm - 1          # calls 4 .. 42 (+ 0: call 43 finds the hook first)
                assert second.calls == hook_off - hook_on - 1     # calls 44 .. 58
                assert third.calls == n_upd - hook_off - 1        # calls 60 .. 99
                assert record.path == "fast" and list(agent.__dict__["_ssac_fast"].values()) == [third]
            return params, tparams, seen
        finally:
            ssa.learning.USE_GRAPHS, ssa.rng.draw_normal, ssa.rng.draw_normal_into = old

    pe, te, se = run(False)
    pr, tr, sr = run(True)
    assert np.array_equal(pe, pr) and np.array_equal(te, tr)
    assert len(se) == len(sr) == 5
    for a, b in zip(se, sr):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])


def test_packed_push_and_n_step_fold_match_the_reference_storage():
    """buffer.push through the packed single-copy path (ring wrap-around, batched and single transitions, uint8
    images) against a plain numpy ring (ReplayBufferStorage.add, replay.py:48-60), and NStepFolder against the
    collection loop's n-step arithmetic (main.py:347-365)."""
    import torch
    import super_sac_amd as ssa
    rng_ = np.random.RandomState(0)
    cap, S, A = 37, 5, 2
    buf = ssa.replay.ReplayBuffer(cap, device=torch.device("cuda"))
    ring = {k: None for k in ("s", "a", "r", "s1", "d")}
    nxt, filled = 0, 0
    for num in (1, 1, 8, 30, 1, 5, 37, 3):
        s = rng_.standard_normal((num, S)).astype(np.float32)
        s1 = rng_.standard_normal((num, S)).astype(np.float32)
        a = rng_.uniform(-1, 1, (num, A)).astype(np.float32)
        r = rng_.standard_normal((num, 1)).astype(np.float32)
        d = (rng_.uniform(size=(num, 1)) < 0.3)
        if num == 1:
            R = buf.push({"obs": s[0]}, a[0], float(r[0, 0]), {"obs": s1[0]}, bool(d[0, 0]))
        else:
            R = buf.push({"obs": s}, a, r, {"obs": s1}, d)
        if ring["s"] is None:
            ring = {"s": np.zeros((cap, S), np.float32), "s1": np.zeros((cap, S), np.float32),
                    "a": np.zeros((cap, A), np.float32), "r": np.zeros((cap, 1), np.float32),
                    "d": np.zeros((cap, 1), np.uint8)}
        rows = np.arange(nxt, nxt + num) % cap
        assert np.array_equal(np.asarray(R), rows)
        ring["s"][rows], ring["s1"][rows], ring["a"][rows], ring["r"][rows], ring["d"][rows] = s, s1, a, r, d
        nxt, filled = (nxt + num) % cap, min(max(nxt + num, filled), cap)
        assert len(buf) == filled
    st = buf._storage
    torch.cuda.synchronize()
    assert np.array_equal(st.s_stack["obs"].cpu().numpy(), ring["s"])
    assert np.array_equal(st.s1_stack["obs"].cpu().numpy(), ring["s1"])
    assert np.array_equal(st.action_stack.cpu().numpy(), ring["a"])
    assert np.array_equal(st.reward_stack.cpu().numpy(), ring["r"])
    assert np.array_equal(st.done_stack.cpu().numpy(), ring["d"])
    # uint8 image observations stay uint8 on the device
    ib = ssa.replay.ReplayBuffer(16, device=torch.device("cuda"))
    img = rng_.randint(0, 256, (6, 3, 8, 8)).astype(np.uint8)
    ib.push({"obs": img}, np.zeros((6, 1), np.float32), np.zeros((6, 1), np.float32), {"obs": img[::-1].copy()},
            np.zeros((6, 1), bool))
    torch.cuda.synchronize()
    assert ib._storage.s_stack["obs"].dtype == torch.uint8
    assert np.array_equal(ib._storage.s_stack["obs"][:6].cpu().numpy(), img)
    assert np.array_equal(ib._storage.s1_stack["obs"][:6].cpu().numpy(), img[::-1])
    # ---- n-step fold: the reference loop's arithmetic on a stream of raw transitions with episode ends
    n_step, gamma = 3, 0.99
    nb = ssa.replay.ReplayBuffer(64, device=torch.device("cuda"))
    folder = ssa.replay.NStepFolder(nb, n_step, gamma)
    from collections import deque
    dq, want = deque([], maxlen=n_step), []
    for t in range(40):
        s = {"obs": rng_.standard_normal(S).astype(np.float32)}
        s1 = {"obs": rng_.standard_normal(S).astype(np.float32)}
        a = rng_.uniform(-1, 1, A).astype(np.float32)
        r, term = float(rng_.standard_normal()), bool(rng_.uniform() < 0.1)
        folder.add(s, a, r, s1, term, done=term)
        dq.append((s, a, r, s1, term))
        if len(dq) == dq.maxlen:  # main.py:358-365
            s_, a_, r_, s1_, d_ = dq.popleft()
            for i, trans in enumerate(dq):
                *_, r_i, s1_, d_ = trans
                r_ += (gamma ** (i + 1)) * r_i
            want.append((s_["obs"], a_, np.float32(r_), s1_["obs"], d_))
        if term:
            folder.clear()
            dq.clear()
    torch.cuda.synchronize()
    assert len(nb) == len(want) > 10
    ns = nb._storage
    assert np.array_equal(ns.s_stack["obs"][:len(want)].cpu().numpy(), np.stack([w[0] for w in want]))
    assert np.array_equal(ns.action_stack[:len(want)].cpu().numpy(), np.stack([w[1] for w in want]))
    assert np.array_equal(ns.reward_stack[:len(want), 0].cpu().numpy(), np.array([w[2] for w in want], np.float32))
    assert np.array_equal(ns.s1_stack["obs"][:len(want)].cpu().numpy(), np.stack([w[3] for w in want]))
    assert np.array_equal(ns.done_stack[:len(want), 0].cpu().numpy(), np.array([w[4] for w in want], np.uint8))


@pytest.mark.parametrize("which", ["dmc", "atari"])
def test_full_size_pixel_critic_update_implicit_vs_im2col(which, monkeypatch):
    """BASELINE configs 3 and 4 END TO END at their full batch (B 512 / B 1024; the update closure bench.py times):
    three critic updates (DrQv2 shift, both encoder passes, encoder backward, clip, Adam, Polyak) with every
    convolution as an implicit GEMM (conv1's and the small maps' weight gradients LDS-staged, the fc forward streamed) against
    the same three updates through im2col + GEMM and the tiled fc kernel -- the path the
    reference-generated fixtures drqv2_pixels / atari_pixels pin at B 8.  Same arithmetic in a different summation
    order: TD targets 2e-4 * max(1,|x|), logs 5e-4; parameters: median 1e-6 and worst element 2 * lr per update (Adam
    moves a weight by ~lr whatever the gradient's size, so a near-zero gradient whose sign differs displaces it that far)."""
    import os
    import random
    import sys
    import torch
    import super_sac_amd as ssa
    from super_sac_amd import conv_encoder
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import bench_pixels
    n_upd, lr = 3, 1e-4

    def run(implicit):
        monkeypatch.setattr(conv_encoder, "USE_IMPLICIT", implicit)
        monkeypatch.setattr(conv_encoder, "USE_IMPLICIT_FIRST", implicit)
        monkeypatch.setattr(conv_encoder, "FC_STREAM", implicit)   # (the fc forward: operand stream / tiled split-K kernel)
        torch.manual_seed(0); np.random.seed(0); random.seed(0)
        step, B = bench_pixels.build(which, torch.device("cuda"))
        tds, logs = [], []
        for _ in range(n_upd):
            step()
            lg, dicts = step.out
            tds.append(dicts[0]["td_target"].cpu().numpy().copy())
            logs.append({k: float(v) for k, v in lg.items()})
        ag, tg = step.objects["agent"], step.objects["target"]
        flat = lambda mods: np.concatenate([p.detach().cpu().numpy().ravel() for m in mods for p in m.parameters()])
        out = dict(td=tds, logs=logs, enc=flat([ag.encoder]), tenc=flat([tg.encoder]), crit=flat(ag.critics),
                   tcrit=flat(tg.critics))
        del step
        torch.cuda.empty_cache()
        return out
    a, b = run(True), run(False)
    for u in range(n_upd):
        dv = float(np.max(np.abs(a["td"][u] - b["td"][u]) / np.maximum(1.0, np.abs(b["td"][u]))))
        assert dv <= 2e-4, f"update {u}: TD targets differ by {dv}"
        for k, v in b["logs"][u].items():
            # (from the second update on the two runs' parameters differ at the lr scale, see above: gradient norms then
            # agree to a few 1e-3 of their size)
            tol = 5e-4 if u == 0 else 5e-3
            assert abs(a["logs"][u][k] - v) <= tol * max(1.0, abs(v)), (u, k, a["logs"][u][k], v)
    for key in ("enc", "tenc", "crit", "tcrit"):
        err = np.abs(a[key] - b[key])
        assert float(np.median(err)) <= 1e-6 and float(err.max()) <= 2 * lr * n_upd, (key, float(np.median(err)), float(err.max()))


def _actor_update_run(chained, hook=True, n_upd=8, shape=(256, 17, 6, 4, 64)):
    import copy, math, random
    import ctypes as C
    from itertools import chain
    import torch
    import super_sac_amd as ssa
    from case_runner import straggler_check
    L, lu = ssa.learning, ssa.learning_utils
    dev = torch.device("cuda")
    B, S, A, N, H = shape

    if True:
        old = (L.ACTOR_CHAIN, ssa.rng.draw_normal, ssa.rng.draw_normal_into)
        L.ACTOR_CHAIN = chained
        gen = torch.Generator(device=dev); gen.manual_seed(11)
        if hook:
            ssa.rng.draw_normal = lambda shape, device: torch.randn(*shape, device=device, generator=gen)
            ssa.rng.draw_normal_into = lambda dst: dst.normal_(generator=gen)
        try:
            torch.manual_seed(3); np.random.seed(3); random.seed(3)
            agent = ssa.Agent(act_space_size=A, encoder=ssa.nets.IdentityEncoder(S),
                              actor_network_cls=ssa.nets.ContinuousStochasticActor,
                              critic_network_cls=ssa.nets.ContinuousCritic, ensemble_size=1, num_critics=N,
                              hidden_size=H, auto_rescale_targets=False, log_std_low=-5.0, log_std_high=2.0)
            agent.to(dev)
            if chained:
                a_arena = ssa.engine.bind_arena(agent.actors[0], "self", [agent.actors[0]], dev)
                assert L._actor_chain_form(a_arena, A, B, agent.critics[0].arena(dev)), "this shape is meant to take the chained launch"
            target = copy.deepcopy(agent)
            buf = ssa.replay.ReplayBuffer(4096, device=dev)
            buf.load_experience(*synth.synth_transitions(2000, S, A, seed=5))
            copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=3e-4)
            aopt = torch.optim.Adam(chain(*(a.parameters() for a in agent.actors)), lr=3e-4)
            eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
            la = torch.Tensor([math.log(0.1)]).to(dev); la.requires_grad = True
            aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(B)])
            for _ in range(4):   # (the critic update records after three calls: fixed batch buffers for the actor update)
                _, dicts = L.critic_update(
                    buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt,
                    log_alphas=[la], batch_size=B, gamma=0.99, critic_clip=None, encoder_clip=None,
                    target_critic_ensemble_n=2, weighted_bellman_temp=None, weight_type=None, pop=False, augmenter=aug,
                    encoder_lambda=0, aug_mix=0.0, discrete=False, random_process=None, noise_clip=None, per=False,
                    update_priorities=False, dr3_coeff=0.0)
            logs, first, ws = [], None, None
            for k in range(n_upd):
                lg = L.online_actor_update(buffer=buf, agent=agent, pop=False, actor_optimizer=aopt, log_alphas=[la],
                                           batch_size=B, clip=None, random_process=None, noise_clip=None, augmenter=aug,
                                           aug_mix=0.0, premade_replay_dicts=dicts)
                logs.append((float(lg["losses/actor_pg_loss"]), float(lg["gradients/random_actor_online_grad"])))
                if k == 0:
                    ws = agent.__dict__["_ssac_ws"]   # (the update's own workspace)
                    first = {n_: ws.get(n_, sh).detach().cpu().numpy().copy() for n_, sh in
                             (("au.c0.y", (N, B, 1)), ("au.dxu0", (N, B, A)), ("au.dout0", (1, B, 2 * A)),
                              ("au.a0.dz1", (1, B, H)), ("au.x0", (B, S + A)), ("au.a0.y", (1, B, 2 * A)))}
            params = torch.cat([p.detach().flatten() for p in agent.actors[0].parameters()]).cpu().numpy()
            return first, logs, params, agent, ws
        finally:
            L.ACTOR_CHAIN, ssa.rng.draw_normal, ssa.rng.draw_normal_into = old


def test_recorded_actor_update_off_the_chained_form_owns_and_refills_its_noise():
    """Round-4 advisor (high): an actor whose online update takes the THREE-launch form reads its noise from a buffer (until
    round 6 that was Humanoid's 376 -> 256 -> 34 actor, whose double-buffered LDS carve does not fit; it takes the chained
    launch single-buffered now, so the form is forced here: learning.ACTOR_CHAIN = False).  The recording decided
    "in-kernel noise" from the generator alone and recorded the address of a temporary: every replay then re-read freed
    memory (frozen or arbitrary noise), silently.  Now the predicate is per member (learning._actor_chain_form): the
    recording owns fixed buffers, refills them before every replay, and an allocation inside a recording asserts.
    Checked here with the stock generator: not the in-kernel form, the sampled action of every update is
    tanh(mu + sd * eps) of the recording's buffer AS REFILLED for that update, and it changes from update to update."""
    import copy, math, random
    from itertools import chain
    import torch
    import super_sac_amd as ssa
    L = ssa.learning
    dev = torch.device("cuda")
    B, S, A, N, H = 64, 376, 17, 2, 256
    torch.manual_seed(13); np.random.seed(13); random.seed(13)
    agent = ssa.Agent(act_space_size=A, encoder=ssa.nets.IdentityEncoder(S),
                      actor_network_cls=ssa.nets.ContinuousStochasticActor, critic_network_cls=ssa.nets.ContinuousCritic,
                      ensemble_size=1, num_critics=N, hidden_size=H, auto_rescale_targets=False, log_std_low=-5.0,
                      log_std_high=2.0)
    agent.to(dev)
    target = copy.deepcopy(agent)
    buf = ssa.replay.ReplayBuffer(4096, device=dev)
    buf.load_experience(*synth.synth_transitions(1500, S, A, seed=9))
    copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=3e-4)
    aopt = torch.optim.Adam(chain(*(a.parameters() for a in agent.actors)), lr=3e-4)
    eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
    la = torch.Tensor([math.log(0.1)]).to(dev); la.requires_grad = True
    aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(B)])
    a_arena = ssa.engine.bind_arena(agent.actors[0], "self", [agent.actors[0]], dev)
    old_chain, L.ACTOR_CHAIN = L.ACTOR_CHAIN, False
    try:
        assert a_arena.fused and not L._actor_chain_form(a_arena, A, B, agent.critics[0].arena(dev)), "the three-launch form is forced here"
        _off_chain_body(L, ssa, agent, target, buf, copt, aopt, eopt, la, aug, B, S, A)
    finally:
        L.ACTOR_CHAIN = old_chain


def _off_chain_body(L, ssa, agent, target, buf, copt, aopt, eopt, la, aug, B, S, A):
    import torch
    for _ in range(4):
        _, dicts = L.critic_update(
            buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt, log_alphas=[la],
            batch_size=B, gamma=0.99, critic_clip=None, encoder_clip=None, target_critic_ensemble_n=2,
            weighted_bellman_temp=None, weight_type=None, pop=False, augmenter=aug, encoder_lambda=0, aug_mix=0.0,
            discrete=False, random_process=None, noise_clip=None, per=False, update_priorities=False, dr3_coeff=0.0)
    acts, rec = [], None
    for k in range(7):   # two eager calls, the recording, four replays
        L.online_actor_update(buffer=buf, agent=agent, pop=False, actor_optimizer=aopt, log_alphas=[la], batch_size=B,
                              clip=None, random_process=None, noise_clip=None, augmenter=aug, aug_mix=0.0,
                              premade_replay_dicts=dicts)
        ws = agent.__dict__["_ssac_ws"]
        x = ws.get("au.x0", (B, S + A))[:, S:].clone()
        if k >= 2:
            rec = next(iter(agent.__dict__["_ssac_actor_rec"].values()))
            assert not rec.in_kernel and rec.eps is not None and rec.list is not None
            y = ws.get("au.a0.y", (1, B, 2 * A))[0]
            mu, raw = y[:, :A], y[:, A:]
            sd = torch.exp(-5.0 + 0.5 * (2.0 - -5.0) * (torch.tanh(raw) + 1.0))
            want = torch.tanh(mu + sd * rec.eps[0])
            assert torch.allclose(x, want, atol=2e-6), (k, float((x - want).abs().max()))
        acts.append(x)
    for k in range(1, 7):
        assert not torch.equal(acts[k], acts[k - 1]), f"update {k} re-used update {k - 1}'s noise"
    assert all(bool(torch.isfinite(a_).all()) for a_ in acts)


def test_actor_update_chained_launch_matches_three_launches():
    """ssac_actor_chain_fused (actor forward -> critics' forward + dQ/da -> actor backward as producer / consumer workgroups
    of ONE launch, learning.ACTOR_CHAIN) against the three launches it replaces, on the same injected noise: the first
    update's intermediate results (Q, dQ/da, dL/d(actor output), dz1) and the logs of eight updates -- two eager, one
    recorded, five replayed -- within fp32 association (the critics' fc1 sums state and action columns separately);
    parameters with counted sign-flip stragglers.  Then the in-kernel noise of a replayed chained update (stock generator; renumbered
    through ssac_replay_value): the action the forward half stored must be tanh(mu + sd * eps) of the Philox stream at the
    update's number."""
    import ctypes as C
    import torch
    import super_sac_amd as ssa
    from case_runner import straggler_check
    lu = ssa.learning_utils
    dev = torch.device("cuda")
    B, S, A, N = 256, 17, 6, 4
    run = _actor_update_run
    # Round 6: Humanoid's actor (376 -> 256 -> 34: a 384-column x tile beside 35 KB of W3 leaves room for ONE weight-staging
    # buffer) takes the chained launch too, its two passes single-buffered (fused_actor_chain_kernel<.., ADBUF = false>),
    # the critics (393 -> 256 -> 1) as 16-row tiles: against the three launches, same injected noise
    hum = (128, 376, 17, 3, 256)
    f3h, l3h, p3h, _, _ = run(False, shape=hum)
    fch, lch, pch, _, _ = run(True, shape=hum)
    for n_ in f3h:
        scale = max(1.0, float(np.abs(f3h[n_]).max()))
        np.testing.assert_allclose(fch[n_], f3h[n_], rtol=0, atol=3e-5 * scale, err_msg="humanoid shape: " + n_)
    np.testing.assert_allclose(np.array(lch), np.array(l3h), rtol=2e-4, atol=1e-6)
    straggler_check(np.abs(pch - p3h), 3e-5, 8 * 2 * 3e-4 * 1.01, "chained actor update (Humanoid shape)", "actor parameters")
    f3, l3, p3, _, _ = run(False)
    fc, lc, pc, _, _ = run(True)
    for n_ in f3:
        scale = max(1.0, float(np.abs(f3[n_]).max()))
        np.testing.assert_allclose(fc[n_], f3[n_], rtol=0, atol=3e-5 * scale, err_msg=n_)
    np.testing.assert_allclose(np.array(lc), np.array(l3), rtol=2e-4, atol=1e-6)
    straggler_check(np.abs(pc - p3), 3e-5, 8 * 2 * 3e-4 * 1.01, "chained actor update", "actor parameters")
    # in-kernel noise: stock generator, recorded chained update; the stored action against the documented Philox stream
    _, _, _, agent, ws = run(True, hook=False, n_upd=5)
    rec = next(iter(agent.__dict__["_ssac_actor_rec"].values()))
    ns = lu.noise_stream(agent, dev)
    assert rec.in_kernel and rec.list is not None and ns[2] == 5   # (five numbered updates: 2 eager, 1 recorded, 2 replayed)
    # a list with numbered launches must be renumbered at every replay: the plain replay entry refuses it (a repeated tag
    # would let a consumer match the previous update's granules)
    assert ssa._lib.lib.ssac_replay(rec.list, ssa.engine.stream()) != 0
    assert b"ssac_replay_value" in ssa._lib.lib.ssac_last_error()
    eps = torch.empty(B, A, device=dev)
    rs = ssa._lib.Rng((ns[0] ^ 0x5DEECE66D1CEB00C) & (2 ** 64 - 1), 0, 4)   # the LAST update was number 4
    ssa._lib.check(ssa._lib.lib.ssac_philox_normal(eps.data_ptr(), B, A, C.byref(rs), ssa.engine.stream()))
    y = ws.get("au.a0.y", (1, B, 2 * A))[0]
    mu, raw = y[:, :A], y[:, A:]
    sd = torch.exp(-5.0 + 0.5 * (2.0 - -5.0) * (torch.tanh(raw) + 1.0))
    want = torch.tanh(mu + sd * eps)
    got = ws.get("au.x0", (B, S + A))[:, S:]
    assert torch.allclose(got, want, atol=2e-6), float((got - want).abs().max())


# launches in the recorded list of ONE online actor update (stock generator; obs 17, act 6, hidden 64, 4 critics, B 128),
# counted at commit 65950e7, the parent of the host refactor that introduced learning._actor_member_plan.  A host refactor
# issues the same launches: the margin is zero.
_ACTOR_LIST_SIZE = {"chained": 2, "three_launches": 5, "two_members": 7}


@pytest.mark.parametrize("setting", sorted(_ACTOR_LIST_SIZE))
def test_recorded_actor_update_is_what_the_member_plan_says(setting):
    """the recording of an online actor update follows learning._actor_member_plan: its noise is in-kernel exactly when the
    plan of EVERY member says so, it owns noise buffers exactly when it is not, and its launch list is as long as the one
    the same setting recorded before the plan existed"""
    import copy, math, random
    from itertools import chain
    import torch
    import super_sac_amd as ssa
    L = ssa.learning
    dev = torch.device("cuda")
    B, S, A, N, H, E = 128, 17, 6, 4, 64, 2 if setting == "two_members" else 1
    old_chain, L.ACTOR_CHAIN = L.ACTOR_CHAIN, setting != "three_launches"
    try:
        torch.manual_seed(3); np.random.seed(3); random.seed(3)
        agent = ssa.Agent(act_space_size=A, encoder=ssa.nets.IdentityEncoder(S),
                          actor_network_cls=ssa.nets.ContinuousStochasticActor, critic_network_cls=ssa.nets.ContinuousCritic,
                          ensemble_size=E, num_critics=N, hidden_size=H, auto_rescale_targets=False, log_std_low=-5.0,
                          log_std_high=2.0)
        agent.to(dev)
        target = copy.deepcopy(agent)
        buf = ssa.replay.ReplayBuffer(4096, device=dev)
        buf.load_experience(*synth.synth_transitions(2000, S, A, seed=5))
        copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=3e-4)
        aopt = torch.optim.Adam(chain(*(a.parameters() for a in agent.actors)), lr=3e-4)
        eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
        las = []
        for _ in range(E):
            la = torch.Tensor([math.log(0.1)]).to(dev); la.requires_grad = True
            las.append(la)
        aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(B)])
        for _ in range(4):   # (the critic update records after three calls: fixed batch buffers for the actor update)
            _, dicts = L.critic_update(
                buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt, log_alphas=las,
                batch_size=B, gamma=0.99, critic_clip=None, encoder_clip=None, target_critic_ensemble_n=2,
                weighted_bellman_temp=None, weight_type=None, pop=False, augmenter=aug, encoder_lambda=0, aug_mix=0.0,
                discrete=False, random_process=None, noise_clip=None, per=False, update_priorities=False, dr3_coeff=0.0)
        for _ in range(4):   # two eager calls, the recording, one replay
            L.online_actor_update(buffer=buf, agent=agent, pop=False, actor_optimizer=aopt, log_alphas=las, batch_size=B,
                                  clip=None, random_process=None, noise_clip=None, augmenter=aug, aug_mix=0.0,
                                  premade_replay_dicts=dicts)
        rec = next(iter(agent.__dict__["_ssac_actor_rec"].values()))
        plans = [L._actor_member_plan("stochastic", None, False, None, ssa.engine.bind_arena(a_, "self", [a_], dev),
                                      c_.arena(dev), A, B, False, False) for a_, c_ in zip(agent.actors, agent.critics)]
        assert all(form == ("fused" if setting == "three_launches" else "chain") for form, _ in plans), plans
        assert rec.list is not None and rec.in_kernel == all(noise == "kernel" for _, noise in plans)
        assert rec.in_kernel == (setting != "three_launches")
        assert (rec.eps is None) == rec.in_kernel
        n = int(ssa._lib.lib.ssac_launch_list_size(rec.list))
        print(setting, "launch list size", n)
        assert n == _ACTOR_LIST_SIZE[setting], (setting, n)
    finally:
        L.ACTOR_CHAIN = old_chain
