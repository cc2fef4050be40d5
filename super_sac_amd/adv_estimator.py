"""Advantage estimator of the AFBC / AWAC actor update (adv_estimator.py:8-90), on the engine's kernels.

A(s, a) = Q(s, a) - V(s) with Q = min over ALL critics of the member (then ``popart(q)`` when the member
has a PopArt layer, adv_estimator.py:31-36) and, for continuous actions, V(s) = mean (``"mean"``) or max
(``"max"``) of Q over n = 4 actions sampled from the member's policy (adv_estimator.py:58-79).  The data
action and the 4 sampled actions are evaluated by ONE ensemble-Q launch on a stacked (5B x (S+A)) batch.
"""
import ctypes as C

import torch

from . import engine, rng
from . import learning_utils as lu
from . import _lib
from ._lib import check, lib

N_SAMPLES = 4  # adv_estimator.py:58 (n=4)


class AdvantageEstimator:
    def __init__(self, agent, discrete_method="indirect", continuous_method="mean", discrete=False):
        assert continuous_method in ["mean", "max"]
        assert discrete_method in ["indirect", "direct"]
        self.agent = agent
        self.cont_method = continuous_method
        self.discrete = discrete
        self.discrete_method = discrete_method

    def __call__(self, obs, action, ensemble_idx):
        return self.forward(obs, action, ensemble_idx)

    def forward(self, obs, action, ensemble_idx):
        out = self.evaluate(obs, action, ensemble_idx)
        return out["adv"].view(-1, 1)

    def evaluate(self, obs, action, ensemble_idx, want=("adv",), log_ptr=0, *, _update=None):
        """dict with the requested (B,) device tensors among adv / mask / prio (one launch chain).
        ``_update`` (internal: learning_utils.adjust_priorities as part of a critic update) = (rng, eps): the stacked
        batch comes from ONE launch, ssac_adv_candidates, and no torch kernel runs between the actor forward and the
        filter, so the chain can sit in a launch list.  rng: the (seed, counter address, offset) of the update's
        TD-target noise -- the candidates are drawn inside the launch at that draw number under their own key -- or None;
        eps: a (N_SAMPLES * B, A) device buffer of injected normals, sample-major, used instead when given.  Every other
        caller (offline_actor_update, compute_filter_stats, use_baseline, agent.adv_estimator(o, a, i)) leaves it None
        and keeps the per-sample launches and host draws."""
        engine.require_gpu()
        agent, i = self.agent, ensemble_idx
        actor, critic, popart = agent.actors[i], agent.critics[i], agent.popart[i]
        s_rep = lu.encode(agent.encoder, obs)
        B, S = s_rep.shape
        dev = s_rep.device
        ws = lu.agent_ws(agent, dev)
        st = engine.stream()
        if self.discrete:
            if self.discrete_method != "indirect":
                raise NotImplementedError("dueling-architecture advantage (adv_estimator.py:37-39)")
            nA = agent.act_space_size
            E = len(agent.actors)
            if _update is not None and E == 1:
                # the single actor's output IS the (1, B, nA) logits block: no copy
                arena = engine.bind_arena(actor, "self", [actor], dev)
                _, _, logits = engine.mlp_forward(arena, s_rep, lu._row_stride(s_rep), 0, B, ws, "adv.a0", save=False)
                assert logits.is_contiguous() and logits.numel() == B * nA
            else:
                logits = ws.get("adv.logits", (E, B, nA))
                for m, ac in enumerate(agent.actors):  # V(s) uses the mean probabilities of ALL ensemble actors
                    arena = engine.bind_arena(ac, "self", [ac], dev)
                    _, _, out = engine.mlp_forward(arena, s_rep, lu._row_stride(s_rep), 0, B, ws, f"adv.a{m}", save=False)
                    logits[m].copy_(out[0])
            c_arena = critic.arena(dev)
            _, _, q = engine.mlp_forward(c_arena, s_rep, lu._row_stride(s_rep), 0, B, ws, f"adv.c{i}", save=False)
            res = {k_: ws.get(f"adv.{k_}{i}", (B,)) for k_ in want}
            check(lib.ssac_adv_filter_discrete(q.data_ptr(), c_arena.n_nets, B, nA, logits.data_ptr(), E,
                                               action.data_ptr(), action.stride(0), popart.ptr if popart else 0,
                                               res["adv"].data_ptr() if "adv" in res else 0,
                                               res["mask"].data_ptr() if "mask" in res else 0,
                                               res["prio"].data_ptr() if "prio" in res else 0, log_ptr, st))
            return res
        A = actor.action_size
        n = N_SAMPLES
        if lu.actor_kind(actor) == "beta":
            raise NotImplementedError("AdvantageEstimator (advantage filter, PER refresh, use_baseline): Beta policies "
                                      "(beta_dist=True) are not supported here")
        # stacked batch: block 0 = (s, a_data), blocks 1..n = (s, a_k)
        X = ws.get(f"adv.x{i}", ((n + 1) * B, S + A))
        Xv = X.view(n + 1, B, S + A)
        a_arena = engine.bind_arena(actor, "self", [actor], dev)
        deterministic = lu.actor_kind(actor) == "deterministic"
        if _update is not None:
            _, _, aout = engine.mlp_forward(a_arena, s_rep, lu._row_stride(s_rep), 0, B, ws, f"adv.a{i}", save=False)
            rng_t, eps_buf = _update
            rs = None
            if not deterministic and eps_buf is None:
                assert rng_t is not None, "candidates without a noise buffer need the update's Philox draw number"
                rs = _lib.Rng(*rng_t)
            assert action.dim() == 2 and action.stride(1) == 1 and action.shape[1] == A
            check(lib.ssac_adv_candidates(
                s_rep.data_ptr(), lu._row_stride(s_rep), action.data_ptr(), action.stride(0), aout.data_ptr(),
                A if deterministic else 2 * A, 0 if deterministic else 1,
                0.0 if deterministic else float(actor.log_std_low), 0.0 if deterministic else float(actor.log_std_high),
                eps_buf.data_ptr() if (eps_buf is not None and not deterministic) else 0,
                C.addressof(rs) if rs is not None else 0, B, S, A, n, X.data_ptr(), st))
            n_fill = 0
        else:
            Xv[:, :, :S].copy_(s_rep.unsqueeze(0).expand(n + 1, B, S))   # device plumbing
            Xv[0, :, S:].copy_(action)
            _, _, aout = engine.mlp_forward(a_arena, s_rep, lu._row_stride(s_rep), 0, B, ws, f"adv.a{i}", save=False)
            n_fill = n
        for k in range(n_fill):
            blk = Xv[k + 1]
            if deterministic:
                # ContinuousDeterministic.sample() is its loc (distributions.py:113-114): no draw, n equal actions
                check(lib.ssac_det_action_fwd(aout.data_ptr(), A, 0, 0.0, 0, 0.0, 0.0, B, A, blk.data_ptr(), S + A, S, st))
                continue
            eps = rng.draw_normal((B, A), dev)  # dist.sample(): one normal draw per sampled action
            check(lib.ssac_tanh_normal_fwd(aout.data_ptr(), 2 * A, eps.data_ptr(), B, A,
                                           float(actor.log_std_low), float(actor.log_std_high),
                                           blk.data_ptr(), S + A, S, 0, st))
        c_arena = critic.arena(dev)
        _, _, q = engine.mlp_forward(c_arena, X, S + A, 0, (n + 1) * B, ws, f"adv.c{i}", save=False)
        res = {k_: ws.get(f"adv.{k_}{i}", (B,)) for k_ in want}
        check(lib.ssac_adv_filter(q.data_ptr(), c_arena.n_nets, B, n, popart.ptr if popart else 0,
                                  1 if self.cont_method == "max" else 0,
                                  res["adv"].data_ptr() if "adv" in res else 0,
                                  res["mask"].data_ptr() if "mask" in res else 0,
                                  res["prio"].data_ptr() if "prio" in res else 0, log_ptr, st))
        return res
