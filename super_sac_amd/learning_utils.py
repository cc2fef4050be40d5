"""Update helpers with the reference's names and signatures (super_sac/learning_utils.py):
``sample_move_and_augment`` (:174), ``compute_td_targets`` (:298), ``compute_backup_weights``
(:357), ``soft_update`` / ``hard_update`` (:160-167), ``GaussianExplorationNoise`` (:18-66).

Every arithmetic step is a kernel of libssac_hip.so; this file only sequences launches and
keeps the reference's host-RNG order (index draw -> augmentation draw -> action noise ->
REDQ subset).
"""
import collections
import ctypes as C
import os
import math
import types

import numpy as np
import torch

from . import augmentations, beta, encoder_base, engine, nets, rng
from . import _lib
from ._lib import check, lib

LOG_WIDTH = 64
MAX_MEMBERS = 8
# slot layout of one update's log block (floats)
L_CRITIC_LOSS, L_TD_ERR, L_CRITIC_GN, L_ENC_GN = 0, 1, 2, 3
L_TD0 = 4            # + 3*i : mean, std, entropy bonus of member i
L_BW = 28            # bellman weights mean, max, min, std
L_ACTOR_LOSS, L_ACTOR_GN = 32, 33
L_ALPHA0 = 34        # + 2*i : alpha_loss_i, alpha_i
L_ADVW, L_BC_TOTAL, L_BC_GN = 50, 51, 52   # AFBC: adv_weights_mean, overall loss, actor grad norm
L_BC0 = 53           # + i : filtered BC loss of member i
L_ENC_INV = 60       # encoder invariance constraint (learning_utils.py:401-409)
L_ACT_INV = 61       # action invariance constraint (learning_utils.py:272-285; not a log key of the reference)
# Markov state-abstraction update (its own log block): losses inverse / contrastive / smoothness / total, then the
# gradient norms of the contrastive model, the inverse model and the encoder; two scratch words for the head kernels
L_MK_LOSS, L_MK_GN_CON, L_MK_GN_INV, L_MK_GN_ENC, L_MK_RAW, L_MK_CON, L_MK_SMOOTH, L_MK_TMP = 40, 44, 45, 46, 47, 48, 49, 56


class LogRing:
    """Ring of device log blocks.  Update functions hand out 0-dim views of a block as log
    values, so nothing synchronises until the caller reads them (the reference blocks on
    ``.item()`` several times per update: learning.py:132, learning_utils.py:351-353)."""

    def __init__(self, device, slots=512):
        self.buf = torch.zeros(slots, LOG_WIDTH, dtype=torch.float32, device=device)
        self.k = 0

    def advance(self):
        self.k = (self.k + 1) % self.buf.shape[0]
        return self.k

    def next(self, adam=None):
        """fresh zeroed block; the same launch advances `adam`'s step when given."""
        self.k = (self.k + 1) % self.buf.shape[0]
        blk = self.buf[self.k]
        check(lib.ssac_begin_update(blk.data_ptr(), LOG_WIDTH, 0 if adam is None else adam.ctl.ptr, 0,
                                    engine.stream()))
        return blk


_rings = {}

# Deferred log finalisation of recorded updates (csrc/ssac_critic_logs.h): the newest recorded update's log block is
# written to its ring slot by the NEXT update's first launch -- or, when somebody looks at one of its values first, by a
# flush launch.  `pending` = (log-ring slot, ssac_deferred_logs struct) of that newest update, per device ring.
DEFERRED_LOGS = True


def flush_pending_logs(owner):
    """write the newest recorded update's log block to its ring slot now (owner: the recording's state object, which
    carries `pending` = that update's log-ring slot, and `deferred` = its ssac_deferred_logs struct)"""
    slot_i = owner.pending
    if slot_i is not None:
        owner.pending = None
        check(lib.ssac_deferred_logs_flush(C.byref(owner.deferred), slot_i, engine.stream()))


class LazyLog(torch.Tensor):
    """a log value of a recorded update: a 0-dim view of its slot of the log ring that makes sure the slot has been
    written before anything reads it (any torch operation on it, float(), .item(), ...)"""

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        for a in args:
            if isinstance(a, LazyLog):
                owner = a.__dict__.get("_ssac_owner")
                if owner is not None and owner.pending == a.__dict__.get("_ssac_slot"):
                    flush_pending_logs(owner)
        return super().__torch_function__(func, types, args, kwargs or {})


def lazy_views(owner, ring, slot_i, index):
    """{log key: LazyLog view} of ring slot slot_i"""
    out = {}
    blk = ring.buf[slot_i]
    for k_, i in index.items():
        v = blk[i].as_subclass(LazyLog)
        v.__dict__["_ssac_owner"], v.__dict__["_ssac_slot"] = owner, slot_i
        out[k_] = v
    return out


def draw_normal(shape, device):
    """action-noise draw site (honours an active graph capture)."""
    if engine.CAPTURE is not None:
        return engine.CAPTURE.normals.pop(0)
    return rng.draw_normal(shape, device)


IN_KERNEL_NOISE = True


def noise_stream(agent, device):
    """[seed, critic-update draws so far, online-actor-update number] of the agent's engine noise stream (Philox4x32-10, include/ssac_hip.h: ssac_rng).  The seed
    is drawn once from torch's device generator, so `torch.manual_seed` still determines the run."""
    ns = agent.__dict__.get("_ssac_noise")
    if ns is None:
        seed = int(torch.randint(0, 2 ** 62, (1,), device=device, dtype=torch.int64))
        ns = agent.__dict__["_ssac_noise"] = [seed, 0, 0]
    if len(ns) < 3:   # (a checkpoint written before the actor updates numbered themselves)
        ns.append(0)
    return ns


def stream_rng(agent, device):
    """the ssac_rng of one update's in-kernel noise, ONE tick of the agent's stream: draw number = the host count, which
    moves on (eager), or capture-time count + device-resident update counter (recorded: learning._host_inputs counts)"""
    ns, cap = noise_stream(agent, device), engine.CAPTURE
    if cap is not None:
        return _lib.Rng(ns[0], cap.tick_ptr, cap.noise_offset)
    ns[1] += 1
    return _lib.Rng(ns[0], 0, ns[1] - 1)


def skip_stream_tick(agent, device):   # (a member another rank owns: the tick its owner's stream_rng takes)
    if engine.CAPTURE is None:
        noise_stream(agent, device)[1] += 1


TdPlan = collections.namedtuple("TdPlan", "head launch noise draws use_entropy")


def td_member_plan(kind, has_process, explore, actor_fused, capture, want_fwd=False, want_bwd=False, target_dbuf=False,
                   target_scalar=False, target_sharded=False, in_kernel=None):
    """Which head produces a' of one member's TD target, in which launch, with noise from where, consuming which host
    draws -- decided HERE for compute_td_targets, skip_td_draws, learning._in_kernel_noise and recording_noise_buffers.
    Pure, of plain values (tests/test_td_plan_cpu.py walks the cross product); CHAIN_LAUNCH, IN_KERNEL_NOISE and the
    generator are read at call time (in_kernel: asked as if they said so).  explore: the verdict's flag; capture: a
    recording is open; want_fwd / want_bwd: the member's requests; target_*: the target critics' arena is fused_dbuf, has
    out_dim 1, belongs to a critic-sharded agent.
    head: "discrete" | "beta" | "explore" (head + process: ssac_explore_action) | "tanh_normal" | "deterministic".
    launch of the head's forward + sample: "chain" (pending, issued with the REDQ subset as ssac_[bf16_]chain_update) |
    "dual" (ssac_actor_sample_critic_fwd) | "fused" (ssac_actor_sample_fused) | "layers" (engine.mlp_forward, then a head
    kernel).  noise: "kernel" (one tick of the agent's Philox stream, stream_rng) | "buffer" (draw_normal).  draws: what
    the member consumes before its REDQ subset, in the reference's order, over "tick", "eps" (the head's), "proc" (the
    process's); Beta's own draws stay inside beta.sample.  use_entropy: the 0/1 of ssac_td_target / ssac_td_spec."""
    if in_kernel is None:
        in_kernel = bool(IN_KERNEL_NOISE and rng.normal_is_stock())
    proc = ("proc",) if has_process else ()
    fuse_sample = kind == "stochastic" and actor_fused and not has_process
    if kind in ("discrete", "beta"):
        head, draws = kind, proc if kind == "beta" else ()
    elif explore and has_process and (capture or in_kernel):
        # every recorded update with a process, and -- one noise stream per run -- the eager calls of the same agents under
        # the stock generator; under a noise hook the eager calls keep the two-kernel sequences (the parity tests' twin)
        head, draws = "explore", ("tick",) if in_kernel else (("eps",) if kind == "stochastic" else ()) + proc
    elif kind == "stochastic":
        head, draws = "tanh_normal", (("tick",) if fuse_sample and in_kernel else ("eps",)) + proc
    else:
        head, draws = "deterministic", proc
    # actor -> target critics chained inside one launch with the critics' forward + TD-independent backward
    chain = bool(CHAIN_LAUNCH and fuse_sample and want_fwd and want_bwd and (not target_sharded or capture)
                 and target_dbuf and target_scalar)
    launch = "chain" if chain else "dual" if fuse_sample and want_fwd else "fused" if fuse_sample else "layers"
    return TdPlan(head, launch, "kernel" if "tick" in draws else "buffer", draws,
                  int(head not in ("discrete", "explore") and not has_process))


def explore_recordable(kind, has_process, discrete, identity_encoder, ensemble_size, per, sharded, launch_mode):
    """May a critic update called with this exploration process be recorded -- as far as the PROCESS is concerned (the
    other clauses of learning.critic_update's gate hold with or without one)?  Pure: tests/test_explore_recording_cpu.py
    walks it over a grid.  No process, or a discrete agent (whose update never looks at it, learning_utils.py:322-328):
    nothing to decide.  Otherwise the head + process run as ONE recorded launch (ssac_explore_action) that exists for the
    library's launch lists, tanh-normal and deterministic heads, an identity encoder, one ensemble member, uniform
    sampling and an unsharded agent; everything else keeps the eager path.  `sharded`: a critic or member shard.
    The same answer decides whether an EAGER update of such an agent draws its noise from the agent's Philox stream
    (stock generator): the warm-up calls and the recorded ones then follow one stream."""
    if not has_process or discrete or kind == "discrete":
        return True
    return (launch_mode == "list" and kind in ("stochastic", "deterministic") and identity_encoder
            and ensemble_size == 1 and not per and not sharded)


def priority_recordable(kind, per_on_device, identity_encoder, ensemble_size, per, dr3, sharded, bf16, launch_mode):
    """May a critic update called with update_priorities=True be recorded -- as far as the PRIORITY REFRESH is concerned
    (learning.critic_update's other clauses hold with or without one)?  Pure: tests/test_priority_recording_cpu.py walks
    it over the grid of its inputs.  The refresh is recorded as ssac_adv_candidates -> ensemble-Q forward ->
    ssac_adv_filter -> ssac_per_assign on the device trees, which exists for the library's launch lists, a buffer with
    its trees in HBM, an identity encoder, one ensemble member, uniform sampling, no DR3, an unsharded fp32 agent and a
    tanh-normal, deterministic or discrete head (not Beta).  A process, PopArt or gradient clipping make no difference.
    The same answer decides whether an EAGER update of such a call draws the candidates from the agent's Philox stream
    (adjust_priorities): the warm-up calls and the recorded ones then follow one stream."""
    return bool(launch_mode == "list" and kind in ("stochastic", "deterministic", "discrete") and per_on_device
                and identity_encoder and ensemble_size == 1 and not per and not dr3 and not sharded and not bf16)


# the backup weights of a recordable ensemble update (members_recordable) from ONE packed forward of every member's target
# critics over the members' stacked batches + ONE ssac_members_sunrise_weights launch, instead of E forwards + E
# ssac_ensemble_min_select + 1 ssac_sunrise_weights per member batch.  A module switch: tests/test_hip_members_recorded.py
# (test_packed_weights_off_gives_the_same_bits) holds the two forms against each other.
PACKED_WEIGHTS = True


def members_recordable(launch_mode, ensemble_size, identity_encoder, kind, per, update_priorities, dr3, process_call, bf16,
                       sharded, weight_type, weight_temp):
    """May a critic update of an agent with ensemble_size > 1 be recorded (SUNRISE)?  Pure: tests/
    test_members_recording_cpu.py walks every clause.  It holds for the library's launch lists, 2 .. MAX_MEMBERS members, an
    identity encoder, a tanh-normal, deterministic or discrete head (not Beta), uniform sampling without a priority refresh
    or DR3, a call that is not a continuous agent's with an exploration process (`process_call`), an fp32 agent, a rank that
    is neither critic- nor member-sharded (`sharded`), and backup weights that are off or "sunrise".  Everything else --
    "softmax" weights among it -- keeps the eager path.  The same answer selects the FORM of the eager calls of such an
    agent (learning._critic_update_eager: stacked gathers, workspace-owned weights, the one-workgroup chained launch, the
    picked gradient norm as a launch of its own), so warm-up, recorded and USE_GRAPHS = False updates leave the same bits."""
    weights_off = weight_type is None or weight_temp is None
    return bool(launch_mode == "list" and 2 <= ensemble_size <= MAX_MEMBERS and identity_encoder
                and kind in ("stochastic", "deterministic", "discrete") and not per and not update_priorities and not dr3
                and not process_call and not bf16 and not sharded and (weights_off or weight_type == "sunrise"))


CallFacts = collections.namedtuple(
    "CallFacts", "launch_mode kind discrete has_process identity_encoder vector_obs ensemble_size per per_on_device "
                 "update_priorities dr3 bf16 critic_sharded member_sharded popart arena_fused weight_type weight_temp "
                 "use_graphs capture cuda sharded_lists")
Verdict = collections.namedtuple("Verdict", "record explore refresh members")


def call_facts(kw, launch_mode, use_graphs, sharded_lists):
    """What the gates of a critic_update(**kw) call look at, read off the agent and the buffer HERE and nowhere else.
    vector_obs: the buffer's observations are one vector array (only then does every member's replay gather leave [s | a]
    in place); bf16: some actor or critic carries the "_ssac_precision" mark; arena_fused: filled for critic-sharded
    agents only -- arena() binds, and an unsharded agent's gate never asked."""
    from . import parallel
    agent, buffer = kw["agent"], kw["buffer"]
    marks = [o.__dict__.get("_ssac_precision") for o in list(agent.actors) + list(agent.critics)]
    st = getattr(buffer, "_storage", None)
    keys = list(st.s_stack.keys()) if st is not None else []
    critic_sharded = parallel.shard_of(agent) is not None
    return CallFacts(
        launch_mode, actor_kind(agent.actors[0]), bool(kw["discrete"]), kw["random_process"] is not None,
        is_identity(agent.encoder), len(keys) == 1 and st.s_stack[keys[0]].dim() == 2, agent.ensemble_size,
        bool(kw["per"]), bool(getattr(buffer, "per_on_device", False)), bool(kw["update_priorities"]),
        bool(kw["dr3_coeff"]), "bf16" in marks, critic_sharded, parallel.member_shard_of(agent) is not None,
        any(agent.popart),
        bool(critic_sharded and agent.critics[0].arena(kw["log_alphas"][0].device).fused),
        kw["weight_type"], kw["weighted_bellman_temp"], bool(use_graphs), engine.CAPTURE is not None,
        torch.cuda.is_available(), bool(sharded_lists))


def recording_verdict(f):
    """CallFacts -> Verdict, pure (tests/test_recording_verdict_cpu.py walks the grid).  record: the call's launches are
    recorded and re-issued (learning.critic_update); explore: head + exploration process run as one launch, recorded or
    eager (explore_recordable); refresh: the call's priority refresh runs as launches on the device trees
    (priority_recordable); members: an ensemble update takes the recordable form (members_recordable)."""
    sharded = f.critic_sharded or f.member_sharded
    process_ok = explore_recordable(f.kind, f.has_process, f.discrete, f.identity_encoder, f.ensemble_size, f.per, sharded,
                                    f.launch_mode)
    refresh = f.update_priorities and priority_recordable(f.kind, f.per_on_device, f.identity_encoder, f.ensemble_size,
                                                          f.per, f.dr3, sharded, f.bf16, f.launch_mode)
    members = members_recordable(f.launch_mode, f.ensemble_size, f.identity_encoder and f.vector_obs, f.kind, f.per,
                                 f.update_priorities, f.dr3, f.has_process and not f.discrete and f.kind != "discrete",
                                 f.bf16, sharded, f.weight_type, f.weight_temp)
    record = bool(
        f.use_graphs and not f.capture and (f.ensemble_size == 1 or members) and not f.per and f.kind != "beta"
        and not f.member_sharded
        # a priority refresh (AWAC / AFBC) is recorded when it runs as launches on the device trees
        and (refresh or not f.update_priorities) and not f.dr3 and f.identity_encoder and process_ok and f.cuda
        # critic-sharded ranks: recorded launch lists only (the collective sits between two segments), continuous
        # actions on the fused kernels (empty subset slots, in-launch TD target)
        and (not f.critic_sharded or (f.launch_mode == "list" and f.sharded_lists and not f.discrete and not f.popart
                                      and f.arena_fused)))
    return Verdict(record, f.has_process and not f.discrete and process_ok, refresh, members)


def recording_noise_buffers(kind, explore, refresh, in_kernel_noise):
    """The noise buffers a recorded critic update owns and refills on the host before every replay: (names filled before
    the REDQ subset is drawn, names filled after it), each in fill order, one rng.draw_normal_into call per name.  That is
    the reference's order on the device generator: the head's eps, the exploration process's noise (`explore`: the call
    carries a process the update looks at), and -- behind the subset, which is a Python-random draw -- the advantage
    estimator's N_SAMPLES candidate draws of a priority refresh (`refresh`) on a tanh-normal policy.  Deterministic and
    discrete heads draw no candidates.  Nothing at all while the noise is drawn inside the launches.  Pure (tests/
    test_priority_recording_cpu.py); learning._RecordedCritic fills its buffers by this list."""
    if in_kernel_noise:
        return [], []
    # (a recorded call carries a process exactly when its verdict says explore; buffer noise: any arena draws the same)
    before = list(td_member_plan(kind, explore, explore, False, True, in_kernel=False).draws)
    after = []
    if refresh and kind == "stochastic":
        from . import adv_estimator
        after = [f"cand{k}" for k in range(adv_estimator.N_SAMPLES)]
    return before, after


def draw_subset(num_critics, k):
    if engine.CAPTURE is not None:
        return list(engine.CAPTURE.ids)
    return rng.draw_subset(num_critics, k)


def log_block(device, adam=None):
    if engine.CAPTURE is not None:
        cap = engine.CAPTURE
        blk = cap.logblk
        if cap.defer_begin and cap.feed and cap.pending_begin is None:
            cap.pending_begin = (blk, 0 if adam is None else adam.ctl.ptr)  # folded into the replay gather
            return blk
        check(lib.ssac_begin_update(blk.data_ptr(), LOG_WIDTH, 0 if adam is None else adam.ctl.ptr,
                                    cap.feed, engine.stream()))
        return blk
    return ring_for(device).next(adam)


def ring_for(device):
    ring = _rings.get(device)
    if ring is None:
        ring = _rings[device] = LogRing(device)
    return ring


_ones = {}


def unit_weight(device):
    """imp_weights of the uniform path: torch.ones(1) (learning_utils.py:180), allocated once."""
    t = _ones.get(device)
    if t is None:
        t = _ones[device] = torch.ones(1, device=device)
    return t


def agent_ws(agent, device):
    ws = agent.__dict__.get("_ssac_ws")
    if ws is None or ws.device != device:
        ws = agent.__dict__["_ssac_ws"] = engine.Workspace(device)
    return ws


class GaussianExplorationNoise:
    """learning_utils.py:18-66.  Inside the updates only ``current_scale`` is read; the noise
    itself is drawn on the device and applied by ``ssac_det_action_fwd``."""

    def __init__(self, action_space, start_scale=1.0, final_scale=0.1, steps_annealed=1000, eps=1e-6):
        assert start_scale >= final_scale
        self.action_space = action_space
        self.start_scale, self.final_scale = start_scale, final_scale
        self.steps_annealed = steps_annealed
        self.current_scale = start_scale
        self._scale_slope = (start_scale - final_scale) / steps_annealed
        self.eps = eps

    def sample(self, action, clip=None, update_schedule=False):
        assert isinstance(action, np.ndarray), "device-side noise is applied inside the update kernels"
        noise = self.current_scale * np.random.randn(*action.shape)
        if clip is not None:
            noise = np.clip(noise, -clip, clip)
        out = np.clip(action + noise, self.action_space.low + self.eps, self.action_space.high - self.eps)
        if update_schedule:
            self.current_scale = max(self.current_scale - self._scale_slope, self.final_scale)
        return out


# ------------------------------------------------------------------------------------------
def _polyak_tensor(t, s, tau):
    check(lib.ssac_polyak(t.data_ptr(), s.data_ptr(), t.numel(), float(tau), engine.stream()))


# soft_update right behind a recorded critic update: no launch -- the update's own weight-gradient launch, still
# waiting in the queue, applies the target update in its Adam epilogue (ssac_late_polyak in include/ssac_hip.h)
LATE_POLYAK = True


def soft_update(target, source, tau):
    """theta_bar <- (1-tau) theta_bar + tau theta over all parameters (learning_utils.py:160-162);
    one launch over the packed arena when both sides are packed ensembles."""
    plan = target.__dict__.get("_ssac_polyak")
    last = source.__dict__.pop("_ssac_last_step", None)  # the recorded update issued last on these critics, if any
    if plan is not None and plan[0] is source:
        # packed ensembles seen before: one C call (the arenas are re-validated by pointer every 256 calls)
        _, ta, sa, tmods, smods, calls = plan
        plan[5] = calls + 1
        if (calls & 255) or (ta.is_bound(tmods) and sa.is_bound(smods)):
            if (last is not None and LATE_POLYAK and last.late_arenas is not None and last.late_arenas[0] is ta
                    and last.late_arenas[1] is sa and last.gs.fast is last and last.gs.path == "fast"):
                rc = lib.ssac_step_polyak(last.handle, float(tau))
                if rc == 1:
                    return  # served (or certain to be) by the update's own weight-gradient launch
                if rc < 0:  # no decision within 2 ms (a stalled queue): settle it the slow way
                    torch.cuda.synchronize()
                    if lib.ssac_step_polyak_done(last.handle) == 1:
                        return
            if ta.shadow is not None:
                check(lib.ssac_bf16_polyak(C.byref(ta.desc()), C.byref(sa.desc()), float(tau), ta.shadow.data_ptr(),
                                           engine.stream()))
            else:
                check(lib.ssac_polyak(ta.params.data_ptr(), sa.params.data_ptr(), ta.params.numel(), float(tau),
                                      engine.stream()))
            return
        del target.__dict__["_ssac_polyak"]
    if hasattr(target, "arena") and hasattr(source, "arena"):
        dev = next(source.parameters()).device
        ta, sa = target.arena(dev), source.arena(dev)
        if ta.params.numel() == sa.params.numel():
            if ta.shadow is not None:  # bf16 mode: the target's shadow is refreshed by the same launch
                check(lib.ssac_bf16_polyak(C.byref(ta.desc()), C.byref(sa.desc()), float(tau), ta.shadow.data_ptr(),
                                           engine.stream()))
            else:
                _polyak_tensor(ta.params, sa.params, tau)
            target.__dict__["_ssac_polyak"] = [source, ta, sa, list(target.nets), list(source.nets), 1]
            return
    # any other module (a pixel encoder: conv / fc / norm tensors): all of its parameters in ONE launch
    pairs = list(zip(target.parameters(), source.parameters()))
    if not pairs:
        return
    n = len(pairs)
    tp_, sp_, cn_ = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_int64 * n)()
    for j, (tp, sp) in enumerate(pairs):
        if not (tp.is_cuda and tp.data.is_contiguous() and sp.data.is_contiguous() and tp.dtype == torch.float32
                and sp.dtype == torch.float32 and tp.numel() == sp.numel()):
            raise RuntimeError("soft_update expects contiguous float32 device parameters of equal size")
        tp_[j], sp_[j], cn_[j] = tp.data_ptr(), sp.data_ptr(), tp.numel()
    check(lib.ssac_polyak_multi(tp_, sp_, cn_, n, float(tau), engine.stream()))


def hard_update(target, source):
    soft_update(target, source, 1.0)


# ------------------------------------------------------------------------------------------
class _Batch:
    """device buffers of one sampled minibatch: xsa = [s | a], x1sa = [s' | (a' written later)]."""
    __slots__ = ("B", "S", "A", "xsa", "x1sa", "r", "d", "key", "pixel", "pending")


class MemberUpdate:
    """what ONE ensemble member's critic update passes between its launches: learning._critic_update_eager makes one per
    member, compute_td_targets and the launchers below fill it in, a recording keeps its records alive.  Identity: i / ig
    (local / global member index), arena (critics), tag (workspace), rd (replay dict), B (rows).  Requests, set before
    compute_td_targets runs: want_fwd -- the online critics' forward may ride in the actor launch (s_rep, X, ldx, h1, h2,
    q); want_bwd -- the TD-independent backward may ride in the target launch (act, ld_act, dz2u, dz1u); dz2_optional --
    dz2u may stay inside the chained launch; lazy_td -- the TD target is left to the critic launch.  Outcomes, set by the
    launch that did the work: fwd_done, bwd_done; w3_snapshot (W3 as the chained launch saw it when it skipped dz2u, else
    None); chain (a PendingChain, None once issued); td with td_spec (ssac_td_spec; None: evaluated
    already), td_logs (its log words), td_keep (tensors the spec points into); bw (backup weights); branch (side stream);
    ss, grads, log_parts / log_nets / log_tiles, n_glob, logs_folded: what the clip and log launches read; td_rng: the
    ssac_rng (seed, counter address, offset) the TD target's noise was drawn with inside its launch, None when it came
    from a buffer or the update has none -- a priority refresh in the same update draws its candidates at that number;
    one_wg_chain (request): the chained launch keeps its one-workgroup form (recordable ensemble updates: the hand-off form
    needs a per-replay tag their recording cannot reach, so their eager calls do without it too)."""
    __slots__ = ("i", "ig", "arena", "tag", "rd", "B", "want_fwd", "s_rep", "X", "ldx", "h1", "h2", "q", "want_bwd", "act",
                 "ld_act", "dz2u", "dz1u", "dz2_optional", "lazy_td", "fwd_done", "bwd_done", "w3_snapshot", "chain", "td",
                 "td_spec", "td_logs", "td_keep", "bw", "branch", "ss", "grads", "log_parts", "log_nets", "log_tiles",
                 "n_glob", "logs_folded", "td_rng", "one_wg_chain")

    def __init__(self, i, ig, arena):
        for f in self.__slots__:
            setattr(self, f, None)
        self.i, self.ig, self.arena, self.tag = i, ig, arena, f"cu.c{i}"
        self.want_fwd = self.want_bwd = self.dz2_optional = self.lazy_td = self.fwd_done = self.bwd_done = False


# target-critic outputs of a REDQ subset: q (n * parts, B, out); xchg_done: reduced over the critic-sharded ranks already
SubsetQ = collections.namedtuple("SubsetQ", "q n parts xchg_done", defaults=(1, False))


class PendingChain(collections.namedtuple("PendingChain", "a_arena s1_rep eps_ptr actor x1 S A logp rng_ptr keep")):
    """MemberUpdate.chain: the actor half of a chained launch (TdPlan.launch "chain") as _actor_sample leaves it for
    _launch_chain, which issues it once the REDQ subset is known; keep: what eps_ptr / rng_ptr point into"""
    __slots__ = ()
    bf16 = property(lambda self: self.a_arena.shadow is not None)   # the launch's bf16-operand family (set_precision)


# actor sample -> target critics chained per workgroup, beside the critics' forward + unscaled backward: ONE launch
CHAIN_LAUNCH = True
# the chained launch in its producer / consumer form (the actor once per tile, the target critics start before a' exists);
# a module constant that tests flip to compare the two forms
CHAIN_PC = True
CHAIN_SPLIT = True   # ... with the target critics' fc2 split by columns over 2 / 4 consumer workgroups while the launch stays one round


def parallel_shard_of(agent):
    from . import parallel
    return parallel.shard_of(agent)


# the replay gather of a critic update rides in the merged actor / critic-forward launch (ssac_gather): no gather launch
FOLD_GATHER = True


def ensure_gathered(bt):
    """issue the replay gather of a batch whose gather was deferred (sample_move_and_augment(_defer_gather=True)) and
    has not been taken over by the merged launch"""
    if bt is None or getattr(bt, "pending", None) is None:
        return
    p, bt.pending = bt.pending, None
    S, A, B = p["S"], p["A"], bt.B
    if p.get("table") is not None:
        # several vector keys side by side (concat_order): one ssac_gather_concat launch, never folded into the merged one
        out = (B, bt.xsa.data_ptr(), bt.xsa.stride(0), bt.x1sa.data_ptr(), bt.x1sa.stride(0), bt.r.data_ptr(), bt.d.data_ptr())
        if p["begin"] is not None:
            blk, ctl = p["begin"]
            check(lib.ssac_gather_concat_begin(C.byref(p["table"]), p["act"], A, p["rew"], p["done"], *out, p["feed"],
                                               blk.data_ptr(), LOG_WIDTH, ctl, engine.stream()))
        else:
            check(lib.ssac_gather_concat(C.byref(p["table"]), p["act"], A, p["rew"], p["done"], p["idx"].data_ptr(), *out,
                                         engine.stream()))
    elif p["begin"] is not None:
        blk, ctl = p["begin"]
        check(lib.ssac_gather_transition_begin(p["s"], p["s1"], p["dtype"], S, p["act"], A, p["rew"], p["done"], B,
                                               bt.xsa.data_ptr(), S + A, bt.x1sa.data_ptr(), S + A, bt.r.data_ptr(),
                                               bt.d.data_ptr(), p["feed"], blk.data_ptr(), LOG_WIDTH, ctl,
                                               engine.stream()))
    else:
        check(lib.ssac_gather_transition(p["s"], p["s1"], p["dtype"], S, p["act"], A, p["rew"], p["done"],
                                         p["idx"].data_ptr(), B, bt.xsa.data_ptr(), S + A, bt.x1sa.data_ptr(), S + A,
                                         bt.r.data_ptr(), bt.d.data_ptr(), engine.stream()))


def gather_struct(bt):
    """the ssac_gather of a batch with a deferred gather (consumes it): handed to the merged launch"""
    p, bt.pending = bt.pending, None
    S, A = p["S"], p["A"]
    cap = engine.CAPTURE
    g = _lib.Gather(p["s"], p["s1"], p["act"], p["rew"], p["done"], S, A, p["idx"].data_ptr(), 0,
                    bt.xsa.data_ptr(), S + A, bt.x1sa.data_ptr(), S + A, bt.r.data_ptr(), bt.d.data_ptr(), 0, 0, -1, 0,
                    -1, 0)
    if p["begin"] is not None:
        blk, ctl = p["begin"]
        g.idx, g.feed, g.logs, g.n_logs, g.ctl = 0, p["feed"], blk.data_ptr(), LOG_WIDTH, ctl
        if cap is not None and cap.tick_ptr:
            g.rng_word = (cap.tick_ptr - cap.idx_dev.data_ptr()) // 4
        if cap is not None:
            g.ids_word = (cap.ids_dev.data_ptr() - cap.idx_dev.data_ptr()) // 4
    g._keep = (p["idx"],)
    return g


def _host_view(idx):
    """replay_dict["priority_idxs"]: numpy for a host-drawn index vector, the lazy host view of a device-drawn one"""
    return idx.numpy() if torch.is_tensor(idx) else idx


def draw_augmentation_orders(augmenter, channels):
    """the application-time draws of one sample_move_and_augment call (AugmentationSequence.draw_orders): s, then s', each
    over the image keys `channels` ({key: channel count}) in the augmenter's key order.  None when the augmenter holds no
    member that draws at application time.  Needs no GPU."""
    return augmenter.draw_orders(channels, channels)


def sample_move_and_augment(buffer, batch_size, augmenter, aug_mix, per=True, _defer_gather=False,
                            _invariance=False, _xsa=None):
    """``_xsa`` (critic_update, recordable ensemble updates): the (B, S + A) block of the members' stacked batch this
    call's gather writes [s | a] to, instead of a tensor of its own (vector buffers)."""
    assert len(buffer) >= batch_size
    if not hasattr(buffer, "draw_uniform_indices") or not hasattr(augmenter, "single_shift"):
        # objects built by the reference's own classes (the shipped scripts construct them before main.super_sac
        # runs: experiments/gym/train_gym.py:84, experiments/dmc/train_dmc_from_pixels.py:62,88) are adopted in place
        from . import adopt
        adopt.adopt_buffer(buffer)
        adopt.adopt_augmenter(augmenter)
    st = buffer._storage
    dev = st.device
    if per:
        # replay.py:163-177: the uniforms from numpy's global generator on the host; total mass, prefix-sum descent and
        # importance weights on the float64 trees in HBM (csrc/ssac_per.hip) -- no synchronisation
        idx_cpu, idx, w = buffer.draw_per_indices(batch_size)
        imp_weights = w if torch.is_tensor(w) else torch.from_numpy(w).to(dev)  # float64 (B,), as the reference hands it over
    else:
        idx_cpu, idx = buffer.draw_uniform_indices(batch_size)
        imp_weights = unit_weight(dev)
    B = batch_size
    keys = list(st.s_stack.keys())
    A = int(np.prod(st.action_stack.shape[1:]))
    r = torch.empty(B, 1, device=dev)
    d = torch.empty(B, 1, device=dev)
    # one randomisation per call, shared by s and s' (augmentations.py:28-29)
    augmenter.change_randomization_params()
    # ... and the application-time draws of the whole call (ColorJitterAug), before any key is augmented: the loop below
    # walks key-major, the reference's augmenter(oo, oo1) batch-major
    orders = draw_augmentation_orders(augmenter, {k: v.shape[1] for k, v in st.s_stack.items() if v.dim() == 4})
    bt = _Batch()
    bt.B, bt.A, bt.pending = B, A, None
    order = concat_order(st)   # ((key, width), ...) of a buffer whose vector keys travel side by side, else None
    vec = order is not None or (len(keys) == 1 and st.s_stack[keys[0]].dim() == 2)
    if vec:
        key = keys[0] if order is None else order[0][0]
        S = st.s_stack[key].shape[1] if order is None else sum(w for _, w in order)
        xsa = torch.empty(B, S + A, device=dev) if _xsa is None else _xsa
        assert tuple(xsa.shape) == (B, S + A) and xsa.stride(1) == 1
        x1sa = torch.empty(B, S + A, device=dev)
        src = st.s_stack[key]
        cap = engine.CAPTURE
        begin = None
        if cap is not None and cap.pending_begin:
            begin, cap.pending_begin = cap.pending_begin, ()  # this gather also does ssac_begin_update's work
        bt.xsa, bt.x1sa, bt.r, bt.d = xsa, x1sa, r, d
        bt.pending = dict(s=src.data_ptr(), s1=st.s1_stack[key].data_ptr(), act=st.action_stack.data_ptr(),
                          rew=st.reward_stack.data_ptr(), done=st.done_stack.data_ptr(), idx=idx, S=S, A=A,
                          begin=begin, feed=cap.feed if begin is not None else 0,
                          dtype=1 if src.dtype == torch.uint8 else 0,
                          table=None if order is None else concat_table(st.s_stack, st.s1_stack, order))
        # (the folded gather, ssac_gather, has one source array: a multi-key row is gathered by a launch of its own)
        if not (_defer_gather and FOLD_GATHER and src.dtype == torch.float32 and order is None):
            ensure_gathered(bt)
        if order is None:
            o, o1 = {key: xsa[:, :S]}, {key: x1sa[:, :S]}
        else:
            # the replay dict still carries every key: each a column view of the one row
            offs = np.cumsum([0] + [w for _, w in order])
            o = {k: xsa[:, c0:c0 + w] for (k, w), c0 in zip(order, offs)}
            o1 = {k: x1sa[:, c0:c0 + w] for (k, w), c0 in zip(order, offs)}
        a = xsa[:, S:]
        bt.S, bt.xsa, bt.x1sa, bt.key, bt.pixel = S, xsa, x1sa, key, False
        assert augmenter.is_identity(), "image augmentations need image observations"
    else:
        shift_aug = augmenter.single_shift()
        # cutout / translate / flip / rotate / window / gamma members: one ssac_aug_chain launch per run of them (and one
        # ssac_drq_shift launch per DrQ-family member of a mixed sequence), the first reading the replay rows through idx
        passes = augmenter.device_passes() if shift_aug is None else None
        k_aug = int(batch_size * aug_mix)
        o, o1 = {}, {}
        for key in keys:
            src, src1 = st.s_stack[key], st.s1_stack[key]
            if src.dim() == 4 and shift_aug is not None:
                n, (c, h, w) = B, src.shape[1:]
                assert h == w
                for dst_dict, s_arr in ((o, src), (o1, src1)):
                    out = torch.empty(B, c, h, w, device=dev)
                    nz = rng.draw_normal((B, c, h, w), dev) if shift_aug.noise else None
                    shift_aug.apply(s_arr, idx, B, c, h, k_aug, out, nz)
                    dst_dict[key] = out
            elif src.dim() == 4 and passes is not None:
                c, h, w = src.shape[1:]
                # (a key outside AugmentationSequence.keys is left alone, augmentations.py:33: gather + convert only)
                listed = augmenter.keys is None or key in augmenter.keys
                k_key = k_aug if listed else 0
                o[key] = passes.run(src, idx, B, c, h, w, k_key, dev, orders and orders[0][key])
                o1[key] = passes.run(src1, idx, B, c, h, w, k_key, dev, orders and orders[1][key])
            else:
                assert augmenter.is_identity(), "unsupported augmentation on the accelerated path"
                o[key] = st.gather_field(src, idx, B)
                o1[key] = st.gather_field(src1, idx, B)
        a = st.gather_field(st.action_stack, idx, B)
        if a.dim() < 2:
            a = a.unsqueeze(1)
        st.gather_field(st.reward_stack, idx, B, dst=r, ld=1)
        st.gather_field(st.done_stack, idx, B, dst=d, ld=1)
        bt.S, bt.xsa, bt.x1sa, bt.key, bt.pixel = None, None, None, None, True
        if _invariance:
            # the invariance constraints (learning_utils.py:272-285, 401-409) look at the FULLY augmented and the
            # un-augmented observation batch (same rows, same randomisation); where the mix already is one of them
            # (aug_mix 1 / 0) that tensor is shared
            ao, oo = {}, {}
            for key in keys:
                src = st.s_stack[key]
                if src.dim() == 4 and shift_aug is not None:
                    c, h, w = src.shape[1:]
                    for dst_dict, n_aug in ((ao, B), (oo, 0)):
                        if n_aug == k_aug:
                            dst_dict[key] = o[key]
                            continue
                        assert not shift_aug.noise, "the noise of DrqAug would have to be re-used across the passes"
                        out = torch.empty(B, c, h, w, device=dev)
                        shift_aug.apply(src, idx, B, c, h, n_aug, out, None)
                        dst_dict[key] = out
                elif src.dim() == 4 and passes is not None:
                    c, h, w = src.shape[1:]
                    listed = augmenter.keys is None or key in augmenter.keys
                    k_key = k_aug if listed else 0
                    for dst_dict, n_aug in ((ao, B if listed else 0), (oo, 0)):
                        # (the same rows under the same randomisation: the order flags of (s, key) again, nothing drawn)
                        dst_dict[key] = o[key] if n_aug == k_key else passes.run(src, idx, B, c, h, w, n_aug, dev,
                                                                                 orders and orders[0][key])
                else:
                    ao[key] = oo[key] = o[key]
            inv_obs = ((ao, None), (oo, None))
    bt.r, bt.d = r, d
    if _invariance and vec:
        inv_obs = ((o, None), (o, None))   # identity augmentation: augmented == original == the batch
    if _invariance:
        return {"primary_batch": (o, a, r, o1, d), "augmented_obs": inv_obs[0], "original_obs": inv_obs[1],
                "priority_idxs": _host_view(idx_cpu), "imp_weights": imp_weights, "_ssac": bt}
    return {"primary_batch": (o, a, r, o1, d), "augmented_obs": None, "original_obs": None,
            "priority_idxs": _host_view(idx_cpu), "imp_weights": imp_weights, "_ssac": bt}


# ------------------------------------------------------------------------------------------
def encode(encoder, obs_dict, dst=None, save=False):
    """state representation of the batch: identity encoders return the (strided) view; pixel
    encoders run the HIP conv engine (conv_encoder.py), two-layer MLP encoders theirs (mlp_encoder.py), and write
    into `dst[:, :emb]` when given."""
    key = getattr(encoder, "ssac_identity_key", None)
    if key is not None:
        return obs_dict[key]
    ck = getattr(encoder, "ssac_concat_keys", None)
    if ck is not None:
        return _concat_rows(ck, obs_dict, dst)
    eng = encoder_base.require_engine(encoder, next(iter(obs_dict.values())).device, obs_dict)
    img = obs_dict[getattr(encoder, "ssac_obs_key", "obs")]
    if dst is None:
        dst = torch.empty(img.shape[0], eng.emb, device=img.device)
    eng.forward(img, dst, dst.stride(0), save)
    return dst[:, :eng.emb]


def encode_stacked(encoder, first, second, ws, tag, dev):
    """two B-row observation batches as ONE 2B-row encoder pass that keeps what backward() needs (`first` in rows [0, B),
    `second` in [B, 2B): the weight gradients of both uses add up inside one backward).  The observations go to the
    workspace buffer `tag` ("cu.img2"), the embeddings to "<tag's prefix>.sall"; returns (engine, embeddings)."""
    eng = encoder_base.require_engine(encoder, dev, first)
    key = getattr(encoder, "ssac_obs_key", "obs")
    B = first[key].shape[0]
    img = ws.get(tag, (2 * B,) + tuple(first[key].shape[1:]))
    img[:B].copy_(first[key])
    img[B:].copy_(second[key])   # (device plumbing: the two observation batches behind one another)
    sall = ws.get(tag.partition(".")[0] + ".sall", (2 * B, eng.emb))
    eng.forward(img, sall, eng.emb, True)
    return eng, sall


def is_identity(encoder):
    """no arithmetic between the observation and the state representation: the encoder hands one key back, or lays
    several vector keys side by side (ssac_concat_keys: an identity over the wider row)"""
    return (getattr(encoder, "ssac_identity_key", None) is not None
            or getattr(encoder, "ssac_concat_keys", None) is not None)


def concat_order(storage):
    """((key, width), ...): the column order in which this replay storage's vector keys are gathered into one row, set
    at first contact with a concatenating encoder (bind_concat_order); None for every other buffer"""
    return storage.__dict__.get("ssac_concat_order")


def bind_concat_order(buffer, encoder):
    """first contact of a concatenating encoder with a buffer: its column order becomes the storage's.  The replay dict's
    tensors are column views of ONE gathered row, so a buffer serves one order: an agent that wants another is refused"""
    st = getattr(buffer, "_storage", None)
    want = getattr(encoder, "ssac_concat_keys", None)
    if st is None or want is None:
        return
    have = st.__dict__.get("ssac_concat_order")
    if have == want:
        return
    name = type(encoder).__name__
    if have is not None:
        raise NotImplementedError(
            f"{name}: this replay buffer's keys are already laid out as {[k for k, _ in have]} for another agent, and its "
            f"batches are column views of that one row; {[k for k, _ in want]} needs a buffer of its own")
    stored = {k: tuple(v.shape[1:]) for k, v in st.s_stack.items()}
    if stored != {k: (w,) for k, w in want}:
        raise NotImplementedError(
            f"{name}: the encoder concatenates {dict(want)}, the replay buffer holds {stored}: every key of the buffer "
            "must be a vector the encoder uses exactly once")
    st.ssac_concat_order = want


def concat_table(s_arrays, s1_arrays, order):
    """the ssac_concat of 2-D fp32 / uint8 arrays {key: tensor} in column order `order` (s1_arrays may be None)"""
    assert 1 <= len(order) <= _lib.MAX_OBS_KEYS
    t = _lib.Concat()
    t.n_keys = len(order)
    for j, (k, w) in enumerate(order):
        s = s_arrays[k]
        assert s.dim() == 2 and s.shape[1] == w and s.is_contiguous() and s.dtype in (torch.float32, torch.uint8)
        s1 = s1_arrays[k] if s1_arrays is not None else None
        assert s1 is None or (s1.shape == s.shape and s1.dtype == s.dtype and s1.is_contiguous())
        t.key[j] = _lib.ConcatKey(s.data_ptr(), 0 if s1 is None else s1.data_ptr(), int(s.dtype == torch.uint8), 0, w)
    t._keep = (s_arrays, s1_arrays)
    return t


def _concat_rows(order, obs_dict, dst=None):
    """encode() of a concatenating encoder.  A replay batch's tensors are column views of one gathered row
    (sample_move_and_augment): when pointers, strides and adjacency say so, the (B, S) strided view of that row -- no
    launch.  Loose tensors: ONE ssac_gather_concat launch (row r = row r) lays them side by side, into dst[:, :S] when
    given"""
    first = obs_dict[order[0][0]]
    B, S = first.shape[0], sum(w for _, w in order)
    ld, ptr = first.stride(0), first.data_ptr()
    views = first.dim() == 2 and ld >= S
    for k, w in order:
        t = obs_dict[k]
        views = (views and t.dim() == 2 and t.shape == (B, w) and t.dtype == torch.float32 and t.stride(1) == 1
                 and t.stride(0) == ld and t.data_ptr() == ptr)
        ptr += 4 * w
    if views:
        return torch.as_strided(first, (B, S), (ld, 1))
    rows = {}
    for k, w in order:
        t = obs_dict[k].flatten(1)
        assert t.shape == (B, w), f"observation key {k!r}: expected {w} values per row, got {tuple(t.shape)}"
        rows[k] = t.contiguous() if t.dtype in (torch.float32, torch.uint8) else t.float().contiguous()
    out = torch.empty(B, S, device=first.device) if dst is None else dst
    assert out.stride(1) == 1 and out.shape[0] == B
    table = concat_table(rows, None, order)
    check(lib.ssac_gather_concat(C.byref(table), 0, 0, 0, 0, 0, B, out.data_ptr(), out.stride(0), 0, 0, 0, 0,
                                 engine.stream()))
    return out[:, :S]


def ensure_adopted(agent, buffer=None):
    """first contact with an agent: add what a foreign (reference-built) agent lacks (adopt.py) and find out whether
    its encoder is an identity map, probing it with one row of the buffer's observations"""
    if agent.__dict__.get("_ssac_adopted") and (buffer is None or agent.encoder.__dict__.get("_ssac_probed")
                                                 or is_identity(agent.encoder)):
        bind_concat_order(buffer, agent.encoder)   # (a concatenating encoder: the buffer's rows take its column order)
        return
    from . import adopt
    adopt.adopt_agent(agent)
    if buffer is not None and not hasattr(buffer, "draw_uniform_indices"):
        adopt.adopt_buffer(buffer, next(agent.actors[0].parameters()).device)
    st = getattr(buffer, "_storage", None) if buffer is not None else None
    if st is not None and not is_identity(agent.encoder):
        rows = {k: v[:1].float() for k, v in st.s_stack.items()}
        if adopt.probe_identity(agent.encoder, rows) is None and adopt.probe_concat(agent.encoder, rows) is None:
            from . import mlp_encoder
            mlp_encoder.find_mlp_encoder(agent.encoder, rows)   # (two-layer MLP encoders: recognised once, here)
    bind_concat_order(buffer, agent.encoder)


def _row_stride(t):
    assert t.dim() == 2 and t.stride(1) == 1, "expected a row-major (B, F) device tensor"
    return t.stride(0)


def _concat_buffer(ws, tag, s_rep, A):
    """(B, S+A) buffer whose first S columns hold s_rep (copy is device plumbing)."""
    B, S = s_rep.shape
    buf = ws.get(tag, (B, S + A))
    buf[:, :S].copy_(s_rep)
    return buf


def actor_kind(actor):
    if isinstance(actor, nets.DiscreteActor) or hasattr(actor, "act_p"):
        return "discrete"
    if getattr(actor, "dist_impl", None) == "deterministic":
        return "deterministic"
    if getattr(actor, "dist_impl", None) == "beta":
        return "beta"   # (Beta head, beta.py: per-layer path only)
    return "stochastic"


def _upload_ids(ws, ids, device, tag):
    if engine.CAPTURE is not None:
        return engine.CAPTURE.ids_dev
    stager = ws.__dict__.setdefault("_stager", None)
    if stager is None:
        from .replay import _IndexStager
        stager = ws.__dict__["_stager"] = _IndexStager(device)
    return stager.upload(torch.tensor(ids, dtype=torch.int32), tag=tag)


def compute_td_targets(logs, replay_dict, agent, target_agent, ensemble_idx, ensemble_n, log_alphas,
                       pop, gamma, random_process, noise_clip, discrete=False, _slot=None, _member=None, _log_idx=None,
                       _explore=False):
    """learning_utils.py:298-354.  ``_explore`` (critic_update only): the call's process passes explore_recordable, so
    head + process may run as ssac_explore_action.  ``_member`` (critic_update only): the member's MemberUpdate record.  Its requests let
    launches here take over the online critics' forward (ssac_actor_sample_critic_fwd) and the TD-independent half of their
    backward pass (ssac_target_fwd_critic_bwdu), and leave the final elementwise step with its three log values to the
    critic launch (``td_spec``; continuous actions, no PopArt); its outcomes say which of them did."""
    t = types.SimpleNamespace(**locals())   # the call: its arguments, and below what its steps share
    m, i = _member, ensemble_idx
    r = t.r = replay_dict["primary_batch"][2]
    dev, B = t.dev, t.B = r.device, r.shape[0]
    ws = t.ws = agent_ws(agent, dev)
    t.slot = _slot if _slot is not None else log_block(dev)
    actor = t.actor = agent.actors[i]
    kind = t.kind = actor_kind(actor)
    t.st, t.aout, t.x1, t.rs = engine.stream(), None, None, None
    pre = not is_identity(target_agent.encoder) and kind != "discrete"   # the encoder writes straight into [s'|a']
    x1_pre = ws.get(f"td.x1.{i}", (B, target_agent.encoder.embedding_dim + actor.action_size)) if pre else None
    s1_rep = t.s1_rep = encode(target_agent.encoder, replay_dict["primary_batch"][3], dst=x1_pre)
    S = t.S = s1_rep.shape[1]
    a_arena = t.a_arena = engine.bind_arena(actor, "self", [actor], dev)
    t_arena = target_agent.critics[i].arena(dev)
    shard = parallel_shard_of(target_agent)
    plan = t.plan = td_member_plan(kind, random_process is not None, _explore, a_arena.fused, engine.CAPTURE is not None,
                                   m is not None and m.want_fwd, m is not None and m.want_bwd, t_arena.fused_dbuf,
                                   t_arena.out_dim == 1, shard is not None)
    bt = t.bt = replay_dict.get("_ssac")
    if plan.launch in ("fused", "layers"):
        ensure_gathered(bt)  # (a deferred replay gather rides in the merged launch only)
    if plan.launch == "layers":
        _, _, t.aout = engine.mlp_forward(a_arena, s1_rep, _row_stride(s1_rep), 0, B, ws, f"td.a{i}", save=False)
    N = t_arena.n_nets if shard is None else shard.num_critics  # the subset is drawn over the GLOBAL ensemble
    assert 0 < ensemble_n <= N
    t.logp = ws.get(f"td.logp{i}", (B,))
    if kind != "discrete":
        A = t.A = actor.action_size
        if bt is not None and bt.x1sa is not None and s1_rep.data_ptr() == bt.x1sa.data_ptr():
            t.x1 = bt.x1sa
        else:
            t.x1 = x1_pre if x1_pre is not None else _concat_buffer(ws, f"td.x1.{i}", s1_rep, A)
        if plan.noise == "kernel":
            t.rs = stream_rng(agent, dev)
            if m is not None:
                m.td_rng = (t.rs.seed, t.rs.counter, t.rs.offset)
        _TD_ACTION[plan.head](t)
    ids = draw_subset(N, ensemble_n)
    X, ldx = (s1_rep, _row_stride(s1_rep)) if kind == "discrete" else (t.x1, S + A)
    sq = _subset_q(ws, shard, t_arena, ids, X, ldx, B, dev, f"td.c{i}", None if kind == "discrete" else m)
    assert m is None or m.chain is None, "a chained launch is still pending"
    td = _td_finish(t, sq, ids, t_arena.out_dim)
    # (discrete: the logits; the reference returns probs here, only used by dr3)
    return td, (s1_rep, t.aout[0] if kind == "discrete" else t.x1[:, S:])


def _td_finish(t, sq, ids, out_dim):
    """the TD target of the subset's outputs sq -- an ssac_td_spec record left to the critic launch where the member asks
    for it, else the ssac_td_target launch --, its three logs, and the subset and [s'|a'] (DR3) into the replay dict"""
    m, i, slot, r = t._member, t.ensemble_idx, t.slot, t.r
    d, log_alpha, popart = t.replay_dict["primary_batch"][4], t.log_alphas[i], t.agent.popart[i]
    lp_ptr, qd = (t.aout.data_ptr(), out_dim) if t.plan.head == "discrete" else (t.logp.data_ptr(), 1)
    td = torch.empty(t.B, 1, device=t.dev)
    if m is not None and m.lazy_td and qd == 1 and not popart:
        m.td_spec = _lib.TdSpec(sq.q.data_ptr(), lp_ptr, r.data_ptr(), d.data_ptr(), log_alpha.data_ptr(),
                                td.data_ptr(), float(t.gamma), sq.n, t.plan.use_entropy, sq.parts)
        m.td_logs = slot[L_TD0 + 3 * i:]
        m.td_keep = (sq.q, t.logp, r, d, log_alpha)
    else:
        assert sq.parts == 1, "partial target Q needs the in-launch TD target (ssac_td_spec.n_parts)"
        check(lib.ssac_td_target(sq.q.data_ptr(), sq.n, t.B, qd, lp_ptr, r.data_ptr(), d.data_ptr(),
                                 log_alpha.data_ptr(), t.plan.use_entropy, float(t.gamma),
                                 popart.ptr if popart else 0, 1 if (popart and t.pop) else 0,
                                 td.data_ptr(), slot[L_TD0 + 3 * i:].data_ptr(), t.st))
    li = i if t._log_idx is None else t._log_idx   # (member-sharded ranks: the member's GLOBAL index names its logs)
    for j, name in enumerate(("mean_td_target", "std_td_target", "entropy_bonus")):
        t.logs[f"td_targets/{name}_{li}"] = slot[L_TD0 + 3 * i + j]
    t.replay_dict["_subset"], t.replay_dict["_x1"] = ids, t.x1
    return td


def _scale_clip(t):
    return float(t.random_process.current_scale), float(t.noise_clip) if t.noise_clip is not None else 0.0


def _process_noise(t):
    """exploration noise on the sampled action: it replaces the entropy term (learning_utils.py:331-335)"""
    if t.random_process is not None:
        noise = draw_normal((t.B, t.A), t.dev)
        check(lib.ssac_exploration_noise(t.x1.data_ptr(), t.S + t.A, t.S, noise.data_ptr(), *_scale_clip(t), t.B, t.A, t.st))


# ---- one body per TdPlan.head: a' into the [s'|a'] buffer t.x1, log pi into t.logp where the head has one
def _td_action_beta(t):
    # a' = a_dist_s1.sample() of the Beta head, log pi of that same x (the transform's cache, learning_utils.py:330-338)
    beta.sample(t.agent, t.aout, t.B, t.A, "td", t.ws.get(f"td.xb{t.ensemble_idx}", (t.B, t.A)), t.x1, t.S + t.A, t.S, t.logp)
    _process_noise(t)


def _td_action_explore(t):
    """a' = process(head(aout)) in one launch (ssac_explore_action; log pi is written but not used).  Noise: the update's
    tick of the agent's Philox stream; inside a recording made under a noise hook, the record's fixed-address buffers (head
    eps, then process noise: the reference's draw order).  Scale: by value, or read from the slot's aux word (recorded)."""
    cap, A, tanh_normal = engine.CAPTURE, t.A, t.kind == "stochastic"
    eps_ptr = noise_ptr = 0
    if t.rs is None:
        assert cap is not None, "eager updates under a noise hook keep the two-kernel sequence"
        if tanh_normal:
            eps_ptr = draw_normal((t.B, A), t.dev).data_ptr()
        noise_ptr = draw_normal((t.B, A), t.dev).data_ptr()
    check(lib.ssac_explore_action(
        t.aout.data_ptr(), 2 * A if tanh_normal else A, int(tanh_normal),
        float(t.actor.log_std_low) if tanh_normal else 0.0, float(t.actor.log_std_high) if tanh_normal else 0.0,
        eps_ptr, noise_ptr, C.addressof(t.rs) if t.rs is not None else 0, cap.scale_ptr if cap is not None else 0,
        *_scale_clip(t), t.B, A, t.x1.data_ptr(), t.S + A, t.S, t.logp.data_ptr() if tanh_normal else 0, t.st))


def _td_action_tanh_normal(t):
    eps = draw_normal((t.B, t.A), t.dev) if t.rs is None else None   # (None: the noise is drawn inside the launch)
    if t.plan.launch == "layers":
        check(lib.ssac_tanh_normal_fwd(t.aout.data_ptr(), 2 * t.A, eps.data_ptr(), t.B, t.A, float(t.actor.log_std_low),
                                       float(t.actor.log_std_high), t.x1.data_ptr(), t.S + t.A, t.S, t.logp.data_ptr(), t.st))
    else:
        _actor_sample(t, eps)
    _process_noise(t)


def _td_action_deterministic(t):
    noise = draw_normal((t.B, t.A), t.dev) if t.random_process is not None else None
    process = (noise.data_ptr(), *_scale_clip(t)) if noise is not None else (0, 0.0, 0.0)
    check(lib.ssac_det_action_fwd(t.aout.data_ptr(), t.A, 0, 0.0, *process, t.B, t.A, t.x1.data_ptr(), t.S + t.A, t.S, t.st))
    if noise is None:
        # a' = loc, and the entropy term is the log-density of Normal(loc, 1e-4) at its own mean (learning_utils.py:336-338
        # on distributions.py:107-114)
        check(lib.ssac_det_logprob(0, t.B, t.A, t.logp.data_ptr(), t.st))


_TD_ACTION = {"beta": _td_action_beta, "explore": _td_action_explore, "tanh_normal": _td_action_tanh_normal,
              "deterministic": _td_action_deterministic}


def _own_gather(bt, x1, X, fp32_only):
    """the ssac_gather struct when the launch's workgroups can fetch their replay rows themselves -- the deferred gather
    of bt writes exactly the launch's [s'|a'] and [s|a] buffers --, else None with the gather done by a launch of its own"""
    if (bt is not None and bt.pending is not None and x1.data_ptr() == bt.x1sa.data_ptr()
            and X.data_ptr() == bt.xsa.data_ptr() and (not fp32_only or bt.pending["dtype"] == 0)):
        return gather_struct(bt)
    ensure_gathered(bt)
    return None


def _actor_sample(t, eps):
    """actor forward + tanh-normal sample + log pi in ONE launch (a' lands in the [s'|a'] buffer), by TdPlan.launch on its
    own ("fused"), with the online critics' forward as extra workgroups ("dual"), or left pending ("chain"); noise: the
    buffer eps, or the update's tick t.rs"""
    m, a_arena, s1_rep, x1, S, A, B = t._member, t.a_arena, t.s1_rep, t.x1, t.S, t.A, t.B
    eps_ptr, rng_ptr = (eps.data_ptr(), 0) if eps is not None else (0, C.addressof(t.rs))
    lo, hi = float(t.actor.log_std_low), float(t.actor.log_std_high)
    if t.plan.launch == "chain":
        # the whole TD-independent part of the update is ONE launch, issued by _subset_q once the REDQ subset is known
        m.chain = PendingChain(a_arena, s1_rep, eps_ptr, t.actor, x1, S, A, t.logp, rng_ptr, eps if eps is not None else t.rs)
        m.fwd_done = True
    elif t.plan.launch == "dual":
        gth = _own_gather(t.bt, x1, m.X, False)
        with engine._timed("dual_fwd") as tm:
            for _ in range(tm.reps):  # 1, except under bench.py's live kernel timing (the launch is idempotent)
                check(lib.ssac_actor_sample_critic_fwd(
                    C.byref(a_arena.desc()), s1_rep.data_ptr(), _row_stride(s1_rep), B, eps_ptr, lo, hi, x1.data_ptr(),
                    S + A, S, t.logp.data_ptr(), rng_ptr, C.byref(m.arena.desc()), m.X.data_ptr(), m.ldx, m.h1.data_ptr(),
                    m.h2.data_ptr(), m.q.data_ptr(), C.byref(gth) if gth is not None else 0, t.st))
        m.fwd_done = True
    else:
        check(lib.ssac_actor_sample_fused(C.byref(a_arena.desc()), s1_rep.data_ptr(), _row_stride(s1_rep), B, eps_ptr, lo, hi,
                                          x1.data_ptr(), S + A, S, t.logp.data_ptr(), 0, 0, 0, rng_ptr, t.st))


# critic-sharded ranks: the exchange of the subset's target Q rides in the chained launch (a tail workgroup behind its
# target-critic workgroups) instead of being a launch of its own behind it; a module constant that tests flip to compare
FUSE_XCHG = True


def _launch_chain(m, t_arena, ids_ptr, n, ws, tag, B, allow_split=True, xchg=None):
    """ssac_chain_update: the pending actor sample (m.chain: PendingChain), the target critics of the n subset slots and
    the online critics' forward + TD-independent backward, ONE launch; returns the target outputs as a SubsetQ"""
    ch, m.chain = m.chain, None
    c_arena, h1, h2, dz2u, dz1u, Xc, ldxc, qc = m.arena, m.h1, m.h2, m.dz2u, m.dz1u, m.X, m.ldx, m.q
    a_arena, s1_rep, x1, S, A, actor = ch.a_arena, ch.s1_rep, ch.x1, ch.S, ch.A, ch.actor
    gth = _own_gather(m.rd.get("_ssac"), x1, Xc, True)
    # column-split target critics (producer / consumer form, fp32 family): every (slot, tile) gets `splits` consumer
    # workgroups and the slot's value arrives as that many partial sums -- read through ssac_td_spec.n_parts
    # (inside a recording the hand-off's tag must change per replay: it then comes from the input ring's update counter,
    # which the launch reaches through the folded gather or the deferred-log struct -- a recording with neither keeps the
    # one-workgroup form)
    cap_ = engine.CAPTURE
    pc_ok = (CHAIN_PC and not m.one_wg_chain
             and (cap_ is None or (gth is not None and gth.feed) or (cap_.feed and cap_.deferred is not None)))
    splits = 1
    if pc_ok and CHAIN_SPLIT and allow_split and c_arena.shadow is None:
        splits = int(lib.ssac_chain_target_splits(C.byref(a_arena.desc()), C.byref(t_arena.desc()),
                                                  C.byref(c_arena.desc()), B, n))
    q1 = ws.get(tag + ".y", (n * splits, B, 1))
    dl_ptr = 0
    if cap_ is not None and cap_.feed and cap_.deferred is not None:
        # recorded update: one extra workgroup of this launch writes the PREVIOUS update's log block to its ring slot
        dl_ptr = C.addressof(cap_.deferred)
        cap_.deferred_chain = True
    if c_arena.shadow is not None:
        # bf16-operand mode: the same launch on v_mfma_f32_32x32x16_bf16, fed from the arenas' bf16 shadows
        assert ch.bf16 and t_arena.shadow is not None, "bf16 mode: set_precision must cover the actor and the target agent too"
        bf = c_arena.bf_buffers(ws, "cu", B)
        # producer / consumer form (csrc/ssac_bf16.hip, bf_chain_pc_kernel), as below for the fp32 family
        ho = ws.get(tag + ".handoff", (B * A,), dtype=torch.int64, zero=True) if (pc_ok and A <= 8) else None
        with engine._timed("chain") as tm:
            for _ in range(tm.reps):
                check(lib.ssac_bf16_chain_update(
                    C.byref(a_arena.desc()), a_arena.shadow.data_ptr(), s1_rep.data_ptr(), _row_stride(s1_rep), B,
                    ch.eps_ptr, float(actor.log_std_low), float(actor.log_std_high), x1.data_ptr(), S + A, S,
                    ch.logp.data_ptr(), ch.rng_ptr, C.byref(t_arena.desc()), t_arena.shadow.data_ptr(), ids_ptr, n,
                    q1.data_ptr(), C.byref(c_arena.desc()), c_arena.shadow.data_ptr(), Xc.data_ptr(), ldxc, qc.data_ptr(),
                    bf["h1t"].data_ptr(), bf["h2t"].data_ptr(), bf["dz2t"].data_ptr(), bf["dz1t"].data_ptr(),
                    bf["xt"].data_ptr(), C.byref(gth) if gth is not None else 0, dl_ptr,
                    ho.data_ptr() if ho is not None else 0, engine.stream()))
        m.bwd_done = True
        return SubsetQ(q1, n, splits)
    skip_dz2 = m.dz2_optional
    # (the head rows W3 as THIS launch sees them: the weight-gradient launch that rebuilds dz2u from h2 cannot read the
    #  arena's W3 -- its own head workgroups are updating it while the fc2 tiles run)
    w3s = ws.get(tag + ".w3s", (c_arena.n_nets, c_arena.hidden))
    # producer / consumer form of the launch (csrc/ssac_fused.hip, fused_chain_pc_kernel): the actor once per tile, a'
    # handed to the tile's target-critic workgroups through tagged granules in this buffer (zeroed once: tag 0 is never used)
    ho = ws.get(tag + ".handoff", (B * A,), dtype=torch.int64, zero=True) if pc_ok else None
    with engine._timed("chain") as tm:
        for _ in range(tm.reps):  # 1, except under bench.py's live kernel timing (the launch is idempotent)
            check(lib.ssac_chain_update(
                C.byref(a_arena.desc()), s1_rep.data_ptr(), _row_stride(s1_rep), B, ch.eps_ptr,
                float(actor.log_std_low), float(actor.log_std_high), x1.data_ptr(), S + A, S,
                ch.logp.data_ptr(), ch.rng_ptr, C.byref(t_arena.desc()), ids_ptr, n,
                q1.data_ptr(), C.byref(c_arena.desc()), Xc.data_ptr(), ldxc, h1.data_ptr(), h2.data_ptr(),
                qc.data_ptr(), 0 if skip_dz2 else dz2u.data_ptr(), dz1u.data_ptr(), w3s.data_ptr(),
                C.byref(gth) if gth is not None else 0, dl_ptr, ho.data_ptr() if ho is not None else 0, splits,
                xchg.handle if (xchg is not None and ho is not None) else 0, engine.stream()))
    if skip_dz2:
        m.w3_snapshot = w3s   # (the weight-gradient launch rebuilds dz2u from h2 and this W3 copy)
    m.bwd_done = True
    return SubsetQ(q1, n, splits, xchg is not None and ho is not None)  # (... the launch reduced q1 over the ranks itself)


def _target_q(m, t_arena, ids_dev, n, X, ldx, B, ws, tag, timed, allow_split=True, xchg=None):
    """the target critics of the n subset slots ids_dev on X, as a SubsetQ: inside member m's pending chained launch, in
    ONE launch with the TD-independent half of m's backward pass (once its forward is done and asks for it), or as a plain
    forward.  timed: bench.py's live kernel timing may repeat the ridden launch (not in a sharded rank's recording)"""
    if m is not None and m.chain is not None:
        return _launch_chain(m, t_arena, ids_dev.data_ptr(), n, ws, tag, B, allow_split, xchg)
    if m is not None and m.want_bwd and m.fwd_done and t_arena.fused_dbuf:
        q1 = ws.get(tag + ".y", (n, B, t_arena.out_dim))
        with engine._timed("dual_bwd" if timed else None) as tm:
            for _ in range(tm.reps):  # 1, except under bench.py's live kernel timing (idempotent launch)
                check(lib.ssac_target_fwd_critic_bwdu(
                    C.byref(t_arena.desc()), ids_dev.data_ptr(), n, X.data_ptr(), ldx, B, q1.data_ptr(),
                    C.byref(m.arena.desc()), m.h1.data_ptr(), m.h2.data_ptr(), m.act.data_ptr(), m.ld_act,
                    m.dz2u.data_ptr(), m.dz1u.data_ptr(), engine.stream()))
        m.bwd_done = True
        return SubsetQ(q1, n)
    _, _, q1 = engine.mlp_forward(t_arena, X, ldx, 0, B, ws, tag, net_ids=ids_dev, n_sel=n, save=False)
    return SubsetQ(q1, n)


def _subset_q(ws, shard, t_arena, ids, X, ldx, B, dev, tag, m=None):
    """target-critic outputs for the REDQ subset `ids`: SubsetQ(q, n, ...) with q of shape (n, B, out).  Sharded: forward of
    the locally owned subset members, elementwise min, MIN all-reduce of the (B x out) partial (the one real exchange step
    of the critic update), n = 1.  m: the member's record -- its pending chained launch or ridden backward is issued here
    (_target_q)."""
    if shard is None:
        return _target_q(m, t_arena, _upload_ids(ws, ids, dev, "sub"), len(ids), X, ldx, B, ws, tag, True)
    from . import parallel
    O = t_arena.out_dim
    qpart = ws.get(tag + ".qpart", (1, B, O))
    cap = engine.CAPTURE
    if cap is not None:
        # recorded launch sequence: a fixed shape for every subset draw -- all len(ids) slots are forwarded, the
        # per-update device id block holds the LOCAL index of the members this rank owns and -1 for the others
        # (their outputs are +inf), and the collective runs between two recorded segments
        n, ch, xchg = len(ids), m.chain if m is not None else None, parallel._exchange
        # (a chained launch: the exchange rides in it when it can; partial sums only when the one-shot exchange will
        # carry them -- it sums a slot's parts before sending)
        x_ = xchg if (ch is not None and FUSE_XCHG and xchg is not None and not ch.bf16
                      and n * B <= xchg.max_floats) else None
        sq = _target_q(m, t_arena, cap.ids_dev, n, X, ldx, B, ws, tag, False, allow_split=xchg is not None, xchg=x_)
        if sq.xchg_done:
            parallel.check_exchange()   # (of the exchanges issued so far: a host load, as all_reduce_min_owned does)
            return sq
        q1, parts = sq.q, sq.parts
        # MIN all-reduce of all n slots at once (n x B x O floats; slots this rank does not own hold +inf): the minimum
        # over the slots is taken where the TD target is evaluated, so no local min launch is needed
        if parallel.one_shot_ready(q1):
            # ONE recorded launch (csrc/ssac_xchg.hip): the update stays one launch list; only the subset members'
            # owners send (the id block, mirrored to device memory by the update's first launch, names them)
            parallel.all_reduce_min_owned(q1, cap.ids_dev, n, parts)
        else:
            assert parts == 1
            cap.collective(lambda: parallel.all_reduce_min(q1))
        return SubsetQ(q1, n, parts)
    local = shard.local_subset(ids)
    if local:
        ids_dev = _upload_ids(ws, local, dev, f"sub{len(local)}")
        _, _, q1 = engine.mlp_forward(t_arena, X, ldx, 0, B, ws, tag, net_ids=ids_dev, n_sel=len(local),
                                      save=False)
        _min_over_nets(q1, len(local), B * O, qpart)
    else:
        qpart.fill_(float("inf"))
    parallel.all_reduce_min(qpart)
    return SubsetQ(qpart, 1)


# ------------------------------------------------------------------------------------------
# Member-sharded ranks (parallel.MemberShard, SURVEY 8(e) "SUNRISE variant"): a member another rank owns still
# CONSUMES its host draws here -- in the order the reference makes them -- so that the generators of every rank (and
# the in-kernel noise counter of this agent) stay in step with the owner's.  `actor` = any local actor (all members
# share class and shape).
# ------------------------------------------------------------------------------------------
def skip_td_draws(agent, actor, B, dev, n_critics, ensemble_n, random_process):
    """the draws of compute_td_targets for one member: what its owner's plan lists (a' noise, exploration noise), then the
    REDQ subset.  A member-sharded owner runs eagerly, without the head + process launch; no member request changes a
    draw.  (The Beta head's own draws are not made here: critic_update refuses member-sharded Beta agents.)"""
    kind = actor_kind(actor)
    fused = kind == "stochastic" and engine.bind_arena(actor, "self", [actor], dev).fused
    for draw in td_member_plan(kind, random_process is not None, False, fused, False).draws:
        if draw == "tick":
            skip_stream_tick(agent, dev)
        else:
            draw_normal((B, actor.action_size), dev)
    draw_subset(n_critics, ensemble_n)


def skip_actor_draws(actor, B, dev, random_process):
    """the draws of online_actor_update for one member: rsample noise, then exploration noise"""
    if actor_kind(actor) == "discrete":
        return
    A = actor.action_size
    draw_normal((B, A), dev)
    if random_process is not None:
        draw_normal((B, A), dev)


def skip_alpha_draws(agent, actor, B, dev):
    """the draw of alpha_update for one member: the policy sample behind log pi"""
    if actor_kind(actor) != "stochastic":
        return
    if engine.bind_arena(actor, "self", [actor], dev).fused and IN_KERNEL_NOISE and rng.normal_is_stock():
        skip_stream_tick(agent, dev)
    else:
        draw_normal((B, actor.action_size), dev)


def member_sharded_sunrise_weights(logs, replay_dicts, agent, target_agent, member_shard, weight_temp, discrete, slot):
    """compute_backup_weights("sunrise") on a member-sharded rank (learning_utils.py:372-382): replay_dicts = the batch
    of EVERY global member (this rank gathered them all: same index draws everywhere).  This rank's members' target
    critics score all E batches, the all-gather completes the (batch, member, row) table, and the weights of the
    members this rank owns are formed from it.  Returns {global member index: (B, 1) weights}."""
    from . import parallel
    ms = member_shard
    E, El = ms.ensemble_size, ms.n_local
    a0 = replay_dicts[0]["primary_batch"][1]
    dev = a0.device
    ws = agent_ws(agent, dev)
    st = engine.stream()
    B = a0.shape[0]
    table = ws.get("bw.table", (E, E, B))   # [batch of member i][member k][row]
    table.zero_()
    for ig, rd in enumerate(replay_dicts):
        o, a = rd["primary_batch"][0], rd["primary_batch"][1]
        ensure_gathered(rd.get("_ssac"))
        s_rep = encode(target_agent.encoder, o)
        S = s_rep.shape[1]
        bt = rd.get("_ssac")
        if discrete:
            x, ldx = s_rep, _row_stride(s_rep)
        elif bt is not None and bt.xsa is not None and s_rep.data_ptr() == bt.xsa.data_ptr():
            x, ldx = bt.xsa, bt.xsa.stride(0)
        else:
            x = _concat_buffer(ws, f"bw.x{ig}", s_rep, a.shape[1])
            x[:, S:].copy_(a)
            ldx = x.stride(0)
        for k in range(El):
            ar = target_agent.critics[k].arena(dev)
            _, _, q = engine.mlp_forward(ar, x, ldx, 0, B, ws, f"bw.c{k}", save=False)
            check(lib.ssac_ensemble_min_select(q.data_ptr(), ar.n_nets, B, ar.out_dim,
                                               a.data_ptr() if discrete else 0, a.stride(0) if discrete else 0,
                                               table[ig, ms.lo + k].data_ptr(), st))
    parallel.all_gather_blocks(table)
    out = {}
    for ig in range(ms.lo, ms.hi):
        w = torch.empty(B, 1, device=dev)
        check(lib.ssac_sunrise_weights(table[ig].data_ptr(), E, B, float(weight_temp), w.data_ptr(),
                                       slot[L_BW:].data_ptr(), st))
        out[ig] = w
    for j, nm in enumerate(("mean", "max", "min", "std")):   # (the LAST owned member's statistics stay in the block)
        logs[f"bellman_weights/{nm}"] = slot[L_BW + j]
    return out


def member_sharded_softmax_scores(replay_dict, agent, target_agent, member_shard, row):
    """The "softmax" backup weights on a member-sharded rank, first half (learning_utils.py:383-393), for the batch of ONE
    global member -- owned or not: EVERY member k's online actor samples a'_k on the target encoder's s' and member k's online
    critics score it.  The draws are made for all E members in member order on every rank (shape-only for the tanh-normal
    policy; a categorical draw on a uniform stand-in for a member another rank holds), this rank's members fill their rows
    of `row` (E x B: [member k][batch row]); the all-gather over the ranks completes the table
    (member_sharded_softmax_finish)."""
    ms = member_shard
    o1 = replay_dict["primary_batch"][3]
    ensure_gathered(replay_dict.get("_ssac"))
    s1_rep = encode(target_agent.encoder, o1)
    B, S = s1_rep.shape
    dev = s1_rep.device
    ws = agent_ws(agent, dev)
    st = engine.stream()
    lds = _row_stride(s1_rep)
    for kg in range(ms.ensemble_size):
        k = ms.local(kg)
        actor = agent.actors[0 if k is None else k]
        kind = actor_kind(actor)
        if kind == "discrete":
            if k is None:   # (a stand-in draw of the same shape keeps the hooks / the generator in step with the owner's)
                rng.draw_categorical(torch.zeros(B, agent.critics[0].arena(dev).out_dim, device=dev))
                continue
            a_arena, c_arena = engine.bind_arena(actor, "self", [actor], dev), agent.critics[k].arena(dev)
            _, _, aout = engine.mlp_forward(a_arena, s1_rep, lds, 0, B, ws, f"bw.a{k}", save=False)
            a1 = rng.draw_categorical(aout[0]).to(torch.float32).view(B, 1)
            _, _, q = engine.mlp_forward(c_arena, s1_rep, lds, 0, B, ws, f"bw.c{k}", save=False)
            check(lib.ssac_ensemble_min_select(q.data_ptr(), c_arena.n_nets, B, c_arena.out_dim, a1.data_ptr(), 1,
                                               row[kg].data_ptr(), st))
        else:
            if kind == "beta":
                beta.refuse("softmax backup weights on a member-sharded agent")
            assert kind == "stochastic", "softmax backup weights sample from a stochastic policy"
            A = actor.action_size
            eps = rng.draw_normal((B, A), dev)   # actor_k(s1_rep).sample(): every rank makes every member's draw
            if k is None:
                continue
            a_arena, c_arena = engine.bind_arena(actor, "self", [actor], dev), agent.critics[k].arena(dev)
            _, _, aout = engine.mlp_forward(a_arena, s1_rep, lds, 0, B, ws, f"bw.a{k}", save=False)
            x1 = _concat_buffer(ws, f"bw.x1.{k}", s1_rep, A)
            check(lib.ssac_tanh_normal_fwd(aout.data_ptr(), 2 * A, eps.data_ptr(), B, A, float(actor.log_std_low),
                                           float(actor.log_std_high), x1.data_ptr(), S + A, S, 0, st))
            _, _, q = engine.mlp_forward(c_arena, x1, S + A, 0, B, ws, f"bw.c{k}", save=False)
            check(lib.ssac_ensemble_min_select(q.data_ptr(), c_arena.n_nets, B, 1, 0, 0, row[kg].data_ptr(), st))


def member_sharded_softmax_finish(logs, table, member_shard, weight_temp, slot):
    """second half: all-gather of the (batch of member i, member k, row) table -- a SUM of disjointly filled blocks -- then
    B softmax_b(-std_k T) for the members this rank owns.  Returns {global member index: (B, 1) weights}."""
    from . import parallel
    ms = member_shard
    E, B = table.shape[1], table.shape[2]
    parallel.all_gather_blocks(table)
    out = {}
    for ig in range(ms.lo, ms.hi):
        w = torch.empty(B, 1, device=table.device)
        check(lib.ssac_softmax_weights(table[ig].data_ptr(), E, B, float(weight_temp), w.data_ptr(), slot[L_BW:].data_ptr(),
                                       engine.stream()))
        out[ig] = w
    for j, nm in enumerate(("mean", "max", "min", "std")):   # (the LAST owned member's statistics stay in the block)
        logs[f"bellman_weights/{nm}"] = slot[L_BW + j]
    return out


def compute_backup_weights(logs, replay_dict, agent, target_agent, weight_type, weight_temp, batch_size,
                           discrete=False, _slot=None, _w=None):
    """learning_utils.py:357-398.  "sunrise": sigmoid(-std_k(Qbar_k(s, a)) T) + 0.5 over the members' TARGET critics
    (discrete: the taken action's column); "softmax": B softmax_b(-std_k(Q_k(s', a'_k)) T) with a'_k sampled from
    member k's ONLINE actor and scored by member k's ONLINE critics on the target encoder's s'.  Q_k = min over the
    member's nets (agent.Critic.forward defaults, agent.py:22).  ``_w`` (critic_update, recordable ensemble updates): the
    (B, 1) tensor the weights are written to -- a recorded launch needs an address that outlives the call."""
    if weight_type is None or weight_temp is None or agent.ensemble_size == 1:
        return 1.0
    assert weight_type in ("sunrise", "softmax"), f"unknown weight_type {weight_type!r}"
    o, a, _, o1, _ = replay_dict["primary_batch"]
    dev = a.device
    ws = agent_ws(agent, dev)
    slot = _slot if _slot is not None else log_block(dev)
    st = engine.stream()
    E = agent.ensemble_size
    bt = replay_dict.get("_ssac")
    if weight_type == "sunrise":
        s_rep = encode(target_agent.encoder, o)
        B, S = s_rep.shape
        if discrete:
            x, ldx = s_rep, _row_stride(s_rep)
        elif bt is not None and bt.xsa is not None and s_rep.data_ptr() == bt.xsa.data_ptr():
            x, ldx = bt.xsa, bt.xsa.stride(0)
        else:
            x = _concat_buffer(ws, "bw.x", s_rep, a.shape[1])
            x[:, S:].copy_(a)
            ldx = x.stride(0)
        qmin = ws.get("bw.qmin", (E, B))
        for k in range(E):
            ar = target_agent.critics[k].arena(dev)
            _, _, q = engine.mlp_forward(ar, x, ldx, 0, B, ws, f"bw.c{k}", save=False)
            check(lib.ssac_ensemble_min_select(q.data_ptr(), ar.n_nets, B, ar.out_dim,
                                               a.data_ptr() if discrete else 0, a.stride(0) if discrete else 0,
                                               qmin[k].data_ptr(), st))
        w = torch.empty(B, 1, device=dev) if _w is None else _w
        check(lib.ssac_sunrise_weights(qmin.data_ptr(), E, B, float(weight_temp), w.data_ptr(),
                                       slot[L_BW:].data_ptr(), st))
    else:
        s1_rep = encode(target_agent.encoder, o1)
        B, S = s1_rep.shape
        lds = _row_stride(s1_rep)
        qmin = ws.get("bw.qmin", (E, B))
        for k, (actor, critic) in enumerate(agent.ensemble):
            a_arena = engine.bind_arena(actor, "self", [actor], dev)
            c_arena = critic.arena(dev)
            _, _, aout = engine.mlp_forward(a_arena, s1_rep, lds, 0, B, ws, f"bw.a{k}", save=False)
            if discrete:
                a1 = rng.draw_categorical(aout[0]).to(torch.float32).view(B, 1)  # actor(s1_rep).sample()
                _, _, q = engine.mlp_forward(c_arena, s1_rep, lds, 0, B, ws, f"bw.c{k}", save=False)
                check(lib.ssac_ensemble_min_select(q.data_ptr(), c_arena.n_nets, B, c_arena.out_dim, a1.data_ptr(), 1,
                                                   qmin[k].data_ptr(), st))
            elif actor_kind(actor) == "beta":
                A = actor.action_size
                x1 = _concat_buffer(ws, f"bw.x1.{k}", s1_rep, A)
                beta.sample(agent, aout, B, A, "backup", ws.get(f"bw.xb{k}", (B, A)), x1, S + A, S)  # actor(s1_rep).sample()
                _, _, q = engine.mlp_forward(c_arena, x1, S + A, 0, B, ws, f"bw.c{k}", save=False)
                check(lib.ssac_ensemble_min_select(q.data_ptr(), c_arena.n_nets, B, 1, 0, 0, qmin[k].data_ptr(), st))
            else:
                A = actor.action_size
                assert actor_kind(actor) == "stochastic", "softmax backup weights sample from a stochastic policy"
                x1 = _concat_buffer(ws, f"bw.x1.{k}", s1_rep, A)
                eps = rng.draw_normal((B, A), dev)  # actor(s1_rep).sample()
                check(lib.ssac_tanh_normal_fwd(aout.data_ptr(), 2 * A, eps.data_ptr(), B, A, float(actor.log_std_low),
                                               float(actor.log_std_high), x1.data_ptr(), S + A, S, 0, st))
                _, _, q = engine.mlp_forward(c_arena, x1, S + A, 0, B, ws, f"bw.c{k}", save=False)
                check(lib.ssac_ensemble_min_select(q.data_ptr(), c_arena.n_nets, B, 1, 0, 0, qmin[k].data_ptr(), st))
        w = torch.empty(B, 1, device=dev)
        check(lib.ssac_softmax_weights(qmin.data_ptr(), E, B, float(weight_temp), w.data_ptr(),
                                       slot[L_BW:].data_ptr(), st))
    for j, nm in enumerate(("mean", "max", "min", "std")):
        logs[f"bellman_weights/{nm}"] = slot[L_BW + j]
    return w


def _fused_tile_rows(desc, n_rows, n_nets):
    """row tile (16 or 32) ssac_mlp3_fwd_fused takes for this launch shape (its choice looks at the launch's size)"""
    tiles = int(lib.ssac_fused_row_tiles(C.byref(desc), n_rows, n_nets))
    return 16 if tiles == (n_rows + 15) // 16 else 32


def members_pack_group(target_agent, E, B, dev):
    """How many networks one packed forward of the members' target critics takes, or 0 when they keep their per-member
    forwards.  The pack needs fused fp32 arenas of one shape; and the fused forward picks 16- or 32-row tiles by the size
    of the launch, whose results differ in the last bits -- so the E N nets go out in groups small enough that the E B-row
    launch takes the tile the B-row forward of one member's N nets takes (sunrise.gin's shape: 10 nets x 1 280 rows as
    groups of 3).  A shape at which no group size does (very large E B) keeps the per-member forwards."""
    arenas = [target_agent.critics[k].arena(dev) for k in range(E)]
    a0 = arenas[0]
    if not all(a.fused and a.shadow is None and (a.n_nets, a.in_dim, a.hidden, a.out_dim, a.stride) ==
               (a0.n_nets, a0.in_dim, a0.hidden, a0.out_dim, a0.stride) for a in arenas):
        return 0
    desc = a0.desc()
    want = _fused_tile_rows(desc, B, a0.n_nets)
    group = min(E * a0.n_nets, MAX_PACK_NETS)
    while group > 0 and _fused_tile_rows(desc, E * B, group) != want:
        group -= 1
    return group


def members_sunrise_weights(logs, xstack, S, agent, target_agent, weight_temp, batch_size, discrete, slot, group):
    """compute_backup_weights("sunrise") of ALL member batches at once (PACKED_WEIGHTS): xstack (E B, S + A) holds the
    members' gathered [s | a] rows member-major.  Three launches: the E target-critic arenas into one pack
    (ssac_polyak_multi, tau 1 -- inside every update, the targets move on Polyak steps a recording does not see), ONE
    forward of the E N nets over the E B rows (`group` nets per launch: members_pack_group), ssac_members_sunrise_weights.  Returns
    the (E, B) workspace tensor of the weights; the bellman_weights/* words are the last member's, as the reference's loop
    leaves them."""
    dev = xstack.device
    ws = agent_ws(agent, dev)
    st = engine.stream()
    E, B = agent.ensemble_size, batch_size
    arenas = [target_agent.critics[k].arena(dev) for k in range(E)]
    a0 = arenas[0]
    N, qd = a0.n_nets, a0.out_dim
    per = N * a0.stride
    pack = ws.get("bw.pack", (E * per,), zero=True)
    t = (C.c_void_p * E)(*[pack.data_ptr() + 4 * k * per for k in range(E)])
    s_ = (C.c_void_p * E)(*[a.params.data_ptr() for a in arenas])
    cnt = (C.c_int64 * E)(*[per] * E)
    check(lib.ssac_polyak_multi(t, s_, cnt, E, 1.0, st))
    q = ws.get("bw.qpack", (E * N, E * B, qd))
    ldx = xstack.stride(0)
    for k0 in range(0, E * N, group):
        k = min(group, E * N - k0)
        desc = _lib.MlpDesc(pack.data_ptr() + 4 * k0 * a0.stride, a0.stride, k, a0.in_dim, a0.hidden, qd)
        check(lib.ssac_mlp3_fwd_fused(C.byref(desc), 0, k, xstack.data_ptr(), ldx, 0, E * B, 0, 0, q[k0:k0 + k].data_ptr(),
                                      st))
    w = ws.get("bw.wall", (E, B))
    check(lib.ssac_members_sunrise_weights(q.data_ptr(), E, N, B, qd, float(weight_temp),
                                           xstack.data_ptr() + 4 * S if discrete else 0, ldx if discrete else 0,
                                           w.data_ptr(), slot[L_BW:].data_ptr(), st))
    for j, nm in enumerate(("mean", "max", "min", "std")):
        logs[f"bellman_weights/{nm}"] = slot[L_BW + j]
    return w


MAX_PACK_NETS = 64   # SSAC_MAX_NETS: the networks of ONE packed forward launch


def _min_over_nets(q, n, B, out):
    """out[b] = min_j q[j][b] using the TD-target kernel in its plain-min configuration
    (gamma=1, r=0, d=0, no entropy, no PopArt): td = 0 + 1*(1-0)*min."""
    dev = q.device
    z = _zeros(dev, B)
    check(lib.ssac_td_target(q.data_ptr(), n, B, 1, 0, z.data_ptr(), z.data_ptr(), z.data_ptr(), 0, 1.0,
                             0, 0, out.data_ptr(), 0, engine.stream()))


_zero_cache = {}


def _zeros(dev, n):
    z = _zero_cache.get((dev, n))
    if z is None:
        z = _zero_cache[(dev, n)] = torch.zeros(n, device=dev)
    return z


# ------------------------------------------------------------------------------------------
# AFBC helpers (learning_utils.py:217-240, 287-295)
# ------------------------------------------------------------------------------------------
def adjust_priorities(logs, replay_dict, agent, buffer, _member=None, _recordable=False):
    """new PER priorities relu(A(s,a)) + 1e-4 from a random ensemble member (fresh policy samples).
    ``_member`` / ``_recordable`` (critic_update only): the update's MemberUpdate record and priority_recordable's answer
    for the call.  A recordable refresh runs as launches only (AdvantageEstimator.evaluate(_update=...)): always inside a
    recording, and in eager calls while the noise comes from the engine's Philox stream -- the candidates then share the
    draw number of this update's TD-target noise (_member.td_rng), so eager and recorded calls follow one stream.  Eager
    calls under a noise hook, or whose head noise is a host draw, keep the present draws and launches."""
    o, a = replay_dict["primary_batch"][0], replay_dict["primary_batch"][1]
    cap = engine.CAPTURE
    if cap is not None:
        # recorded: learning._host_inputs makes the reference's random.choice per update; the rows are the indices of
        # THIS update in the recording's input block, the priorities the estimator's fixed workspace tensor
        assert _recordable and agent.ensemble_size == 1
        res = agent.adv_estimator.evaluate(o, a, 0, want=("prio",), _update=(_member.td_rng, cap.cand))
        buffer._per.assign_recorded(cap.idx_dev, res["prio"].reshape(-1), buffer._storage.size)
        return
    member = rng.choice(range(agent.ensemble_size))
    kind = actor_kind(agent.actors[member])
    if (_recordable and IN_KERNEL_NOISE and rng.normal_is_stock()
            and (kind != "stochastic" or _member.td_rng is not None)):
        res = agent.adv_estimator.evaluate(o, a, member, want=("prio",), _update=(_member.td_rng, None))
    else:
        res = agent.adv_estimator.evaluate(o, a, member, want=("prio",))
    # (the reference blocks here, .cpu() in learning_utils.py:293; with the trees in HBM the new priorities and the
    # indices they belong to never leave the device)
    new_priorities = res["prio"].reshape(-1)
    if not getattr(buffer, "per_on_device", False):
        new_priorities = new_priorities.cpu().numpy()
    buffer.update_priorities(replay_dict["priority_idxs"], new_priorities)


def compute_filter_stats(buffer, agent, augmenter, batch_size):
    """percentage of a uniform batch the binary advantage filter accepts (learning_utils.py:217-238)."""
    rd = sample_move_and_augment(buffer=buffer, batch_size=batch_size, augmenter=augmenter, aug_mix=0.0,
                                 per=False)
    o, a = rd["primary_batch"][0], rd["primary_batch"][1]
    member = rng.choice(range(agent.ensemble_size))
    res = agent.adv_estimator.evaluate(o, a, member, want=("mask",))
    return float(res["mask"].sum() / res["mask"].numel() * 100.0)
