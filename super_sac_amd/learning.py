"""The three update functions of the reference's training loop, same names and keyword
arguments (super_sac/learning.py:18-141 critic_update, :344-421 online_actor_update,
:222-263 alpha_update; call sites main.py:380-405, :492-510, :529-542).

What changes underneath: the per-critic Python loop + autograd + per-parameter Adam of the
reference become ensemble-batched HIP launches -- forward of all N critics in three launches,
hand-derived backward, and weight-gradient GEMMs whose epilogue is the Adam step -- and the
logs stay on the device until somebody reads them.
"""
import collections
import ctypes as C
import functools
import operator
import os
import struct
import types

import numpy as np
import torch

from . import adv_estimator, beta, encoder_base, engine, parallel, rng
from . import learning_utils as lu
from . import _lib
from ._lib import check, lib


# how a repeated update is re-issued: "list" = the library's recorded launch list (ssac_replay), "graph" = a
# hipGraph captured through torch.cuda.graph (leaves a ~13 us idle tail per launch on MI355X)
LAUNCH_MODE = os.environ.get("SSAC_LAUNCH_MODE", "list")


class _LaunchList:
    """recorded launch segments with host callables (collectives of the sharded update) between them"""

    def __init__(self):
        self.parts = []  # list handles (int) and callables, in issue order

    def add_list(self, handle):
        if not handle:
            raise RuntimeError("libssac_hip: " + lib.ssac_last_error().decode())
        if lib.ssac_launch_list_size(handle) > 0:
            self.parts.append(handle)
        else:
            lib.ssac_launch_list_free(handle)

    def replay(self):
        st = engine.stream()
        for part in self.parts:
            if callable(part):
                part()
            else:
                check(lib.ssac_replay(part, st))

    def __del__(self):
        for part in self.parts:
            if not callable(part):
                try:
                    lib.ssac_launch_list_free(part)
                except Exception:
                    pass


FUSED_ACTOR = True  # the online actor update in four fused launches
# ... of which the first three are ONE (ssac_actor_chain_fused: actor forward / critics' forward + dQ/da / actor backward as
# producer and consumer workgroups of a single launch).  Module constant; tests/test_hip_cases.py flips it for the A/B.
ACTOR_CHAIN = True
FEED_SLOTS = 32  # pinned input ring of a captured update: how far the host may run ahead of the GPU
# evaluate the TD target inside the critic launch instead of a launch of its own (continuous, no PopArt)
SHARDED_LISTS = True  # recorded launch lists on critic-sharded ranks
FOLD_BEGIN = True  # fold ssac_begin_update into the replay gather
# Log finalisation inside the weight-gradient launch: the last workgroup to ARRIVE (a device-scope ticket drawn after
# its write-through partial stores -- no fence, so none of the 17 MB of freshly written Adam state is flushed) sums the
# partials and publishes the log block; the separate 1-workgroup logs launch (~5 us per update) disappears.
FOLD_LOGS = True
LAZY_TD = True
# Run the online critics' forward as a parallel branch beside the actor -> target critics -> TD-target chain.
# Off by default: on MI355X a cross-stream join costs ~10 us of signalling (measured, also inside a HIP graph),
# more than the overlap wins at the metric shape (6.6k vs 7.15k updates/s); tests exercise both settings.
SPLIT_FORWARD = False


# the TD-independent half of the critics' backward pass inside the target-critic launch (rank-1 loss gradient); a module
# knob, not an environment switch: tests turn it off to compare against the launch forms other configurations take
RANK1_BWD = True
SKIP_DZ2 = True  # dz2u stays inside the chained launch (rebuilt from h2 by the weight gradient)
EVENT_EVERY = 8  # must divide FEED_SLOTS
FOLD_LOSS = True  # rank-1 backward: dL/dq evaluated inside the weight-gradient launch
DUAL_LAUNCH = True  # critic forward inside the actor-sample launch


DUAL_MAX_WG = 320


def _dual_fits(arena, n_rows):
    """worth merging while the actor's tiles (16 rows) and the critic forward's (32 rows at this size) are about one
    round of workgroups (one per CU; a few more still pay for themselves because the merged path also carries the
    replay gather, the rank-1 backward and the folded loss gradient: Humanoid N 16 at B 512 = 288 workgroups, +4 %)"""
    return (n_rows + 15) // 16 + arena.n_nets * ((n_rows + 31) // 32) <= DUAL_MAX_WG


def _split_forward(n_nets, n_rows):
    """the branch pays off while the critic forward leaves CUs free for the small actor / target launches
    it runs beside: one 32-row workgroup per CU, at most 192 of the 256 CUs."""
    return SPLIT_FORWARD and n_nets * ((n_rows + 31) // 32) <= 192


def _clip_and_step(adam, members, clip, slot_norm, member_shard=None, joint_ss=None):
    """clip_grad_norm_ over ALL listed arenas jointly, then Adam from the stored gradients
    (learning.py:122-130 / :413-416).  members: list of (arena, key, grads, sumsq).  member_shard: the joint norm runs
    over the members of EVERY rank (one SUM all-reduce of this rank's squared norm).  joint_ss: the members' sumsq
    buffers as ONE tensor they are views of, in member order (recordable ensemble updates: no concatenation between the
    launches)."""
    st = engine.stream()
    if joint_ss is not None:
        allss = joint_ss
    else:
        allss = members[0][3] if len(members) == 1 else torch.cat([m[3] for m in members])
    if member_shard is not None:
        allss = allss.sum().reshape(1)   # (device plumbing: one scalar to exchange)
        parallel.all_reduce_sum(allss)
    check(lib.ssac_clip_coef(adam.ctl.ptr, allss.data_ptr(), allss.numel(), float(clip), 0, st))
    for arena, key, grads, _ in members:
        m, v = adam.moments_for(key, arena.params)
        check(lib.ssac_adam_step(arena.params.data_ptr(), m.data_ptr(), v.data_ptr(), grads.data_ptr(),
                                 arena.params.numel(), adam.ctl.ptr, st))
        if arena.shadow is not None:
            arena.sync_shadow()   # bf16 mode: the operand copies follow the freshly stepped masters


def _encoder_step(encoder, encoder_optimizer, encoder_clip, dX, emb, ws, slot, dev, inv=None, accumulate=False,
                  step=True):
    """encoder backward from the critics' input gradients + clip + encoder_optimizer.step()
    (learning.py:121,127-129); logs the (clipped) encoder gradient norm (learning.py:137).
    inv = (as_rep, os_rep, encoder_lambda, stacked): the encoder invariance constraint (learning.py:114-117) adds
    lambda * d||as_rep - os_rep||_F / d as_rep -- to the critics' rows when the augmented batch IS the critic batch,
    to rows [B, 2B) of a stacked pass otherwise."""
    eng = encoder_base.encoder_engine(encoder, dev)
    B = dX.shape[1]
    stacked = inv is not None and inv[3]
    d_rep = ws.get("cu.drep2" if stacked else "cu.drep", (2 * B if stacked else B, emb))
    torch.sum(dX[:, :, :emb], dim=0, out=d_rep[:B])  # device plumbing: sum of N small slices
    if inv is not None:
        as_rep, os_rep, lam, _ = inv
        tgt = d_rep[B:] if stacked else d_rep[:B]
        check(lib.ssac_frobenius_diff_bwd(as_rep.data_ptr(), lu._row_stride(as_rep), os_rep.data_ptr(),
                                          lu._row_stride(os_rep), B, emb, float(lam), tgt.data_ptr(), emb,
                                          0 if stacked else 1, slot[lu.L_ENC_INV:].data_ptr(),
                                          slot[lu.L_CRITIC_LOSS:].data_ptr(), engine.stream()))
    # ensemble members share the encoder: member i > 0 adds its gradient to the arena, the clip + optimizer step
    # follows the last member (learning.py:47-130: one backward over the summed loss, one encoder_optimizer.step())
    eng.backward(d_rep, accumulate=accumulate)
    if step:
        eng.optimizer_step(encoder_optimizer, encoder_clip, norm_out=slot[lu.L_ENC_GN:])


USE_GRAPHS = True   # replay the critic update's launch sequence as one HIP graph when it is static
GRAPH_WARMUP = 3    # eager calls before capture (workspace allocation, arena binding, kernel attributes)


class _SlotLayout(collections.namedtuple(
        "_SlotLayout", "B n_sub n_pad ids_off logslot_off draw_off nbytes slot_words logslot_word")):
    """byte layout of one slot of a recorded critic update's input ring, from (B, n_sub):
        [B int64 replay indices | n_pad int32 subset ids | int32 log-ring slot, int32 pad | int64 noise draw number]
    n_pad = n_sub rounded up to 8 bytes; ids_off, logslot_off, draw_off = where the last three start; nbytes = the slot
    rounded up to whole 16-byte words (ssac_feed contract); slot_words, logslot_word = nbytes and logslot_off in the
    4-byte words ssac_feed counts in; aux_off = the pad word, which carries the bits of one float per update (the
    exploration process's scale, ssac_step_run_aux; zero otherwise).  The ONE place that knows it: the staging and device views, ssac_feed, the capture's
    draw-number address and ssac_step_create all read these fields (tests/test_critic_recording_cpu.py holds them to
    ssac_step_create's geometry check)."""
    __slots__ = ()

    def __new__(cls, B, n_sub):
        n_pad = (n_sub + 1) // 2 * 2
        logslot_off = 8 * B + 4 * n_pad
        nbytes = (logslot_off + 16 + 15) // 16 * 16
        return super().__new__(cls, B, n_sub, n_pad, 8 * B, logslot_off, logslot_off + 8, nbytes, nbytes // 4, logslot_off // 4)

    @property
    def aux_off(self):
        return self.logslot_off + 4

    def host_views(self, stage):
        """of a (slots, nbytes) uint8 numpy array: indices (slots, B) int64, [ids..., log slot at [n_pad], aux word at
        [n_pad + 1]] (slots, n_pad + 2) int32, draw number (slots, 1) int64"""
        return (stage[:, :self.ids_off].view(np.int64), stage[:, self.ids_off:self.draw_off].view(np.int32),
                stage[:, self.draw_off:self.draw_off + 8].view(np.int64))


class _FeedRing:
    """the input ring of a recorded update (ssac_feed_ring_alloc): device-resident on large-BAR systems"""

    def __init__(self, nbytes):
        p, d = C.c_void_p(), C.c_int()
        check(lib.ssac_feed_ring_alloc(nbytes, C.byref(p), C.byref(d)))
        self.ptr, self.device_resident = p.value, bool(d.value)

    def __del__(self):
        try:
            lib.ssac_feed_ring_free(self.ptr, int(self.device_resident))
        except Exception:
            pass


class _RecordedCritic:
    """one recorded critic update of an agent (agent.__dict__["_ssac_graphs"][key]), every field it ever holds.
    The call: refs pins the objects whose ids are in the key (buffer, target agent, critic optimizer, log_alpha, the
    exploration process or None).
    The inputs, made once by prepare() (feed is None before) -- what follows from the call and the agent: dev, log_ring
    (the device's LogRing), shard and n_critics (the GLOBAL ensemble); and the fixed addresses: layout (_SlotLayout); inbuf, the device block
    the first launch pulls a slot into, with its views idx_dev / ids_dev; stage, the host copy of the ring the slots are
    composed in, with np_idx / np_i32 / np_draw; ring (_FeedRing); feed (the ssac_feed struct on the device); and what
    the call's verdict (learning_utils.recording_verdict) asks for: n_members (E under verdict.members, else 1); eps_dev
    (injected noise of the first member's head, stochastic actors; else None); proc_dev and scale_ptr (verdict.explore:
    the process's injected noise, and the device address of the slot mirror's aux word, where ssac_explore_action reads
    its scale; else None and 0); refresh (verdict.refresh) and cand_dev (the candidates' injected noise, (N_SAMPLES * B,
    A) sample-major: a refresh on a tanh-normal policy; else None); fill (per member the buffers _host_inputs refills
    under injected noise, (before, after) its subset draw: lu.recording_noise_buffers, one eps buffer per member);
    logblk (the log block the launches write); late_word (late-bound Polyak decision word, or None).
    What a recording produced, dropped by drop_recording() (graph is None: nothing recorded): graph (_LaunchList or
    CUDAGraph), dicts (the replay dicts handed back), members (the MemberUpdate records a replay reads), log_index
    ({log key: word of logblk}), log_views ({ring slot: {log key: 0-dim view}}), in_kernel_noise (the noise source it was
    recorded with), deferred (its ssac_deferred_logs, None: logs finalised at once), late_arenas ((target, online) arenas
    of the late-bound Polyak, or None), td_stats.
    Progress: fast (the _FastStep over the recording's launch lists; None: not built, retired because a parameter moved, or
    dropped with its recording), calls (critic_update calls with this key, warm-up included), k (updates issued on the ring, by either
    replayer), path ("fast": the C step issued the last one, "slow": Python did), pending (log-ring slot of the newest
    update whose block has not been written yet, deferred logs only), events (slot-reuse events of the Python path), pick
    (the member learning.py:135 picked for the update about to be issued: an ensemble's aux word)."""
    __slots__ = ("refs", "dev", "log_ring", "shard", "n_critics",
                 "layout", "inbuf", "idx_dev", "ids_dev", "stage", "np_idx", "np_i32", "np_draw", "ring", "feed", "eps_dev",
                 "proc_dev", "scale_ptr", "refresh", "cand_dev", "fill", "logblk", "late_word",
                 "graph", "dicts", "members", "log_index", "log_views", "in_kernel_noise", "deferred", "late_arenas",
                 "td_stats", "fast",
                 "calls", "k", "path", "pending", "events", "n_members", "pick")

    def __init__(self, refs):
        for f in self.__slots__:
            setattr(self, f, None)
        self.refs = refs
        self.members, self.log_views, self.in_kernel_noise = [], {}, False
        self.calls, self.k, self.path = 0, 0, "slow"
        self.n_members, self.pick = 1, 0

    def prepare(self, agent, B, n_sub, verdict):
        """One fixed device block holds the per-update inputs (_SlotLayout).  The host writes them into slot k % FEED_SLOTS
        of the input ring; the first recorded launch pulls the slot in (ssac_feed in include/ssac_hip.h), so an update is
        ONE graph launch and no copy node.  verdict.members, E > 1: the layout of (E B, E n_sub) holds every member's index
        draw and subset member-major -- B and n_sub below are the slot's."""
        E = self.n_members = agent.ensemble_size if verdict.members else 1
        explore, refresh = verdict.explore, verdict.refresh
        rows = B
        B, n_sub = E * B, E * n_sub
        dev = self.dev = self.refs[3].device
        self.log_ring = lu.ring_for(dev)
        self.shard = parallel.shard_of(agent)
        self.n_critics = agent.num_critics if self.shard is None else self.shard.num_critics
        lay = self.layout = _SlotLayout(B, n_sub)
        self.inbuf = torch.zeros(lay.nbytes, dtype=torch.uint8, device=dev)
        self.idx_dev = self.inbuf[:lay.ids_off].view(torch.int64)
        self.ids_dev = self.inbuf[lay.ids_off:lay.logslot_off].view(torch.int32)[:n_sub]
        # the slots are composed in ordinary host memory (numpy views: a fraction of the cost of torch indexing) and
        # copied into the input ring with ONE ssac_feed_write each; the ring itself is uncached device memory the
        # host stores into over the PCIe BAR when the system allows it, pinned host memory otherwise
        self.stage = np.zeros((FEED_SLOTS, lay.nbytes), np.uint8)
        self.np_idx, self.np_i32, self.np_draw = lay.host_views(self.stage)
        self.ring = _FeedRing(FEED_SLOTS * lay.nbytes)
        self.events = [None] * (FEED_SLOTS // EVENT_EVERY)
        actor = agent.actors[0]
        kind = lu.actor_kind(actor)
        eps = [torch.empty(rows, actor.action_size, device=dev) if kind == "stochastic" else None for _ in range(E)]
        self.eps_dev = eps[0]
        # an exploration process inside the update (TD3 / DDPG / AWAC): its noise, and where its scale arrives
        self.proc_dev = torch.empty(B, actor.action_size, device=dev) if explore else None
        self.scale_ptr = self.inbuf.data_ptr() + lay.aux_off if explore else 0
        # a priority refresh inside the update (AWAC / AFBC): the candidates' noise, one block of B rows per sample
        self.refresh = refresh
        n_cand = adv_estimator.N_SAMPLES
        self.cand_dev = (torch.empty(n_cand * B, actor.action_size, device=dev)
                         if refresh and kind == "stochastic" else None)
        named = {"proc": self.proc_dev}
        if self.cand_dev is not None:
            named.update({f"cand{k}": self.cand_dev[k * B:(k + 1) * B] for k in range(n_cand)})
        before, after = lu.recording_noise_buffers(kind, explore, refresh, False)
        self.fill = tuple(([dict(named, eps=e)[n_] for n_ in before], [named[n_] for n_ in after]) for e in eps)
        self.logblk = torch.zeros(lu.LOG_WIDTH, device=dev)
        # late-bound Polyak (include/ssac_hip.h): the decision word the update's first launch writes
        self.late_word = torch.zeros(4, dtype=torch.int32, device=dev) if lu.LATE_POLYAK else None
        self.feed = engine.DeviceStruct(_lib.Feed(self.ring.ptr, self.inbuf.data_ptr(), self.log_ring.buf.data_ptr(), 0,
                                                  FEED_SLOTS, lay.slot_words, lay.logslot_word, lu.LOG_WIDTH,
                                                  self.late_word.data_ptr() if self.late_word is not None else 0), dev)

    def drop_recording(self):
        """record again (a noise hook was installed or removed since): forget what the recording produced, the C step
        that borrows its launch lists included; the inputs and the progress stay.  The retired step stays in
        agent.__dict__["_ssac_fast"] until the next one takes its key: _FastStep.still_valid's `gs.fast is not self` is what
        keeps it from running over the freed lists."""
        lu.flush_pending_logs(self)  # (while the old recording's device structs are alive)
        self.graph = self.dicts = self.log_index = self.deferred = self.late_arenas = self.td_stats = self.fast = None
        self.members, self.log_views, self.in_kernel_noise = [], {}, False

    def views(self, slot_i):
        """log values of log-ring slot slot_i (built once per slot)"""
        v = self.log_views.get(slot_i)
        if v is None:
            if self.deferred is not None:
                v = lu.lazy_views(self, self.log_ring, slot_i, self.log_index)
            else:
                blk = self.log_ring.buf[slot_i]
                v = {k_: blk[i] for k_, i in self.log_index.items()}
            self.log_views[slot_i] = v
        return v


def critic_update(buffer, agent, target_agent, critic_optimizer, encoder_optimizer, log_alphas,
                  batch_size, gamma, critic_clip, encoder_clip, target_critic_ensemble_n,
                  weighted_bellman_temp, weight_type, pop, augmenter, encoder_lambda, random_process,
                  noise_clip, aug_mix=0.75, discrete=False, per=False, update_priorities=False,
                  dr3_coeff=0.0):
    """learning.py:18-141.  When the launch sequence is static (one ensemble member -- or several under
    learning_utils.members_recordable, DESIGN.md 7f --, vector
    observations, uniform sampling, single rank) it is captured once into a HIP graph and replayed:
    the host then only draws the indices / REDQ subset / noise, uploads them into fixed-address
    buffers and issues one graph launch, instead of ~15 kernel launches."""
    kw = dict(locals())   # (first statement: exactly the arguments)
    # ---- fast path: this exact call has been recorded already (ssac_step: one C call re-issues the update)
    fast = agent.__dict__.get("_ssac_fast")
    if fast is not None and USE_GRAPHS and engine.CAPTURE is None:
        fs = fast.get(_fast_key(kw))
        if fs is not None and fs.still_valid():
            return fs.run()
    lu.ensure_adopted(agent, buffer)
    lu.ensure_adopted(target_agent, buffer)
    encoder_base.refuse_unsupported(agent, "critic_update", encoder_lambda=encoder_lambda)
    shard = parallel.shard_of(agent)
    is_beta = lu.actor_kind(agent.actors[0]) == "beta"
    if is_beta and (shard is not None or parallel.member_shard_of(agent) is not None):
        beta.refuse("critic_update on a critic- or member-sharded agent")
    verdict = _verdict_of(kw)
    if not verdict.record:
        return _critic_update_eager(_verdict=verdict, **kw)
    key = (id(buffer), id(target_agent), id(critic_optimizer), batch_size, float(gamma), critic_clip,
           target_critic_ensemble_n, bool(pop), bool(discrete), id(log_alphas[0]), engine.USE_FUSED,
           id(random_process), noise_clip,   # (noise_clip is baked into the recorded argument bytes)
           bool(update_priorities))          # (the two call forms of an AFBC loop keep one recording each)
    if verdict.members:
        key += (weight_type, weighted_bellman_temp)   # (an ensemble's backup weights are part of the recorded launches)
    cache = agent.__dict__.setdefault("_ssac_graphs", {})  # lives and dies with the agent
    gs = cache.get(key)
    if gs is None:
        # the key's ids, pinned
        gs = cache[key] = _RecordedCritic((buffer, target_agent, critic_optimizer, log_alphas[0], random_process))
    gs.calls += 1
    if gs.calls <= GRAPH_WARMUP or len(buffer) < batch_size:
        return _critic_update_eager(_verdict=verdict, **kw)
    return _critic_update_graphed(gs, kw, verdict)


def _verdict_of(kw):
    """what a critic_update(**kw) call may record, decided once per call (learning_utils.recording_verdict)"""
    return lu.recording_verdict(lu.call_facts(kw, LAUNCH_MODE, USE_GRAPHS, SHARDED_LISTS))


_fast_values = operator.itemgetter("batch_size", "gamma", "critic_clip", "encoder_clip", "target_critic_ensemble_n",
                                   "weighted_bellman_temp", "weight_type", "pop", "encoder_lambda", "noise_clip", "discrete",
                                   "per", "update_priorities", "dr3_coeff")


def _fast_key(kw):   # what identifies a recorded call critic_update(**kw) among its agent's recordings
    return (id(kw["buffer"]), id(kw["target_agent"]), id(kw["critic_optimizer"]), id(kw["log_alphas"][0]),
            id(kw["augmenter"]), id(kw["random_process"]), engine.USE_FUSED) + _fast_values(kw)


def _slot_codes(row, ids, shard):
    # sharded: the LOCAL index of a subset member this rank owns, -(owner rank + 1) for one that lives elsewhere
    for j, v in enumerate(ids):
        row[j] = v if shard is None else shard.slot_code(v)


def _host_inputs(gs, buffer, agent, in_kernel_noise):
    """what the host contributes to one recorded update, whoever re-issues it: every host-RNG draw of the update in the
    reference's order -- per member its indices -> (augmentation: none here) -> its injected noise -> its REDQ subset of
    the GLOBAL ensemble, into the member's block of the slot; behind the last member the one whose gradient norm is logged
    (learning.py:135: gs.pick, an ensemble's aux word) and a refresh's member pick --, the update's log-ring slot, a sharded
    rank's exchange check, the draw number of the agent's noise stream (one draw per member step, as eager)"""
    lay, E = gs.layout, gs.n_members
    B, n = lay.B // E, lay.n_sub // E
    if gs.refresh:
        # the recorded ssac_per_assign checks priority > 0 on the device: what the last update found is raised now
        buffer._per._raise_pending()
    rows, ids = [], []
    for i in range(E):
        before, after = ((), ()) if in_kernel_noise else gs.fill[i]
        buffer.total_sample_calls += 1
        rows.append(rng.draw_indices(len(buffer), B))
        for buf in before:
            # injected noise (parity tests) goes straight into the update's input buffers: the head's eps, behind it the
            # exploration process's (learning_utils.py:331-335)
            rng.draw_normal_into(buf)
        ids += rng.draw_subset(gs.n_critics, n)
        for buf in after:
            rng.draw_normal_into(buf)  # ... and the estimator's candidates of a priority refresh (adv_estimator.py:58-79)
    idx_cpu = rows[0] if E == 1 else torch.cat(rows)
    pick = rng.choice(agent.critics)  # learning.py:135
    gs.pick = 0 if E == 1 else next(j for j, c_ in enumerate(agent.critics) if c_ is pick)
    if gs.refresh:
        rng.choice(range(agent.ensemble_size))  # the refresh's member pick (learning_utils.py:289)
    slot_i = gs.log_ring.advance()
    if gs.shard is not None and gs.k % EVENT_EVERY == 0:
        parallel.check_exchange()
    draw = 0
    if in_kernel_noise:
        ns = lu.noise_stream(agent, gs.dev)
        draw = ns[1]
        ns[1] += E
    return idx_cpu, ids, slot_i, draw


def _in_kernel_noise(gs, agent):
    """does a recording of gs draw its action noise inside its launches (the agent's Philox stream)?  The TD plan's noise
    source (learning_utils.td_member_plan) on the recording's facts: the fused actor-sample launch does (wide action heads
    take the per-layer path), and so does the head + process launch (ssac_explore_action), whatever the actor's arena
    looks like -- a recorded call carries a process exactly when its verdict said explore (gs.proc_dev)."""
    actor, explore = agent.actors[0], gs.proc_dev is not None
    kind = lu.actor_kind(actor)
    fused = kind == "stochastic" and not explore and engine.bind_arena(actor, "self", [actor], gs.dev).fused
    return lu.td_member_plan(kind, explore, explore, fused, True).noise == "kernel"


def _aux_word(gs, kw):
    """the slot's aux word of the update about to be issued: the member whose gradient norm is logged (gs.pick) for an
    ensemble, which carries no process (the gate); the process's scale NOW (the acting loop anneals it), as the int32
    with the float's bits, for a recording with a process; 0 otherwise"""
    if gs.n_members > 1:
        return gs.pick
    if gs.proc_dev is None:
        return 0
    return struct.unpack("<i", struct.pack("<f", float(kw["random_process"].current_scale)))[0]


def _close_update(gs, agent, idx_cpu, ids, slot_i):
    """the update has been issued: count it, hand every member's replay dict its rows and subset, hand out this slot's
    log views.  Draws nothing (_host_inputs has made the update's picks)."""
    gs.k += 1
    if gs.deferred is not None:
        gs.pending = slot_i   # (the previous update's block is written by the launch just issued)
    E = gs.n_members
    B, n = gs.layout.B // E, gs.layout.n_sub // E
    idx_np = idx_cpu.numpy()
    for i, rd in enumerate(gs.dicts):
        rd["priority_idxs"] = idx_np[i * B:(i + 1) * B]
        rd["_subset"] = ids[i * n:(i + 1) * n]
    return dict(gs.views(slot_i)), gs.dicts


def _flush_other_recordings(agent, keep=None):
    """Deferred log finalisation keeps update k's partials in name-keyed workspace tensors of the AGENT until the next
    update of the same recording writes the block.  Any other critic update on the agent (an eager call, a second
    recording, a re-recording) would overwrite them first: finalise the pending block now."""
    for g in agent.__dict__.get("_ssac_graphs", {}).values():
        if g is not keep and g.pending is not None:
            lu.flush_pending_logs(g)


class _FastStep:
    """the recorded critic update behind ONE C call per update (ssac_step_run, include/ssac_hip.h): what stays in
    Python is _host_inputs and _close_update; the C step composes the slot, keeps the slot-reuse events and re-issues
    the launch lists.  Built over a recording whose lists have no host callable between them."""

    def __init__(self, gs, kw):
        self.gs, self.kw = gs, kw
        self.buffer, self.agent = kw["buffer"], kw["agent"]
        lay = gs.layout
        self.B = lay.B // gs.n_members
        h = lib.ssac_step_create(gs.ring.ptr, FEED_SLOTS, lay.nbytes, lay.B, lay.n_sub, lay.ids_off, lay.logslot_off,
                                 lay.draw_off, EVENT_EVERY)
        if not h:
            raise RuntimeError("libssac_hip: " + lib.ssac_last_error().decode())
        self.handle = h
        for part in gs.graph.parts:
            check(lib.ssac_step_add_list(h, part))
        self.ids_c = (C.c_int32 * max(lay.n_sub, 1))()
        self.in_kernel_noise = gs.in_kernel_noise
        self.late_arenas = gs.late_arenas   # (target arena, online arena) of the late-bound Polyak
        self.calls = 0
        # a few parameter addresses checked on every call (cheap), all of them every 256 calls
        tgt = kw["target_agent"]
        self.arenas = []
        for i in range(gs.n_members):   # (every member's arenas: an ensemble update launches on all of them)
            actor = self.agent.actors[i]
            self.arenas += [(self.agent.critics[i].arena(gs.dev), list(self.agent.critics[i].nets)),
                            (tgt.critics[i].arena(gs.dev), list(tgt.critics[i].nets)),
                            (engine.bind_arena(actor, "self", [actor], gs.dev), [actor])]
        self.probes = []
        for arena, mods in self.arenas:
            lins = engine.MlpArena.linear_triples(mods[0]) + engine.MlpArena.linear_triples(mods[-1])
            for lin in (lins[0], lins[-1]):
                self.probes.append((lin.weight, lin.weight.data_ptr()))
        # the log views of every ring slot, built now (~7 ms, once): built on a slot's first visit they cost the first
        # 512 replayed updates ~11 us of host time each -- 30 us per step instead of 17, enough to starve the device in
        # short bursts right after recording (tools/burst_parts.py)
        for slot_i in range(gs.log_ring.buf.shape[0]):
            gs.views(slot_i)

    def still_valid(self):
        gs = self.gs
        if gs.fast is not self or LAUNCH_MODE != "list" or len(self.buffer) < self.B:
            return False
        if (gs.eps_dev is not None or gs.proc_dev is not None) and rng.normal_is_stock() != self.in_kernel_noise:
            return False  # a noise hook was installed / removed: the slow path records the update again
        self.calls += 1
        if self.calls & 255 == 0:
            if not all(arena.is_bound(mods) for arena, mods in self.arenas):
                gs.fast = None
                return False
        else:
            for p, ptr in self.probes:
                if p.data_ptr() != ptr:
                    gs.fast = None
                    return False
        return True

    def run(self):
        gs, agent = self.gs, self.agent
        if gs.path != "fast":
            # the Python path issued updates of this recording since: line the step up with the ring's device counter
            # (its slot-reuse events know nothing about those updates, so let them finish first)
            torch.cuda.synchronize()
            check(lib.ssac_step_seek(self.handle, gs.k))
            gs.path = "fast"
        if len(agent.__dict__["_ssac_graphs"]) > 1:
            _flush_other_recordings(agent, keep=gs)
        idx_cpu, ids, slot_i, draw = _host_inputs(gs, self.buffer, agent, self.in_kernel_noise)
        _slot_codes(self.ids_c, ids, gs.shard)
        if gs.proc_dev is None and gs.n_members == 1:
            check(lib.ssac_step_run(self.handle, idx_cpu.data_ptr(), self.ids_c, slot_i, draw, engine.stream()))
        else:
            check(lib.ssac_step_run_aux(self.handle, idx_cpu.data_ptr(), self.ids_c, slot_i, _aux_word(gs, self.kw), draw,
                                        engine.stream()))
        if self.late_arenas is not None:
            agent.critics[0].__dict__["_ssac_last_step"] = self   # a soft_update that follows needs no launch
        return _close_update(gs, agent, idx_cpu, ids, slot_i)

    def __del__(self):
        try:
            lib.ssac_step_destroy(self.handle)
        except Exception:
            pass


def _critic_update_graphed(gs, kw, verdict):
    """one update of a recording from Python: the recording call itself, the hipGraph mode, lists with a collective
    between segments, and whatever the C step (_FastStep) does not serve"""
    buffer, agent = kw["buffer"], kw["agent"]
    agent.critics[0].__dict__.pop("_ssac_last_step", None)
    if gs.path == "fast":  # (the C step's slot-reuse events are not visible from here)
        torch.cuda.synchronize()
        gs.path = "slow"
    if gs.feed is None:
        gs.prepare(agent, kw["batch_size"], kw["target_critic_ensemble_n"], verdict)
    in_kernel_noise = _in_kernel_noise(gs, agent)
    if gs.graph is not None and gs.in_kernel_noise != in_kernel_noise:
        gs.drop_recording()
    _flush_other_recordings(agent, keep=gs if gs.graph is not None else None)
    idx_cpu, ids, slot_i, draw = _host_inputs(gs, buffer, agent, in_kernel_noise)
    _write_slot(gs, idx_cpu, ids, slot_i, draw, _aux_word(gs, kw))
    if gs.graph is None:
        _record(gs, kw, verdict, idx_cpu, ids, in_kernel_noise)   # (the launches run now AND are recorded)
    else:
        gs.graph.replay()  # ONE host call re-issues the whole update
    _mark_group(gs)
    out = _close_update(gs, agent, idx_cpu, ids, slot_i)
    if gs.fast is None and LAUNCH_MODE == "list" and all(not callable(p_) for p_ in gs.graph.parts):
        gs.fast = agent.__dict__.setdefault("_ssac_fast", {})[_fast_key(kw)] = _FastStep(gs, kw)
    return out


def _write_slot(gs, idx_cpu, ids, slot_i, draw, aux=0):
    """the Python replayer's half of ssac_step_run(_aux), before the launches: update gs.k's inputs into its slot of the ring"""
    k = gs.k
    # slot reuse: the replay that read this slot FEED_SLOTS updates ago must have finished.  One event per group of
    # EVENT_EVERY updates (recorded after the group's last update; an event costs a barrier packet on the queue).  No
    # event: the C step issued that group, and the switch away from it synchronised the device.
    ev = gs.events[((k - FEED_SLOTS) // EVENT_EVERY) % len(gs.events)]
    if k % EVENT_EVERY == 0 and k >= FEED_SLOTS and ev is not None:
        ev.synchronize()
    s, nbytes = k % FEED_SLOTS, gs.layout.nbytes
    gs.np_idx[s] = idx_cpu.numpy()
    row = gs.np_i32[s]
    _slot_codes(row, ids, gs.shard)
    row[gs.layout.n_pad] = slot_i
    row[gs.layout.n_pad + 1] = aux
    gs.np_draw[s, 0] = draw
    check(lib.ssac_feed_write(gs.ring.ptr + s * nbytes, gs.stage.ctypes.data + s * nbytes, nbytes))


def _mark_group(gs):
    """... and behind them: the event of a group of EVENT_EVERY updates follows its last update"""
    if gs.k % EVENT_EVERY == EVENT_EVERY - 1:
        gi = (gs.k // EVENT_EVERY) % len(gs.events)
        if gs.events[gi] is None:
            gs.events[gi] = torch.cuda.Event()
        gs.events[gi].record()


def _record(gs, kw, verdict, idx_cpu, ids, in_kernel_noise):
    """run the update once with its launches recorded (a launch list, cut into segments around the collectives of a
    sharded rank, or a hipGraph) against the record's fixed-address inputs, and fill in what the recording produced"""
    buffer, agent, B, dev = kw["buffer"], kw["agent"], kw["batch_size"], gs.dev
    kind = lu.actor_kind(agent.actors[0])
    gs.in_kernel_noise = in_kernel_noise
    # (the injected noise buffers in the reference's draw order: member by member the head's eps, then the process's noise)
    normals = [buf for before, _ in gs.fill for buf in before]
    ctx = engine.CaptureCtx(idx_cpu, gs.idx_dev, ids, gs.ids_dev, [] if in_kernel_noise else normals,
                            gs.logblk, feed=gs.feed.ptr)
    if gs.n_members > 1:
        E_ = gs.n_members
        ctx.members = (E_, gs.layout.B // E_, gs.layout.n_sub // E_)
        ctx.pick_ptr = gs.inbuf.data_ptr() + gs.layout.aux_off
    ctx.scale_ptr = gs.scale_ptr
    ctx.cand = None if in_kernel_noise else gs.cand_dev
    if in_kernel_noise:
        ctx.tick_ptr = gs.inbuf.data_ptr() + gs.layout.draw_off
        ctx.noise_offset = 0
    st_ = buffer._storage
    keys_ = list(st_.s_stack.keys())
    # vector observations in one array: the whole-transition gather is the update's first launch and takes
    # over ssac_begin_update's work (ensemble_size 1: a single gather per update)
    # (... or several vector arrays gathered side by side for a concatenating encoder: ssac_gather_concat_begin)
    ctx.defer_begin = (FOLD_BEGIN and agent.ensemble_size == 1
                       and ((len(keys_) == 1 and st_.s_stack[keys_[0]].dim() == 2) or lu.concat_order(st_) is not None))
    c_arena_ = agent.critics[0].arena(dev)
    if (lu.DEFERRED_LOGS and LAUNCH_MODE == "list" and FOLD_LOGS and _loss_folds(B) and LAZY_TD and ctx.defer_begin
            and not kw["critic_clip"] and kind == "stochastic" and not any(agent.popart) and c_arena_.out_dim == 1):
        # deferred log finalisation (csrc/ssac_critic_logs.h): the buffers the weight-gradient launch will leave
        # its partials in are workspace tensors with fixed names, so the struct can be built before the body runs
        ws_ = lu.agent_ws(agent, dev)
        # ... and they belong to THIS recording: the next update's first launch finishes the previous block from them
        # whether or not a flush has written it already, so an update of another call form in between (a second
        # recording of the agent -- update_priorities on and off in turn -- or an eager call) must not write over them
        ws_.scope = (f"@{id(gs):x}", ("cu.tdstats", "cu.c0.fparts", "cu.ss0"))
        N_ = c_arena_.n_nets
        ttot_ = (engine.bf16_tiles_total(c_arena_) if c_arena_.shadow is not None
                 else engine.wgrad_tiles_total(c_arena_))
        gs.td_stats = ws_.get("cu.tdstats", (4,), zero=True)
        ctx.deferred = _lib.DeferredLogs(
            ws_.get("cu.c0.fparts", (N_ * 2,)).data_ptr(), N_, N_ * ttot_, ws_.get("cu.ss0", (N_ * ttot_,)).data_ptr(),
            gs.td_stats.data_ptr(), lu.L_TD0, B, float(N_ if gs.shard is None else gs.n_critics), 0, gs.feed.ptr)
        t_arena_ = kw["target_agent"].critics[0].arena(dev)
        if (gs.late_word is not None and (c_arena_.shadow is None) == (t_arena_.shadow is None)
                and t_arena_.params.numel() == c_arena_.params.numel()):
            # late-bound Polyak: the weight-gradient launch carries the target arena and waits for the decision
            ctx.late = gs.late_word.data_ptr()
            ctx.late_target = t_arena_

    gs.members = []   # the members' records: what a replay reads lives as long as the recording

    def body():
        logs_, dicts_ = _critic_update_eager(_records=gs.members, _verdict=verdict, **kw)
        assert not ctx.pending_begin, "deferred ssac_begin_update was never issued"
        assert ctx.deferred_used == ctx.deferred_chain, "deferred log finalisation: chain / weight-gradient mismatch"
        gs.deferred = ctx.deferred if ctx.deferred_used else None
        gs.late_arenas = ((ctx.late_target, agent.critics[0].arena(dev))
                          if (ctx.deferred_used and ctx.late_used) else None)
        if not ctx.published:
            check(lib.ssac_publish_logs(gs.logblk.data_ptr(), gs.feed.ptr, engine.stream()))
        return logs_, dicts_
    engine.CAPTURE = ctx
    try:
        if LAUNCH_MODE == "graph":
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                logs, dicts = body()
            graph.replay()
        else:
            # launch list: this call's launches run normally AND are recorded for the later calls
            graph = _LaunchList()

            def collective(fn):
                graph.add_list(lib.ssac_record_end())
                fn()
                graph.parts.append(fn)
                check(lib.ssac_record_begin())
            ctx.collective = collective
            check(lib.ssac_record_begin())
            try:
                logs, dicts = body()
            finally:
                handle = lib.ssac_record_end()
            graph.add_list(handle)
    finally:
        engine.CAPTURE = None
        lu.agent_ws(agent, dev).scope = None
    gs.graph, gs.dicts = graph, dicts
    base = gs.logblk.data_ptr()
    gs.log_index = {k_: (v.data_ptr() - base) // 4 for k_, v in logs.items()}
    gs.log_views = {}   # the 0-dim views handed out as log values, built once per ring slot (gs.views)


def _loss_folds(n_rows):
    """may the weight-gradient launch that follows a rank-1 backward evaluate dL/dq itself (the loss-fold form)?"""
    return FOLD_LOSS and n_rows <= 4096   # the library's limit (include/ssac_hip.h, ssac_mlp_wgrad_all_lossfold: "n_rows <= 4096")


def _critic_update_eager(buffer, agent, target_agent, critic_optimizer, encoder_optimizer, log_alphas, batch_size, gamma,
                         critic_clip, encoder_clip, target_critic_ensemble_n, weighted_bellman_temp, weight_type, pop,
                         augmenter, encoder_lambda, random_process, noise_clip, aug_mix=0.75, discrete=False, per=False,
                         update_priorities=False, dr3_coeff=0.0, _records=None, _verdict=None):
    """the ensemble-level flow; _records (a list, the recording's) receives the members' MemberUpdate records; _verdict:
    critic_update's, made here when the call comes from elsewhere"""
    c = types.SimpleNamespace(**locals())   # the call: its arguments, and below what every member shares
    verdict = _verdict if _verdict is not None else _verdict_of(vars(c))
    engine.require_gpu()
    if engine.CAPTURE is None:
        agent.critics[0].__dict__.pop("_ssac_last_step", None)
        _flush_other_recordings(agent)
    E = c.E = agent.ensemble_size
    assert E <= lu.MAX_MEMBERS
    # member-sharded rank (parallel.MemberShard, SURVEY 8(e) "SUNRISE variant"): `agent` holds the members [ms.lo, ms.hi)
    # of an ensemble of E_glob; the loss is averaged over the GLOBAL ensemble, every member's host draws are made here
    ms = c.ms = parallel.member_shard_of(agent)
    E_glob = c.E_glob = E if ms is None else ms.ensemble_size
    if ms is not None:
        assert lu.is_identity(agent.encoder), "member sharding: a trainable encoder is shared by all members (not sharded)"
        assert not per and not update_priorities and not dr3_coeff, "member sharding covers the online critic update"
        assert weight_type in (None, "sunrise", "softmax"), f"unknown weight_type {weight_type!r}"
    dev = c.dev = log_alphas[0].device
    ws = c.ws = lu.agent_ws(agent, dev)
    adam = c.adam = engine.adam_group(critic_optimizer, dev)
    slot = c.slot = lu.log_block(dev, adam)  # one launch: clear the log block + advance the Adam step
    logs = c.logs = {}
    st = c.st = engine.stream()
    c.train_enc = not lu.is_identity(agent.encoder)
    # head + exploration process as one launch (recorded updates, and eager ones on the agent's Philox stream)
    c.explore = verdict.explore
    # An ensemble update that may be recorded takes ONE form in every call -- warm-up, recording, replay
    # and USE_GRAPHS = False alike: the members' gathers write into one stacked [s | a] batch, the backup weights and the
    # gradient-norm partials live in workspace tensors, the chained launch keeps its one-workgroup form and the picked
    # member's gradient norm is a launch of its own.
    c.members_form = verdict.members
    c.xstack = c.ss_all = None
    c.weights_on = weight_type is not None and weighted_bellman_temp is not None
    c.packed = False
    if c.members_form:
        st_ = buffer._storage
        S_ = next(iter(st_.s_stack.values())).shape[1]
        A_ = int(np.prod(st_.action_stack.shape[1:]))
        c.S = S_
        c.xstack = ws.get("cu.xstack", (E * batch_size, S_ + A_))
        c.pack_group = (lu.members_pack_group(target_agent, E, batch_size, dev)
                        if (c.weights_on and lu.PACKED_WEIGHTS) else 0)
        c.packed = c.pack_group > 0
    # Two passes over the ensemble members, as the reference's single backward at the end implies (learning.py:45-130):
    # every member's batch, TD target and backup weights are computed BEFORE any critic is updated -- the "softmax"
    # weights of member i look at the ONLINE critics of ALL members (learning_utils.py:383-393).
    members = [] if _records is None else _records
    all_rd = c.all_rd = []   # member-sharded ranks: every global member's batch, in member order
    # member-sharded "softmax" weights (round 5): every member's policy samples on EVERY member's batch, drawn in the
    # reference's order -- right behind that batch's TD draws -- by every rank; the table is completed after the loop
    ms_softmax = (ms is not None and weight_type == "softmax" and weighted_bellman_temp is not None and E_glob > 1)
    sm_table = c.sm_table = ws.get("bw.table", (E_glob, E_glob, batch_size)) if ms_softmax else None
    if ms_softmax:
        sm_table.zero_()   # [batch of member i][member k][row]
    for ig in range(E_glob):
        i = ig if ms is None else ms.local(ig)
        if i is not None:
            members.append(lu.MemberUpdate(i, ig, agent.critics[i].arena(dev)))
            _member_targets(members[-1], c)
        else:
            # a member another rank owns: its batch (this rank's target critics score it for the sunrise weights) and
            # its host draws, in the reference's order -- sample, action noise, REDQ subset
            rd = lu.sample_move_and_augment(buffer=buffer, batch_size=batch_size, augmenter=augmenter,
                                            aug_mix=aug_mix, per=per, _invariance=bool(encoder_lambda))
            lu.skip_td_draws(agent, agent.actors[0], batch_size, dev, target_agent.critics[0].arena(dev).n_nets,
                             target_critic_ensemble_n, random_process)
            if ms_softmax:
                lu.member_sharded_softmax_scores(rd, agent, target_agent, ms, sm_table[ig])
            all_rd.append(rd)
    if ms is not None and weight_type is not None and weighted_bellman_temp is not None and E_glob > 1:
        if ms_softmax:
            wts = lu.member_sharded_softmax_finish(logs, sm_table, ms, weighted_bellman_temp, slot)
        else:
            wts = lu.member_sharded_sunrise_weights(logs, all_rd, agent, target_agent, ms, weighted_bellman_temp, discrete, slot)
        for m in members:
            m.bw = wts[ms.lo + m.i]
    if c.packed:
        # every member's gather has left its rows in the stacked batch: all E weight vectors from three launches
        wts = lu.members_sunrise_weights(logs, c.xstack, c.S, agent, target_agent, weighted_bellman_temp, batch_size,
                                         discrete, slot, c.pack_group)
        for m in members:
            m.bw = wts[m.i]
    for m in members:
        _member_step(m, c)
        m.rd["td_target"] = m.td
    if critic_clip:
        _clip_and_step(adam, [(m.arena, ("critic", m.i), m.grads, m.ss) for m in members], critic_clip, None, ms,
                       joint_ss=c.ss_all.view(-1) if c.ss_all is not None else None)
    # encoder: identity encoders carry no trainable tensor on this path (their dummy Linear(1,1)
    # never receives a gradient, nets/__init__.py:24), so encoder_optimizer.step() is a no-op.
    logs["losses/last_member_critic_td_error"] = slot[lu.L_TD_ERR]
    logs["losses/critic_overall_loss"] = slot[lu.L_CRITIC_LOSS]
    if ms is not None:
        # learning.py:135 picks over the GLOBAL ensemble (the same Python draw on every rank); a rank that does not hold
        # the picked member logs the gradient norm of its first one
        k = ms.local(rng.choice(range(E_glob))) or 0
    else:
        pick = agent.critics[0] if engine.CAPTURE is not None else rng.choice(agent.critics)  # learning.py:135
        k = next(j for j, c_ in enumerate(agent.critics) if c_ is pick)
    ss_k = members[k].ss
    clip_ctl = adam.ctl.ptr if critic_clip else 0
    done_norm = logs_done_in_wgrad = any(m.logs_folded for m in members)
    for m in members:
        if m.log_parts is None or logs_done_in_wgrad:
            continue
        want = m.i == k and not c.members_form   # (a recordable ensemble update: the picked norm follows the loop)
        cap = engine.CAPTURE
        last = cap is not None and cap.feed and m is members[-1] and (done_norm or want)
        check(lib.ssac_critic_logs(m.log_parts.data_ptr(), m.log_nets, m.log_tiles, m.B, float(E_glob * m.n_glob),
                                   ss_k.data_ptr() if want else 0, ss_k.numel() if want else 0, clip_ctl, slot.data_ptr(),
                                   C.addressof(m.td_spec) if m.td_spec is not None else 0,
                                   m.td_logs.data_ptr() if m.td_spec is not None else 0, cap.feed if last else 0, st))
        if last:
            cap.published = True
        done_norm = done_norm or want
    if not done_norm and c.members_form and engine.CAPTURE is not None:
        # recorded: the pick of THIS update sits in the slot's aux word; the launch carries every member's buffer
        table = (C.c_void_p * E)(*[m.ss.data_ptr() for m in members])
        check(lib.ssac_group_norms_pick(table, E, engine.CAPTURE.pick_ptr, 1, ss_k.numel(), clip_ctl,
                                        slot[lu.L_CRITIC_GN:].data_ptr(), st))
    elif not done_norm:
        check(lib.ssac_group_norms(ss_k.data_ptr(), 1, ss_k.numel(), clip_ctl, slot[lu.L_CRITIC_GN:].data_ptr(), st))
    logs["gradients/critic_random_grad"] = slot[lu.L_CRITIC_GN]
    logs["gradients/encoder_criticloss_grad_norm"] = slot[lu.L_ENC_GN]
    if update_priorities:  # learning.py:139-140: advantage-based priorities on the LAST member's batch
        lu.adjust_priorities(logs, members[-1].rd, agent, buffer, _member=members[-1],
                             _recordable=verdict.refresh)
    return logs, [m.rd for m in members]


def _set_critic_input(m, c):
    """m.X, m.ldx for the online critics under an identity encoder: [s | a] (continuous) or s (discrete)"""
    (o, a), bt = m.rd["primary_batch"][:2], m.rd.get("_ssac")
    s_rep = m.s_rep = lu.encode(c.agent.encoder, o)
    if bt is not None and bt.xsa is not None and s_rep.data_ptr() == bt.xsa.data_ptr():
        m.X, m.ldx = bt.xsa, bt.xsa.stride(0)
    elif c.discrete:
        m.X, m.ldx = s_rep, lu._row_stride(s_rep)
    else:
        x = m.X = lu._concat_buffer(c.ws, f"cu.x{m.i}", s_rep, a.shape[1])
        x[:, s_rep.shape[1]:].copy_(a)
        m.ldx = x.stride(0)


def _member_targets(m, c):
    """first pass over member m: batch, critic input, TD target, backup weights (requests in, outcomes out: MemberUpdate)"""
    arena, ws, tag, agent = m.arena, c.ws, m.tag, c.agent
    N, qd, H = arena.n_nets, arena.out_dim, arena.hidden
    # when the merged actor / critic-forward launch will run, its workgroups fetch their own replay rows
    # (ssac_gather) and the update has no gather launch
    dual_ok = (DUAL_LAUNCH and arena.fused_dbuf and not c.train_enc and not c.dr3_coeff and not c.discrete
               and _dual_fits(arena, c.batch_size) and not _split_forward(N, c.batch_size))
    if c.members_form:
        m.one_wg_chain = True
        if engine.CAPTURE is not None:
            engine.CAPTURE.set_member(m.i)   # the draw sites below hand out THIS member's block of the update's inputs
    B_ = c.batch_size
    rd = m.rd = lu.sample_move_and_augment(buffer=c.buffer, batch_size=c.batch_size, augmenter=c.augmenter, aug_mix=c.aug_mix,
                                           per=c.per, _defer_gather=dual_ok, _invariance=bool(c.encoder_lambda),
                                           _xsa=c.xstack[m.i * B_:(m.i + 1) * B_] if c.xstack is not None else None)
    a, B = rd["primary_batch"][1], rd["primary_batch"][2].shape[0]
    m.B = B
    # The online critics' FORWARD does not depend on the TD target: on a second stream (a parallel graph
    # branch) it overlaps the actor -> target critics -> TD-target chain, which occupies few CUs.
    if arena.fused and not c.train_enc and not c.dr3_coeff and _split_forward(N, B):
        _set_critic_input(m, c)
        with engine.side_stream(c.dev, defer_join=True) as m.branch:
            with engine._timed("critic_fwd"):
                m.h1, m.h2, m.q = engine.mlp_forward(arena, m.X, m.ldx, 0, B, ws, tag)
    if dual_ok and m.branch is None:
        # the critics' forward rides in the actor's launch (when compute_td_targets uses the fused sample
        # launch); the critic launch of the second pass is then only the backward half
        _set_critic_input(m, c)
        m.want_fwd = True
        m.h1, m.h2, m.q = ws.get(tag + ".h1", (N, B, H)), ws.get(tag + ".h2", (N, B, H)), ws.get(tag + ".y", (N, B, qd))
        if RANK1_BWD and qd == 1:
            # and the TD-independent half (rank-1 loss gradient) of the backward pass rides in the target critics' launch
            m.want_bwd, m.act, m.ld_act = True, a, a.stride(0)
            m.dz2u, m.dz1u = ws.get(tag + ".dz2", (N, B, H)), ws.get(tag + ".dz1", (N, B, H))
            # dz2u = W3 (.) [h2 > 0] need not leave the chained launch when the weight-gradient launch that follows
            # is the loss-fold form: its fc2 tiles rebuild it from the saved h2 while staging (same values, bit for
            # bit; 5 MB less written per update at the metric shape).  The chain launch reports whether it skipped.
            m.dz2_optional = bool(SKIP_DZ2 and _loss_folds(B) and arena.shadow is None
                                  and parallel.shard_of(agent) is None and H % 4 == 0)
    m.lazy_td = bool(arena.fused and LAZY_TD and not c.dr3_coeff)
    m.td, _ = lu.compute_td_targets(
        logs=c.logs, replay_dict=rd, agent=agent, target_agent=c.target_agent, ensemble_idx=m.i, log_alphas=c.log_alphas,
        ensemble_n=c.target_critic_ensemble_n, pop=c.pop, gamma=c.gamma, random_process=c.random_process,
        noise_clip=c.noise_clip, discrete=c.discrete, _slot=c.slot, _member=m, _log_idx=m.ig, _explore=c.explore)
    lu.ensure_gathered(rd.get("_ssac"))  # (no-op when the merged launch took the gather)
    c.all_rd.append(rd)
    if c.sm_table is not None:
        lu.member_sharded_softmax_scores(rd, agent, c.target_agent, c.ms, c.sm_table[m.ig])
    if c.packed:
        return   # (the weights of all member batches follow the loop: lu.members_sunrise_weights)
    m.bw = 1.0 if c.ms is not None else lu.compute_backup_weights(
        logs=c.logs, replay_dict=rd, agent=agent, target_agent=c.target_agent, weight_type=c.weight_type,
        weight_temp=c.weighted_bellman_temp, batch_size=c.batch_size, discrete=c.discrete, _slot=c.slot,
        _w=ws.get(f"bw.w{m.i}", (B, 1)) if c.members_form else None)


def _encoder_input(m, c):
    """online encoder WITH gradient (learning.py:83): the embedding goes straight into member m's critic input; returns
    _encoder_step's `inv` (the invariance constraint's operands, or None)"""
    agent, rd, ws, i, B = c.agent, m.rd, c.ws, m.i, m.B
    o, a = rd["primary_batch"][:2]
    xin = ws.get(f"cu.x{i}", (B, m.arena.in_dim))
    inv = None
    okey = getattr(agent.encoder, "ssac_obs_key", "obs")
    # (the invariance constraint looks at the LAST member's batch only: learning.py:114-117 read the replay
    # dict the member loop left behind)
    lam_i = c.encoder_lambda if i == c.E - 1 else 0
    if lam_i and rd["augmented_obs"][0][okey] is not o[okey]:
        # encoder invariance on a partly augmented batch: the fully augmented observations need an encoder
        # pass of their own WITH gradient -- one stacked 2B-row pass [o ; ao], whose backward then receives
        # the critics' gradient in rows [0, B) and the constraint's in rows [B, 2B)
        eng, sall = lu.encode_stacked(agent.encoder, o, rd["augmented_obs"][0], ws, "cu.img2", c.dev)
        xin[:, :eng.emb].copy_(sall[:B])
        s_rep, as_rep, stacked = xin[:, :eng.emb], sall[B:], True
    else:
        s_rep = lu.encode(agent.encoder, o, dst=xin, save=True)
        as_rep, stacked = s_rep, False
    if lam_i:
        oo = rd["original_obs"][0]
        if oo[okey] is o[okey]:
            os_rep = ws.get("cu.osrep", (B, s_rep.shape[1]))
            os_rep.copy_(s_rep)   # un-augmented batch: the target of the constraint is the embedding itself
        else:
            os_rep = lu.encode(agent.encoder, oo, dst=ws.get("cu.osrep", (B, s_rep.shape[1])), save=False)
        inv = (as_rep, os_rep, c.encoder_lambda, stacked)
        c.logs["encoder_constraint_loss"] = c.slot[lu.L_ENC_INV]
    if not c.discrete:
        xin[:, s_rep.shape[1]:].copy_(a)
    m.s_rep, m.X, m.ldx = s_rep, xin, xin.stride(0)
    return inv


def _dr3_stacked(m, c, td, weight_ptr, pp, dopop, denom, a, B):
    """DR3 (learning.py:100-108): the critics also run on (s', a'); both batches go through the per-layer
    kernels as ONE stacked 2B-row batch, the co-adaptation gradient enters at the fc2 pre-activations"""
    arena, rd, ws, tag, slot, st = m.arena, m.rd, c.ws, m.tag, c.slot, c.st
    N, qd, H = arena.n_nets, arena.out_dim, arena.hidden
    assert not c.train_enc and parallel.shard_of(c.agent) is None, "DR3 is supported for identity encoders on a single rank"
    x1 = rd.get("_x1")
    X1 = x1 if x1 is not None else lu.encode(c.target_agent.encoder, rd["primary_batch"][3])
    Xc = ws.get(f"cu.xcat{m.i}", (2 * B, arena.in_dim))
    Xc[:B].copy_(torch.as_strided(m.X, (B, arena.in_dim), (m.ldx, 1)))
    Xc[B:].copy_(X1[:, :arena.in_dim])
    ch1, ch2, cq = engine.mlp_forward(arena, Xc, arena.in_dim, 0, 2 * B, ws, tag + ".dr3", force_layers=True)
    qc = ws.get(tag + ".dr3.qc", (N, B, qd))
    qc.copy_(cq[:, :B])
    dqc = ws.get(tag + ".dr3.dqc", (N, B, qd))
    check(lib.ssac_critic_loss_bwd(qc.data_ptr(), N, B, qd, a.data_ptr(), a.stride(0), td.data_ptr(),
                                   weight_ptr, pp, dopop, denom, dqc.data_ptr(), slot.data_ptr(), st))
    dq2 = ws.get(tag + ".dr3.dq", (N, 2 * B, qd), zero=True)
    dq2[:, :B].copy_(dqc)
    dparts = ws.get(tag + ".dr3.parts", (int(lib.ssac_dr3_blocks()),))
    coef = float(c.dr3_coeff) / denom / (N * B)

    def dr3_hook(dz2_, _h2=ch2, _parts=dparts):
        check(lib.ssac_dr3_add(dz2_.data_ptr(), _h2.data_ptr(), N, B, H, coef, _parts.data_ptr(), st))
    engine.mlp_backward(arena, dq2, Xc, arena.in_dim, 0, ch1, ch2, 2 * B, ws, tag + ".dr3", adam=c.adam,
                        adam_key=("critic", m.i), grads=m.grads, sumsq=m.ss, after_dz2=dr3_hook)
    fca = dparts.sum() / (N * B)
    c.logs[f"dr3_dotproduct_{m.i}"] = fca
    # the logged overall loss includes the regulariser (learning.py:108, 133)
    slot[lu.L_CRITIC_LOSS:lu.L_CRITIC_LOSS + 1].add_(fca * (float(c.dr3_coeff) / denom))


def _lossfold_args(m, c, weight_ptr, pp, dopop, denom, B):
    """engine.weight_grads(lossfold=...): dz2u / dz1u exist already; what depends on the TD target is one scalar per
    (net, row), dL/dq, and the weight-gradient launch evaluates it itself (per workgroup, in LDS): no loss launch at all"""
    arena, ws, slot, td, spec = m.arena, c.ws, c.slot, m.td, m.td_spec
    lossfold = dict(q=m.q, td_ptr=0 if spec is not None else td.data_ptr(), spec_ptr=C.addressof(spec) if spec is not None else 0,
                    weight_ptr=weight_ptr, popart_ptr=pp, pop=dopop, denom=denom, w3_snapshot=m.w3_snapshot,
                    partials=ws.get(m.tag + ".fparts", (arena.n_nets * 2,)), dz2_from_h2=m.w3_snapshot is not None)
    if arena.shadow is not None:
        lossfold["bf"] = arena.bf_buffers(ws, "cu", B)
    cap = engine.CAPTURE
    if cap is not None and cap.deferred is not None and cap.deferred_chain and spec is not None:
        cap.deferred_used = True
        # recorded update: the launch leaves partials + TD statistics behind and advances the input ring;
        # the next update's first launch (or a flush) writes the ring slot
        late_ptr = cap.late or 0
        if cap.late is not None:
            cap.late_used = True
            lossfold["late_target"] = cap.late_target.params
            if arena.shadow is not None:
                lossfold["target_shadow"] = cap.late_target.shadow
        lossfold["logfold"] = _lib.LogFold(0, slot.data_ptr(), 0, cap.feed, cap.deferred.td_stats, late_ptr)
    elif FOLD_LOGS and c.E_glob == 1 and not c.critic_clip:
        # the log finalisation rides in the weight-gradient launch (its last workgroup to arrive): no logs launch
        lossfold["logfold"] = _lib.LogFold(
            ws.get("cu.done", (1,), dtype=torch.int32, zero=True).data_ptr(), slot.data_ptr(),
            m.td_logs.data_ptr() if spec is not None else 0, cap.feed if (cap is not None and cap.feed) else 0, 0, 0)
    return lossfold


def _member_step(m, c):
    """second pass over member m: loss gradient, backward, encoder step, weight gradient, in the form its record selects"""
    arena, rd, i, ws, tag, slot, st, agent = m.arena, m.rd, m.i, c.ws, m.tag, c.slot, c.st, c.agent
    N, qd, H, a, B = arena.n_nets, arena.out_dim, arena.hidden, rd["primary_batch"][1], m.B
    td, bw, branch, train_enc = m.td, m.bw, m.branch, c.train_enc
    # ---- the critics' input, weights and buffers
    inv = _encoder_input(m, c) if train_enc else None
    if m.X is None:
        _set_critic_input(m, c)

    def encoder_step(dX):
        _encoder_step(agent.encoder, c.encoder_optimizer, c.encoder_clip, dX, m.s_rep.shape[1], ws, slot, c.dev, inv,
                      accumulate=i > 0, step=i == c.E - 1)
    if c.encoder_lambda and not train_enc:
        # identity encoder: augmented == original observations (only the identity augmentation applies to vectors),
        # the constraint is exactly zero and has no parameter to reach (learning_utils.py:401-409)
        c.logs["encoder_constraint_loss"] = slot[lu.L_ENC_INV]
    X, ldx = m.X, m.ldx
    shard = parallel.shard_of(agent)
    n_glob = m.n_glob = N if shard is None else shard.num_critics  # loss is averaged over the GLOBAL ensemble
    denom = float(c.E_glob * n_glob)
    popart = agent.popart[i]
    weight_ptr = 0 if isinstance(bw, float) else bw.data_ptr()  # imp_weights is ones(1) on the uniform path
    if c.per:
        # learning.py:96-98 multiplies (B,1) errors by the (B,) importance weights: a (B,B) outer product
        # whose mean is mean(w) * mean(bw * err^2) -- i.e. every row's weight is scaled by mean(w)
        wrow = ws.get(f"cu.w{i}", (B, 1))
        scale = rd["imp_weights"].mean().to(torch.float32)
        if isinstance(bw, float):
            wrow.fill_(1.0)
        else:
            wrow.copy_(bw.view(B, 1))
        wrow.mul_(scale)
        weight_ptr = wrow.data_ptr()
    pp, dopop = (popart.ptr if popart else 0), (1 if (popart and c.pop) else 0)
    ttot = engine.bf16_tiles_total(arena) if arena.shadow is not None else engine.wgrad_tiles_total(arena)
    if c.members_form:
        if c.ss_all is None:
            c.ss_all = ws.get("cu.ssall", (c.E, N * ttot))   # (the members' arenas have one shape: the
        assert c.ss_all.shape[1] == N * ttot                  #  reference builds them in one constructor call)
        ss = m.ss = c.ss_all[i]
    else:
        ss = m.ss = ws.get(f"cu.ss{i}", (N * ttot,))
    dq = ws.get(f"cu.dq{i}", (N, B, qd))
    grads = m.grads = ws.get(f"cu.g{i}", (arena.params.numel(),), zero=True) if c.critic_clip else None
    fused_form = arena.fused and not c.dr3_coeff
    if fused_form:
        dz2, dz1 = ws.get(tag + ".dz2", (N, B, H)), ws.get(tag + ".dz1", (N, B, H))
        tiles = int(lib.ssac_fused_row_tiles(C.byref(arena.desc()), B, N))
        parts = ws.get(tag + ".parts", (N * tiles * 2,))
        spec_ptr = C.addressof(m.td_spec) if m.td_spec is not None else 0  # the TD target is evaluated inside the critic launch
    if m.w3_snapshot is not None and not (m.bwd_done and _loss_folds(B)):
        raise RuntimeError("internal: the chained launch skipped dz2u but no loss-fold weight-gradient launch follows")
    # ---- the launch form (a merged launch of the first pass implies arena.fused and no DR3)
    lossfold = None
    if c.dr3_coeff:
        _dr3_stacked(m, c, td, weight_ptr, pp, dopop, denom, a, B)
    elif m.bwd_done and _loss_folds(B):
        lossfold = _lossfold_args(m, c, weight_ptr, pp, dopop, denom, B)
    elif m.bwd_done:
        # rank-1 backward done: a single-workgroup launch writes the N x B scalars dL/dq for the weight-gradient launch to read
        loss_bwd, td_arg = ((lib.ssac_critic_loss_bwd_lazy, spec_ptr) if m.td_spec is not None else
                            (lib.ssac_critic_loss_bwd, td.data_ptr()))
        check(loss_bwd(m.q.data_ptr(), N, B, qd, a.data_ptr(), a.stride(0), td_arg, weight_ptr, pp, dopop, denom,
                       dq.data_ptr(), slot.data_ptr(), st))
    elif branch is not None or m.fwd_done:
        # loss gradient + head backward + backward-data on the saved forward: ONE launch
        if branch is not None:
            branch.join()
        with engine._timed("critic_bwd") as tm:
            for _ in range(tm.reps):  # 1, except under bench.py's live kernel timing (idempotent launch)
                check(lib.ssac_critic_bwd_fused(
                    C.byref(arena.desc()), B, td.data_ptr(), weight_ptr, a.data_ptr(), a.stride(0), pp, dopop, denom,
                    m.h1.data_ptr(), m.h2.data_ptr(), m.q.data_ptr(), dq.data_ptr(), dz2.data_ptr(), dz1.data_ptr(),
                    parts.data_ptr(), spec_ptr, st))
    elif arena.fused:
        # forward of all N critics + loss gradient + backward-data: ONE launch
        m.h1, m.h2, m.q = ws.get(tag + ".h1", (N, B, H)), ws.get(tag + ".h2", (N, B, H)), ws.get(tag + ".y", (N, B, qd))
        with engine._timed("critic_fused") as tm:
            for _ in range(tm.reps):  # 1, except under bench.py's live kernel timing (idempotent launch)
                check(lib.ssac_critic_fwd_bwd_fused(
                    C.byref(arena.desc()), X.data_ptr(), ldx, B, td.data_ptr(), weight_ptr, a.data_ptr(),
                    a.stride(0), pp, dopop, denom, m.h1.data_ptr(), m.h2.data_ptr(), m.q.data_ptr(),
                    dq.data_ptr(), dz2.data_ptr(), dz1.data_ptr(), parts.data_ptr(), spec_ptr, st))
    else:  # the per-layer family
        if arena.shadow is not None:
            raise NotImplementedError("bf16 mode needs the fused kernel family (hidden % 32 == 0, <= 256)")
        h1, h2, q = engine.mlp_forward(arena, X, ldx, 0, B, ws, tag)
        check(lib.ssac_critic_loss_bwd(q.data_ptr(), N, B, qd, a.data_ptr(), a.stride(0), td.data_ptr(), weight_ptr, pp,
                                       dopop, denom, dq.data_ptr(), slot.data_ptr(), st))
        if train_enc:
            dX = engine.mlp_backward(arena, dq, X, ldx, 0, h1, h2, B, ws, tag, need_dx=True, update=False)
            encoder_step(dX)
            dz2, dz1 = ws.get(tag + ".dz2", (N, B, arena.hidden)), ws.get(tag + ".dz1", (N, B, arena.hidden))
            engine.weight_grads(arena, X, ldx, 0, h1, h2, dq, dz2, dz1, B, adam=c.adam, adam_key=("critic", i), grads=grads, sumsq=ss)
        else:
            engine.mlp_backward(arena, dq, X, ldx, 0, h1, h2, B, ws, tag, adam=c.adam, adam_key=("critic", i), grads=grads, sumsq=ss)
    if not fused_form:
        return
    # ---- the fused forms' common tail: encoder step, weight gradients, what the log launch will read
    if train_enc:  # dL/d(embedding) = sum over critics of dz1 W1[:, :emb], BEFORE W1 is updated
        dX = ws.get(tag + ".dx", (N, B, arena.in_dim))
        check(lib.ssac_mlp_layer_dgrad(C.byref(arena.desc()), 0, 0, N, dz1.data_ptr(), H, B * H, 0, 0, 0,
                                       B, dX.data_ptr(), arena.in_dim, B * arena.in_dim, st))
        encoder_step(dX)
    if arena.shadow is not None and lossfold is None:
        raise NotImplementedError(
            "bf16 mode covers the chained critic update (continuous single-output critics, stochastic actor, "
            "identity encoder, with or without PopArt / gradient clipping; no DR3, no discrete critics)")
    m.logs_folded = bool(engine.weight_grads(
        arena, X, ldx, 0, m.h1, m.h2, dq, dz2, dz1, B, adam=c.adam, adam_key=("critic", i), grads=grads, sumsq=ss,
        rowscale=dq if (m.bwd_done and lossfold is None) else None, lossfold=lossfold,
        target=lossfold.get("late_target") if lossfold is not None else None))
    if m.logs_folded and lossfold["logfold"].feed:
        engine.CAPTURE.published = True
    m.log_parts, m.log_nets, m.log_tiles = ((lossfold["partials"], N, 1) if lossfold is not None else
                                            (parts, 0 if m.bwd_done else N, tiles))


def _actor_chain_form(a_arena, A, B, c_arena):
    """does this member's online actor update take the chained launch (ssac_actor_chain_fused)?  Asked by
    _actor_member_plan alone, which turns it into the member's launch form and noise source: a member on the three-launch
    form reads its noise from a buffer, which a recording must own and refill before every replay.
    (B <= 2048 = SSAC_ACTOR_CHAIN_MAX_ROWS: the chained launch's actor workgroups wait for critic tiles dispatched behind
    them and must leave them CUs to run on.)
    Round 6: an actor whose carve holds only ONE weight-staging buffer (Humanoid's 376 -> 256 -> 34) can take the chained
    launch too, its two passes single-buffered -- `fused`, not `fused_dbuf` -- and the form is taken only while the launch
    is ONE RESIDENT ROUND (actor tiles + critic tiles <= 256 workgroups).  Measured: Humanoid with N = 16 critics is 32 + 512
    workgroups; the actor workgroups then sit on 32 CUs through two and a half rounds of critic tiles and the chained launch
    is SLOWER than the three launches, 177.2 against 162.8 us per actor update (profiles/r6_kernel_stats.md)."""
    if not (ACTOR_CHAIN and a_arena.fused and A <= 32 and a_arena.hidden * A <= 512 * 9 and B <= 2048 and c_arena.fused_dbuf
            and c_arena.out_dim == 1):
        return False
    tiles_c = int(lib.ssac_fused_row_tiles(C.byref(c_arena.desc()), B, c_arena.n_nets)) * c_arena.n_nets
    return (B + 15) // 16 + tiles_c <= 256


def _actor_member_plan(kind, random_process, use_baseline, clip, a_arena, c_arena, A, B, sharded, rec_buffers):
    """THE decision of one member's online actor update, made once: (form, noise).  Everything that has to agree with the
    launch site asks here -- whether the update can be recorded, where a recording's noise comes from, what a member-
    sharded rank skips for a member another rank owns.
    form: "chain" (ssac_actor_chain_fused, _actor_chain_form), "fused" (the three launches; on a critic-sharded rank with
    the routing and exchange steps between the second and the third), "layers" (the per-layer family).
    noise: "kernel" (the chained launch with the stock generator draws it from the engine's Philox stream: no buffer, no
    draw from the device generator), "recording" (the recording's fixed buffers, refilled by the caller before every
    replay: a recording with a member off the chained launch owns one per member), "draw" (a fresh draw on the host)."""
    if not (FUSED_ACTOR and kind == "stochastic" and random_process is None and not use_baseline and not clip
            and a_arena.fused and c_arena.fused_dbuf and c_arena.out_dim == 1):
        return "layers", "draw"
    if sharded:   # (every rank makes the same draw)
        return "fused", "draw"
    chain = _actor_chain_form(a_arena, A, B, c_arena)
    if rec_buffers:
        noise = "recording"
    else:
        noise = "kernel" if (chain and lu.IN_KERNEL_NOISE and rng.normal_is_stock()) else "draw"
    return ("chain" if chain else "fused"), noise


def _member_plan(agent, i, B, dev, random_process, use_baseline, clip, rec_buffers=False):
    """_actor_member_plan of the agent's member i at B rows -> (form, noise, the actor's arena, the critics' arena).  (Keyed by everything the plan reads -- the arenas by their
    dimensions, the switches and the noise hook by their current values -- the answer is cached on the agent: a replayed
    update asks on every call.)"""
    actor = agent.actors[i]
    a_arena, c_arena = engine.bind_arena(actor, "self", [actor], dev), agent.critics[i].arena(dev)
    args = (lu.actor_kind(actor), random_process, use_baseline, clip, a_arena, c_arena, actor.action_size, B,
            parallel.shard_of(agent) is not None, bool(rec_buffers))
    key = (args[0], random_process is None, bool(use_baseline), bool(clip), a_arena.fused, a_arena.hidden, c_arena.fused_dbuf,
           c_arena.in_dim, c_arena.hidden, c_arena.out_dim, c_arena.n_nets) + args[6:] + (
           FUSED_ACTOR, ACTOR_CHAIN, lu.IN_KERNEL_NOISE, rng.normal_is_stock())
    memo = agent.__dict__.setdefault("_ssac_actor_plan_memo", {})
    if key not in memo:
        if len(memo) > 16:
            memo.clear()
        memo[key] = _actor_member_plan(*args)
    return memo[key] + (a_arena, c_arena)


class _RecordedActor:
    """one recorded online actor update: calls so far, the launch list, its fixed log block (blk) with the logs' word index,
    the noise buffers it owns (eps; None: in_kernel), and per call the log ring's buffer (ring) and this call's slot of it;
    published: the recorded log step writes the finished block to that slot itself"""
    __slots__ = ("calls", "list", "blk", "eps", "index", "in_kernel", "published", "ring", "slot")

    def __init__(self):
        self.calls, self.list, self.blk, self.eps, self.index, self.ring, self.slot = 0, None, None, None, None, None, 0
        self.in_kernel = False
        self.published = False

    def __del__(self):
        if self.list:
            try:
                lib.ssac_launch_list_free(self.list)
            except Exception:
                pass


def online_actor_update(buffer, agent, pop, actor_optimizer, log_alphas, batch_size, clip,
                        random_process, noise_clip, augmenter, aug_mix, premade_replay_dicts=None,
                        per=False, discrete=False, use_baseline=False):
    """learning.py:344-421.  On the fused path (continuous stochastic actor, no clipping / exploration process /
    baseline) the update is four launches + a log launch; called repeatedly on the batch buffers of a recorded critic
    update (premade_replay_dicts at fixed addresses) it is recorded after two calls and re-issued from ONE C call.
    Which launch form a member takes and where its noise comes from is decided in ONE place, _actor_member_plan: the
    test below for "can be recorded", the recording's choice of noise source and the launch site in
    _online_actor_update all read its answer."""
    engine.require_gpu()
    lu.ensure_adopted(agent, buffer)
    encoder_base.refuse_unsupported(agent, "online_actor_update")
    kw = dict(buffer=buffer, agent=agent, pop=pop, actor_optimizer=actor_optimizer, log_alphas=log_alphas,
              batch_size=batch_size, clip=clip, random_process=random_process, noise_clip=noise_clip,
              augmenter=augmenter, aug_mix=aug_mix, premade_replay_dicts=premade_replay_dicts, per=per,
              discrete=discrete, use_baseline=use_baseline)
    if lu.actor_kind(agent.actors[0]) == "beta":
        if use_baseline:
            beta.refuse("online_actor_update(use_baseline=True)")
        if parallel.shard_of(agent) is not None or parallel.member_shard_of(agent) is not None:
            beta.refuse("online_actor_update on a critic- or member-sharded agent")
    dev = log_alphas[0].device
    recordable = (USE_GRAPHS and LAUNCH_MODE == "list" and FUSED_ACTOR and engine.CAPTURE is None
                  and premade_replay_dicts is not None and not discrete and parallel.shard_of(agent) is None
                  and parallel.member_shard_of(agent) is None and lu.is_identity(agent.encoder))
    # ... and every member on a fused form
    plans = recordable and [_member_plan(agent, i, batch_size, dev, random_process, use_baseline, clip)[:2]
                            for i in range(len(agent.actors))]
    if not plans or any(form == "layers" for form, _ in plans):
        return _online_actor_update(**kw)
    ptrs = tuple(lu.encode(agent.encoder, rd_["primary_batch"][0]).data_ptr() for rd_ in premade_replay_dicts)
    key = (id(actor_optimizer), ptrs, batch_size, bool(pop), tuple(id(la_) for la_ in log_alphas), engine.USE_FUSED)
    cache = agent.__dict__.setdefault("_ssac_actor_rec", {})
    rec = cache.get(key)
    if rec is None:
        if len(cache) > 8:
            cache.clear()
        rec = cache[key] = _RecordedActor()
    rec.calls += 1
    if rec.calls <= 2:
        return _online_actor_update(**kw)
    A = agent.actors[0].action_size
    ring = lu.ring_for(dev)
    # the chained launch (ACTOR_CHAIN) with the stock generator draws its noise in the kernel: no buffers, no launches
    # (... if every member takes it: a member on the three-launch form reads a buffer this recording must own)
    in_kernel = all(noise == "kernel" for _, noise in plans)
    if rec.list is None:
        rec.blk = torch.zeros(lu.LOG_WIDTH, device=dev)
        rec.in_kernel = in_kernel
        rec.eps = None if rec.in_kernel else [torch.empty(batch_size, A, device=dev) for _ in agent.actors]
    elif rec.in_kernel != in_kernel:
        # a noise hook was installed / removed (or the form switched) since the recording: record again
        del cache[key]
        return online_actor_update(**kw)
    if rec.eps is not None:
        for e_ in rec.eps:
            rng.draw_normal_into(e_)  # a_dist.rsample() of every member, in member order (learning.py:392)
    rec.ring, rec.slot = ring.buf, ring.advance()   # this call's slot of the log ring
    if rec.list is None:
        check(lib.ssac_record_begin())
        try:
            logs = _online_actor_update(**kw, rec=rec)
        finally:
            rec.list = lib.ssac_record_end()
        base = rec.blk.data_ptr()
        rec.index = {k_: (v.data_ptr() - base) // 4 for k_, v in logs.items()}
    else:
        ns_upd = lu.noise_stream(agent, dev)
        # (this update's number: tags, noise draws -- and, when the log launch publishes, the ring slot it writes)
        if rec.published:
            check(lib.ssac_replay_value2(rec.list, engine.stream(), ns_upd[2], rec.slot))
        else:
            check(lib.ssac_replay_value(rec.list, engine.stream(), ns_upd[2]))
        ns_upd[2] += 1
        rng.choice(agent.actors)  # learning.py:417-419 (keeps the Python RNG stream in step)
    if not rec.published:
        ring.buf[rec.slot].copy_(rec.blk)   # this call's log block -> its own ring slot (device-to-device, no sync)
    blk = ring.buf[rec.slot]
    return {k_: blk[i] for k_, i in rec.index.items()}


class _ActorMember:
    """ONE ensemble member's online actor update: i / ig (local / global member index), actor and a_arena, c_arena (its
    critics), popart, log_alpha, rd (replay dict), s_rep with its row stride lds, and the plan: form, noise"""
    __slots__ = ("i", "ig", "actor", "a_arena", "c_arena", "popart", "log_alpha", "rd", "s_rep", "lds", "form", "noise")


def _online_actor_update(buffer, agent, pop, actor_optimizer, log_alphas, batch_size, clip,
                         random_process, noise_clip, augmenter, aug_mix, premade_replay_dicts=None,
                         per=False, discrete=False, use_baseline=False, rec=None):
    """the ensemble-level flow; rec: the _RecordedActor whose launches are being recorded (None: an eager call)"""
    c = types.SimpleNamespace(**locals())   # the call: its arguments, and below what every member shares
    dev = c.dev = log_alphas[0].device
    ws = c.ws = lu.agent_ws(agent, dev)
    adam = c.adam = engine.adam_group(actor_optimizer, dev)
    # (a RECORDED update clears its fixed log block and advances the Adam step by a recorded launch of its first member)
    slot = c.slot = rec.blk if rec is not None else lu.log_block(dev, adam)
    # this update's number: hand-off tags and in-kernel noise draws of the chained launches (checkpointed with the agent's
    # noise stream, so a resumed run continues the sequence)
    ns_upd = c.ns_upd = lu.noise_stream(agent, dev)
    st = c.st = engine.stream()
    # member-sharded rank (parallel.MemberShard): the loss is averaged over the GLOBAL ensemble (learning.py:409), and the
    # members other ranks own still take their host draws here, in member order
    ms = parallel.member_shard_of(agent)
    E_glob = c.E_glob = len(agent.actors) if ms is None else ms.ensemble_size
    c.inv_e = 1.0 / E_glob
    c.clip_members, member_ss = [], []
    rec_buffers = rec is not None and rec.eps is not None
    for ig in range(E_glob):
        i = ig if ms is None else ms.local(ig)
        if i is None:
            assert not use_baseline, "use_baseline is not supported on member-sharded ranks"
            if premade_replay_dicts is None:
                lu.sample_move_and_augment(buffer=buffer, batch_size=batch_size, augmenter=augmenter, aug_mix=aug_mix, per=per)
            # (what the member's owner consumes from the device generator: nothing when its chained launch draws the noise
            # in the kernel -- members share their shapes, so this rank's first member answers for the absent one)
            if _member_plan(agent, 0, batch_size, dev, random_process, use_baseline, clip, rec_buffers)[1] != "kernel":
                lu.skip_actor_draws(agent.actors[0], batch_size, dev, random_process)
            continue
        m = _ActorMember()
        m.i, m.ig, m.popart, m.log_alpha = i, ig, agent.popart[i], log_alphas[i]
        if premade_replay_dicts is not None:
            m.rd = premade_replay_dicts[i]
        else:
            m.rd = lu.sample_move_and_augment(buffer=buffer, batch_size=batch_size, augmenter=augmenter,
                                              aug_mix=aug_mix, per=per)
        s_rep = m.s_rep = lu.encode(agent.encoder, m.rd["primary_batch"][0])  # no gradient to the encoder (learning.py:378-380)
        m.lds = lu._row_stride(s_rep)
        m.actor = agent.actors[i]
        m.form, m.noise, m.a_arena, m.c_arena = _member_plan(agent, i, s_rep.shape[0], dev, random_process, use_baseline, clip,
                                                             rec_buffers)
        member_ss.append(_actor_member_layers(m, c) if m.form == "layers" else _actor_member_fused(m, c))
    ns_upd[2] += 1
    _step_and_log_norm(agent, adam, clip, c.clip_members, member_ss, slot[lu.L_ACTOR_GN:], ms)
    return {"gradients/random_actor_online_grad": slot[lu.L_ACTOR_GN], "losses/actor_pg_loss": slot[lu.L_ACTOR_LOSS]}


def _actor_member_fused(m, c):
    """the "chain" and "fused" forms of member m -- four launches instead of ~15 (include/ssac_hip.h, "the online actor
    update"): sample + [s|a] rows, critics' forward + unscaled dQ/da, arg-min routing + tanh-normal backward + actor
    backward-data (the three as ONE chained launch on the "chain" form), weight gradients + Adam; then the two log values.
    -> the member's sum-of-squares slots for the norm launch, None when its own log step wrote the norm already"""
    ws, st, i, rec, slot, adam, inv_e = c.ws, c.st, m.i, c.rec, c.slot, c.adam, c.inv_e
    actor, a_arena, c_arena, s_rep, lds, log_alpha = m.actor, m.a_arena, m.c_arena, m.s_rep, m.lds, m.log_alpha
    (B, S), A, H, N = s_rep.shape, actor.action_size, a_arena.hidden, c_arena.n_nets
    lo, hi = float(actor.log_std_low), float(actor.log_std_high)
    pp, dopop = (m.popart.ptr if m.popart else 0), (1 if (m.popart and c.pop) else 0)
    # ---- work space
    xpi = ws.get(f"au.x{i}", (B, S + A))
    logp = ws.get(f"au.logp{i}", (B,))
    ah1, ah2 = ws.get(f"au.a{i}.h1", (1, B, H)), ws.get(f"au.a{i}.h2", (1, B, H))
    aout = ws.get(f"au.a{i}.y", (1, B, 2 * A))
    q = ws.get(f"au.c{i}.y", (N, B, 1))
    dxu = ws.get(f"au.dxu{i}", (N, B, A))
    tiles = int(lib.ssac_fused_row_tiles(C.byref(a_arena.desc()), B, 1))
    parts = ws.get(f"au.parts{i}", (tiles,))
    d_out = ws.get(f"au.dout{i}", (1, B, 2 * A))
    dz2, dz1 = ws.get(f"au.a{i}.dz2", (1, B, H)), ws.get(f"au.a{i}.dz1", (1, B, H))
    # ---- the noise, as a_dist.rsample() makes it (learning.py:392) unless the chained launch draws it in the kernel
    eps = None   # (kept alive to the end of the member's launches: the kernels read it asynchronously)
    if m.noise == "recording":
        eps = rec.eps[i]   # the draw was written into a fixed buffer by the caller
    elif m.noise == "draw":
        # (never inside a recording: a replay would re-read a buffer long returned to the allocator)
        assert rec is None, "recorded actor update: the noise must come from the kernel or from the recording's buffers"
        eps = rng.draw_normal((B, A), c.dev)
    eps_ptr = eps.data_ptr() if eps is not None else 0
    # ---- the launches.  The first member of a RECORDED update also clears the log block and advances the Adam step: inside
    #      its chained launch, or by a begin launch in front of a member the chained launch does not take
    begin = rec is not None and m.ig == 0
    if m.form == "chain":
        ho = ws.get(f"au.handoff{i}", (int(lib.ssac_actor_chain_handoff_words(B, N, A)),), dtype=torch.int64, zero=True)
        rs = None
        if m.noise == "kernel":
            # (its own stream: the critic updates number their draws from the same seed)
            # (the GLOBAL member index: a member-sharded rank draws its members' noise as the unsharded run does)
            rs = _lib.Rng((c.ns_upd[0] ^ 0x5DEECE66D1CEB00C) & (2 ** 64 - 1), 0, (m.ig << 40) + c.ns_upd[2])
        check(lib.ssac_actor_chain_fused(
            C.byref(a_arena.desc()), s_rep.data_ptr(), lds, B, eps_ptr, C.byref(rs) if rs is not None else None, lo, hi,
            xpi.data_ptr(), S + A, logp.data_ptr(), ah1.data_ptr(), ah2.data_ptr(), aout.data_ptr(),
            C.byref(c_arena.desc()), q.data_ptr(), dxu.data_ptr(), log_alpha.data_ptr(), 1, inv_e, pp, dopop,
            d_out.data_ptr(), dz2.data_ptr(), dz1.data_ptr(), parts.data_ptr(), ho.data_ptr(), c.ns_upd[2],
            slot.data_ptr() if begin else 0, lu.LOG_WIDTH if begin else 0, adam.ctl.ptr if begin else 0, st))
    else:
        if begin:
            check(lib.ssac_begin_update(slot.data_ptr(), lu.LOG_WIDTH, adam.ctl.ptr, 0, st))
        check(lib.ssac_actor_sample_concat_fused(C.byref(a_arena.desc()), s_rep.data_ptr(), lds, B, eps_ptr, lo, hi,
                                                 xpi.data_ptr(), S + A, logp.data_ptr(), ah1.data_ptr(), ah2.data_ptr(),
                                                 aout.data_ptr(), 0, st))
        check(lib.ssac_critic_fwd_dx_fused(C.byref(c_arena.desc()), xpi.data_ptr(), S + A, B, S, A, q.data_ptr(),
                                           dxu.data_ptr(), st))
        # (a critic-sharded rank: the actor backward reads the GLOBAL min Q and the dQ/da row routed from its owner)
        qsel, nsel, dsel = (q, N, dxu) if parallel.shard_of(c.agent) is None else _route_over_ranks(m, c, q, dxu)
        check(lib.ssac_actor_bwd_fused(C.byref(a_arena.desc()), ah1.data_ptr(), ah2.data_ptr(), B, qsel.data_ptr(), nsel,
                                       dsel.data_ptr(), aout.data_ptr(), eps_ptr, logp.data_ptr(), log_alpha.data_ptr(), 1,
                                       lo, hi, inv_e, pp, dopop, d_out.data_ptr(), dz2.data_ptr(), dz1.data_ptr(),
                                       parts.data_ptr(), st))
    # ---- weight gradients + Adam, the log step, and (recorded single-member update) the ring slot
    ss = ws.get(f"au.ss{i}", (engine.wgrad_tiles_total(a_arena),))
    one = c.E_glob == 1   # (then the logged actor is this one: both logs in one launch)
    # (a recorded update of a single-member agent: the log step also writes the finished block to its slot of the log
    #  ring -- the replay names the slot, ssac_replay_value2 -- instead of a copy launch behind every replay)
    pub = rec if one else None
    ring_ptr, ring_slot = (pub.ring.data_ptr(), pub.slot) if pub is not None else (0, 0)
    folded = False
    if one and engine.actor_fold_applies(a_arena, None, ss, None, None, None):
        # ... and the log step itself rides in the weight-gradient launch: its last workgroup to finish sums the
        # tiles' loss terms and the gradient-norm partials (ssac_actor_logs' arithmetic), no launch of its own
        done = ws.get(f"au.logdone{i}", (1,), dtype=torch.int32, zero=True)
        af = _lib.ActorLogFold(done.data_ptr(), parts.data_ptr(), tiles, B, inv_e, lu.LOG_WIDTH,
                               slot[lu.L_ACTOR_LOSS:].data_ptr(), slot[lu.L_ACTOR_GN:].data_ptr(), slot.data_ptr(),
                               ring_ptr, ring_slot)
        folded = bool(engine.weight_grads(a_arena, s_rep, lds, 0, ah1, ah2, d_out, dz2, dz1, B, adam=adam,
                                          adam_key=("actor", i), sumsq=ss, actor_fold=af))
    if not folded:
        engine.weight_grads(a_arena, s_rep, lds, 0, ah1, ah2, d_out, dz2, dz1, B, adam=adam, adam_key=("actor", i), sumsq=ss)
        check(lib.ssac_actor_logs(parts.data_ptr(), tiles, B, inv_e, ss.data_ptr() if one else 0, ss.numel(),
                                  slot[lu.L_ACTOR_LOSS:].data_ptr(), slot[lu.L_ACTOR_GN:].data_ptr() if one else 0,
                                  slot.data_ptr(), lu.LOG_WIDTH, ring_ptr, ring_slot, st))
    if pub is not None:
        pub.published = True
    return None if one else ss


def _route_over_ranks(m, c, q, dxu):
    """critic-sharded rank, between the critics' forward and the actor backward -- the two exchange steps of SURVEY 8(e):
    local arg-min, MIN over the ranks, the global arg-min's owner keeps its dQ/da row, SUM over the ranks.
    -> (global min Q, 1, routed dQ/da): what ssac_actor_bwd_fused takes in place of (q, N, dxu)"""
    ws, st, i, rank = c.ws, c.st, m.i, parallel.shard_of(c.agent).rank
    N, B, A = dxu.shape
    qloc, qglob = ws.get(f"au.qloc{i}", (B,)), ws.get(f"au.qmin{i}", (B,))
    dsel = ws.get(f"au.da{i}", (1, B, A))
    check(lib.ssac_actor_route_local(q.data_ptr(), dxu.data_ptr(), N, B, A, qloc.data_ptr(), qglob.data_ptr(),
                                     dsel.data_ptr(), st))
    parallel.all_reduce_min(qglob)
    # (bit-equal minima on two ranks: the lowest rank keeps the row, as torch.min keeps the first index)
    claim = ws.get(f"au.claim{i}", (B,))
    check(lib.ssac_actor_route_claim(qloc.data_ptr(), qglob.data_ptr(), B, rank, claim.data_ptr(), st))
    parallel.all_reduce_min(claim)
    check(lib.ssac_actor_route_mask(claim.data_ptr(), rank, B, A, dsel.data_ptr(), st))
    parallel.all_reduce_sum(dsel)
    return qglob, 1, dsel


def _exploration_noise(c, xpi, S, B, A):
    """exploration noise on the sampled action, no entropy term (learning.py:393-395); the gradient passes through the
    clamp unchanged (learning_utils.py:56-59).  -> the draw (the caller keeps it alive: the kernel reads it asynchronously)"""
    noise = rng.draw_normal((B, A), c.dev)
    check(lib.ssac_exploration_noise(xpi.data_ptr(), S + A, S, noise.data_ptr(), float(c.random_process.current_scale),
                                     float(c.noise_clip) if c.noise_clip is not None else 0.0, B, A, c.st))
    return noise


def _actor_member_layers(m, c):
    """the "layers" form of member m: every actor kind, exploration process, baseline and clip, on the per-layer family.
    Host draws in the reference's order: rsample noise (Beta: beta.sample in its place), process noise, then the
    advantage estimator's.  -> the member's sum-of-squares slots"""
    ws, st, i, slot, inv_e, random_process = c.ws, c.st, m.i, c.slot, c.inv_e, c.random_process
    actor, a_arena, c_arena, s_rep, lds, log_alpha = m.actor, m.a_arena, m.c_arena, m.s_rep, m.lds, m.log_alpha
    (B, S), N, kind, shard = s_rep.shape, c_arena.n_nets, lu.actor_kind(actor), parallel.shard_of(c.agent)
    pp, dopop = (m.popart.ptr if m.popart else 0), (1 if (m.popart and c.pop) else 0)
    ah1, ah2, aout = engine.mlp_forward(a_arena, s_rep, lds, 0, B, ws, f"au.a{i}")
    if kind == "discrete":
        A = a_arena.out_dim
        _, _, q = engine.mlp_forward(c_arena, s_rep, lds, 0, B, ws, f"au.c{i}", save=False)
        if shard is not None:  # elementwise min over the local critics, then over the ranks
            qm = ws.get(f"au.qmin{i}", (1, B, A))
            lu._min_over_nets(q, N, B * A, qm)
            parallel.all_reduce_min(qm)
            q, N = qm, 1
        d_out = ws.get(f"au.dout{i}", (1, B, A))
        check(lib.ssac_discrete_actor_loss_bwd(aout.data_ptr(), q.data_ptr(), N, B, A, log_alpha.data_ptr(), pp, dopop,
                                               inv_e, d_out.data_ptr(), slot[lu.L_ACTOR_LOSS:].data_ptr(), st))
    else:
        A = actor.action_size
        xpi = lu._concat_buffer(ws, f"au.x{i}", s_rep, A)
        logp = ws.get(f"au.logp{i}", (B,))
        eps = rng.draw_normal((B, A), c.dev) if kind != "beta" else None  # a_dist.rsample() (learning.py:392)
        noise = None   # (kept alive to the end of the member's launches)
        use_entropy = 1 if random_process is None else 0
        if kind == "beta":
            # a_dist.rsample() of the Beta head; x is kept for the reparameterised backward
            xb = beta.sample(c.agent, aout, B, A, "actor", ws.get(f"au.xb{i}", (B, A)), xpi, S + A, S, logp)
        elif kind == "stochastic":
            check(lib.ssac_tanh_normal_fwd(aout.data_ptr(), 2 * A, eps.data_ptr(), B, A, float(actor.log_std_low),
                                           float(actor.log_std_high), xpi.data_ptr(), S + A, S, logp.data_ptr(), st))
        if kind in ("beta", "stochastic"):
            if random_process is not None:
                noise = _exploration_noise(c, xpi, S, B, A)
        elif random_process is not None:
            noise = rng.draw_normal((B, A), c.dev)
            check(lib.ssac_det_action_fwd(aout.data_ptr(), A, eps.data_ptr(), 1e-4, noise.data_ptr(),
                                          float(random_process.current_scale),
                                          float(c.noise_clip) if c.noise_clip is not None else 0.0, B, A,
                                          xpi.data_ptr(), S + A, S, st))
        else:
            # deterministic actor without a process: a = loc + 1e-4 eps, entropy term = its Normal(loc, 1e-4)
            # log-density (no gradient: a - loc does not depend on the actor; learning.py:396-399)
            check(lib.ssac_det_action_fwd(aout.data_ptr(), A, eps.data_ptr(), 1e-4, 0, 0.0, 0.0, B, A,
                                          xpi.data_ptr(), S + A, S, st))
            check(lib.ssac_det_logprob(eps.data_ptr(), B, A, logp.data_ptr(), st))
        ch1, ch2, q = engine.mlp_forward(c_arena, xpi, S + A, 0, B, ws, f"au.c{i}")
        dq = ws.get(f"au.dq{i}", (N, B, 1))
        qmin_ptr = 0
        if shard is not None:  # min over ALL critics: local min, then MIN all-reduce over ranks
            qmin = ws.get(f"au.qmin{i}", (B,))
            lu._min_over_nets(q, N, B, qmin)
            parallel.all_reduce_min(qmin)
            qmin_ptr = qmin.data_ptr()
        if c.use_baseline:
            # learning.py:401: vals = A(s, a_theta) = Q'(s, a_theta) - V(s) from the advantage estimator (four fresh
            # policy samples, drawn after the rsample; adv_estimator.py:31-36 applies the PopArt layer whenever
            # the member has one).  V has no gradient: the routing of dL/dq is the plain path's.
            assert shard is None, "use_baseline is not supported on critic-sharded ranks"
            res = c.agent.adv_estimator.evaluate(m.rd["primary_batch"][0], xpi[:, S:], i, want=("adv",))
            check(lib.ssac_actor_loss_bwd_adv(q.data_ptr(), N, B, logp.data_ptr(), log_alpha.data_ptr(), use_entropy, pp,
                                              1 if m.popart else 0, inv_e, res["adv"].data_ptr(), dq.data_ptr(),
                                              slot[lu.L_ACTOR_LOSS:].data_ptr(), st))
        else:
            check(lib.ssac_actor_loss_bwd(q.data_ptr(), N, B, logp.data_ptr(), log_alpha.data_ptr(), use_entropy, pp,
                                          dopop, inv_e, qmin_ptr, dq.data_ptr(), slot[lu.L_ACTOR_LOSS:].data_ptr(), st))
        # dQ/da through the arg-min critic of every row; critic weights are NOT updated here
        dX = engine.mlp_backward(c_arena, dq, xpi, S + A, 0, ch1, ch2, B, ws, f"au.c{i}", need_dx=True, update=False)
        n_dx, ld_dx, s_dx, col_dx = N, S + A, B * (S + A), S
        if shard is not None:  # SUM all-reduce of the (B x A) action gradient
            da = ws.get(f"au.da{i}", (1, B, A))
            torch.sum(dX[:, :, S:], dim=0, out=da[0])
            parallel.all_reduce_sum(da)
            dX, n_dx, ld_dx, s_dx, col_dx = da, 1, A, B * A, 0
        d_out = ws.get(f"au.dout{i}", (1, B, a_arena.out_dim))
        if kind == "beta":
            check(lib.ssac_beta_bwd(dX.data_ptr(), n_dx, ld_dx, s_dx, col_dx, aout.data_ptr(), 2 * A, xb.data_ptr(), B, A,
                                    log_alpha.data_ptr(), use_entropy, inv_e, 0, d_out.data_ptr(), 2 * A, st))
        elif kind == "stochastic":
            check(lib.ssac_tanh_normal_bwd(dX.data_ptr(), n_dx, ld_dx, s_dx, col_dx, aout.data_ptr(), 2 * A,
                                           eps.data_ptr(), B, A, float(actor.log_std_low), float(actor.log_std_high),
                                           log_alpha.data_ptr(), use_entropy, inv_e, d_out.data_ptr(), 2 * A, st))
        else:
            check(lib.ssac_det_action_bwd(dX.data_ptr(), n_dx, ld_dx, s_dx, col_dx, aout.data_ptr(), A, B, A,
                                          d_out.data_ptr(), A, st))
    return _actor_backward(a_arena, d_out, s_rep, lds, ah1, ah2, B, ws, "au", i, c.adam, c.clip, c.clip_members)[1]


def _actor_backward(a_arena, d_out, x, ldx, h1, h2, n_rows, ws, pre, i, adam, clip, clip_members, need_dx=False):
    """backward of actor member i from dL/d(output): into a gradient buffer for the clip (the member joins clip_members),
    or with Adam in the epilogue of the weight-gradient launch.  -> (dX when need_dx, the member's sum-of-squares slots)"""
    ss = ws.get(f"{pre}.ss{i}", (engine.wgrad_tiles_total(a_arena),))
    if clip:
        grads = ws.get(f"{pre}.g{i}", (a_arena.params.numel(),), zero=True)
        dX = engine.mlp_backward(a_arena, d_out, x, ldx, 0, h1, h2, n_rows, ws, f"{pre}.a{i}", grads=grads, sumsq=ss,
                                 need_dx=need_dx)
        clip_members.append((a_arena, ("actor", i), grads, ss))
    else:
        dX = engine.mlp_backward(a_arena, d_out, x, ldx, 0, h1, h2, n_rows, ws, f"{pre}.a{i}", adam=adam,
                                 adam_key=("actor", i), sumsq=ss, need_dx=need_dx)
    return dX, ss


def _step_and_log_norm(agent, adam, clip, clip_members, member_ss, norm_out, ms=None):
    """what closes an actor update: clip and step, refresh the bf16 shadows, pick the logged member (the reference's
    random.choice, learning.py:210-212 / 417-419) and write its gradient norm to norm_out"""
    if clip:
        _clip_and_step(adam, clip_members, clip, None, member_shard=ms)
    for actor in agent.actors:  # bf16 mode: the actor step ran on the fp32 masters; refresh the shadows
        for ar in actor.__dict__.get("_ssac_arenas", {}).values():
            ar.sync_shadow()
    if ms is not None:   # the pick is over the GLOBAL ensemble; a rank that does not hold it logs its first member's norm
        k = ms.local(rng.choice(range(ms.ensemble_size))) or 0
    else:
        pick = rng.choice(agent.actors)
        k = next(j for j, a_ in enumerate(agent.actors) if a_ is pick)
    if member_ss[k] is not None:  # (None: the fused path's log launch wrote the norm already)
        check(lib.ssac_group_norms(member_ss[k].data_ptr(), 1, member_ss[k].numel(), adam.ctl.ptr if clip else 0,
                                   norm_out.data_ptr(), engine.stream()))


def _bc_head_bwd(head, out_ptr, ld_out, a, mask_ptr, B, A, lo, hi, scale, d_out_ptr, ld_d, log_ptr, total_ptr, st):
    """ONE behavioural-cloning loss launch: scale * -mean(mask * log pi(a | .)) of the data action `a` under the `head`
    ("discrete", "deterministic": Normal(tanh(out), 1e-4), distributions.py:107-114, else the tanh-normal with log-std
    bounds lo / hi), its gradient to d_out, the unscaled loss to log_ptr and the scaled one added to total_ptr"""
    if head == "discrete":
        check(lib.ssac_bc_discrete_bwd(out_ptr, a.data_ptr(), a.stride(0), mask_ptr, B, A, scale, d_out_ptr, log_ptr,
                                       total_ptr, st))
    elif head == "deterministic":
        check(lib.ssac_bc_det_logprob_bwd(out_ptr, ld_out, a.data_ptr(), a.stride(0), mask_ptr, B, A, scale, d_out_ptr,
                                          ld_d, log_ptr, total_ptr, st))
    else:
        check(lib.ssac_bc_logprob_bwd(out_ptr, ld_out, a.data_ptr(), a.stride(0), mask_ptr, B, A, lo, hi, scale,
                                      d_out_ptr, ld_d, log_ptr, total_ptr, st))


def _action_invariance_bwd(head, out_o, aug_ptr, ld, a_inv, olp, B, A, lo, hi, scale, d_out_ptr, log_ptr, total_ptr, st):
    """ONE launch of the action invariance constraint (learning_utils.py:272-285): loss and gradient at the actor's output
    on the AUGMENTED observations (aug_ptr, leading dimension ld, as d_out's), against the action a_inv sampled at the
    original ones with log-probability olp there -- a deterministic head's is tanh(out_o), which the kernel takes itself"""
    if head == "discrete":
        check(lib.ssac_action_invariance_discrete_bwd(out_o.data_ptr(), aug_ptr, a_inv.data_ptr(), B, A, scale,
                                                      d_out_ptr, log_ptr, total_ptr, st))
    elif head == "deterministic":
        check(lib.ssac_action_invariance_det_bwd(out_o.data_ptr(), ld, aug_ptr, ld, B, A, scale, d_out_ptr, ld, log_ptr,
                                                 total_ptr, st))
    else:
        check(lib.ssac_action_invariance_bwd(aug_ptr, ld, a_inv.data_ptr(), A, olp.data_ptr(), B, A, lo, hi, scale,
                                             d_out_ptr, ld, log_ptr, total_ptr, st))


_OfflinePlan = collections.namedtuple("_OfflinePlan",
                                      "head out_cols row_blocks inv_draw masked train_enc enc_grad enc_path")


@functools.lru_cache(maxsize=None)
def _offline_member_plan(kind, discrete, filter_, invariance, pixel, update_encoder, A):
    """THE decision of one member's offline actor update, made once from the call's flags (invariance: bool(actor_lambda));
    touches no device and draws nothing.  The Beta refusals of offline_actor_update have passed.
    head: the BC loss launch -- "discrete", "beta", "deterministic" or "tanh_normal"; out_cols: the head's columns.
    row_blocks: 2 with the invariance constraint (the BC rows and the AUGMENTED rows as one stacked pass), else 1.
    inv_draw: the host draw of the constraint's step (1) -- "categorical" (rng.draw_categorical), "normal"
      (rng.draw_normal((B, A))), None (no constraint, or a deterministic head: its sample is tanh(out), no draw).
    masked: the advantage filter's row mask weighs the BC loss.
    train_enc: the BC warm-up (main.py:292-312) trains a pixel encoder THROUGH the BC loss, then clip + encoder_optimizer.step().
    enc_grad: the actor's input gradient is wanted -- also for the constraint alone, which reaches the encoder through the
      AUGMENTED observations whether or not update_encoder is set (only encoder_optimizer.step() depends on it).
    enc_path: where that gradient goes -- "stacked" (the stacked pass's engine.backward, stepped behind the last member),
      "single" (_encoder_step), None."""
    head = "discrete" if discrete else kind if kind in ("beta", "deterministic") else "tanh_normal"
    train_enc = update_encoder and pixel
    enc_grad = train_enc or (invariance and pixel)
    return _OfflinePlan(
        head=head, out_cols=A if head in ("discrete", "deterministic") else 2 * A, row_blocks=2 if invariance else 1,
        inv_draw={"discrete": "categorical", "tanh_normal": "normal"}.get(head) if invariance else None,
        masked=filter_, train_enc=train_enc, enc_grad=enc_grad,
        enc_path="stacked" if (enc_grad and invariance) else "single" if train_enc else None)


class _OfflineMember:
    """ONE ensemble member's offline actor update: i, actor and a_arena, plan (_offline_member_plan), lo / hi (log-std
    bounds of a tanh-normal head), rd (replay dict), mask (the advantage filter's rows, None: all); of the invariance
    constraint's step (1): out_o (the actor at the original observations), a_inv and olp (the action sampled there and
    its log-probability) and eps (the draw, kept alive to the end of the member's launches); s_rep (the actor's B or 2B
    input rows) with its row stride lds, and eng (the encoder engine behind a stacked pixel pass)"""
    __slots__ = ("i", "actor", "a_arena", "plan", "lo", "hi", "rd", "mask", "out_o", "a_inv", "olp", "eps", "s_rep", "lds",
                 "eng")


def _offline_inputs(m, c):
    """the member's replay dict, the advantage filter's mask (the estimator draws its candidates here), the arena"""
    if c.premade_replay_dicts is not None:
        m.rd = c.premade_replay_dicts[m.i]
    else:
        m.rd = lu.sample_move_and_augment(buffer=c.buffer, batch_size=c.batch_size, augmenter=c.augmenter,
                                          aug_mix=c.aug_mix, per=c.per, _invariance=m.plan.row_blocks == 2)
    m.mask = None
    if m.plan.masked:
        o, a = m.rd["primary_batch"][0], m.rd["primary_batch"][1]
        m.mask = c.agent.adv_estimator.evaluate(o, a, m.i, want=("mask",), log_ptr=c.log + 4 * lu.L_ADVW)["mask"]
        c.logs["losses/adv_weights_mean"] = c.slot[lu.L_ADVW]
    m.a_arena = engine.bind_arena(m.actor, "self", [m.actor], c.dev)


def _offline_invariance_sample(m, c):
    """action invariance (learning_utils.py:272-285), step (1): at the ORIGINAL observations, without gradient, sample an
    action from the actor's distribution and keep its log-probability there"""
    if m.rd.get("augmented_obs") is None:
        raise NotImplementedError("actor_lambda needs replay dicts made with the invariance observations")
    ws, i, B, A, enc = c.ws, m.i, c.batch_size, m.actor.action_size, c.agent.encoder
    os_rep = lu.encode(enc, m.rd["original_obs"][0], dst=ws.get("bc.osrep", (B, enc.embedding_dim)) if c.pixel else None)
    _, _, m.out_o = engine.mlp_forward(m.a_arena, os_rep, lu._row_stride(os_rep), 0, B, ws, f"bc.o{i}", save=False)
    m.olp = ws.get(f"bc.olp{i}", (B,))
    m.a_inv = m.eps = None   # a deterministic head's o_dist.sample() is tanh(out_o): no draw
    if m.plan.inv_draw == "categorical":
        m.a_inv = ws.get(f"bc.ainv{i}", (B,))
        m.a_inv.copy_(rng.draw_categorical(m.out_o[0]))   # o_dist.sample() (device generator, as the reference)
    elif m.plan.inv_draw == "normal":
        m.a_inv = ws.get(f"bc.ainv{i}", (B, A))
        m.eps = rng.draw_normal((B, A), c.dev)
        check(lib.ssac_tanh_normal_fwd(m.out_o.data_ptr(), 2 * A, m.eps.data_ptr(), B, A, m.lo, m.hi, m.a_inv.data_ptr(), A,
                                       0, m.olp.data_ptr(), c.st))


def _offline_representation(m, c):
    """the rows the actor runs on.  With the invariance constraint the BC rows and the AUGMENTED rows go through the
    encoder / actor as ONE stacked 2B-row pass: their weight gradients add up inside one backward"""
    enc, o, B = c.agent.encoder, m.rd["primary_batch"][0], c.batch_size
    m.eng = None
    if m.plan.row_blocks == 1:
        m.s_rep = lu.encode(enc, o, save=m.plan.train_enc)
    elif c.pixel:
        m.eng, m.s_rep = lu.encode_stacked(enc, o, m.rd["augmented_obs"][0], c.ws, "bc.img2", c.dev)
    else:
        s_rep, as_rep = lu.encode(enc, o), lu.encode(enc, m.rd["augmented_obs"][0])
        m.s_rep = c.ws.get("bc.x2", (2 * B, s_rep.shape[1]))
        m.s_rep[:B].copy_(s_rep)
        m.s_rep[B:].copy_(as_rep)
    m.lds = lu._row_stride(m.s_rep)


def _offline_loss_head(m, c):
    """the actor on the member's rows, the BC loss head on rows [0, B), the invariance constraint on rows [B, 2B)
    -> (h1, h2 of the forward, dL/d(output))"""
    ws, st, slot, i, plan, B, A = c.ws, c.st, c.slot, m.i, m.plan, c.batch_size, m.actor.action_size
    a, rows, O, total_ptr = m.rd["primary_batch"][1], plan.row_blocks * B, plan.out_cols, c.log + 4 * lu.L_BC_TOTAL
    ah1, ah2, aout = engine.mlp_forward(m.a_arena, m.s_rep, m.lds, 0, rows, ws, f"bc.a{i}")
    d_out = ws.get(f"bc.dout{i}", (1, rows, O))
    if plan.head == "beta":
        # plain behavioural cloning, loss_i = -mean(log pi(a_data|s)) (learning_utils.py:241-269, filter_=False) with
        # x = (clamp(a, +-0.99) + 1) / 2; the two loss logs are reduced from log pi on the device
        xg, lpg = ws.get(f"bc.xb{i}", (B, A)), ws.get(f"bc.lpb{i}", (B,))
        beta.given_logp(aout, B, A, a, lpg, xg)
        check(lib.ssac_beta_bwd(0, 0, 0, 0, 0, aout.data_ptr(), 2 * A, xg.data_ptr(), B, A, 0, 0, -c.inv_e, 1,
                                d_out.data_ptr(), 2 * A, st))
        loss_i = lpg.mean().neg()
        slot[lu.L_BC0 + i].copy_(loss_i)
        slot[lu.L_BC_TOTAL].add_(loss_i * c.inv_e)
    else:
        _bc_head_bwd(plan.head, aout.data_ptr(), O, a, engine._ptr(m.mask), B, A, m.lo, m.hi, c.inv_e, d_out.data_ptr(), O,
                     c.log + 4 * (lu.L_BC0 + i), total_ptr, st)
    if plan.row_blocks == 2:
        _action_invariance_bwd(plan.head, m.out_o, aout[0, B:].data_ptr(), O, m.a_inv, m.olp, B, A, m.lo, m.hi,
                               float(c.actor_lambda) * c.inv_e, d_out[0, B:].data_ptr(), c.log + 4 * lu.L_ACT_INV,
                               total_ptr, st)
    return ah1, ah2, d_out


def _offline_backward(m, c, ah1, ah2, d_out):
    """the actor's backward and the encoder's share of it (ensemble members share the encoder: member i > 0 adds its
    gradient, the clip / step follows the last member)  -> the member's sum-of-squares slots"""
    ws, i, plan, B, S, last = c.ws, m.i, m.plan, c.batch_size, m.s_rep.shape[1], m.i == c.E - 1
    dX, ss = _actor_backward(m.a_arena, d_out, m.s_rep, m.lds, ah1, ah2, plan.row_blocks * B, ws, "bc", i, c.adam,
                             c.actor_clip, c.clip_members, need_dx=plan.enc_grad)
    if plan.enc_path == "stacked":
        # the BC rows carry a gradient only when the encoder is trained through the BC loss (filtered_bc_loss computes
        # s_rep without gradient otherwise), the augmented rows always do; the encoder is clipped and logged either
        # way and stepped only with update_encoder (learning.py:203-208)
        d_rep = ws.get("bc.drep2", (2 * B, S))
        d_rep.copy_(dX[0])
        if not plan.train_enc:
            d_rep[:B].zero_()
        m.eng.backward(d_rep, accumulate=i > 0)
        if last:
            m.eng.optimizer_step(c.encoder_optimizer, c.encoder_clip, norm_out=c.slot[lu.L_ENC_GN:], step=plan.train_enc)
    elif plan.enc_path == "single":  # (dX was taken before the epilogue of the weight-gradient launch touched W1)
        _encoder_step(c.agent.encoder, c.encoder_optimizer, c.encoder_clip, dX, S, ws, c.slot, c.dev, accumulate=i > 0,
                      step=last)
    return ss


def offline_actor_update(buffer, agent, actor_optimizer, encoder_optimizer, batch_size, actor_clip,
                         update_encoder, encoder_clip, augmenter, actor_lambda, aug_mix,
                         premade_replay_dicts=None, per=True, discrete=False, filter_=True):
    """learning.py:144-219: advantage-filtered behavioural cloning (AWAC / AFBC actor update), optionally on a
    prioritised batch whose priorities are refreshed from the advantage afterwards.  What a member's update consists of
    is decided in ONE place, _offline_member_plan; the steps below read that answer."""
    engine.require_gpu()
    lu.ensure_adopted(agent, buffer)
    encoder_base.refuse_unsupported(agent, "offline_actor_update", actor_lambda=actor_lambda)
    if not discrete and lu.actor_kind(agent.actors[0]) == "beta":
        if filter_:
            beta.refuse("offline_actor_update with the advantage filter (filter_=True)")
        if actor_lambda:
            beta.refuse("offline_actor_update with the action invariance constraint (actor_lambda)")
    c = types.SimpleNamespace(**locals())   # the call: its arguments, and below what every member shares
    E = c.E = agent.ensemble_size
    pixel = c.pixel = not lu.is_identity(agent.encoder)
    dev = c.dev = next(agent.actors[0].parameters()).device
    c.ws = lu.agent_ws(agent, dev)
    adam = c.adam = engine.adam_group(actor_optimizer, dev)
    slot = c.slot = lu.log_block(dev, adam)
    c.log = slot.data_ptr()   # (word k of the fp32 log block: c.log + 4 * k, the address slot[k:] has)
    logs = c.logs = {}
    c.st = engine.stream()
    c.inv_e = 1.0 / E
    c.clip_members, member_ss = [], []
    for i in range(E):
        m = _OfflineMember()
        m.i, actor = i, agent.actors[i]
        m.actor = actor
        plan = m.plan = _offline_member_plan(lu.actor_kind(actor), bool(discrete), bool(filter_), bool(actor_lambda), pixel,
                                             bool(update_encoder), actor.action_size)
        m.lo, m.hi = (float(actor.log_std_low), float(actor.log_std_high)) if plan.head == "tanh_normal" else (0.0, 0.0)
        _offline_inputs(m, c)
        if plan.row_blocks == 2:
            _offline_invariance_sample(m, c)
        _offline_representation(m, c)
        ah1, ah2, d_out = _offline_loss_head(m, c)
        logs[f"losses/filterd_bc_loss_{i}"] = slot[lu.L_BC0 + i]
        member_ss.append(_offline_backward(m, c, ah1, ah2, d_out))
    logs["losses/filtered_bc_overall_loss"] = slot[lu.L_BC_TOTAL]
    _step_and_log_norm(agent, adam, actor_clip, c.clip_members, member_ss, slot[lu.L_BC_GN:])
    logs["gradients/actor_offline_grad_norm"] = slot[lu.L_BC_GN]
    logs["gradients/encoder_offline_actorloss_grad_norm"] = slot[lu.L_ENC_GN]  # identity encoders: no gradient
    if per:
        lu.adjust_priorities(logs, m.rd, agent, buffer)
    return logs


def markov_state_abstraction_update(buffer, agent, optimizer, batch_size, augmenter, aug_mix, discrete,
                                    inverse_coeff, contrastive_coeff, smoothness_coeff, smoothness_max_dist,
                                    grad_clip):
    """learning.py:266-341: the self-supervised abstraction loss of "Learning Markov State Abstractions for Deep RL" --
    inverse model (which action led from s to s'), contrastive model (is (s, s') a real transition; negatives by
    shuffling s' over the batch) and a smoothness hinge on ||s' - s|| -- trained through ONE optimizer over
    chain(encoder, inverse_model, contrastive_model) (main.py:218-224).

    The two MLPs run on the engine's forward / backward kernels; a pixel encoder takes s and s' as ONE stacked 2B-row
    pass (the weight gradients of the two uses add up inside its backward).  Loss heads: ssac_bc_logprob_bwd /
    ssac_bc_discrete_bwd (log-probability of the data action), ssac_bce_sigmoid_bwd, ssac_markov_smoothness_bwd."""
    engine.require_gpu()
    lu.ensure_adopted(agent, buffer)
    encoder_base.refuse_unsupported(agent, "markov_state_abstraction_update")
    if not discrete and getattr(agent.inverse_model, "dist_impl", None) == "beta":
        beta.refuse("markov_state_abstraction_update with a Beta inverse model")
    inv, con = agent.inverse_model, agent.contrastive_model
    dev = next(inv.parameters()).device
    ws = lu.agent_ws(agent, dev)
    adam = engine.adam_group(optimizer, dev)
    slot = lu.log_block(dev, adam)  # a log block of its own; advances the optimizer step
    st = engine.stream()
    rd = lu.sample_move_and_augment(buffer=buffer, batch_size=batch_size, augmenter=augmenter, aug_mix=aug_mix,
                                    per=False)
    o, a, _, o1, _ = rd["primary_batch"]
    B = batch_size
    ident = lu.is_identity(agent.encoder)
    if ident:
        s_rep, s1_rep = lu.encode(agent.encoder, o), lu.encode(agent.encoder, o1)
        D = s_rep.shape[1]
    else:
        eng, s_all = lu.encode_stacked(agent.encoder, o, o1, ws, "mk.img", dev)
        D = eng.emb
        s_rep, s1_rep = s_all[:B], s_all[B:]
    # ---- inputs: [s | s'] for the inverse model; [s | s'] over [s | s'[perm]] for the contrastive model
    perm = rng.draw_permutation(B)
    perm_dev = perm.to(dev)
    x_inv = ws.get("mk.xinv", (B, 2 * D))
    x_inv[:, :D].copy_(s_rep)
    x_inv[:, D:].copy_(s1_rep)
    x_con = ws.get("mk.xcon", (2 * B, 2 * D))
    x_con[:B].copy_(x_inv)
    x_con[B:, :D].copy_(s_rep)
    torch.index_select(s1_rep, 0, perm_dev, out=x_con[B:, D:])
    i_arena = engine.bind_arena(inv, "self", [inv], dev)
    c_arena = engine.bind_arena(con, "self", [con], dev)
    ih1, ih2, iout = engine.mlp_forward(i_arena, x_inv, 2 * D, 0, B, ws, "mk.inv")
    ch1, ch2, cout = engine.mlp_forward(c_arena, x_con, 2 * D, 0, 2 * B, ws, "mk.con")
    # ---- loss heads (each also leaves its share of d markov_loss / d output)
    A = inv.action_size
    if discrete:
        head, O, lo, hi, inv_scale, coeff = "discrete", A, 0.0, 0.0, 1.0, float(inverse_coeff)
    else:
        # -a_dist.log_prob(a).mean(): the mean runs over the B x A per-dimension log-probabilities (learning.py:298)
        head, O, lo, hi = "tanh_normal", 2 * A, float(inv.log_std_low), float(inv.log_std_high)
        inv_scale, coeff = 1.0 / A, float(inverse_coeff) / A
    d_iout = ws.get("mk.dinv", (1, B, O))
    _bc_head_bwd(head, iout.data_ptr(), O, a, 0, B, A, lo, hi, coeff, d_iout.data_ptr(), O, slot[lu.L_MK_RAW:].data_ptr(),
                 slot[lu.L_MK_TMP:].data_ptr(), st)
    d_cout = ws.get("mk.dcon", (1, 2 * B, 1))
    check(lib.ssac_bce_sigmoid_bwd(cout.data_ptr(), B, 2 * B, float(contrastive_coeff), d_cout.data_ptr(),
                                   slot[lu.L_MK_CON:].data_ptr(), st))
    d_all = None if ident else ws.get("mk.dall", (2 * B, D))
    check(lib.ssac_markov_smoothness_bwd(s_rep.data_ptr(), lu._row_stride(s_rep), s1_rep.data_ptr(),
                                         lu._row_stride(s1_rep), B, D, float(smoothness_max_dist),
                                         float(smoothness_coeff), engine._ptr(None if ident else d_all[:B]), D,
                                         engine._ptr(None if ident else d_all[B:]), D, 0,
                                         slot[lu.L_MK_SMOOTH:].data_ptr(), st))
    check(lib.ssac_markov_logs(slot[lu.L_MK_RAW:].data_ptr(), inv_scale, slot[lu.L_MK_CON:].data_ptr(),
                               slot[lu.L_MK_SMOOTH:].data_ptr(), float(inverse_coeff), float(contrastive_coeff),
                               float(smoothness_coeff), slot[lu.L_MK_LOSS:].data_ptr(), st))
    # ---- backward: gradients stored (the clip needs the joint norm first), input gradients only for a real encoder
    members = []
    for tag, arena, d_out, x, h1, h2, rows in (("mk.inv", i_arena, d_iout, x_inv, ih1, ih2, B),
                                               ("mk.con", c_arena, d_cout, x_con, ch1, ch2, 2 * B)):
        grads = ws.get(tag + ".g", (arena.params.numel(),), zero=True)
        ss = ws.get(tag + ".ss", (engine.wgrad_tiles_total(arena),))
        dx = engine.mlp_backward(arena, d_out, x, 2 * D, 0, h1, h2, rows, ws, tag, grads=grads, sumsq=ss,
                                 need_dx=not ident)
        members.append((arena, ("markov", tag), grads, ss, dx))
    allss = [members[0][3], members[1][3]]
    if not ident:
        dxi, dxc = members[0][4][0], members[1][4][0]
        d_all[:B] += dxi[:, :D]
        d_all[:B] += dxc[:B, :D]
        d_all[:B] += dxc[B:, :D]
        d_all[B:] += dxi[:, D:]
        d_all[B:] += dxc[:B, D:]
        d_all[B:].index_add_(0, perm_dev, dxc[B:, D:])  # (a permutation: every row receives exactly one addend)
        eng.backward(d_all)
        ss_enc = ws.get("mk.enc.ss", (int(lib.ssac_sumsq_blocks()),))
        eng.grad_sumsq(ss_enc)
        allss.append(ss_enc)
    # ---- clip_grad_norm_ over chain(encoder, inverse, contrastive) jointly, then optimizer.step() (learning.py:321-330)
    cat = torch.cat(allss)
    check(lib.ssac_clip_coef(adam.ctl.ptr, cat.data_ptr(), cat.numel(), float(grad_clip) if grad_clip else 0.0, 0, st))
    for arena, key_, grads, _, _ in members:
        m, v = adam.moments_for(key_, arena.params)
        check(lib.ssac_adam_step(arena.params.data_ptr(), m.data_ptr(), v.data_ptr(), grads.data_ptr(),
                                 arena.params.numel(), adam.ctl.ptr, st))
        arena.sync_shadow()
    if not ident:
        eng.adam_step(adam)
    # ---- logs (learning.py:332-340): the norms are read after the clip rescaled the gradients
    scale = adam.ctl.ptr if grad_clip else 0
    for (arena, _, _, ss, _), off in zip(members, (lu.L_MK_GN_INV, lu.L_MK_GN_CON)):
        check(lib.ssac_group_norms(ss.data_ptr(), 1, ss.numel(), scale, slot[off:].data_ptr(), st))
    if not ident:
        check(lib.ssac_group_norms(allss[2].data_ptr(), 1, allss[2].numel(), scale, slot[lu.L_MK_GN_ENC:].data_ptr(), st))
    return {"gradients/contrastive_model_grad_norm": slot[lu.L_MK_GN_CON],
            "gradients/inverse_model_grad_norm": slot[lu.L_MK_GN_INV],
            "gradients/encoder_markovloss_grad_norm": slot[lu.L_MK_GN_ENC],
            "losses/markov_loss": slot[lu.L_MK_LOSS + 3],
            "losses/inverse_model_loss": slot[lu.L_MK_LOSS],
            "losses/contrastive_model_loss": slot[lu.L_MK_LOSS + 1],
            "losses/smoothness_loss": slot[lu.L_MK_LOSS + 2]}


def alpha_update(buffer, agent, optimizers, batch_size, log_alphas, augmenter, aug_mix, target_entropy,
                 premade_replay_dicts, discrete):
    engine.require_gpu()
    lu.ensure_adopted(agent, buffer)
    encoder_base.refuse_unsupported(agent, "alpha_update")
    dev = log_alphas[0].device
    ws = lu.agent_ws(agent, dev)
    if engine.CAPTURE is None:
        # this update's block of the log ring as it stands: ssac_alpha_update ASSIGNS its two entries per member and nothing
        # else of the block is handed out, so no launch is spent on clearing it (one of the update's three launches, round 6)
        ring = lu.ring_for(dev)
        slot = ring.buf[ring.advance()]
    else:
        slot = lu.log_block(dev)
    logs = {}
    st = engine.stream()
    ms = parallel.member_shard_of(agent)   # member-sharded rank: log_alphas / optimizers are the LOCAL members'
    if ms is not None and lu.actor_kind(agent.actors[0]) == "beta":
        beta.refuse("alpha_update on a member-sharded agent")
    for ig in range(agent.ensemble_size if ms is None else ms.ensemble_size):
        i = ig if ms is None else ms.local(ig)
        if i is None:   # a member another rank owns: its host draws, in member order
            if premade_replay_dicts is None:
                lu.sample_move_and_augment(buffer=buffer, batch_size=batch_size, augmenter=augmenter, per=False,
                                           aug_mix=aug_mix)
            lu.skip_alpha_draws(agent, agent.actors[0], batch_size, dev)
            continue
        if premade_replay_dicts is not None:
            rd = premade_replay_dicts[i]
        else:
            rd = lu.sample_move_and_augment(buffer=buffer, batch_size=batch_size, augmenter=augmenter,
                                            per=False, aug_mix=aug_mix)
        o = rd["primary_batch"][0]
        s_rep = lu.encode(agent.encoder, o)
        B, S = s_rep.shape
        actor = agent.actors[i]
        a_arena = engine.bind_arena(actor, "self", [actor], dev)
        kind = lu.actor_kind(actor)
        fused_sample = kind == "stochastic" and a_arena.fused
        if not fused_sample:
            _, _, aout = engine.mlp_forward(a_arena, s_rep, lu._row_stride(s_rep), 0, B, ws, f"al.a{i}")
        if kind == "discrete":
            lp_ptr, n_act = aout.data_ptr(), a_arena.out_dim
        else:
            A = actor.action_size
            logp = ws.get(f"al.logp{i}", (B,))
            if fused_sample:
                # actor forward + a_dist.sample() + log pi (learning.py:255) in ONE launch; the noise comes from the
                # agent's Philox stream unless a noise hook is installed (then it is drawn like everywhere else)
                scratch = ws.get(f"al.act{i}", (B, A))
                if lu.IN_KERNEL_NOISE and rng.normal_is_stock():
                    rs = lu.stream_rng(agent, dev)
                    eps_ptr, rng_ptr = 0, C.addressof(rs)
                else:
                    eps = rng.draw_normal((B, A), dev)
                    eps_ptr, rng_ptr = eps.data_ptr(), 0
                check(lib.ssac_actor_sample_fused(C.byref(a_arena.desc()), s_rep.data_ptr(), lu._row_stride(s_rep), B,
                                                  eps_ptr, float(actor.log_std_low), float(actor.log_std_high),
                                                  scratch.data_ptr(), A, 0, logp.data_ptr(), 0, 0, 0, rng_ptr, st))
            elif kind == "beta":
                # a_dist.log_prob(a_dist.sample()) of the Beta head (learning.py:255)
                beta.sample(agent, aout, B, A, "alpha", ws.get(f"al.xb{i}", (B, A)), logp=logp)
            elif kind == "stochastic":
                eps = rng.draw_normal((B, A), dev)  # a_dist.sample() (learning.py:255)
                scratch = ws.get(f"al.act{i}", (B, A))
                check(lib.ssac_tanh_normal_fwd(aout.data_ptr(), 2 * A, eps.data_ptr(), B, A,
                                               float(actor.log_std_low), float(actor.log_std_high),
                                               scratch.data_ptr(), A, 0, logp.data_ptr(), st))
            else:
                import math
                logp.fill_(A * (-math.log(1e-4) - 0.5 * math.log(2 * math.pi)))
            lp_ptr, n_act = logp.data_ptr(), 1
        adam = engine.adam_group(optimizers[i], dev)
        la = log_alphas[i]
        m, v = adam.moments_for("log_alpha", la.data)
        check(lib.ssac_alpha_update(la.data_ptr(), m.data_ptr(), v.data_ptr(), adam.ctl.ptr, lp_ptr, B,
                                    n_act, float(target_entropy), slot[lu.L_ALPHA0 + 2 * i:].data_ptr(), st))
        logs[f"losses/alpha_loss_{ig}"] = slot[lu.L_ALPHA0 + 2 * i]
        logs[f"alphas/alpha_{ig}"] = slot[lu.L_ALPHA0 + 2 * i + 1]
    return logs
