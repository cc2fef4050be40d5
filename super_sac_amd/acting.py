"""The acting path as ONE C call per environment step (agent.py:204-315; csrc/ssac_act.hip).

``Agent.forward`` / ``Agent.sample_action`` with a numpy observation of an identity-encoder agent (a concatenating encoder over
several vector keys counts as one once an update has recognised it: the host lays the row out in the encoder's order), of a pixel-encoder agent
on uint8 or float32 frames, or of an agent with a two-layer MLP encoder (below), take this path: the first call at a given (rule, num_envs) RECORDS the rule's launches -- every actor's
forward (+ tanh-normal sample from the engine's Philox stream, in the kernel), SUNRISE's ensemble-Q passes on the stacked
candidates, the rule's reduction (UCB arg-max / mean of mean actions / categorical draw / arg-max of mean probabilities) and
the publish step -- into a launch list of an ``ssac_act`` plan; every later call is ``ssac_act_run``: the observation is
written straight into device-visible memory, the list is re-issued, the action arrives in pinned host memory.  No torch op,
no hipMemcpy, no stream synchronisation.  Measured (bench.py ``secondary.acting``): see profiles/r6_acting.md.

Discrete agents under SUNRISE's UCB rule (agent.py:259-304, the ``if self.discrete:`` branch) record the packed actors' and the
packed critics' forwards on the state representation and ONE reduction launch (ssac_act_ucb_discrete: a categorical draw per
member, the gather, mean + bonus * std, arg-max); their plan is keyed ("sample", n, bonus).  A pack above SSAC_MAX_NETS
networks is forwarded by several packed launches inside the same list; the reductions take up to 32 members.

Pixel agents: the encoder's launches are recorded in front of the rule's, reading the uint8 frames where the host wrote them.
With ``acting.FLOAT32_FRAMES = True`` (off by default: float frames then act on the general path, as they always did),
float32 frames (a frame-stack or normalising wrapper) get a plan of their own, keyed (rule, num_envs, bonus, "float32"): its
list starts with ssac_act_ingest_f32, which moves the frames out of the host-written buffer for the encoder's first launch.
``rolling=True`` -- the default of the training loop (main.super_sac, evaluation.run_env) -- is the same call as
``rolling=False`` for an encoder whose forward_rolling / reset_rolling are the pass-through inherited from ``Encoder`` (this
package's or the reference's; no shipped encoder overrides them): the plan is not keyed on it, both share one noise stream.

MLP-encoder agents (``--shared_encoder`` of the reference's gym / dmc / d4rl scripts, its visgrid encoder, nets.MlpEncoder: what
mlp_encoder.find_mlp_encoder recognises -- on the first acting call, if no update has looked at the encoder yet, with the
shapes of that observation and a probe that moves no global random stream): the observation under the encoder's
``ssac_obs_key`` may have any shape with num_envs * in_features elements (visgrid hands over (18, 18)) and any dtype that
``np.ascontiguousarray(v, np.float32)`` converts as ``_process_obs``'s ``.float()`` does -- the identity plan's rule; the plan's
observation buffer holds float32 rows and its key is (rule, num_envs, bonus) whatever dtype the caller hands over.  The
encoder's forward (MlpEncoderEngine.forward_ptr, in the form the engine picks for that many rows) is recorded in front of the
rule's launches, from the observation buffer into a plan-owned (num_envs, embedding) buffer; its launches point into the
engine's arena, so an optimizer step or an in-place load_state_dict is seen by the next call, and the encoder's first-layer
weight pointer is part of the plan's signature, so a deep copy, a ``.to()`` or a re-packed arena drops the plan.
``rolling=True`` follows the pixel rule.  Measured: profiles/mlp_encoder.md ("Acting").

What stays on the general path (agent.py's eager code, unchanged): MLP-encoder agents the update functions refuse (bf16-marked
networks, critic- or member-sharded agents), encoders that override their rolling interface (they keep
state between calls) under ``rolling=True``, float32 frames unless FLOAT32_FRAMES is set, float64 and other frame dtypes, injected noise
(a hook on ``rng.draw_normal`` -- the parity tests), ensembles above 32 members, UCB networks outside the fused kernels' shapes
(hidden > 256), ``from_cpu=False`` callers, Beta actors (beta_dist=True), and every (agent, rule, num_envs) whose recording
failed once (the call that met the failure included: it is served by the general path, the key is not tried again).  Host RNG contract: the Python ``random`` draws of the reference (``random.choice`` of the
acting actor / of the logged distribution) are consumed exactly as before."""
import ctypes as C
import random
import warnings
import weakref

import numpy as np
import torch

from . import _lib, engine, nets, rng
from . import learning_utils as lu
from ._lib import check, lib

ENABLED = True
FLOAT32_FRAMES = False                 # record pixel plans for float32 frames as well (off: they act on the general path, as before)
_PLANS = weakref.WeakKeyDictionary()   # agent -> {(rule, num_envs, bonus) [+ ("float32",) for float frames]: _Plan}
_FAILED = weakref.WeakKeyDictionary()  # agent -> {plan key}: a recording failed, the general path serves the key from then on
_SERIAL = [0]
MAX_MEMBERS = 32                       # SSAC_ACT_MAX_MEMBERS: what the rules' reduction kernels take
MAX_NETS = 64                          # SSAC_MAX_NETS: the networks of ONE packed forward launch
_STREAM_SALT = 0x41C7A11D5EEDB00C      # the acting noise stream: the agent's engine seed under another key


class _Plan:
    def __init__(self, agent, rule, n, dev, pixel_shape=None, pixel_dtype=np.uint8, mlp_in=None):
        self.rule, self.n, self.dev = rule, n, dev
        self.S = agent.encoder.embedding_dim
        self.pixel_shape = pixel_shape    # (C, H, W) of an image observation that goes through the pixel encoder, or None
        self.mlp_in = mlp_in              # values per row of an observation that goes through a two-layer MLP encoder, or None
        self.obs_dtype = np.dtype(np.float32 if pixel_shape is None else pixel_dtype)   # what the host writes: uint8 / float32 frames
        self.key = getattr(agent.encoder, "ssac_identity_key", None) if pixel_shape is None and mlp_in is None \
            else getattr(agent.encoder, "ssac_obs_key", "obs")
        # a concatenating encoder's ((key, width), ...): the host lays the row out in that order (act)
        self.concat = getattr(agent.encoder, "ssac_concat_keys", None) if self.key is None else None
        self.discrete = bool(agent.discrete)
        self.A = agent.act_space_size
        self.out_floats = n if self.discrete else n * self.A
        obs_bytes = 4 * n * (self.S if mlp_in is None else mlp_in) if pixel_shape is None \
            else n * int(np.prod(pixel_shape)) * self.obs_dtype.itemsize
        self.handle = lib.ssac_act_create(obs_bytes, self.out_floats)
        if not self.handle:
            raise RuntimeError("libssac_hip: " + lib.ssac_last_error().decode())
        self.obs_dev = lib.ssac_act_obs(self.handle)
        self.counter = lib.ssac_act_counter(self.handle)
        _SERIAL[0] += 1
        self.serial = _SERIAL[0]
        self.result = np.empty(self.out_floats, np.float32)
        self.bufs = []        # device tensors the recorded launches point at
        self.outs = []        # per actor: its head output (n x out_dim), what return_dist hands back
        self.sig = None
        self.lists = {}       # which-actor -> list index

    def buf(self, *shape):
        t = torch.zeros(*shape, device=self.dev)
        self.bufs.append(t)
        return t

    def rng_for(self, agent, member):
        seed = (lu.noise_stream(agent, self.dev)[0] ^ _STREAM_SALT) & (2 ** 64 - 1)
        return _lib.Rng(seed, self.counter, (self.serial << 48) + (member << 40))

    def __del__(self):
        try:
            if self.handle:
                lib.ssac_act_destroy(self.handle)
        except Exception:   # noqa: BLE001  (interpreter shutdown)
            pass


def _signature(agent, with_critics):
    sig = [a.fc1.weight.data_ptr() for a in agent.actors]
    if not lu.is_identity(agent.encoder):
        conv = _conv_module(agent)
        mlp = None if conv is not None else agent.encoder.__dict__.get("_ssac_mlp_desc")
        # (an MLP encoder's first-layer weight: a deep copy, a .to() or a re-packed arena moves it)
        sig.append(conv.conv1.weight.data_ptr() if conv is not None else mlp[0].weight.data_ptr() if mlp else 0)
    if with_critics:
        sig += [c.nets[0].fc1.weight.data_ptr() for c in agent.critics]
    return tuple(sig)


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _conv_module(agent):
    """the convolutional module inside the agent's encoder wrapper (found once per encoder object)"""
    enc = agent.encoder
    if "_ssac_conv_mod" not in enc.__dict__:
        from . import conv_encoder
        enc.__dict__["_ssac_conv_mod"] = conv_encoder.find_conv_module(enc)
    return enc.__dict__["_ssac_conv_mod"]


def _pixel_obs(agent, obs, num_envs):
    """(key, (C, H, W), dtype) when the observation is a uint8 -- with FLOAT32_FRAMES also a float32 -- image batch for a pixel
    encoder of this package, else None (float64 and every other dtype: the general path)"""
    conv = _conv_module(agent)   # (first: recognising a plain conv stack settles its observation key)
    key = getattr(agent.encoder, "ssac_obs_key", None)
    if key is None:
        return None
    v = obs.get(key)
    if conv is None or not isinstance(v, np.ndarray) or not (v.dtype == np.uint8 or (FLOAT32_FRAMES and v.dtype == np.float32)):
        return None
    shape = tuple(v.shape[-3:])
    if len(shape) != 3 or v.size != num_envs * int(np.prod(shape)) or shape[0] != conv.conv1.in_channels:
        return None
    return key, shape, v.dtype


def _probe_shapes(obs, num_envs):
    """{key: shape-only tensor with a leading batch axis} of a numpy observation, as _process_obs would batch it"""
    return {k: torch.empty(((1,) if num_envs == 1 else ()) + tuple(v.shape), device="meta")
            for k, v in obs.items() if isinstance(v, np.ndarray)}


def _mlp_obs(agent, obs, num_envs):
    """(key, values per row) when the observation feeds a two-layer MLP encoder (mlp_encoder.find_mlp_encoder: an encoder
    nobody has looked at yet is recognised here, on its first acting call, with the shapes of this observation; the probe
    moves no global random stream) and has num_envs rows of lin0.in_features values -- in any shape and any dtype that
    converts to float32, the identity plan's rule -- else None.  Agents the update functions refuse with such an encoder
    (encoder_base.refuse_unsupported: bf16-marked networks, critic- or member-sharded agents) act on the general path"""
    from . import mlp_encoder, parallel
    enc = agent.encoder
    if _conv_module(agent) is not None:
        return None
    desc = mlp_encoder.find_mlp_encoder(enc, None if mlp_encoder.is_mlp_encoder(enc) else _probe_shapes(obs, num_envs))
    if desc is None:
        return None
    lin0, key = desc[0], desc[3]
    v = obs.get(key)
    if not isinstance(v, np.ndarray) or v.size != num_envs * lin0.in_features:
        return None
    if any(o.__dict__.get("_ssac_precision") == "bf16" for o in list(agent.actors) + list(agent.critics)):
        return None
    if parallel.shard_of(agent) is not None or parallel.member_shard_of(agent) is not None:
        return None
    return key, lin0.in_features


def _inherits_rolling(cls):
    """the class's rolling interface is the pass-through it inherited -- forward_rolling = forward, reset_rolling a no-op
    (nets.Encoder here; nets/__init__.py:26-30 of the reference, for adopted agents: its Encoder is found among the bases by
    name, the package is not imported) -- i.e. neither function is overridden: the function OBJECTS are compared"""
    bases = [nets.Encoder] + [b for b in cls.__mro__ if (b.__module__, b.__name__) == ("super_sac.nets", "Encoder")]
    found = tuple(getattr(cls, name, None) for name in ("forward_rolling", "reset_rolling"))
    return None not in found and any(found == tuple(b.__dict__.get(name) for name in ("forward_rolling", "reset_rolling"))
                                     for b in bases)


def _rolling_passthrough(enc):
    """no state between the calls of this encoder: rolling=True computes what rolling=False does (asked once per encoder object)"""
    if "_ssac_roll_pass" not in enc.__dict__:
        enc.__dict__["_ssac_roll_pass"] = _inherits_rolling(type(enc)) and "forward_rolling" not in enc.__dict__ \
            and "reset_rolling" not in enc.__dict__
    return enc.__dict__["_ssac_roll_pass"]


def _eligible(agent, obs, num_envs, sample, rolling):
    if not (ENABLED and isinstance(obs, dict) and engine.CAPTURE is None):
        return False
    if lu.is_identity(agent.encoder):
        # (a foreign concatenating encoder is recognised by the first update that meets it, learning_utils.ensure_adopted,
        #  never here: until then its calls take the general path)
        concat = getattr(agent.encoder, "ssac_concat_keys", None)
        for key, width in concat or ((agent.encoder.ssac_identity_key, agent.encoder.embedding_dim),):
            v = obs.get(key)
            if not isinstance(v, np.ndarray) or v.size != num_envs * width:
                return False
    elif (rolling and not _rolling_passthrough(agent.encoder)) or \
            (_pixel_obs(agent, obs, num_envs) is None and _mlp_obs(agent, obs, num_envs) is None):
        return False          # (an encoder that overrides its rolling interface keeps state between calls: the general path)
    E = len(agent.actors)
    if E > MAX_MEMBERS or agent.act_space_size > 64:
        return False
    kind = lu.actor_kind(agent.actors[0])
    if kind == "beta":
        return False          # (the recorded rules sample the tanh-normal head: Beta actors act on the general path)
    if sample and kind == "stochastic" and not rng.normal_is_stock():
        return False          # injected noise: the general path draws it through the hook
    if sample and agent.ucb_bonus > 0 and (kind not in ("stochastic", "discrete") or E < 2 or len(agent.critics) != E):
        return False
    return True


def _arena_ok(agent, dev, with_critics, sample):
    """every network the rule touches has a launchable forward: the fused MLP kernel, or -- networks outside its shapes, e.g.
    DrQv2's hidden-1024 actor -- the per-layer GEMM family (three launches); the UCB rule's sampling kernels are fused-only"""
    arenas = [engine.bind_arena(a, "self", [a], dev) for a in agent.actors]
    if len(arenas) > 1 and (with_critics or not sample) and not _packable(arenas):
        return False          # (the rules that pack the actors: forward, the UCB rules; a plain sample is one actor's launch)
    if with_critics:
        # the UCB rules: two packs (the members' shapes and, for the tanh-normal head, the log-std bounds must agree), a
        # member's critics inside one packed launch, the reduction's member and action limits
        c_arenas = [c.arena(dev) for c in agent.critics]
        a0 = agent.actors[0]
        if not agent.discrete and any((float(a_.log_std_low), float(a_.log_std_high)) !=
                                      (float(a0.log_std_low), float(a0.log_std_high)) for a_ in agent.actors):
            return False
        return (all(a.fused for a in arenas) and all(c.fused for c in c_arenas) and _packable(c_arenas)
                and len(c_arenas) == len(arenas) and 2 <= len(arenas) <= MAX_MEMBERS
                and all(c.n_nets == c_arenas[0].n_nets for c in c_arenas) and 1 <= c_arenas[0].n_nets <= MAX_NETS
                and agent.act_space_size <= 64)
    return all(a.fused for a in arenas) or lu.actor_kind(agent.actors[0]) != "stochastic"


def _packable(arenas):
    a0 = arenas[0]
    return all((a.in_dim, a.hidden, a.out_dim, a.stride) == (a0.in_dim, a0.hidden, a0.out_dim, a0.stride) for a in arenas)


def _fwd_desc(plan, desc, n_nets, fused, hidden, out_dim, x_ptr, ldx, n_rows, y):
    """y (n_nets x n_rows x out) = MLP(x) for every net of `desc` (shared input rows): one fused launch, or three per-layer
    launches through plan-owned activations (mlps.py:123-129).  More than SSAC_MAX_NETS nets: one such launch (group) per
    SSAC_MAX_NETS nets, each on its slice of the arena and of y"""
    st = engine.stream()
    if n_nets > MAX_NETS:
        for k0 in range(0, n_nets, MAX_NETS):
            k = min(MAX_NETS, n_nets - k0)
            part = _lib.MlpDesc(desc.params + 4 * k0 * desc.net_stride, desc.net_stride, k, desc.in_dim, desc.hidden, desc.out_dim)
            _fwd_desc(plan, part, k, fused, hidden, out_dim, x_ptr, ldx, n_rows, y[k0:k0 + k])
        return
    if fused:
        check(lib.ssac_mlp3_fwd_fused(C.byref(desc), 0, n_nets, x_ptr, ldx, 0, n_rows, 0, 0, y.data_ptr(), st))
        return
    h1, h2 = plan.buf(n_nets, n_rows, hidden), plan.buf(n_nets, n_rows, hidden)
    check(lib.ssac_mlp_layer_fwd(C.byref(desc), 0, 0, n_nets, x_ptr, ldx, 0, n_rows, h1.data_ptr(), hidden, n_rows * hidden, 1, st))
    check(lib.ssac_mlp_layer_fwd(C.byref(desc), 1, 0, n_nets, h1.data_ptr(), hidden, n_rows * hidden, n_rows, h2.data_ptr(), hidden,
                                 n_rows * hidden, 1, st))
    check(lib.ssac_mlp_layer_fwd(C.byref(desc), 2, 0, n_nets, h2.data_ptr(), hidden, n_rows * hidden, n_rows, y.data_ptr(), out_dim,
                                 n_rows * out_dim, 0, st))


def _fwd(plan, arena, x_ptr, ldx, n_rows, y):
    _fwd_desc(plan, arena.desc(), arena.n_nets, arena.fused, arena.hidden, arena.out_dim, x_ptr, ldx, n_rows, y)


class _Pack:
    """the members' networks of one role in ONE plan-owned arena: the members of an ensemble are separate allocations (one arena
    per actor, one per member's critics), so a forward of all of them is one launch PER MEMBER -- ~11 us each for a 16-row
    tile.  A plan copies them into a pack at the head of every call (one multi-tensor launch, a few MB: ~5 us) and runs ONE
    fused launch over the pack instead."""

    def __init__(self, plan, arenas):
        a0 = arenas[0]
        assert all((a.in_dim, a.hidden, a.out_dim, a.stride) == (a0.in_dim, a0.hidden, a0.out_dim, a0.stride) for a in arenas)
        self.n_nets = sum(a.n_nets for a in arenas)
        self.buf = plan.buf(self.n_nets * a0.stride)
        self.srcs = [a.params for a in arenas]
        self.desc = _lib.MlpDesc(self.buf.data_ptr(), a0.stride, self.n_nets, a0.in_dim, a0.hidden, a0.out_dim)
        self.out_dim, self.hidden, self.fused = a0.out_dim, a0.hidden, all(a.fused for a in arenas)

    def segments(self):
        off, out = 0, []
        for s in self.srcs:
            out.append((self.buf.data_ptr() + 4 * off, s.data_ptr(), s.numel()))
            off += s.numel()
        return out


def _pack_launch(packs):
    """one launch: every pack <- its members' arenas (ssac_polyak_multi with tau = 1: t <- 0 t + 1 s)"""
    segs = [sg for p in packs for sg in p.segments()]
    n = len(segs)
    t = (C.c_void_p * n)(*[s[0] for s in segs])
    s_ = (C.c_void_p * n)(*[s[1] for s in segs])
    cnt = (C.c_int64 * n)(*[s[2] for s in segs])
    check(lib.ssac_polyak_multi(t, s_, cnt, n, 1.0, engine.stream()))


def _record(plan, agent, which):
    """_record_launches, or False when it failed: whatever a launch refused (a shape outside its limits, a pack the arena
    checks did not foresee) must not reach the environment loop -- the caller drops the plan and the general path acts"""
    try:
        _record_launches(plan, agent, which)
    except Exception as exc:   # noqa: BLE001  (a refused launch raises RuntimeError, a broken expectation AssertionError)
        plan.error = f"{type(exc).__name__}: {exc}"
        return False
    return True


def _record_launches(plan, agent, which):
    """record the launches of plan.rule for acting actor `which` (None: the rule involves every actor)"""
    dev, n, S, A = plan.dev, plan.n, plan.S, plan.A
    st = engine.stream()
    kind = lu.actor_kind(agent.actors[0])
    E = len(agent.actors)
    arenas = [engine.bind_arena(a, "self", [a], dev) for a in agent.actors]
    if not plan.outs:
        plan.outs = [plan.buf(n, ar.out_dim) for ar in arenas]
        plan.res = plan.buf(max(plan.out_floats, 1))
        plan.logp = plan.buf(max(n * E, 1))
    check(lib.ssac_record_begin())
    done = False
    try:
        x_in = plan.obs_dev      # what the actors read: the observation itself, or the encoder's output
        if plan.pixel_shape is not None:
            # the pixel encoder's forward straight from the uint8 observation buffer (the cast and the /255 normalisation
            # happen in the first layer's patch gather), into a buffer of this plan -- the same launches as lu.encode.
            # float32 frames: one pass (ssac_act_ingest_f32, 16-byte loads and stores) moves them out of the host-written
            # buffer into a plan-owned one first; the encoder reads that as any float image
            plan.srep = plan.buf(n, S)
            img_ptr, u8 = plan.obs_dev, 1
            if plan.obs_dtype == np.float32:
                plan.frames = plan.buf((n * int(np.prod(plan.pixel_shape)) + 3) // 4 * 4)
                check(lib.ssac_act_ingest_f32(plan.obs_dev, plan.frames.data_ptr(), n * int(np.prod(plan.pixel_shape)), st))
                img_ptr, u8 = plan.frames.data_ptr(), 0
            plan.conv_engine.forward_ptr(img_ptr, (n,) + plan.pixel_shape, u8, plan.srep.data_ptr(), S, False)
            x_in = plan.srep.data_ptr()
        elif plan.mlp_in is not None:
            # the MLP encoder's forward on the float32 rows where the host wrote them, into a buffer of this plan; the hidden
            # rows live in the engine's workspace (the plan holds the engine), the launches point into its arena
            plan.srep = plan.buf(n, S)
            plan.enc_engine.forward_ptr(plan.obs_dev, (n, plan.mlp_in), 0, plan.srep.data_ptr(), S, False)
            x_in = plan.srep.data_ptr()
        if plan.rule == "forward":
            if E > 1:   # one launch over the packed actors; plan.outs[e] are views of its output
                pa = _Pack(plan, arenas)
                packed_out = plan.buf(E, n, pa.out_dim)
                plan.outs = [packed_out[e] for e in range(E)]
                _pack_launch([pa])
                _fwd_desc(plan, pa.desc, E, pa.fused, pa.hidden, pa.out_dim, x_in, S, n, packed_out)
            else:
                _fwd(plan, arenas[0], x_in, S, n, plan.outs[0])
            if plan.discrete:
                check(lib.ssac_act_discrete(_ptr_array(plan.outs), E, A, n, A, 0, None, plan.res.data_ptr(), st))
            else:
                check(lib.ssac_act_mean_tanh(_ptr_array(plan.outs), E, arenas[0].out_dim, n, A, plan.res.data_ptr(), st))
        elif plan.rule == "ucb":
            # agent.py:262-300: a candidate per actor on the rows of x = [s | a_k] (E n rows), every member's critics on x,
            # mean + bonus * std over the members, arg-max over the candidates
            # Six launches whatever the ensemble size: the members' networks copied into two packs, ONE forward of all actors,
            # the candidates (tanh-normal samples from the engine's Philox stream, member e at offset e << 40 of the plan's
            # stream) beside the state columns, ONE ensemble-Q forward of every member's critics on the E n stacked rows, the
            # rule's reduction, the publish step
            x = plan.buf(E * n, S + A)
            c_arenas = [c.arena(dev) for c in agent.critics]
            pa, pc = _Pack(plan, arenas), _Pack(plan, c_arenas)
            packed_out = plan.buf(E, n, pa.out_dim)
            plan.outs = [packed_out[e] for e in range(E)]
            N = c_arenas[0].n_nets
            q = plan.buf(pc.n_nets, E * n, 1)
            _pack_launch([pa, pc])
            check(lib.ssac_mlp3_fwd_fused(C.byref(pa.desc), 0, E, x_in, S, 0, n, 0, 0, packed_out.data_ptr(), st))
            r = plan.rng_for(agent, 0)
            a0 = agent.actors[0]
            assert all((float(a_.log_std_low), float(a_.log_std_high)) == (float(a0.log_std_low), float(a0.log_std_high))
                       for a_ in agent.actors)
            check(lib.ssac_act_candidates(packed_out.data_ptr(), E, n, A, x_in, S, S, float(a0.log_std_low),
                                          float(a0.log_std_high), C.byref(r), 1 << 40, x.data_ptr(), S + A, st))
            # (a pack above SSAC_MAX_NETS critics -- 8 members x 10 -- goes out as several packed launches)
            _fwd_desc(plan, pc.desc, pc.n_nets, True, pc.hidden, 1, x.data_ptr(), S + A, E * n, q)
            qs = [q[c * N:(c + 1) * N] for c in range(len(c_arenas))]
            check(lib.ssac_ucb_select(_ptr_array(qs), len(qs), N, E, n, float(agent.ucb_bonus), x.data_ptr(), S + A, S, A,
                                      plan.res.data_ptr(), st))
        elif plan.rule == "ducb":
            # agent.py:259-304, the discrete branch: a categorical candidate per actor, every member's critics on the state
            # representation (all A values of a row in one pass: no stacked candidates), the value of every candidate for
            # every member, mean + bonus * std over the members, arg-max over the candidates.  Five launches whatever the
            # ensemble size (below SSAC_MAX_NETS critics): the two packs, ONE forward of all actors, ONE of all critics, the
            # rule's kernel (member e draws at offset e << 40 of the plan's stream), the publish step
            c_arenas = [c.arena(dev) for c in agent.critics]
            pa, pc = _Pack(plan, arenas), _Pack(plan, c_arenas)
            assert pa.out_dim == A and pc.out_dim == A and pa.fused and pc.fused and len(c_arenas) == E
            packed_out = plan.buf(E, n, A)
            plan.outs = [packed_out[e] for e in range(E)]
            N = c_arenas[0].n_nets
            q = plan.buf(pc.n_nets, n, A)
            _pack_launch([pa, pc])
            _fwd_desc(plan, pa.desc, E, True, pa.hidden, A, x_in, S, n, packed_out)
            _fwd_desc(plan, pc.desc, pc.n_nets, True, pc.hidden, A, x_in, S, n, q)
            r = plan.rng_for(agent, 0)
            check(lib.ssac_act_ucb_discrete(packed_out.data_ptr(), q.data_ptr(), E, N, n, A, float(agent.ucb_bonus), C.byref(r),
                                            1 << 40, plan.res.data_ptr(), st))
        else:   # "sample": one actor's draw (agent.py:301-309)
            actor, ar, out = agent.actors[which], arenas[which], plan.outs[which]
            if plan.discrete:
                _fwd(plan, ar, x_in, S, n, out)
                r = plan.rng_for(agent, which)
                check(lib.ssac_act_discrete(_ptr_array([out]), 1, A, n, A, 1, C.byref(r), plan.res.data_ptr(), st))
            elif kind == "stochastic":
                # (tanh-normal samples lie inside (-1, 1): _process_act's clamp is the identity)
                r = plan.rng_for(agent, which)
                check(lib.ssac_actor_sample_fused(
                    C.byref(ar.desc()), x_in, S, n, 0, float(actor.log_std_low), float(actor.log_std_high),
                    plan.res.data_ptr(), A, 0, plan.logp.data_ptr(), 0, 0, out.data_ptr(), C.byref(r), st))
            else:   # deterministic actor: sample() = loc = tanh(out) (distributions.py:107-114)
                _fwd(plan, ar, x_in, S, n, out)
                check(lib.ssac_act_mean_tanh(_ptr_array([out]), 1, ar.out_dim, n, A, plan.res.data_ptr(), st))
        check(lib.ssac_act_publish(plan.handle, plan.res.data_ptr(), plan.out_floats, st))
        done = True
    finally:
        lst = lib.ssac_record_end()
        if not done and lst:
            lib.ssac_launch_list_free(lst)   # (the partial list of a recording that failed)
    # (the recording pass issued the launches too -- on whatever the observation buffer held -- and advanced the device-side
    #  call counter: ssac_act_add_list drains the device and re-reads the count)
    idx = lib.ssac_act_add_list(plan.handle, lst)
    if idx < 0:
        if lst:
            lib.ssac_launch_list_free(lst)   # (not taken over by the plan)
        raise RuntimeError("libssac_hip: " + lib.ssac_last_error().decode())
    plan.lists[which] = idx


def _plan_key(agent, obs, num_envs, sample):
    """(rule, ucb, the key of the call's plan in _PLANS[agent])"""
    ucb = bool(sample and agent.ucb_bonus > 0)
    rule = ("ducb" if agent.discrete else "ucb") if ucb else ("sample" if sample else "forward")
    # (the discrete UCB rule is keyed as the sample rule it replaces, told apart by its bonus)
    # (... and never by `rolling`: a pass-through rolling call is the same call.  float32 frames of a pixel agent: a plan of
    #  their own beside the uint8 one)
    pkey = ("sample" if rule == "ducb" else rule, num_envs, float(agent.ucb_bonus) if ucb else 0.0)
    if not lu.is_identity(agent.encoder) and _conv_module(agent) is not None \
            and obs[agent.encoder.ssac_obs_key].dtype == np.float32:
        pkey += ("float32",)  # (frames only: an MLP encoder's plan holds float32 rows whatever dtype the caller hands over)
    return rule, ucb, pkey


def act(agent, obs, num_envs, sample, return_dist=False, rolling=False):
    """the fast path's answer -- (action as numpy, dist_out or None) -- or None when the call is not eligible"""
    if not _eligible(agent, obs, num_envs, sample, rolling):
        return None
    dev = next(agent.actors[0].parameters()).device
    rule, ucb, pkey = _plan_key(agent, obs, num_envs, sample)
    failed = _FAILED.get(agent)
    if failed and pkey in failed:
        return None
    plans = _PLANS.get(agent)
    plan = None if plans is None else plans.get(pkey)
    sig = _signature(agent, ucb)
    if plan is None or plan.sig != sig:
        if not _arena_ok(agent, dev, ucb, sample):
            return None
        pix = None if lu.is_identity(agent.encoder) else _pixel_obs(agent, obs, num_envs)
        mlp = None if lu.is_identity(agent.encoder) or pix is not None else _mlp_obs(agent, obs, num_envs)
        eng = None
        if pix is not None:
            from . import conv_encoder
            eng = conv_encoder.conv_engine(agent.encoder, dev)   # (the module's own engine: its parameters live in its arena)
            if eng is None:
                return None
        elif mlp is not None:
            from . import encoder_base
            eng = encoder_base.encoder_engine(agent.encoder, dev)   # (recognised by _eligible: the one lookup finds its engine)
            if eng is None:
                return None
        plans = _PLANS.setdefault(agent, {})
        if len(plans) > 12:
            plans.clear()
        plan = plans[pkey] = _Plan(agent, rule, num_envs, dev, *(() if pix is None else pix[1:]),
                                   mlp_in=None if mlp is None else mlp[1])
        plan.conv_engine = eng if pix is not None else None
        plan.enc_engine = eng if mlp is not None else None
        plan.sig = _signature(agent, ucb)   # (binding the arenas may have re-pointed the parameters)
    # the reference's host draws, in its order: random.choice(act_dists) under UCB (for the logged distribution),
    # random.choice(self.actors) otherwise (agent.py:262, 301)
    which = None
    # (a recording may fail and hand the call to the general path, which makes the host draw itself: the generator's state
    #  is kept -- a ~2 us copy -- only while the plan still has a list to record, i.e. for the first few calls of a plan)
    host_state = random.getstate() if len(plan.lists) < (len(agent.actors) if rule == "sample" else 1) else None
    if ucb:
        which_dist = rng.choice(range(len(agent.actors)))
    elif rule == "sample":
        which = which_dist = rng.choice(range(len(agent.actors)))
    if which not in plan.lists and not _record(plan, agent, which):
        # the recording failed: no half-built plan stays behind, the key is not tried again, and the general path serves
        # this call -- it makes the reference's host draw itself, so the one made above is handed back
        _FAILED.setdefault(agent, {})[pkey] = plan.error
        warnings.warn(f"super_sac_amd.acting: recording the {rule} rule for {num_envs} environment(s) failed ({plan.error}); "
                      "these calls take the general path from now on", RuntimeWarning, stacklevel=3)
        plans.pop(pkey, None)
        if not plans:
            _PLANS.pop(agent, None)
        random.setstate(host_state)
        return None
    if plan.concat is None:
        v = np.ascontiguousarray(obs[plan.key], dtype=plan.obs_dtype)
    else:
        # the row in the encoder's column order, every key converted as the identity plan converts its one key
        v = np.concatenate([np.ascontiguousarray(obs[k], np.float32).reshape(num_envs, w) for k, w in plan.concat], axis=1)
    rc = lib.ssac_act_run(plan.handle, plan.lists[which], v.ctypes.data, v.nbytes, plan.result.ctypes.data, plan.out_floats,
                          engine.stream())
    if rc:
        raise RuntimeError("libssac_hip: " + lib.ssac_last_error().decode())
    n, A = num_envs, plan.A
    if plan.discrete:
        out = plan.result.astype(np.int64).reshape(n, 1)
    else:
        out = plan.result.reshape(n, A).copy()
    if num_envs == 1:
        out = out[0]
    dist_out = None
    if return_dist:
        dist_out = plan.outs[which_dist].clone()   # the chosen actor's raw head output (distribution parameters)
    return out, dist_out
