"""What the trainable-encoder engines (conv_encoder.ConvEncoderEngine, mlp_encoder.MlpEncoderEngine) share, and the one
lookup of an encoder's engine.  ``EncoderEngine`` owns the flat parameter arena (the parameters re-pointed at views of
``flat`` exactly like the MLP ensembles; ``grads`` has the same layout, so clip_grad_norm_ and Adam are two launches), the
accumulate form of ``backward`` and the clip + Adam tail; a subclass packs its parameters with ``_pack`` and provides
``emb``, ``forward``, ``forward_ptr``, ``_backward(d_rep)`` and what it keeps in ``saved``.
"""
import torch

from . import engine
from ._lib import check, lib


def arena_layout(numels):
    """offsets (each a multiple of 4 floats) and the total length of a flat arena holding tensors of `numels` elements"""
    offs, o = [], 0
    for n in numels:
        offs.append(o)
        o += (n + 3) // 4 * 4
    return offs, o


class EncoderEngine:
    moments_key = None   # of this arena's Adam moments in the optimizer's group (checkpoints key on it)

    def _pack(self, plist, device):
        """move the parameters `plist` into one flat fp32 arena on `device` and re-point their ``.data`` at views of it"""
        self.device = torch.device(device)
        self.plist = plist
        self.offs, self.numel = arena_layout([p.numel() for p in plist])
        self.flat = torch.zeros(self.numel, dtype=torch.float32, device=self.device)
        with torch.no_grad():
            for p, off in zip(plist, self.offs):
                v = self.flat[off:off + p.numel()].view(p.shape)
                v.copy_(p.data.to(device=self.device, dtype=torch.float32))
                p.data = v
        self.grads = torch.zeros_like(self.flat)
        self.ws = engine.Workspace(self.device)
        self.saved = None

    def is_bound(self):
        return all(p.data_ptr() == self.flat.data_ptr() + 4 * off for p, off in zip(self.plist, self.offs))

    def _seg(self, k, tensor=None):
        t = self.flat if tensor is None else tensor
        return t[self.offs[k]:self.offs[k] + self.plist[k].numel()]

    def backward(self, d_rep, accumulate=False):
        """d_rep (B, emb) contiguous = dL/d(embedding).  Fills self.grads (flat, same layout as the parameters);
        accumulate=True ADDS to it instead (the members of an ensemble share one encoder and the reference runs ONE
        backward over the sum of their losses, learning.py:47-121)."""
        if not accumulate:
            return self._backward(d_rep)
        keep, tmp = self.grads, self.__dict__.get("_gtmp")
        if tmp is None:
            tmp = self.__dict__["_gtmp"] = torch.zeros_like(self.flat)
        self.grads = tmp
        try:
            self._backward(d_rep)
        finally:
            self.grads = keep
        keep.add_(tmp)   # (device plumbing: one elementwise pass over the gradient arena)

    def grad_sumsq(self, ss):
        """partial sums of squares of the gradient arena into `ss` (ssac_sumsq_blocks() floats): what ssac_clip_coef reads"""
        check(lib.ssac_sumsq(self.grads.data_ptr(), self.numel, ss.data_ptr(), engine.stream()))

    def adam_step(self, adam):
        """Adam on the arena from the stored gradients, scaled by the clip coefficient in `adam`'s control block"""
        m, v = adam.moments_for(self.moments_key, self.flat)
        check(lib.ssac_adam_step(self.flat.data_ptr(), m.data_ptr(), v.data_ptr(), self.grads.data_ptr(),
                                 self.numel, adam.ctl.ptr, engine.stream()))

    def optimizer_step(self, optimizer, clip, norm_out=None, step=True):
        """clip_grad_norm_(encoder.parameters(), clip) + encoder_optimizer.step() (learning.py:127-129).
        step=False: clip and log only (offline_actor_update without update_encoder, learning.py:203-208)."""
        st = engine.stream()
        adam = engine.adam_group(optimizer, self.device)
        if step:
            adam.advance()
        nb = int(lib.ssac_sumsq_blocks())
        ss = self.ws.get("o.ss", (nb,))
        self.grad_sumsq(ss)
        check(lib.ssac_clip_coef(adam.ctl.ptr, ss.data_ptr(), nb, float(clip) if clip else 0.0, 0, st))
        if norm_out is not None:
            check(lib.ssac_group_norms(ss.data_ptr(), 1, nb, adam.ctl.ptr, norm_out.data_ptr(), st))
        if step:
            self.adam_step(adam)


def cached_engine(module, slot, device, make):
    """the engine kept in ``module.__dict__[slot]``, reused if and only if it was built for `module`, on the same device
    ("cuda" names the current one), and the parameters still live in its arena (a deepcopy or a ``.to()`` may have moved
    them out); otherwise ``make(device)`` packs a new one"""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    eng = module.__dict__.get(slot)
    if eng is None or eng.module is not module or eng.device != device or not eng.is_bound():
        eng = module.__dict__[slot] = make(device)
    return eng


def encoder_engine(encoder, device, obs_dict=None):
    """the engine behind a trainable encoder: the convolution engine (conv_encoder.py) or the MLP engine (mlp_encoder.py),
    else None"""
    from . import conv_encoder, mlp_encoder
    if not mlp_encoder.is_mlp_encoder(encoder):   # (one recognised already holds no convolutional module: no walk over it)
        eng = conv_encoder.conv_engine(encoder, device)
        if eng is not None:
            return eng
    return mlp_encoder.mlp_engine(encoder, device, obs_dict)


def require_engine(encoder, device, obs_dict=None):
    """encoder_engine, or the refusal of an encoder of no known kind"""
    eng = encoder_engine(encoder, device, obs_dict)
    if eng is None:
        raise NotImplementedError(f"{type(encoder).__name__}: this encoder has no HIP path")
    return eng


def module_forward(encoder, x):
    """forward() of this package's own encoder modules (nets.py): the embedding of `x` through the module's engine"""
    engine.require_gpu(x)
    eng = require_engine(encoder, x.device)
    out = torch.empty(x.shape[0], eng.emb, device=x.device)
    eng.forward(x, out, eng.emb, save=False)
    return out


def refuse_unsupported(agent, where, encoder_lambda=0.0, actor_lambda=0.0):
    """what an agent with an MLP encoder cannot ask of `where` (an update function's name), each with its reason"""
    from . import mlp_encoder, parallel
    if not mlp_encoder.is_mlp_encoder(agent.encoder):   # (learning_utils.ensure_adopted has looked at the encoder by now)
        return
    name = type(agent.encoder).__name__
    if encoder_lambda or actor_lambda:
        which = "encoder_lambda" if encoder_lambda else "actor_lambda"
        raise NotImplementedError(
            f"{where}: {which} != 0 with the MLP encoder {name}: vector observations have only the identity augmentation, "
            "so the reference's invariance constraint is the norm of a zero tensor; pass 0")
    if any(o.__dict__.get("_ssac_precision") == "bf16" for o in list(agent.actors) + list(agent.critics)):
        raise NotImplementedError(
            f"{where}: set_precision('bf16') with the MLP encoder {name}: the bf16 operand mode covers agents whose encoder "
            "is an identity")
    if parallel.shard_of(agent) is not None or parallel.member_shard_of(agent) is not None:
        raise NotImplementedError(
            f"{where}: critic- or member-sharded agents with the MLP encoder {name}: a trainable encoder is shared by all "
            "members and is not sharded (trainable pixel encoders are refused likewise)")
