"""CPU: learning._offline_member_plan -- the ONE decision "which loss head, how many rows, which host draw and which way
to the encoder does this member's offline actor update take" -- against a verbatim restatement of the expressions that
offline_actor_update's member loop spelled out in place (commit 42f6868: det, O, rows, train_enc, enc_grad, the branch
taken at each of its three branch sites and the host draw of the invariance constraint's step (1)), over the full cross
product of their inputs.  The combinations the update refuses (a Beta head with the advantage filter or the invariance
constraint) are shown to be refused by offline_actor_update's own code, in front of everything else.  No kernel runs."""
import itertools
import types

import pytest

KINDS = ("stochastic", "deterministic", "discrete", "beta")
B = 8   # (any batch size: the plan counts row blocks, the parent counted rows)


# ---- the parent's loop body, restated: what it computed and which branch it took at each site
def _p_member(kind, discrete, filter_, actor_lambda, pixel, update_encoder, A):
    train_enc = bool(update_encoder) and pixel
    enc_grad = train_enc or (bool(actor_lambda) and pixel)
    mask = "estimator" if filter_ else None
    det = not discrete and kind == "deterministic"
    O = A if (discrete or det) else 2 * A
    rows = B
    draw = None
    if actor_lambda:
        if discrete:
            draw = "categorical"      # rng.draw_categorical(out_o[0])
        elif det:
            draw = None               # o_dist.sample() is tanh(out_o)
        else:
            draw = "normal"           # rng.draw_normal((B, A), dev)
        if pixel:
            rep = "encode_stacked"    # site 1: the representation
        else:
            rep = "two encodes + copies"
        rows = 2 * B
    else:
        rep = "encode"
    if discrete:                      # site 2: the loss head
        head = "discrete"
    elif kind == "beta":
        head = "beta"
    elif det:
        head = "deterministic"
    else:
        head = "tanh_normal"
    if enc_grad and actor_lambda:     # site 3: the encoder's share
        enc = "stacked"
    elif train_enc:
        enc = "single"
    else:
        enc = None
    return dict(train_enc=train_enc, enc_grad=enc_grad, mask=mask, O=O, rows=rows, draw=draw, rep=rep, head=head, enc=enc)


def _p_refused(kind, discrete, filter_, actor_lambda):
    if not discrete and kind == "beta":
        if filter_:
            return "advantage filter"
        if actor_lambda:
            return "action invariance"
    return None


def _rep_site(plan, pixel):
    """the branch the representation step takes, from what it reads: the plan and the call's `pixel`"""
    if plan.row_blocks == 2:
        return "encode_stacked" if pixel else "two encodes + copies"
    return "encode"


def test_the_plan_is_the_parents_expressions(monkeypatch):
    import super_sac_amd as ssa
    L = ssa.learning
    # offline_actor_update up to its refusals, without a device: what stands in front of them is switched off
    monkeypatch.setattr(L.engine, "require_gpu", lambda: None)
    monkeypatch.setattr(L.lu, "ensure_adopted", lambda agent, buffer: None)
    monkeypatch.setattr(L.encoder_base, "refuse_unsupported", lambda *a, **k: None)
    seen, refused = 0, 0
    for kind, discrete, filter_, lam, pixel, upd, A in itertools.product(
            KINDS, (False, True), (False, True), (0, 0.5), (False, True), (False, True), (1, 6)):
        what = (kind, discrete, filter_, lam, pixel, upd, A)
        why = _p_refused(kind, discrete, filter_, lam)
        if why is not None:
            actor = types.SimpleNamespace(dist_impl="beta", action_size=A)
            assert L.lu.actor_kind(actor) == kind
            # (an agent of nothing but its actors: anything past the refusals would fail on it with another error)
            with pytest.raises(NotImplementedError, match=f"{why}.*Beta"):
                L.offline_actor_update(None, types.SimpleNamespace(actors=[actor]), None, None, B, None, upd, None, None,
                                       lam, 0.0, per=False, discrete=discrete, filter_=filter_)
            refused += 1
            continue
        plan = L._offline_member_plan(kind, discrete, filter_, bool(lam), pixel, bool(upd), A)
        want = _p_member(*what)
        assert plan.head == want["head"], what
        assert plan.out_cols == want["O"], what
        assert plan.row_blocks * B == want["rows"], what
        assert plan.masked == (want["mask"] is not None), what
        assert plan.inv_draw == want["draw"], what
        assert plan.train_enc == want["train_enc"] and plan.enc_grad == want["enc_grad"], what
        assert plan.enc_path == want["enc"], what
        assert _rep_site(plan, pixel) == want["rep"], what
        # the stacked backward needs the engine that encode_stacked returned 60 lines earlier
        assert plan.enc_path != "stacked" or want["rep"] == "encode_stacked", what
        # the invariance launch runs exactly when the second row block exists
        assert (plan.row_blocks == 2) == bool(lam), what
        seen += 1
    assert refused == 1 * 1 * 3 * 2 * 2 * 2          # beta, continuous, (filter, lambda) != (off, 0)
    assert seen + refused == 4 * 2 * 2 * 2 * 2 * 2 * 2
