"""GPU: ssac_gather_concat (csrc/ssac_gather_concat.hip) -- the whole-transition replay gather for observations that are
several vector arrays laid side by side -- against numpy.  Copies and uint8 -> float casts: every comparison is exact.
Outputs carry three padding columns per row, pre-filled with a sentinel that must come back untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CAP = 300          # rows of the replay arrays
SENTINEL = -777.25
PAD = 3

# name -> (widths, index of the uint8 key or None)
LAYOUTS = {"K1": ((7,), None), "K2": ((1, 3), None), "K3-u8": ((7, 1, 130), 1), "K8": ((1,) * 8, None)}


def _ssa():
    import super_sac_amd as ssa
    return ssa


def _arrays(widths, u8, A, seed=0):
    """replay arrays on the host: per key s / s1 (CAP x w), act (CAP x A), rew (CAP), done (CAP) uint8"""
    g = np.random.RandomState(100 + seed + 7 * len(widths) + A)
    s, s1 = [], []
    for j, w in enumerate(widths):
        if j == u8:
            s.append(g.randint(0, 256, (CAP, w)).astype(np.uint8)); s1.append(g.randint(0, 256, (CAP, w)).astype(np.uint8))
        else:
            s.append(g.standard_normal((CAP, w)).astype(np.float32)); s1.append(g.standard_normal((CAP, w)).astype(np.float32))
    act = g.uniform(-1, 1, (CAP, A)).astype(np.float32)
    rew = g.standard_normal(CAP).astype(np.float32)
    done = (g.uniform(size=CAP) < 0.3).astype(np.uint8)
    return s, s1, act, rew, done


def _indices(n, seed=0):
    """n replay rows: the last row of the capacity, row 0, repeated rows (n > 2), the rest random"""
    g = np.random.RandomState(200 + seed + n)
    idx = g.randint(0, CAP, n).astype(np.int64)
    idx[0] = CAP - 1
    if n > 2:
        idx[1], idx[2], idx[-1] = 0, idx[n // 2], idx[n // 2]
    return idx


def _table(ssa, s_dev, s1_dev, widths, n_keys=None):
    t = ssa._lib.Concat()
    t.n_keys = len(widths) if n_keys is None else n_keys
    for j, w in enumerate(widths):
        t.key[j] = ssa._lib.ConcatKey(s_dev[j].data_ptr(), s1_dev[j].data_ptr() if s1_dev is not None else 0,
                                      int(s_dev[j].dtype == torch.uint8), 0, w)
    return t


def _outputs(n, S, A, dev):
    full = lambda *shape: torch.full(shape, SENTINEL, device=dev)
    return full(n, S + A + PAD), full(n, S + A + PAD), full(n), full(n)


def _expected(s, s1, act, rew, done, idx, S, A):
    n = len(idx)
    xsa = np.full((n, S + A + PAD), SENTINEL, np.float32)
    x1sa = np.full((n, S + A + PAD), SENTINEL, np.float32)
    xsa[:, :S] = np.concatenate([a[idx].astype(np.float32) for a in s], 1)
    xsa[:, S:S + A] = act[idx]
    x1sa[:, :S] = np.concatenate([a[idx].astype(np.float32) for a in s1], 1)
    return xsa, x1sa, rew[idx], done[idx].astype(np.float32)


def _same(t, want):
    got = t.cpu().numpy()
    return got.shape == want.shape and np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


@pytest.mark.parametrize("A", [1, 6])
@pytest.mark.parametrize("n", [1, 5, 257])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_gather_equals_numpy(layout, n, A):
    ssa = _ssa()
    lib, dev = ssa._lib.lib, torch.device("cuda")
    widths, u8 = LAYOUTS[layout]
    S = sum(widths)
    s, s1, act, rew, done = _arrays(widths, u8, A)
    idx = _indices(n)
    up = lambda a: torch.from_numpy(a).to(dev)
    s_d, s1_d, act_d, rew_d, done_d, idx_d = [up(a) for a in s], [up(a) for a in s1], up(act), up(rew), up(done), up(idx)
    table = _table(ssa, s_d, s1_d, widths)
    xsa, x1sa, r, d = _outputs(n, S, A, dev)
    ld = S + A + PAD
    ssa._lib.check(lib.ssac_gather_concat(C.byref(table), act_d.data_ptr(), A, rew_d.data_ptr(), done_d.data_ptr(),
                                          idx_d.data_ptr(), n, xsa.data_ptr(), ld, x1sa.data_ptr(), ld, r.data_ptr(),
                                          d.data_ptr(), 0))
    torch.cuda.synchronize()
    e_xsa, e_x1sa, e_r, e_d = _expected(s, s1, act, rew, done, idx, S, A)
    assert _same(xsa, e_xsa) and _same(x1sa, e_x1sa) and _same(r, e_r) and _same(d, e_d)
    if len(widths) == 1:
        # one key: the bytes ssac_gather_transition leaves
        t_xsa, t_x1sa, t_r, t_d = _outputs(n, S, A, dev)
        ssa._lib.check(lib.ssac_gather_transition(s_d[0].data_ptr(), s1_d[0].data_ptr(), 0, S, act_d.data_ptr(), A,
                                                  rew_d.data_ptr(), done_d.data_ptr(), idx_d.data_ptr(), n,
                                                  t_xsa.data_ptr(), ld, t_x1sa.data_ptr(), ld, t_r.data_ptr(),
                                                  t_d.data_ptr(), 0))
        torch.cuda.synchronize()
        for a, b in ((xsa, t_xsa), (x1sa, t_x1sa), (r, t_r), (d, t_d)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("n", [1, 5, 257])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_row_r_is_row_r_without_an_index_vector(layout, n):
    """idx == NULL: the form encode() uses on loose tensors.  First only s -> xsa (everything else NULL), then the whole
    transition of rows 0 .. n-1"""
    ssa = _ssa()
    lib, dev = ssa._lib.lib, torch.device("cuda")
    widths, u8 = LAYOUTS[layout]
    S, A = sum(widths), 6
    s, s1, act, rew, done = _arrays(widths, u8, A, seed=1)
    up = lambda a: torch.from_numpy(a).to(dev)
    s_d, s1_d, act_d, rew_d, done_d = [up(a) for a in s], [up(a) for a in s1], up(act), up(rew), up(done)
    rows = np.arange(n)
    e_xsa, e_x1sa, e_r, e_d = _expected(s, s1, act, rew, done, rows, S, A)
    # s only, into a (n, S + PAD) buffer
    out = torch.full((n, S + PAD), SENTINEL, device=dev)
    ssa._lib.check(lib.ssac_gather_concat(C.byref(_table(ssa, s_d, None, widths)), 0, 0, 0, 0, 0, n, out.data_ptr(), S + PAD,
                                          0, 0, 0, 0, 0))
    torch.cuda.synchronize()
    want = np.full((n, S + PAD), SENTINEL, np.float32)
    want[:, :S] = e_xsa[:, :S]
    assert _same(out, want)
    # the whole transition
    xsa, x1sa, r, d = _outputs(n, S, A, dev)
    ld = S + A + PAD
    ssa._lib.check(lib.ssac_gather_concat(C.byref(_table(ssa, s_d, s1_d, widths)), act_d.data_ptr(), A, rew_d.data_ptr(),
                                          done_d.data_ptr(), 0, n, xsa.data_ptr(), ld, x1sa.data_ptr(), ld, r.data_ptr(),
                                          d.data_ptr(), 0))
    torch.cuda.synchronize()
    assert _same(xsa, e_xsa) and _same(x1sa, e_x1sa) and _same(r, e_r) and _same(d, e_d)


def test_encode_lays_loose_tensors_side_by_side():
    """learning_utils.encode of a concatenating encoder: loose tensors go through the idx == NULL launch (also into a
    wider dst), column views of one row come back as the strided view of that row -- no copy"""
    ssa = _ssa()
    lu, dev = ssa.learning_utils, torch.device("cuda")
    enc = ssa.nets.ConcatEncoder({"obs": 5, "goal": 2, "task": 4}, order=["task", "obs", "goal"])
    g = torch.Generator().manual_seed(9)
    o = {k: torch.randn(37, w, generator=g).to(dev) for k, w in (("obs", 5), ("goal", 2), ("task", 4))}
    want = torch.cat([o["task"], o["obs"], o["goal"]], 1)
    got = lu.encode(enc, o)
    assert got.shape == (37, 11) and torch.equal(got, want) and torch.equal(enc(o), want)
    dst = torch.full((37, 14), SENTINEL, device=dev)
    got = lu.encode(enc, o, dst=dst)
    assert got.data_ptr() == dst.data_ptr() and torch.equal(dst[:, :11], want) and bool((dst[:, 11:] == SENTINEL).all())
    row = torch.randn(37, 14, generator=g).to(dev)
    views = {"task": row[:, 0:4], "obs": row[:, 4:9], "goal": row[:, 9:11]}
    got = lu.encode(enc, views)
    assert got.data_ptr() == row.data_ptr() and got.stride() == (14, 1) and torch.equal(got, row[:, :11])
    # views in another column order are loose tensors
    views = {"obs": row[:, 0:5], "task": row[:, 5:9], "goal": row[:, 9:11]}
    got = lu.encode(enc, views)
    assert got.data_ptr() != row.data_ptr() and torch.equal(got, torch.cat([row[:, 5:9], row[:, 0:5], row[:, 9:11]], 1))


def test_begin_form_reads_the_feed_slot_and_starts_the_update():
    """ssac_gather_concat_begin: indices from the current slot of the input ring; workgroup 0 mirrors the slot into the
    device block, clears the log block and advances the optimizer step (ssac_begin_update's work)"""
    ssa = _ssa()
    lib, dev = ssa._lib.lib, torch.device("cuda")
    widths, u8 = LAYOUTS["K3-u8"]
    S, A, n = sum(widths), 6, 70
    s, s1, act, rew, done = _arrays(widths, u8, A, seed=2)
    idx = _indices(n, seed=2)
    up = lambda a: torch.from_numpy(a).to(dev)
    s_d, s1_d, act_d, rew_d, done_d = [up(a) for a in s], [up(a) for a in s1], up(act), up(rew), up(done)
    slot_words, n_slots = 2 * n + 4, 2          # (n int64 indices + one spare 16-byte granule; a multiple of 4)
    ring = ssa.learning._FeedRing(4 * slot_words * n_slots)
    slots = np.zeros((n_slots, slot_words), np.uint32)
    slots[1, :2 * n] = idx.view(np.uint32)
    slots[1, 2 * n:] = 0xABCD
    ssa._lib.check(lib.ssac_feed_write(ring.ptr, slots.ctypes.data, slots.nbytes))
    inbuf = torch.zeros(slot_words, dtype=torch.int32, device=dev)
    log_ring = torch.zeros(4, 64, device=dev)
    feed = ssa.engine.DeviceStruct(ssa._lib.Feed(ring.ptr, inbuf.data_ptr(), log_ring.data_ptr(), 1, n_slots, slot_words,
                                                 2 * n, 64, 0), dev)   # tick 1: the second slot
    logs = torch.full((64,), 5.0, device=dev)
    ctl = ssa.engine.DeviceStruct(ssa._lib.AdamCtl(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, clip_coef=1.0, step=4,
                                                   lr_d=1e-3, beta1_d=0.9, beta2_d=0.999), dev)
    xsa, x1sa, r, d = _outputs(n, S, A, dev)
    ld = S + A + PAD
    table = _table(ssa, s_d, s1_d, widths)
    ssa._lib.check(lib.ssac_gather_concat_begin(C.byref(table), act_d.data_ptr(), A, rew_d.data_ptr(), done_d.data_ptr(), n,
                                                xsa.data_ptr(), ld, x1sa.data_ptr(), ld, r.data_ptr(), d.data_ptr(),
                                                feed.ptr, logs.data_ptr(), 64, ctl.ptr, 0))
    torch.cuda.synchronize()
    e_xsa, e_x1sa, e_r, e_d = _expected(s, s1, act, rew, done, idx, S, A)
    assert _same(xsa, e_xsa) and _same(x1sa, e_x1sa) and _same(r, e_r) and _same(d, e_d)
    assert np.array_equal(inbuf.cpu().numpy().view(np.uint32), slots[1])
    assert bool((logs == 0).all()) and ctl.read().step == 5
    assert abs(ctl.read().step_size - 1e-3 / (1 - 0.9 ** 5)) < 1e-9


def _refusal_cases():
    def k(n_keys):
        return lambda a: a["table"].__setattr__("n_keys", n_keys)

    def key_field(j, **kw):
        def f(a):
            for name, v in kw.items():
                setattr(a["table"].key[j], name, v)
        return f
    return {
        "no keys": k(0), "nine keys": k(9), "negative key count": k(-1),
        "NULL s": key_field(1, s=0), "NULL s1": key_field(0, s1=0),
        "elems 0": key_field(1, elems=0), "elems -3": key_field(0, elems=-3),
        "dtype 2": key_field(1, dtype=2), "dtype -1": key_field(0, dtype=-1),
        "ld_x too small": lambda a: a.__setitem__("ld_x", a["S"] + a["A"] - 1),
        "ld_x1 too small": lambda a: a.__setitem__("ld_x1", a["S"] - 1),
        "indexed without act": lambda a: a.__setitem__("act", 0),
        "indexed without x1sa": lambda a: a.__setitem__("x1sa", 0),
    }


@pytest.mark.parametrize("begin", [False, True], ids=["plain", "begin"])
@pytest.mark.parametrize("what", sorted(_refusal_cases()))
def test_refusals_return_an_error_and_write_nothing(what, begin):
    ssa = _ssa()
    lib, dev = ssa._lib.lib, torch.device("cuda")
    widths, A, n = (3, 2), 2, 5
    S = sum(widths)
    s, s1, act, rew, done = _arrays(widths, None, A, seed=3)
    up = lambda a: torch.from_numpy(a).to(dev)
    s_d, s1_d, act_d, rew_d, done_d = [up(a) for a in s], [up(a) for a in s1], up(act), up(rew), up(done)
    idx_d = up(_indices(n))
    xsa, x1sa, r, d = _outputs(n, S, A, dev)
    logs = torch.full((64,), SENTINEL, device=dev)
    a = dict(table=_table(ssa, s_d, s1_d, widths), S=S, A=A, ld_x=S + A + PAD, ld_x1=S + A + PAD, act=act_d.data_ptr(),
             x1sa=x1sa.data_ptr())
    _refusal_cases()[what](a)
    if begin:
        # (a refusal comes before anything looks at the feed: its address only has to be non-NULL)
        feed = torch.zeros(64, dtype=torch.uint8, device=dev)
        rc = lib.ssac_gather_concat_begin(C.byref(a["table"]), a["act"], A, rew_d.data_ptr(), done_d.data_ptr(), n,
                                          xsa.data_ptr(), a["ld_x"], a["x1sa"], a["ld_x1"], r.data_ptr(), d.data_ptr(),
                                          feed.data_ptr(), logs.data_ptr(), 64, 0, 0)
    else:
        rc = lib.ssac_gather_concat(C.byref(a["table"]), a["act"], A, rew_d.data_ptr(), done_d.data_ptr(), idx_d.data_ptr(),
                                    n, xsa.data_ptr(), a["ld_x"], a["x1sa"], a["ld_x1"], r.data_ptr(), d.data_ptr(), 0)
    assert rc != 0
    msg = lib.ssac_last_error().decode()
    assert msg.startswith("ssac_gather_concat_begin: " if begin else "ssac_gather_concat: "), msg
    torch.cuda.synchronize()
    for t in (xsa, x1sa, r, d, logs):
        assert bool((t == SENTINEL).all()), f"{what}: a refused call wrote to an output"


def test_begin_form_needs_a_feed():
    ssa = _ssa()
    lib = ssa._lib.lib
    assert lib.ssac_gather_concat_begin(C.byref(ssa._lib.Concat()), 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) != 0
    assert lib.ssac_last_error().decode() == "ssac_gather_concat_begin: needs a feed"
