"""GPU: the refusals of the fused launchers (csrc/ssac_fused.hip), pinned text for text.

Each case calls one entry point of the C ABI with ONE defect and asserts a non-zero status and the exact
``ssac_last_error()``.  Every refusal listed here returns before any HIP call: nothing is launched.  The pointers that
are present are real (tiny) device buffers.  Shapes: actor 4 -> 32 -> 4 (A = 2), critics and targets 6 -> 32 -> 1 with
2 nets, 16 rows.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, A, H, N, B = 4, 2, 32, 2, 16
MAX_NETS = 64            # SSAC_MAX_NETS
CHAIN_MAX_ROWS = 2048    # SSAC_ACTOR_CHAIN_MAX_ROWS


@pytest.fixture(scope="module")
def env():
    import super_sac_amd
    from super_sac_amd import _lib
    dev = torch.device(DEV)
    arena = super_sac_amd.engine.MlpArena
    nets = {"actor": arena(1, S, H, 2 * A, dev), "critics": arena(N, S + A, H, 1, dev),
            "targets": arena(N, S + A, H, 1, dev), "critics2": arena(N, S + A, H, 2, dev)}
    pool = torch.zeros(64 * 256, dtype=torch.float32, device=dev)   # 64 distinct buffers of 256 floats
    return {"lib": _lib.lib, "mod": _lib, "nets": nets, "pool": pool, "next": [0], "keep": []}


def _buf(env):
    i = env["next"][0]
    env["next"][0] = (i + 1) % 64
    return env["pool"].data_ptr() + i * 256 * 4


def _desc(env, name, **fields):
    d = env["nets"][name].desc()
    for k, v in fields.items():
        setattr(d, k, v)
    env["keep"].append(d)
    return C.byref(d)


def _gather(env, x1sa, **fields):
    g = env["mod"].Gather()
    for k in ("s", "s1", "act", "rew", "done", "idx", "xsa", "rew_out", "done_out"):
        setattr(g, k, _buf(env))
    g.s_elems, g.a_elems, g.ld_x, g.ld_x1, g.x1sa, g.ids_word = S, A, S + A, S + A, x1sa, -1
    for k, v in fields.items():
        setattr(g, k, v)
    env["keep"].append(g)
    return C.byref(g)


# argument names of each entry point, in ABI order (include/ssac_hip.h)
ORDER = {
    "ssac_mlp3_fwd_fused": "nets net_ids n_sel X ldx x_net_stride n_rows H1 H2 Y stream",
    "ssac_actor_sample_fused": "actor X ldx n_rows eps lo hi act_dst ld_act act_col0 logp H1 H2 out rng stream",
    "ssac_actor_sample_concat_fused": "actor X ldx n_rows eps lo hi xsa ld_xsa logp H1 H2 out rng stream",
    "ssac_actor_sample_critic_fwd": "actor Xa ldxa n_rows eps lo hi act_dst ld_act act_col0 logp rng critics Xc ldxc H1 H2 Q "
                                    "gather stream",
    "ssac_chain_update": "actor Xa ldxa n_rows eps lo hi x1sa ld_x1 act_col0 logp rng targets net_ids n_sel Qt critics Xc ldxc "
                         "H1 H2 Q DZ2u DZ1u W3_snapshot gather deferred handoff target_splits xchg stream",
    "ssac_critic_fwd_bwd_fused": "nets X ldx n_rows td weight act ld_act popart pop denom H1 H2 Q DQ DZ2 DZ1 partials lazy_td "
                                 "stream",
    "ssac_critic_bwd_fused": "nets n_rows td weight act ld_act popart pop denom H1 H2 Q DQ DZ2 DZ1 partials lazy_td stream",
    "ssac_actor_chain_fused": "actor X ldx n_rows eps rng lo hi xsa ld_xsa logp H1 H2 out critics Q DXu log_alpha use_entropy "
                              "inv_members popart pop d_out DZ2 DZ1 partials handoff update_no begin_logs n_logs begin_ctl "
                              "stream",
}
ABSENT = {"net_ids", "rng", "gather", "deferred", "xchg", "stream", "popart", "lazy_td", "W3_snapshot", "begin_logs", "begin_ctl",
          "weight", "act"}
NUMBERS = {"n_sel": N, "ldx": S + A, "ldxa": S + A, "ldxc": S + A, "x_net_stride": 0, "n_rows": B, "lo": -10.0, "hi": 2.0,
           "ld_act": S + A, "ld_xsa": S + A, "ld_x1": S + A, "act_col0": S, "target_splits": 1, "pop": 0, "denom": float(B),
           "use_entropy": 1, "inv_members": 1.0, "update_no": -1, "n_logs": 0}


def _call(env, fn, **defect):
    """every argument valid (a device buffer, or absent where the ABI allows it), then the defect on top"""
    args = []
    for name in ORDER[fn].split():
        if name in defect:
            v = defect[name]
        elif name in ("actor", "critics", "targets"):
            v = _desc(env, name)
        elif name == "nets":
            v = _desc(env, "critics")
        elif name in ABSENT:
            v = None
        elif name in NUMBERS:
            v = NUMBERS[name]
        else:
            v = _buf(env)
        args.append(v)
    status = getattr(env["lib"], fn)(*args)
    return status, env["lib"].ssac_last_error().decode()


def _refused(env, fn, text, **defect):
    status, msg = _call(env, fn, **defect)
    assert status != 0, f"{fn} accepted {sorted(defect)}"
    assert msg == text


def test_mlp3_fwd_hidden_48(env):
    _refused(env, "ssac_mlp3_fwd_fused", "ssac_mlp3_fwd_fused: shape not supported by the fused path",
             nets=_desc(env, "critics", hidden=48))


def test_mlp3_fwd_n_sel_65(env):
    _refused(env, "ssac_mlp3_fwd_fused", "ssac_mlp3_fwd_fused: n_sel out of range", n_sel=MAX_NETS + 1)


def test_actor_sample_no_noise(env):
    _refused(env, "ssac_actor_sample_fused", "ssac_actor_sample_fused: neither eps nor an rng stream given", eps=None)


def test_actor_sample_concat_no_noise(env):
    _refused(env, "ssac_actor_sample_concat_fused", "ssac_actor_sample_concat_fused: neither eps nor an rng stream given",
             eps=None)


def test_actor_sample_concat_ld_too_small(env):
    _refused(env, "ssac_actor_sample_concat_fused", "ssac_actor_sample_concat_fused: bad output", ld_xsa=S + A - 1)


def test_sample_critic_fwd_h1_null(env):
    _refused(env, "ssac_actor_sample_critic_fwd", "ssac_actor_sample_critic_fwd: H1 / H2 / Q missing", H1=None)


def test_sample_critic_fwd_gather_sizes(env):
    _refused(env, "ssac_actor_sample_critic_fwd", "ssac_actor_sample_critic_fwd: gather sizes do not match the networks",
             gather=_gather(env, _buf(env), s_elems=S + 1))


def test_sample_critic_fwd_gather_incomplete(env):
    _refused(env, "ssac_actor_sample_critic_fwd", "ssac_actor_sample_critic_fwd: incomplete ssac_gather",
             gather=_gather(env, _buf(env), rew_out=None))


def test_sample_critic_fwd_no_input(env):
    _refused(env, "ssac_actor_sample_critic_fwd", "ssac_actor_sample_critic_fwd: Xa / Xc missing", Xa=None)


def test_chain_update_splits_3(env):
    _refused(env, "ssac_chain_update", "ssac_chain_update: target_splits is 1, 2 or 4", target_splits=3)


def test_chain_update_splits_without_handoff(env):
    _refused(env, "ssac_chain_update",
             "ssac_chain_update: column-split target critics need the hand-off form and hidden 256", target_splits=2,
             handoff=None)


def test_chain_update_two_output_critics(env):
    _refused(env, "ssac_chain_update", "ssac_chain_update: single-output critics only", critics=_desc(env, "critics2"))


def test_chain_update_x1sa_null(env):
    _refused(env, "ssac_chain_update", "ssac_chain_update: missing buffer", x1sa=None)


def test_chain_update_no_dz2u_no_snapshot(env):
    _refused(env, "ssac_chain_update", "ssac_chain_update: DZ2u == NULL needs the W3 snapshot buffer", DZ2u=None)


def test_chain_update_act_col0(env):
    _refused(env, "ssac_chain_update", "ssac_chain_update: [s'|a'] layout does not match the networks", act_col0=S + 1)


def test_chain_update_gather_other_x1sa(env):
    x1sa = _buf(env)
    _refused(env, "ssac_chain_update", "ssac_chain_update: incomplete ssac_gather", x1sa=x1sa,
             gather=_gather(env, x1sa + 4))


def test_critic_fwd_bwd_no_td(env):
    _refused(env, "ssac_critic_fwd_bwd_fused", "ssac_critic_fwd_bwd_fused: no TD target given", td=None)


def test_critic_bwd_no_td(env):
    _refused(env, "ssac_critic_bwd_fused", "ssac_critic_bwd_fused: no TD target given", td=None)


def test_critic_bwd_h1_null(env):
    _refused(env, "ssac_critic_bwd_fused", "ssac_critic_bwd_fused: needs the saved forward (H1, H2, Q)", H1=None)


def test_actor_chain_critic_input(env):
    _refused(env, "ssac_actor_chain_fused",
             "ssac_actor_chain_fused: critic input is not [s | a] / too many action columns",
             critics=_desc(env, "critics", in_dim=S + A + 1))


def test_actor_chain_handoff_null(env):
    _refused(env, "ssac_actor_chain_fused", "ssac_actor_chain_fused: missing argument", handoff=None)


def test_actor_chain_too_many_rows(env):
    _refused(env, "ssac_actor_chain_fused",
             "ssac_actor_chain_fused: more than SSAC_ACTOR_CHAIN_MAX_ROWS batch rows (use the three launches)",
             n_rows=CHAIN_MAX_ROWS + 16)


def test_chain_form_2(env):
    lib = env["lib"]
    assert lib.ssac_chain_form(2) != 0
    assert lib.ssac_last_error().decode() == ("ssac_chain_form: 0 (one workgroup per CU), 1 (co-resident 16-row tiles where "
                                              "they apply), -1 (the library's default)")


def test_fused_tile_rows_8(env):
    lib = env["lib"]
    assert lib.ssac_fused_tile_rows(8) != 0
    assert lib.ssac_last_error().decode() == "ssac_fused_tile_rows: 0 (auto), 16, 32, 17 (16 rows, single staging buffer)"
