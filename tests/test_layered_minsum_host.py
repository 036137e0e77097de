"""
Layered schedule of the min-sum decoders, host side (no GPU): the numpy restatement that the GPU tests compare against
(tests/layered_minsum_reference.py) is itself pinned -- by a two-check graph worked out by hand and by an independently
written scalar loop --, the input sets of the GPU tests are shown to exercise both answers of the syndrome, the layered
walk needs fewer iterations than the flooding oracle, and the ``schedule`` keyword of the five decoder classes reaches
the engine descriptor (or is refused) without a device.
"""
import numpy as np
import pytest
import torch

import layered_minsum_cases as cs
import layered_minsum_reference as ref


class _Graph:
    """the fields of TannerGraph the restatement reads"""

    def __init__(self, n, checks):
        self.n, self.m = n, len(checks)
        self.check_ptr = np.cumsum([0] + [len(c) for c in checks]).astype(np.int32)
        self.var_idx = np.asarray([v for c in checks for v in c], dtype=np.int32)
        self.E = int(self.var_idx.size)


# checks {v0, v1, v2} and {v2, v3}; llr = [2, -2, 4, 0]: |2| == |-2| is a tie in check 0, v3 is exactly 0.
#   check 0: u = [2, -2, 4], m1 = m2 = 2, raw = [2, 2, 2], prod = [-1, +1, -1]
#   check 1: u = [P_2, 0], arg-min v3 (0): raw = [0, P_2], prod = [sgn(0) = 0, +1]
# NMS, beta = 0.5:          r0 = [-1, 1, -1] -> P = [1, -1, 3, 0];  r1 = [0, 0.5 * 3] -> P_3 = 1.5
# OMS, beta = 0.5, a = .25: r0 = +-(relu(2 - .5) - .25) = [-1.25, 1.25, -1.25] -> P = [.75, -.75, 2.75, 0];
#                           r1 = [0 * (relu(0 - .5) - .25) = 0, relu(2.75 - .5) - .25 = 2] -> P_3 = 2
# The second iteration takes the same messages off again (u is what it was) and puts the same ones on: a fixed point.
HAND = {
    ref.NMS: ([1.0, -1.0, 3.0, 1.5], [-1.0, 1.0, -1.0, 0.0, 1.5], None),
    ref.OMS: ([0.75, -0.75, 2.75, 2.0], [-1.25, 1.25, -1.25, 0.0, 2.0], 0.25),
}


@pytest.mark.parametrize("form", [ref.NMS, ref.OMS])
@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("fn", [ref.restate, ref.restate_scalar])
def test_restatement_on_a_graph_worked_out_by_hand(form, T, fn):
    g = _Graph(4, [[0, 1, 2], [2, 3]])
    llr = np.asarray([[2.0, -2.0, 4.0, 0.0]], dtype=np.float32)
    want_P, want_R, a = HAND[form]
    beta_e = np.full((T, g.E), 0.5, dtype=np.float32)
    a_e = None if a is None else np.full((T, g.E), a, dtype=np.float32)
    bits, P, iters, succ, R = fn(g, llr, T, form, beta_e, a_e, early_stop=True)
    np.testing.assert_array_equal(P[0], np.asarray(want_P, dtype=np.float32))
    np.testing.assert_array_equal(R[0], np.asarray(want_R, dtype=np.float32))
    np.testing.assert_array_equal(bits[0], [0, 1, 0, 0])
    assert not succ[0] and iters[0] == T                  # check 0 stays unsatisfied (v1 alone is negative)
    # without the offset's zero rule the message into v2 from check 1 would be -+0.25
    assert R[0, 3] == 0.0
    # T = 0 returns the LLRs
    b0, P0, i0, s0, R0 = fn(g, llr, 0, form, beta_e[:0], a_e, early_stop=False)
    np.testing.assert_array_equal(P0, llr)
    assert i0[0] == 0 and not R0.any() and not s0[0]      # v1 < 0 alone leaves check 0 unsatisfied
    assert fn(g, np.abs(llr), 0, form, beta_e[:0], a_e, early_stop=False)[3][0]       # fixed T: success = syndrome of the LLRs


@pytest.mark.parametrize("fn", [ref.restate, ref.restate_scalar])
def test_offset_message_of_a_degree_1_check_at_an_exact_zero(fn):
    """a degree-1 check has no OTHER edge: its sign product is 1 and raw is the edge's own |u|, so u == 0 does not zero the
    offset message (raw == 0 means "prod == 0" on every wider check).  checks {v0}, {v0, v1}; llr = [0, 3]; beta .5, a .25:
      check 0: u = 0, r = relu(0 - .5) - .25 = -.25 -> P_0 = -.25
      check 1: u = [-.25, 3]; v0: raw 3, prod +1, r = 2.25 -> P_0 = 2;  v1: raw .25, prod -1, r = -(0 - .25) = .25 -> P_1 = 3.25"""
    g = _Graph(2, [[0], [0, 1]])
    llr = np.asarray([[0.0, 3.0]], dtype=np.float32)
    beta_e, a_e = np.full((1, 3), 0.5, dtype=np.float32), np.full((1, 3), 0.25, dtype=np.float32)
    _, P, _, succ, R = fn(g, llr, 1, ref.OMS, beta_e, a_e)
    np.testing.assert_array_equal(P[0], np.asarray([2.0, 3.25], dtype=np.float32))
    np.testing.assert_array_equal(R[0], np.asarray([-0.25, 2.25, 0.25], dtype=np.float32))
    assert succ[0]
    _, P, _, _, R = fn(g, llr, 1, ref.NMS, beta_e, None)              # normalised form: .5 * 0 = 0 either way
    np.testing.assert_array_equal(R[0], np.asarray([0.0, 1.5, 0.0], dtype=np.float32))


@pytest.mark.parametrize("family", ["n2d1", "n2d_oms", "edge_nms", "edge_oms"])
@pytest.mark.parametrize("early_stop", [True, False])
def test_restatement_equals_scalar_loop_on_toy_code(family, early_stop):
    code = cs.load("toy")
    dec = cs.make(family, code, 10, seed=77)
    beta_e, a_e = cs.edge_tables(dec, family, 10)
    llr = cs.input_llr("toy")
    want = ref.restate_scalar(code.tanner_graph(), llr, 10, cs.form_of(family), beta_e, a_e, early_stop)
    got = ref.restate(code.tanner_graph(), llr, 10, cs.form_of(family), beta_e, a_e, early_stop)
    for g_, w_ in zip(got, want):
        np.testing.assert_array_equal(g_, w_)


def test_scalar_loop_on_a_graph_with_degree_0_and_1_checks():
    code = cs.load("lw4")
    dec = cs.make("n2d_oms", code, 4, seed=5)
    beta_e, a_e = cs.edge_tables(dec, "n2d_oms", 4)
    llr = cs.input_llr("lw4")
    want = ref.restate_scalar(code.tanner_graph(), llr, 4, ref.OMS, beta_e, a_e, True)
    got = ref.restate(code.tanner_graph(), llr, 4, ref.OMS, beta_e, a_e, True)
    for g_, w_ in zip(got, want):
        np.testing.assert_array_equal(g_, w_)


@pytest.mark.parametrize("name", sorted(cs.INPUT_SETS))
def test_input_sets_decode_between_20_and_80_percent(name):
    """a condition on the inputs, not a measurement: both answers of the syndrome occur in every set"""
    _, _, iters, succ, _ = cs.reference(name)
    frac = float(succ.mean())
    print(f"{name}: restatement decodes {frac:.3f}, iterations {np.bincount(iters).tolist()}")
    assert 0.2 <= frac <= 0.8, (name, frac)
    llr = cs.input_llr(name)
    assert np.all(llr[0, :3] == 0.0) and np.all(llr[1] == np.round(llr[1])) and np.all(np.isfinite(llr))


def test_lane_width_codes_have_the_checks_they_are_for():
    for lw in cs.LANE_WIDTHS:
        dc = cs.load(f"lw{lw}").tanner_graph().dc
        assert dc.max() == lw and (dc == 1).any() and (dc == 0).any(), (lw, dc)
    assert cs.load("wide").tanner_graph().dc.max() == 129


@pytest.mark.parametrize("name,B,snr", [("small_96_48", 500, 3.0), ("ira_1998_1512", 128, 5.0)])
def test_layered_needs_fewer_iterations_than_flooding_oracle(name, B, snr, oracle_mod):
    code = cs.load(name)
    tg = code.tanner_graph()
    og = oracle_mod.OracleGraph(n=tg.n, check_ptr=tg.check_ptr, var_idx=tg.var_idx)
    llr = cs.awgn(np.random.default_rng(31), B, tg.n, snr)
    lay = ref.restate(tg, llr, 10, ref.NMS, np.full((10, tg.E), 0.7, dtype=np.float32))[2]
    flo = oracle_mod.basic_minsum(og, llr, 0.7, T=10, dtype=np.float32)[2]
    print(f"{name} at {snr} dB: layered {lay.mean():.2f}, flooding {flo.mean():.2f} iterations")
    assert lay.mean() < flo.mean()


# ---- the schedule keyword ---------------------------------------------------------------------------------------------
class _Recorder:
    """stands in for engine.DecodeEngine: records the keywords the host class builds the engine with"""
    calls = []

    def __init__(self, graph, **kw):
        type(self).calls.append(kw)
        self.np_dtype = np.float32


@pytest.fixture
def recorded(monkeypatch):
    import engine
    _Recorder.calls = []
    monkeypatch.setattr(engine, "DecodeEngine", _Recorder)
    monkeypatch.setattr(engine, "_require_gpu", lambda device: torch.device("cuda", 0))
    return _Recorder.calls


def _build_engine(dec, family):
    return dec._engine(torch.float32, None) if family == "basic" else dec._get_engine(None)


@pytest.mark.parametrize("family", cs.FAMILIES)
def test_schedule_reaches_the_engine_descriptor(family, recorded):
    import _native as nat
    code = cs.load("toy")
    _build_engine(cs.make(family, code, 3, seed=1, schedule="layered"), family)
    _build_engine(cs.make(family, code, 3, seed=1, schedule="flooding"), family)
    _build_engine(cs.make(family, code, 3, seed=1, schedule=None), family)
    lay, flo, default = recorded
    assert lay["schedule"] == nat.SCHED_LAYERED
    assert "schedule" not in flo and "schedule" not in default          # the keyword dict of today
    assert set(lay) - {"schedule"} == set(default)
    for k in default:
        same = np.array_equal(lay[k], default[k]) if isinstance(default[k], np.ndarray) else lay[k] == default[k]
        assert same, k


def test_ldpc_decoder_copy_of_the_edge_decoder_takes_the_keyword(recorded):
    import _native as nat
    import ldpc_decoder
    dec = ldpc_decoder.NeuralMinSumDecoder(cs.load("toy"), 2, schedule="layered")
    dec._get_engine(None)
    assert recorded[0]["schedule"] == nat.SCHED_LAYERED
    assert "schedule" not in dict(dec.state_dict())


@pytest.mark.parametrize("family", cs.FAMILIES)
def test_unknown_schedule_raises_value_error(family):
    for bad in ("paper", "Layered", True, None, ""):
        with pytest.raises(ValueError):
            if bad is None:
                from ldpc_decoder import BasicMinSumDecoder
                BasicMinSumDecoder(cs.load("toy"), 0.7, schedule=None)
            else:
                cs.make(family, cs.load("toy"), 2, seed=1, schedule=bad)


def test_schedule_is_keyword_only_and_changes_neither_init_nor_state_dict():
    from neural_2d_decoder import Neural2DMinSumDecoder
    code = cs.load("toy")
    with pytest.raises(TypeError):
        Neural2DMinSumDecoder(code, 2, 3, "layered")
    torch.manual_seed(4)
    a = Neural2DMinSumDecoder(code, 2, 3)
    torch.manual_seed(4)
    b = Neural2DMinSumDecoder(code, 2, 3, schedule="layered")
    assert list(a.state_dict()) == list(b.state_dict())
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k])


def test_schedule_is_part_of_the_engine_cache_key(recorded):
    dec = cs.make("n2d2", cs.load("toy"), 3, seed=1, schedule="flooding")
    dec._get_engine(None)
    dec._get_engine(None)
    assert len(recorded) == 1
    dec.schedule = "layered"
    dec._get_engine(None)
    assert len(recorded) == 2 and "schedule" in recorded[1]
    basic = cs.make("basic", cs.load("toy"), 3, seed=1, schedule="flooding")
    basic._engine(torch.float32, None)
    basic.schedule = "layered"
    basic._engine(torch.float32, None)
    assert len(recorded) == 4 and "schedule" in recorded[3] and "schedule" not in recorded[2]


# ---- refusals: a layered decoder has no gradient path ------------------------------------------------------------------
NEURAL = [f for f in cs.FAMILIES if f != "basic"]


@pytest.mark.parametrize("family", NEURAL)
def test_joint_posterior_loss_is_refused(family):
    dec = cs.make(family, cs.load("toy"), 3, seed=1)
    with pytest.raises(NotImplementedError, match="layered"):
        dec.joint_posterior_loss(torch.zeros(2, 7))


@pytest.mark.parametrize("family", NEURAL)
def test_forward_with_autograd_on_is_refused(family):
    dec = cs.make(family, cs.load("toy"), 3, seed=1)
    assert any(p.requires_grad for p in dec.parameters())
    with torch.enable_grad():      # stated, not inherited: the GPU file runs this test under its module-wide no_grad fixture
        with pytest.raises(NotImplementedError, match="layered"):
            dec(torch.zeros(2, 7))
        for p in dec.parameters():
            p.requires_grad_(False)
        with pytest.raises(NotImplementedError, match="layered"):      # the LLRs asking for a gradient: refused too
            dec(torch.zeros(2, 7, requires_grad=True))
