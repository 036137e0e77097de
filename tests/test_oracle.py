"""
CPU tests of the oracle (oracle/ldpc_oracle.c): the C restatement of the reference's
decode loops must reproduce every golden vector captured from the REAL reference
(tests/golden/*.npz, written by oracle/make_golden.py in the build container).
This is what pins the oracle; the GPU tests then compare the HIP engine with it.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden_sub, load_golden, weights_dict

PKG_DATA = os.path.join(os.path.dirname(GOLDEN), "..", "implementation-of-neural-ldpc-decoders-with-degree-specific-weight-sharing-and-rcq-quantization_amd", "data")


def graph_of(oracle, gold):
    if "H" in gold:
        return oracle.OracleGraph(gold["H"].astype(np.int64))
    z = np.load(os.path.join(PKG_DATA, str(gold["graph"]) + ".npz"))
    return oracle.OracleGraph(n=int(z["n"]), check_ptr=z["check_ptr"], var_idx=z["var_idx"].astype(np.int64))


def bitwise_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ third-party arithmetic
def test_sum_association_orders(oracle_mod):
    """torch.sum fp32 / np.sum fp64 of 1-D contiguous arrays, N = 0..575"""
    g = load_golden("sums")
    for x32, y32, x64, y64, n in zip(g["x32"], g["y32"], g["x64"], g["y64"], g["n"]):
        if n >= 0:
            assert bitwise_equal(oracle_mod.sum_f32(x32[:n]), y32), f"torch order N={n}"
            assert bitwise_equal(oracle_mod.sum_f64(x64[:n]), y64), f"numpy order N={n}"
        else:
            m = -n - 1
            assert bitwise_equal(oracle_mod.sum_f32(x32[:m]), y32), f"torch order (alphabet) N={m}"


def test_quantizer_known_answers(oracle_mod):
    g = load_golden("quantizer")
    # the repo's only deterministic vector (rcq_decoder.py:607-611, comprehensive_test.py:259-263)
    thr = oracle_mod.quantizer_thresholds(3, 5.0, 1.5)
    np.testing.assert_array_equal(np.asarray(thr), g["kat_thresholds"])
    assert thr == [0.0, 0.9622504486493761, 2.721655269759087, 5.0]
    np.testing.assert_array_equal(oracle_mod.quantize(g["kat_x"], thr), g["kat_codes"])
    np.testing.assert_array_equal(g["kat_codes"], [6, 5, 0, 2, 2])
    assert bitwise_equal(oracle_mod.dequantize(g["kat_codes"], thr), g["kat_deq"])
    for ci, (bc, C_, gm) in enumerate(g["sweep_cfg"]):
        thr = oracle_mod.quantizer_thresholds(int(bc), float(C_), float(gm))
        np.testing.assert_array_equal(np.asarray(thr), g[f"sweep{ci}_thresholds"])
        np.testing.assert_array_equal(oracle_mod.quantize(g[f"sweep{ci}_x"], thr), g[f"sweep{ci}_codes"])
        assert bitwise_equal(oracle_mod.dequantize(g[f"sweep{ci}_codes"], thr), g[f"sweep{ci}_deq"])


def test_quantizer_schedule(oracle_mod):
    # T=10 -> iterations 0-2 / 3-5 / 6-9, T=20 -> 0-5 / 6-12 / 13-19
    np.testing.assert_array_equal(oracle_mod.quantizer_schedule(10, 3), [0, 0, 0, 1, 1, 1, 2, 2, 2, 2])
    np.testing.assert_array_equal(oracle_mod.quantizer_schedule(20, 3), [0] * 6 + [1] * 7 + [2] * 7)
    np.testing.assert_array_equal(oracle_mod.quantizer_schedule(7, 1), [0] * 7)
    np.testing.assert_array_equal(oracle_mod.quantizer_schedule(9, 2), [0, 0, 0, 1, 1, 1, 1, 1, 1])


# ------------------------------------------------------------------ decoders vs golden
@pytest.mark.parametrize("name", ["toy_basic", "small_basic", "ira_basic"])
def test_basic_golden(name, oracle_mod):
    g = load_golden(name)
    og = graph_of(oracle_mod, g)
    bits, post, iters, succ = oracle_mod.basic_minsum(og, g["llr"], float(g["factor"]), int(g["T"]))
    np.testing.assert_array_equal(bits, g["bits"])
    np.testing.assert_array_equal(iters, g["iters"])
    np.testing.assert_array_equal(succ, g["success"])


def _check_neural(oracle_mod, og, sub):
    beta = weights_dict(sub["beta_keys"], sub["beta_vals"])
    alpha = weights_dict(sub["alpha_keys"], sub["alpha_vals"])
    bits, post, iters, _ = oracle_mod.neural2d(og, sub["llr"], int(sub["wtype"]), int(sub["T"]), beta, alpha)
    np.testing.assert_array_equal(bits, sub["bits"])
    np.testing.assert_array_equal(iters, sub["iters"])
    assert bitwise_equal(post, sub["posterior"])          # bit-exact, sign of zero included


def test_neural2d_golden(oracle_mod):
    g = load_golden("toy_neural2d")
    og = graph_of(oracle_mod, g)
    for w in (1, 2, 3, 4):
        _check_neural(oracle_mod, og, golden_sub(g, f"t{w}"))
        _check_neural(oracle_mod, og, golden_sub(g, f"t{w}d"))      # randn*0.1 init: negative betas
    g = load_golden("small_neural2d")
    og = graph_of(oracle_mod, g)
    for w in (1, 2, 3, 4):
        _check_neural(oracle_mod, og, golden_sub(g, f"t{w}"))
    g = load_golden("ira_neural2d")
    _check_neural(oracle_mod, graph_of(oracle_mod, g), g)


def _check_rcq(oracle_mod, og, sub):
    qp = [tuple(x) for x in sub["qp"]]
    bits, post, iters, succ, codes = oracle_mod.rcq(og, sub["llr"], int(sub["bc"]), qp, int(sub["T"]), trace_codes=True)
    np.testing.assert_array_equal(bits, sub["bits"])
    np.testing.assert_array_equal(iters, sub["iters"])
    np.testing.assert_array_equal(succ, sub["success"])
    for r, it in enumerate(sub["iters"]):                            # every iteration's 3-bit codes, CSR order
        np.testing.assert_array_equal(codes[r, :it], sub["codes"][r, :it])


def _check_wrcq(oracle_mod, og, sub):
    qp = [tuple(x) for x in sub["qp"]]
    beta = weights_dict(sub["beta_keys"], sub["beta_vals"])
    alpha = weights_dict(sub["alpha_keys"], sub["alpha_vals"])
    bits, post, iters, _, codes = oracle_mod.weighted_rcq(og, sub["llr"], int(sub["bc"]), qp, int(sub["wtype"]),
                                                          int(sub["T"]), beta, alpha, trace_codes=True)
    np.testing.assert_array_equal(bits, sub["bits"])
    np.testing.assert_array_equal(iters, sub["iters"])
    assert bitwise_equal(post, sub["posterior"])
    for r, it in enumerate(sub["iters"]):
        np.testing.assert_array_equal(codes[r, :it], sub["codes"][r, :it])


def test_rcq_golden(oracle_mod):
    g = load_golden("toy_rcq")
    og = graph_of(oracle_mod, g)
    _check_rcq(oracle_mod, og, golden_sub(g, "rcq"))
    _check_rcq(oracle_mod, og, golden_sub(g, "rcq4"))
    for w in (1, 2, 3, 4):
        _check_wrcq(oracle_mod, og, golden_sub(g, f"w{w}"))
    _check_wrcq(oracle_mod, og, golden_sub(g, "w2d"))
    g = load_golden("small_rcq")
    og = graph_of(oracle_mod, g)
    _check_rcq(oracle_mod, og, golden_sub(g, "rcq"))
    _check_wrcq(oracle_mod, og, golden_sub(g, "w2"))
    _check_wrcq(oracle_mod, og, golden_sub(g, "w1"))
    g = load_golden("ira_rcq")
    _check_rcq(oracle_mod, graph_of(oracle_mod, g), g)
    g = load_golden("ira_wrcq")
    _check_wrcq(oracle_mod, graph_of(oracle_mod, g), g)


def test_dvbs2_wrcq_golden(oracle_mod):
    if not os.path.exists(os.path.join(GOLDEN, "dvbs2_wrcq.npz")):
        pytest.skip("dvbs2 golden not generated")
    g = load_golden("dvbs2_wrcq")
    _check_wrcq(oracle_mod, graph_of(oracle_mod, g), g)


@pytest.mark.parametrize("name", ["toy_offset_edge", "small_offset_edge"])
def test_offset_and_edge_weight_golden(name, oracle_mod):
    """Neural2DOffsetMinSumDecoder types 1-4, NeuralMinSumDecoder, NeuralOffsetMinSumDecoder"""
    g = load_golden(name)
    og = graph_of(oracle_mod, g)
    for w in (1, 2, 3, 4):
        sub = golden_sub(g, f"o{w}")
        beta = weights_dict(sub["beta_keys"], sub["beta_vals"])
        alpha = weights_dict(sub["alpha_keys"], sub["alpha_vals"])
        bits, post, iters, _ = oracle_mod.neural2d_offset(og, sub["llr"], w, int(sub["T"]), beta, alpha)
        np.testing.assert_array_equal(bits, sub["bits"])
        np.testing.assert_array_equal(iters, sub["iters"])
        np.testing.assert_array_equal(post, sub["posterior"])
    for tag, offset in (("nms", False), ("oms", True)):
        sub = golden_sub(g, tag)
        beta = weights_dict(sub["beta_keys"], sub["beta_vals"])
        bits, post, iters, _ = oracle_mod.neural_minsum(og, sub["llr"], int(sub["T"]), beta, offset=offset)
        np.testing.assert_array_equal(bits, sub["bits"])
        np.testing.assert_array_equal(iters, sub["iters"])
        np.testing.assert_array_equal(post, sub["posterior"])


def test_layered_rcq_golden(oracle_mod):
    """RCQMinSumDecoder(layered=True) as the reference executes it (rcq_decoder.py:281-350)"""
    g = load_golden("layered_rcq")
    for tag, og in (("toy", oracle_mod.OracleGraph(g["toy_H"].astype(np.int64))),
                    ("small", graph_of(oracle_mod, {"graph": "small_96_48"}))):
        bits, post, iters, succ = oracle_mod.rcq_layered(og, g[f"{tag}_llr"], 3, [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)],
                                                         int(g[f"{tag}_T"]))
        np.testing.assert_array_equal(bits, g[f"{tag}_bits"])
        np.testing.assert_array_equal(iters, g[f"{tag}_iters"])
        np.testing.assert_array_equal(succ, g[f"{tag}_success"])


# ------------------------------------------------------------------ 2, 32, 64 and 128 quantiser levels
WIDTH_RCQ = ["rcq2", "rcq6", "rcq7", "rcq8"]
WIDTH_WRCQ = ["w2b6", "w2b8", "w1b8"]


def test_rcq_widths_golden(oracle_mod):
    """RCQMinSumDecoder at bc 2, 6, 7, 8, WeightedRCQDecoder type 2 at bc 6, 8 and type 1 at bc 8, every iteration's codes:
    a code is one byte, sign * L + level, and at bc = 8 the oracle's uint8 trace has to carry bit 7 and level 127"""
    g = load_golden("rcq_widths")
    og = graph_of(oracle_mod, g)
    for tag in WIDTH_RCQ:
        sub = golden_sub(g, tag)
        assert int(sub["bc"]) == int(tag[3:]) and int(sub["T"]) == 6 and sub["llr"].shape == (16, 96)
        _check_rcq(oracle_mod, og, sub)
    for tag in WIDTH_WRCQ:
        sub = golden_sub(g, tag)
        assert (int(sub["wtype"]), int(sub["bc"])) == (int(tag[1]), int(tag[3:]))
        _check_wrcq(oracle_mod, og, sub)
    # the fixture itself: the reference wrote codes with bit 7 set, the saturated code of either sign among them
    for tag in ("rcq8", "w2b8", "w1b8"):
        sub = golden_sub(g, tag)
        ran = np.concatenate([sub["codes"][r, :it].ravel() for r, it in enumerate(sub["iters"])])
        assert (ran >= 128).any() and (ran == 127).any() and (ran == 255).any(), tag
    assert 0 < int(golden_sub(g, "rcq8")["success"].sum()) < 16


@pytest.mark.parametrize("bc", [2, 8])
def test_layered_rcq_widths_golden(bc, oracle_mod):
    """RCQMinSumDecoder(layered=True) of the reference at 2 and 128 levels"""
    g = load_golden("rcq_widths")
    sub = golden_sub(g, f"lay{bc}")
    assert int(sub["bc"]) == bc
    og = graph_of(oracle_mod, g)
    bits, post, iters, succ = oracle_mod.rcq_layered(og, sub["llr"], bc, [tuple(x) for x in sub["qp"]], int(sub["T"]))
    np.testing.assert_array_equal(bits, sub["bits"])
    np.testing.assert_array_equal(iters, sub["iters"])
    np.testing.assert_array_equal(succ, sub["success"])
    assert bitwise_equal(post, sub["oracle_posterior"])
    assert len(np.unique(sub["iters"])) >= 2


def test_quantizer_width_sweeps(oracle_mod):
    """quantize / dequantize on, one ulp below and one ulp above every threshold of 32-, 64- and 128-level quantisers"""
    g = load_golden("rcq_widths")
    assert sorted(int(c[0]) for c in g["wsweep_cfg"]) == [6, 7, 8, 8]
    for ci, (bc, C_, gm) in enumerate(g["wsweep_cfg"]):
        thr = oracle_mod.quantizer_thresholds(int(bc), float(C_), float(gm))
        assert len(thr) == 2 ** (int(bc) - 1)
        np.testing.assert_array_equal(np.asarray(thr), g[f"wsweep{ci}_thresholds"])
        codes = g[f"wsweep{ci}_codes"]
        np.testing.assert_array_equal(oracle_mod.quantize(g[f"wsweep{ci}_x"], thr), codes)
        assert bitwise_equal(oracle_mod.dequantize(codes, thr), g[f"wsweep{ci}_deq"])
        assert len(np.unique(codes)) == 2 * len(thr)                     # every code value, both signs of every level


# ------------------------------------------------------------------ oracle self-consistency
def test_fixed_iteration_mode_and_threads(oracle_mod):
    """early_stop=False runs T iterations; success = final syndrome; threads do not change results"""
    g = load_golden("small_basic")
    og = graph_of(oracle_mod, g)
    x = g["llr"]
    b1, p1, i1, s1 = oracle_mod.basic_minsum(og, x, 0.7, 12, early_stop=False, threads=1)
    b2, p2, i2, s2 = oracle_mod.basic_minsum(og, x, 0.7, 12, early_stop=False, threads=4)
    assert np.all(i1 == 12) and np.array_equal(b1, b2) and bitwise_equal(p1, p2) and np.array_equal(s1, s2)
    H = np.zeros((og.m, og.n), dtype=np.int64)
    H[og.rows, og.var_idx] = 1
    np.testing.assert_array_equal(s1, (H @ b1.T % 2).sum(axis=0) == 0)


def test_basic_fp32_posterior_equals_neural2d_type3(oracle_mod):
    """Basic in fp32 is Neural2D type 3 with every beta = 0.7 (SURVEY 8c cross-check)"""
    g = load_golden("small_basic")
    og = graph_of(oracle_mod, g)
    x = g["llr"].astype(np.float32)
    dcs = sorted(set(og.dc.tolist()))
    beta = {f"iter_{t}_dc{d}": float(np.float32(0.7)) for t in range(12) for d in dcs}
    b1, p1, i1, _ = oracle_mod.basic_minsum(og, x, 0.7, 12, dtype=np.float32)
    b2, p2, i2, _ = oracle_mod.neural2d(og, x, 3, 12, beta, {})
    assert np.array_equal(b1, b2) and np.array_equal(i1, i2) and bitwise_equal(p1, p2)


# ------------------------------------------------------------------ capped decodes (the GPU tests' per-iteration reference)
@pytest.mark.parametrize("name,tag", [("toy_rcq", "rcq"), ("toy_rcq", "rcq4"), ("toy_rcq", "w2d"), ("small_rcq", "rcq"),
                                      ("small_rcq", "w1"), ("ira_rcq", None), ("ira_wrcq", None), ("dvbs2_wrcq", None)]
                         + [("rcq_widths", tag) for tag in WIDTH_RCQ + WIDTH_WRCQ])
def test_oracle_capped_is_a_prefix_of_the_full_decode(name, tag, oracle_mod):
    """oracle_capped (tests/test_gpu_parity.py) is what every capped GPU decode is held to: t iterations of the T-iteration
    schedule.  Fixed T: its code trace is the first t slices of the full trace, every iteration count is t, success is the
    syndrome of its bits.  Early stop: a codeword that stops within t has the full decode's outputs, any other one reports
    t iterations and no success.  At t = T it gives the reference's golden bits, iterations, codes (and posterior)."""
    from rcq_decoder import _quantizer_schedule
    from test_gpu_parity import oracle_capped, rcq_trace_block
    g, sub, kw = rcq_trace_block(name, tag)
    og = graph_of(oracle_mod, g)
    T, llr = int(sub["T"]), sub["llr"]
    H = np.zeros((og.m, og.n), dtype=np.int64)
    H[og.rows, og.var_idx] = 1
    # the oracle's schedule is an independent restatement: it must be the one the decoders hand to the engine
    np.testing.assert_array_equal(oracle_mod.quantizer_schedule(T, len(kw["qp"])), _quantizer_schedule(len(kw["qp"]), T))
    fb, fp, fi, fs, fc = oracle_capped(oracle_mod, og, llr, t=T, T=T, early_stop=False, trace_codes=True, **kw)
    eb, ep, ei, es, ec = oracle_capped(oracle_mod, og, llr, t=T, T=T, early_stop=True, trace_codes=True, **kw)
    np.testing.assert_array_equal(eb, sub["bits"])
    np.testing.assert_array_equal(ei, sub["iters"])
    if "success" in sub:
        np.testing.assert_array_equal(es, sub["success"])
    assert bitwise_equal(ep, sub["posterior"] if "posterior" in sub else sub["oracle_posterior"])
    for r, it in enumerate(sub["iters"]):
        np.testing.assert_array_equal(ec[r, :it], sub["codes"][r, :it])
    for t in range(1, T + 1):
        b, p, i, s, c = oracle_capped(oracle_mod, og, llr, t=t, T=T, early_stop=False, trace_codes=True, **kw)
        assert c.shape == (len(llr), t, og.E) and np.array_equal(c, fc[:, :t]), f"t={t}: code trace is not a prefix"
        assert np.all(i == t)
        np.testing.assert_array_equal(s, (H @ b.T % 2).sum(axis=0) == 0)
        if t == T:
            assert np.array_equal(b, fb) and bitwise_equal(p, fp) and np.array_equal(s, fs)
        b, p, i, s, c = oracle_capped(oracle_mod, og, llr, t=t, T=T, early_stop=True, trace_codes=True, **kw)
        done = ei <= t
        assert np.array_equal(i[done], ei[done]) and np.array_equal(s[done], es[done]) and np.array_equal(b[done], eb[done])
        assert bitwise_equal(p[done], ep[done])
        assert np.all(i[~done] == t) and not s[~done].any()
        for r in range(len(llr)):
            np.testing.assert_array_equal(c[r, :i[r]], ec[r, :i[r]])
        if len(kw["qp"]) == 1 and kw["kind"] == "rcq":
            # one quantiser and no weights: nothing depends on T, the capped decode is the plain T = t decode
            ob, op, oi, os_ = oracle_mod.rcq(og, llr, kw["bc"], kw["qp"], t, early_stop=True)
            assert np.array_equal(b, ob) and bitwise_equal(p, op) and np.array_equal(i, oi) and np.array_equal(s, os_)


def test_oracle_capped_float_decoders(oracle_mod):
    """the helper's floating-point kinds at t = T are the oracle's own decoders; Basic has no per-iteration table, so at any
    t it is the plain T = t decode"""
    from test_gpu_parity import oracle_capped
    g = load_golden("small_basic")
    og = graph_of(oracle_mod, g)
    rng = np.random.default_rng(3)
    x32 = g["llr"].astype(np.float32)
    T = 8
    for early in (True, False):
        for t in (1, 4, T):
            for x in (g["llr"], x32):
                got = oracle_capped(oracle_mod, og, x, "basic", t, T, early_stop=early)
                want = oracle_mod.basic_minsum(og, x, 0.7, t, early_stop=early, dtype=x.dtype.type)
                assert all(bitwise_equal(a, b) for a, b in zip(got, want))
    keys = sorted({f"iter_{t}_dc{d}" for t in range(T) for d in og.dc.tolist()})
    beta = {k: float(np.float32(rng.uniform(0.1, 1.0))) for k in keys}
    alpha = {f"iter_{t}_dv{d}": float(np.float32(rng.uniform(0.1, 0.5))) for t in range(T) for d in og.dv.tolist()}
    for early in (True, False):
        got = oracle_capped(oracle_mod, og, x32, "neural2d", T, T, early_stop=early, wtype=2, beta=beta, alpha=alpha)
        want = oracle_mod.neural2d(og, x32, 2, T, beta, alpha, early_stop=early)
        assert all(bitwise_equal(a, b) for a, b in zip(got, want))
        got = oracle_capped(oracle_mod, og, x32, "offset", T, T, early_stop=early, wtype=2, beta=beta, alpha=alpha)
        want = oracle_mod.neural2d_offset(og, x32, 2, T, beta, alpha, early_stop=early)
        assert all(bitwise_equal(a, b) for a, b in zip(got, want))
        # t < T reads rows 0..t-1 of the T-row tables: the same as a t-iteration decoder given the same first t rows
        t = 3
        got = oracle_capped(oracle_mod, og, x32, "neural2d", t, T, early_stop=early, wtype=2, beta=beta, alpha=alpha)
        want = oracle_mod.neural2d(og, x32, 2, t, beta, alpha, early_stop=early)
        assert all(bitwise_equal(a, b) for a, b in zip(got, want))
