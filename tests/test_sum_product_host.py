"""
Sum-product decoder, host side (no GPU): the numpy restatement against the closed form, the conditions under which the GPU
tests may compare decisions, and the API facts.
"""
import inspect
import os
import re

import numpy as np
import pytest

import spa_reference as R
from conftest import ROOT

# the tolerance input sets of tests/test_gpu_sum_product.py: (code, SNR in dB, frames)
INPUT_SETS = (("small_96_48", 3.0, 400), ("small_96_48", 5.0, 400), ("ira_1998_1512", 5.5, 48))
T = 10


def closed_form(x):
    """2 atanh(prod over the OTHER edges of tanh(x / 2)) in float64, [..., dc] -> [..., dc]"""
    t = np.tanh(np.asarray(x, dtype=np.float64) / 2.0)
    out = np.empty_like(t)
    for k in range(t.shape[-1]):
        out[..., k] = 2.0 * np.arctanh(np.prod(np.delete(t, k, axis=-1), axis=-1))
    return out


@pytest.mark.parametrize("dc", range(2, 9))
def test_restatement_is_the_definition(dc):
    rng = np.random.default_rng(100 + dc)
    x = rng.uniform(-12.0, 12.0, size=(2000, dc))
    got = R.check_update(x)
    assert got.dtype == np.float64
    np.testing.assert_allclose(got, closed_form(x), rtol=1e-9, atol=0.0)
    np.testing.assert_allclose(R.check_update(x, 0.75), 0.75 * closed_form(x), rtol=1e-9, atol=0.0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.longdouble])
@pytest.mark.parametrize("dc", [2, 3, 5, 8])
def test_zero_input_gives_zeros_on_the_other_edges(dc, dtype):
    rng = np.random.default_rng(dc)
    for zero in (0.0, -0.0):
        for k in range(dc):
            x = rng.uniform(-12.0, 12.0, size=(50, dc)).astype(dtype)
            x[:, k] = zero
            out = R.check_update(x)
            others = np.delete(out, k, axis=-1)
            assert np.all(others == 0), (dc, k, zero)
            if dc > 2:
                assert np.all(out[:, k] != 0)           # the zero edge's own message does not see its zero


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.longdouble])
@pytest.mark.parametrize("dc", [2, 3, 4, 7, 8])
def test_update_is_odd_bit_for_bit(dc, dtype):
    rng = np.random.default_rng(10 * dc)
    x = rng.uniform(-12.0, 12.0, size=(200, dc)).astype(dtype)
    base = R.check_update(x)
    for k in range(dc):
        y = x.copy()
        y[:, k] = -y[:, k]
        out = R.check_update(y)
        want = -base
        want[:, k] = base[:, k]                          # edge k's own message does not depend on its input
        assert np.array_equal(out, want), (dc, k)
    assert np.array_equal(R.check_update(-x), base if dc % 2 else -base)   # dc - 1 inputs feed each message


def test_huge_and_tiny_inputs_stay_finite():
    for dtype, big in ((np.float32, 3e38), (np.float64, 3e38)):
        x = np.array([[big, 0.5, -big, 1e30, 1e-30, big]], dtype=dtype)
        for dc in range(2, 7):
            out = R.check_update(x[:, :dc])
            assert np.all(np.isfinite(out)), (dtype, dc, out)


def test_degree_one_check_is_refused():
    with pytest.raises(ValueError):
        R.Graph(3, [0, 1, 3], [0, 1, 2])
    with pytest.raises(ValueError):
        R.check_update(np.ones((1, 1)))


@pytest.mark.parametrize("name,snr,frames", INPUT_SETS)
def test_tolerance_inputs_are_decisive(name, snr, frames):
    """What lets the GPU tests compare decisions: a frame is non-decisive when, at some iteration t up to its float64 stop
    iteration, some |posterior| < 8 D_t (D_t: float32 against float64 restatement).  At most 1 % of the frames may be."""
    import codes
    g = R.Graph.of(codes.load_code(name, max_iterations=T).tanner_graph())
    x = R.awgn_inputs(g.n, frames, snr)
    lo, hi = R.decode(g, x, T, np.float32), R.decode(g, x, T, np.float64)
    flags, D = R.non_decisive(lo, hi, hi["stop_iterations"])
    print(f"{name} {snr} dB {frames} frames: D_0 {D[0]:.3g} D_{T - 1} {D[-1]:.3g} non-decisive {int(flags.sum())}")
    assert flags.sum() <= 0.01 * frames
    assert np.all(D > 0) and np.all(D < 1e-3)
    decisive = ~flags
    assert np.array_equal(lo["stop_iterations"][decisive], hi["stop_iterations"][decisive])
    assert np.array_equal(lo["stop_bits"][decisive], hi["stop_bits"][decisive])


def test_early_stop_outputs_follow_the_stop_rule():
    import codes
    g = R.Graph.of(codes.load_code("small_96_48", max_iterations=T).tanner_graph())
    x = R.awgn_inputs(g.n, 60, 3.0)
    r = R.decode(g, x, T, np.float64)
    for b in range(60):
        ok = r["ok"][:, b]
        first = int(np.argmax(ok)) + 1 if ok.any() else T
        assert r["stop_iterations"][b] == first and r["stop_success"][b] == ok.any()
        assert np.array_equal(r["stop_bits"][b], r["bits"][first - 1, b])
        assert np.array_equal(r["stop_posterior"][b], r["posterior"][first - 1, b])
    assert len(set(r["stop_iterations"])) > 2


def test_api_facts():
    import _native as nat
    import ldpc_decoder
    from ldpc_decoder import BasicMinSumDecoder, SumProductDecoder

    header = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    assert re.search(r"\bLDPC_C2V_SPA\s*=\s*3\b", header)
    assert re.search(r"#define\s+LDPC_HIP_ABI_VERSION\s+1\b", header)
    assert nat.C2V_SPA == 3 and (nat.C2V_NMS, nat.C2V_RCQ, nat.C2V_OMS) == (0, 1, 2)

    sig = inspect.signature(SumProductDecoder.__init__)
    assert list(sig.parameters) == ["self", "code", "scale"] and sig.parameters["scale"].default == 1.0
    dsig = inspect.signature(SumProductDecoder.decode)
    assert list(dsig.parameters) == ["self", "llr", "early_stop", "device"]
    assert dsig.parameters["early_stop"].default is True and dsig.parameters["device"].default is None
    assert list(inspect.signature(SumProductDecoder._engine).parameters) == ["self", "torch_dtype", "device"]
    assert list(inspect.signature(SumProductDecoder._get_engine).parameters) == ["self", "device"]
    # one decode body, shared through a common base
    assert SumProductDecoder.decode is BasicMinSumDecoder.decode
    assert not issubclass(SumProductDecoder, BasicMinSumDecoder) and not issubclass(BasicMinSumDecoder, SumProductDecoder)

    # BasicMinSumDecoder is what it was
    bsig = inspect.signature(BasicMinSumDecoder.__init__)
    assert list(bsig.parameters) == ["self", "code", "factor", "schedule"]
    assert bsig.parameters["factor"].default == 0.7 and bsig.parameters["schedule"].default == "flooding"
    assert bsig.parameters["schedule"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(BasicMinSumDecoder.decode) == dsig
    assert not hasattr(BasicMinSumDecoder, "_get_engine")
    code = ldpc_decoder.create_test_ldpc_code()
    b = BasicMinSumDecoder(code)
    assert (b.factor, b.schedule, b.code) == (0.7, "flooding", code)
    with pytest.raises(ValueError):
        BasicMinSumDecoder(code, schedule="spa")
    s = SumProductDecoder(code, 0.9)
    assert (s.scale, s.code, s.schedule) == (0.9, code, "flooding")
