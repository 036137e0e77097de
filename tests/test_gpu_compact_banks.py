"""
GPU tests (-m gpu) of the compact fixed-T kernel (resident_decode<..., CPT>) on the jointly placed slot layout: odd row
stride, check positions permuted inside their degrees, the rows of every check permuted (csrc/ldpc_plan.h:
cpt_place_banks).  Every per-slot table (cvar, bslot, oaslot, edge_of_slot, the variables' slot offsets) is filled from
the permuted map, so the per-edge check-to-variable messages of the last iteration (ldpc_debug_resident_c2v, CSR order)
and every decode output must equal the streaming engine's bit for bit: Basic, Neural-2D (both sharing types; one beta
slot per edge where the type gives one) and RCQ, on the (1998,1512) code and on random codes that take the compact
plan, with clipped (infinite) LLRs as in test_gpu_parity (a NaN is outside the decoders' domain).
"""
import numpy as np
import pytest
import torch

from test_gpu_compact_grid import QP, assert_compact, assert_same_as_stream, llrs, make_code
from test_gpu_parity import assert_codes

pytestmark = pytest.mark.gpu

NAMES = ["ira", "spread", "full_round0"]


@pytest.fixture(autouse=True)
def inference_mode(monkeypatch):
    monkeypatch.setenv("LDPC_ENGINE_MODE", "auto")
    with torch.no_grad():
        yield


def placement_of(eng):
    import _native
    g = eng.graph
    slots = np.zeros(g.E, np.int32)
    base = np.zeros(g.E, np.int32)
    pos = np.zeros(len(g.check_ptr) - 1, np.int32)
    geo = np.zeros(2, np.int32)
    rc = eng._lib.ldpc_debug_compact_banks(eng.handle, 0, 0, 0, None, None, _native.ptr(slots), _native.ptr(pos), None,
                                           _native.ptr(base), None, None, _native.ptr(geo))
    assert rc == 0, "the engine has no compact plan"
    return slots, base, pos, geo


def clipped(llr, seed):
    """test_gpu_parity's saturated inputs: scattered +-inf in the direction of the sample, a third of one codeword +inf"""
    rng = np.random.default_rng(seed)
    llr = llr.copy()
    sat = rng.random(llr.shape) < 0.02
    llr[sat] = np.where(llr[sat] >= 0, np.inf, -np.inf)
    llr[0, : llr.shape[1] // 3] = np.inf
    return llr


def c2v_both(eng, x):
    """per-edge C2V of the last iteration: (compact resident kernel, streaming engine), CSR edge order"""
    res, _, _ = eng.debug_resident_c2v(x, early_stop=False)
    eng.set_mode("stream")
    eng.decode(x, early_stop=False)
    ref = eng.debug_c2v(x.shape[0])
    eng.set_mode("auto")
    return res.cpu().numpy(), ref.cpu().numpy()


def assert_values_equal(res, ref):
    assert res.dtype == np.float32 and ref.dtype == np.float32
    bad = res.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), f"{int(bad.sum())} per-edge C2V values differ from the streaming engine"


@pytest.mark.parametrize("name", NAMES)
def test_the_rows_of_the_shipped_plan_are_permuted(name, gpu_device):
    """the cases below exercise what they claim to: the decoder runs a placement that differs from CSR rows"""
    from ldpc_decoder import BasicMinSumDecoder
    eng = BasicMinSumDecoder(make_code(name), 0.7)._engine(torch.float32, gpu_device)
    assert_compact(eng)
    slots, base, pos, geo = placement_of(eng)
    assert geo[0] % 2 == 1
    assert len(np.unique(slots)) == len(slots) and slots.max() < geo[1]
    assert np.any(slots // geo[0] != base // geo[0]), "no row moved"
    assert np.any(slots % geo[0] != base % geo[0]), "no check moved"


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("inf", [False, True])
def test_basic_c2v_and_outputs_equal_the_streaming_engine(name, inf, gpu_device):
    from ldpc_decoder import BasicMinSumDecoder
    code = make_code(name)
    llr = llrs(50, 35, code.n)
    if inf:
        llr = clipped(llr, 51)
    x = torch.from_numpy(llr).to(gpu_device)
    eng = BasicMinSumDecoder(code, 0.7)._engine(torch.float32, gpu_device)
    assert_compact(eng)
    assert_same_as_stream(eng, x)
    assert_values_equal(*c2v_both(eng, x))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("wtype", [1, 2])
def test_neural2d_c2v_and_outputs_equal_the_streaming_engine(name, wtype, gpu_device):
    """distinct weights in every slot and iteration: an edge that read another edge's beta slot would show"""
    from neural_2d_decoder import Neural2DMinSumDecoder
    code = make_code(name)
    rng = np.random.default_rng(60 + wtype)
    dec = Neural2DMinSumDecoder(code, weight_sharing_type=wtype, max_iterations=10)
    for p in dec.beta_weights.values():
        p.fill_(float(np.float32(rng.uniform(0.5, 1.0))))
    for p in dec.alpha_weights.values():
        p.fill_(float(np.float32(rng.uniform(0.8, 1.2))))
    x = torch.from_numpy(llrs(61, 33, code.n)).to(gpu_device)
    eng = dec._get_engine(gpu_device)
    assert_compact(eng)
    assert_same_as_stream(eng, x)
    assert_values_equal(*c2v_both(eng, x))


def test_a_neural2d_sharing_type_runs_per_edge_beta_slots(gpu_device):
    """bit 31 of the check words: the per-lane form of the check phase, which reads bslot by slot"""
    import _native
    from neural_2d_decoder import Neural2DMinSumDecoder
    per_edge = []
    for wtype in (1, 2):
        eng = Neural2DMinSumDecoder(make_code("spread"), weight_sharing_type=wtype, max_iterations=10)._get_engine(gpu_device)
        words = np.zeros(8, np.uint32)
        assert eng._lib.ldpc_debug_compact_checks(eng.handle, 0, 0, 0, None, None, _native.ptr(words)) == 0
        per_edge.append(bool(np.all(words[words != 0] >> 31)))
    assert any(per_edge)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("inf", [False, True])
def test_rcq_codes_and_outputs_equal_the_streaming_engine(name, inf, gpu_device):
    """the streaming engine keeps the 3-bit codes, the resident one the reconstructed values: compared as
    test_gpu_parity compares them (codes_of / assert_codes)"""
    from rcq_decoder import RCQMinSumDecoder, _quantizer_schedule, _threshold_table
    code = make_code(name)
    llr = llrs(70, 21, code.n)
    if inf:
        llr = clipped(llr, 71)
    x = torch.from_numpy(llr).to(gpu_device)
    dec = RCQMinSumDecoder(code, 3, 8, QP, 10)
    eng = dec._get_engine(gpu_device)
    assert_compact(eng)
    assert_same_as_stream(eng, x)
    vals, want = c2v_both(eng, x)
    tau = _threshold_table(dec.quantizers)[_quantizer_schedule(len(dec.quantizers), 10)[9]]
    L = len(tau)
    mag = np.abs(vals)
    level = np.full(vals.shape, 255, np.int64)
    for k in range(L):
        level[mag == tau[k]] = k
    assert np.all(level != 255), "a resident C2V value is not a reconstruction level"
    assert_codes(np.where(np.signbit(vals), L, 0) + level, want, L)
