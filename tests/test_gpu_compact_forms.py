"""
GPU tests (-m gpu) of ALL EIGHT compact fixed-T kernels (resident_decode<2, FORM, BPC, NL, 495, 0, float, false, true, true>,
FORM in {NMS, OMS, RCQ}, BPC = one beta slot per check, NL = 4 or the run-time level count) and of the table flags that
switch code inside them (unit_alpha, rcq_zero0, a check-side alpha table of the offset form; every alpha is read from global
memory), on plans with mixed cells, partly filled and empty waves, scalar-counted next to per-lane check waves and degree-1
and degree-2 checks: the codes `tails` and `fallback` of test_gpu_compact_checks, `spread` of test_gpu_compact_grid and the
(1998,1512) code.  The families, weights and inputs are those of tests/compact_forms_cases.py; its inputs DECODE in part
(tests/test_compact_forms.py), so the compact plan's own syndrome has to report True and False.

Every case, at early_stop=False under LDPC_ENGINE_MODE=auto,
  * asserts through DecodeEngine.info()["resident_kernel"] (ldpc_debug_resident_kernel: the launcher's own selection) that the
    compact plan runs and which instantiation and flags;
  * equals the streaming engine bit for bit in bits, posterior, iterations, success and packed_bits;
  * equals the CPU oracle: bits, iterations, success exactly; the posterior within POST_TOL = 1e-5 relative to max(1, |ref|)
    for the floating-point forms and exactly for the RCQ forms (as test_gpu_parity requires);
  * has the per-edge check-to-variable messages of its last iteration (ldpc_debug_resident_c2v, CSR edge order) equal the
    streaming engine's: bitwise for the floating-point forms, as quantiser codes for RCQ (test_gpu_parity.assert_codes).

Default case list (the suite's time budget): every family at T = 10, B = 37 on the three small codes; the
(1998,1512) code with one family per instantiation at one batch size; T = 1 for every family on one code each; per
instantiation one decode at B = 1 and one capped at 8 of 10 iterations.  The last test of the matrix asserts that the cases
that ran reported every instantiation and flag variant of compact_forms_cases.COVERAGE.

Two behaviours that only show across decodes: a weight update that flips unit_alpha on a live engine, and a seeded property
test over random graphs that take the compact plan (LDPC_FUZZ_SEEDS widens it).
"""
import numpy as np
import pytest
import torch

import _native
import compact_forms_cases as cf
from test_gpu_compact_banks import assert_values_equal
from test_gpu_compact_grid import POST_TOL, assert_post, assert_same_as_stream
from test_gpu_parity import assert_codes

pytestmark = pytest.mark.gpu

assert POST_TOL == 1e-5


@pytest.fixture(autouse=True)
def inference_mode(monkeypatch):
    monkeypatch.setenv("LDPC_ENGINE_MODE", "auto")
    with torch.no_grad():
        yield


def kernel_of(eng):
    """(FORM, BPC, NL, unit_alpha, rcq_zero0, oms_alpha) of the fixed-T decode, which must run the compact plan"""
    info = eng.info()
    assert info["engine"] == "resident" and info["threads_per_workgroup"] == 512 and info["workgroups_per_cu"] >= 3
    assert info["compact_plan"] is not None
    k = info["resident_kernel"]["fixed_T"]
    assert k["plan"] == "compact" and k["G"] == 2 and not k["split"] and not k["alpha_in_lds"]
    assert k["ms"] == k["row_stride"] == 495
    return (k["form"], k["bpc"], k["nl"], k["unit_alpha"], k["rcq_zero0"], k["oms_alpha"])


def engine_of(dec, gpu_device):
    eng = dec._get_engine(gpu_device)
    eng.set_mode("auto")
    return eng


def rcq_codes(dec, vals, t_last):
    """quantiser codes of reconstructed values (1 - 2*sign) * tau[level] of iteration t_last - 1 (test_gpu_compact_banks)"""
    from rcq_decoder import _quantizer_schedule, _threshold_table
    tau = _threshold_table(dec.quantizers)[_quantizer_schedule(len(dec.quantizers), int(dec.max_iterations))[t_last - 1]]
    L = len(tau)
    assert len(np.unique(tau)) == L
    level = np.full(vals.shape, 255, np.int64)
    for k in range(L):
        level[np.abs(vals) == tau[k]] = k
    assert np.all(level != 255), "a resident C2V value is not a reconstruction level"
    return np.where(np.signbit(vals), L, 0) + level, L


def assert_c2v_equal(dec, eng, x, cap=None):
    """per-edge C2V of the last executed iteration: compact resident kernel == streaming engine"""
    kw = {"max_iters": cap} if cap else {}
    res, _, _ = eng.debug_resident_c2v(x, early_stop=False, **kw)
    eng.set_mode("stream")
    eng.decode(x, early_stop=False, **kw)
    ref = eng.debug_c2v(x.shape[0], **kw).cpu().numpy()
    eng.set_mode("auto")
    res = res.cpu().numpy()
    if eng.c2v_form == _native.C2V_RCQ:                          # the streaming engine keeps 1-byte codes
        got, L = rcq_codes(dec, res, cap or int(dec.max_iterations))
        assert_codes(got, ref, L)
    else:
        assert_values_equal(res, ref)


def assert_equals_oracle(res, want, rcq):
    ob, op, oi, os_ = want
    np.testing.assert_array_equal(res.bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(res.iterations.cpu().numpy(), oi)
    np.testing.assert_array_equal(res.success.cpu().numpy().astype(bool), os_)
    if rcq:
        np.testing.assert_array_equal(res.posterior.cpu().numpy(), op)
    else:
        assert_post(res.posterior.cpu().numpy(), op)


_decoders = {}         # (family, code, T) -> decoder: the B = 1 and capped cases decode on the engine of the full case
_ran = set()           # kernel tuples reported by the cases that ran


def decoder_of(family, codename, T):
    key = (family, codename, T)
    if key not in _decoders:
        _decoders[key] = cf.build_decoder(family, cf.make_code(codename, T), T, cf.seed_of("w", family, codename, T))[0]
    return _decoders[key]


@pytest.mark.parametrize("case", cf.default_cases(), ids=cf.case_id)
def test_form_matrix(case, gpu_device, oracle_mod):
    fam = cf.FAMILIES[case.family]
    dec = decoder_of(case.family, case.code, case.T)
    eng = engine_of(dec, gpu_device)
    kernel = kernel_of(eng)
    assert kernel == fam.kernel
    _ran.add(kernel)
    _, llr = cf.case_inputs(case)
    x = torch.from_numpy(llr).to(gpu_device)
    kw = {"max_iters": case.cap} if case.cap else {}
    res = assert_same_as_stream(eng, x, **kw)
    assert_equals_oracle(res, cf.expected(oracle_mod, case), fam.kernel[0] == "RCQ")
    assert_c2v_equal(dec, eng, x, case.cap or None)


def test_form_matrix_ran_every_instantiation_and_flag():
    """(FORM, BPC, NL, unit_alpha, rcq_zero0, oms_alpha) as the launcher's selection reported them in the cases above, against
    the literal list compact_forms_cases.COVERAGE.  Reads what test_form_matrix recorded in this process: it needs the whole
    matrix to have run before it (the file in its own order, one process), and fails under -k or a reordering plugin."""
    assert sorted(_ran) == sorted(cf.COVERAGE)


@pytest.mark.parametrize("family", list(cf.FAMILIES))
def test_failure_confined_to_the_last_check_wave(family, gpu_device, oracle_mod):
    """inputs built so that a codeword's unsatisfied checks all sit in the last, partly filled check wave of `tails` (the
    host file asserts it from the oracle's bits), in a workgroup with a codeword that decodes: success must be False"""
    llr, want, confined = cf.last_wave_case(oracle_mod, family)
    assert len(confined) >= 1
    dec = decoder_of(family, cf.LAST_WAVE_CODE, cf.T_FULL)
    eng = engine_of(dec, gpu_device)
    assert kernel_of(eng) == cf.FAMILIES[family].kernel
    x = torch.from_numpy(llr).to(gpu_device)
    res = assert_same_as_stream(eng, x)
    assert not res.success.cpu().numpy().astype(bool)[confined].any()
    assert_equals_oracle(res, want, cf.FAMILIES[family].kernel[0] == "RCQ")
    assert_c2v_equal(dec, eng, x)


def test_resident_kernel_hook_with_a_live_decoder(gpu_device):
    """the error branches the host file cannot reach: NULL output, a decoder off the resident engine, a layered schedule"""
    from rcq_decoder import RCQMinSumDecoder
    eng = engine_of(decoder_of("n2d-4", "tails", cf.T_FULL), gpu_device)
    out = np.zeros(12, np.int32)
    assert eng._lib.ldpc_debug_resident_kernel(eng.handle, 0, None) == -1
    assert eng._lib.ldpc_debug_resident_kernel(eng.handle, 0, _native.ptr(out)) == 0 and out[0] == 2
    assert eng._lib.ldpc_debug_resident_kernel(eng.handle, 1, _native.ptr(out)) == 0 and out[0] != 2
    eng.set_mode("stream")
    assert eng._lib.ldpc_debug_resident_kernel(eng.handle, 0, _native.ptr(out)) == -3
    assert eng.info()["resident_kernel"] is None
    eng.set_mode("auto")
    lay = RCQMinSumDecoder(cf.make_code("fallback"), 3, 8, cf.QP3, cf.T_FULL, layered=True)._get_engine(gpu_device)
    lay.set_mode("auto")
    assert lay.info()["resident_kernel"] is None
    assert lay._lib.ldpc_debug_resident_kernel(lay.handle, 0, _native.ptr(out)) == -3


def test_per_lane_and_scalar_check_waves_both_run(gpu_device):
    """rcq_zero0 decides at plan time whether a wave is scalar-counted: the select form keeps the scalar waves of `tails`, a
    quantiser with tau_0 != 0 and a per-edge beta run every wave per lane"""
    scalar = {}
    for family in ("wrcq3-2", "rcq3-g0", "wrcq4-2", "wrcq4-2-g0", "wrcq3-1", "oms2d-2", "n2d-3", "n2d-1"):
        eng = engine_of(decoder_of(family, "tails", cf.T_FULL), gpu_device)
        scalar[family] = eng.info()["compact_plan"]["scalar_check_waves"]
    assert scalar == {"wrcq3-2": 5, "rcq3-g0": 0, "wrcq4-2": 5, "wrcq4-2-g0": 0, "wrcq3-1": 0, "oms2d-2": 0, "n2d-3": 5,
                      "n2d-1": 0}


# ---- a weight update flips unit_alpha on one engine --------------------------------------------------------------
@pytest.mark.parametrize("kind", ["neural2d", "wrcq"])
def test_weight_update_flips_unit_alpha(kind, gpu_device, oracle_mod):
    """sharing type 2 on `tails`: every alpha exactly 1.0 (variable-phase MODE 2), random alphas (MODE 0, alpha from global
    memory), every alpha 1.0 again -- each decode on the SAME engine equals the streaming engine and the oracle"""
    from neural_2d_decoder import Neural2DMinSumDecoder
    from rcq_decoder import WeightedRCQDecoder
    from test_gpu_parity import oracle_capped
    T = cf.T_FULL
    code = cf.make_code("tails", T)
    og = cf.oracle_graph(oracle_mod, code)
    rng = np.random.default_rng(cf.seed_of("flip", kind))
    dec = (Neural2DMinSumDecoder(code, weight_sharing_type=2, max_iterations=T) if kind == "neural2d" else
           WeightedRCQDecoder(code, 3, 8, cf.QP3, weight_sharing_type=2, max_iterations=T))
    llr = cf.llrs_mix(cf.seed_of("flip-llr", kind), cf.B_FULL, code.n, (3.0, 6.0))
    x = torch.from_numpy(llr).to(gpu_device)
    extra = dict(bc=3, qp=cf.QP3) if kind == "wrcq" else {}
    cf.fill(dec.beta_weights, rng, 0.5, 1.0)
    engines = set()
    for step, unit in enumerate((True, False, True)):
        if step == 2:                                            # the reference's checkpoint path
            sd = {k: (torch.ones_like(v) if k.startswith("alpha_weights.") else v) for k, v in dec.state_dict().items()}
            dec.load_state_dict(sd)
        elif unit:
            cf.fill(dec.alpha_weights, rng, 1.0, 1.0)
        else:
            cf.fill(dec.alpha_weights, rng, 0.8, 1.2)           # in-place fill_ (version counter)
        eng = engine_of(dec, gpu_device)
        engines.add(id(eng))
        kernel = kernel_of(eng)
        assert kernel[3] == unit, f"decode {step}: unit_alpha {kernel[3]}"
        res = assert_same_as_stream(eng, x)
        beta = {k: float(v.item()) for k, v in dec.beta_weights.items()}
        alpha = {k: float(v.item()) for k, v in dec.alpha_weights.items()}
        want = oracle_capped(oracle_mod, og, llr, kind, T, T, early_stop=False, wtype=2, beta=beta, alpha=alpha, **extra)
        assert 0 < int(want[3].sum()) < len(want[3])
        assert_equals_oracle(res, want, kind == "wrcq")
        assert_c2v_equal(dec, eng, x)
    assert len(engines) == 1, "the weight update built a new engine"


# ---- seeded property test -------------------------------------------------------------------------------------------------
_property = {"ran": 0, "skipped": 0}


@pytest.mark.parametrize("seed", cf.property_seeds())
def test_random_compact_graphs_agree_with_stream_and_oracle(seed, gpu_device, oracle_mod):
    """a random graph in the compact plan's range, a family of the matrix, T in 1..8, B in 1..70, the 3 / 5 dB mix: compact
    plan == streaming engine == oracle.  A graph the planner refuses is skipped (at most a third of the seeds, below)."""
    from test_compact_layout import layout
    _, cp, vi, n = cf.property_graph(seed)
    _property["ran"] += 1
    if layout(cp, vi, n)[0] != 0:
        _property["skipped"] += 1
        pytest.skip("the compact planner refuses this graph")
    code, family, T, B, llr = cf.property_case(seed)
    dec, wkw = cf.build_decoder(family, code, T, cf.seed_of("property-w", seed))
    eng = engine_of(dec, gpu_device)
    assert kernel_of(eng) == cf.FAMILIES[family].kernel
    x = torch.from_numpy(llr).to(gpu_device)
    res = assert_same_as_stream(eng, x)
    want = cf.oracle_run(oracle_mod, cf.oracle_graph(oracle_mod, code), family, wkw, llr, T, T)
    assert_equals_oracle(res, want, cf.FAMILIES[family].kernel[0] == "RCQ")


def test_property_skips_stay_under_the_cap():
    """counts what the property cases above recorded in this process (same caveat as the coverage test of the matrix)"""
    assert 3 * _property["skipped"] <= max(_property["ran"], len(cf.property_seeds()))
