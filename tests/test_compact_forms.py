"""
Host side (no GPU) of tests/test_gpu_compact_forms.py: properties of its case list that hold before any kernel runs.

* The inputs decode.  For every (family, code) case at T = 10 the CPU oracle alone reports success for at least 20 % and
  failure for at least 20 % of the 37 codewords, and at least one workgroup pair (codewords 2k, 2k + 1) finishes
  differently: the compact plan's syndrome (res_syndrome_slots) has to give both answers, and both inside one workgroup.
* One decode per family fails ONLY in the last, partly filled check wave of `tails` (inputs built for it): a syndrome that
  skipped that wave would call it a success.
* The case list names all eight compact instantiations and the flag variants the coverage test of the GPU file expects.
* The seeded property test's graphs mostly qualify for the compact plan: ldpc_debug_compact_layout(NULL, ...) refuses at most
  a third of the default seeds.
* ldpc_debug_resident_kernel rejects a NULL decoder without touching a device.
"""
import numpy as np
import pytest

import compact_forms_cases as cf

FULL_CASES = [c for c in cf.default_cases() if c.T == cf.T_FULL and c.B == cf.B_FULL and not c.cap]


@pytest.mark.parametrize("case", FULL_CASES, ids=cf.case_id)
def test_the_oracle_decodes_part_of_every_batch(case, oracle_mod):
    _, _, iters, success = cf.expected(oracle_mod, case)
    assert np.all(iters == case.T)
    ok, B = int(success.sum()), len(success)
    print(f"{cf.case_id(case)}: {ok} of {B} decode at {cf.snr_of(case.family, case.code)} dB")
    assert 5 * ok >= B and 5 * (B - ok) >= B
    pairs = success[0:B - 1:2] != success[1:B:2]
    assert pairs.any(), "no workgroup holds a codeword that decodes next to one that does not"


@pytest.mark.parametrize("family", list(cf.FAMILIES))
def test_a_decode_fails_in_the_last_check_wave_alone(family, oracle_mod):
    """from the oracle's bits: at least one codeword whose unsatisfied checks are all among the 20 checks of the last wave of
    `tails`, next to codewords that decode (the odd rows carry the all-zero codeword)"""
    llr, (bits, _, _, success), confined = cf.last_wave_case(oracle_mod, family)
    print(f"{family}: rows {confined.tolist()} fail in the last check wave alone")
    assert len(confined) >= 1 and not success[confined].any()
    assert success[1::2].all() and not bits[1::2].any()
    assert any(success[r ^ 1] for r in confined if (r ^ 1) < len(success)), "no such codeword shares a workgroup with a success"


def test_the_case_list_covers_every_instantiation_and_flag():
    cases = cf.default_cases()
    assert len(set(cases)) == len(cases)
    assert {f.kernel for f in cf.FAMILIES.values()} == set(cf.COVERAGE) and len(set(cf.COVERAGE)) == len(cf.COVERAGE)
    assert {k[:3] for k in cf.COVERAGE} == set(cf.INSTANTIATIONS) and len(cf.INSTANTIATIONS) == 8
    for inst, fam in cf.INSTANTIATIONS.items():
        assert cf.FAMILIES[fam].kernel[:3] == inst
        mine = [c for c in cases if c.family == fam]
        assert any(c.B == 1 for c in mine) and any(c.cap and c.cap < c.T for c in mine) and any(c.code == "ira" for c in mine)
    for fam in cf.FAMILIES:
        mine = [c for c in cases if c.family == fam]
        assert {c.code for c in mine if c.T == cf.T_FULL and c.B == cf.B_FULL and not c.cap} >= set(cf.SMALL_CODES)
        assert any(c.T == 1 for c in mine)
    flags = lambda form, i: {k[i] for k in cf.COVERAGE if k[0] == form}
    assert flags("NMS", 3) == {True, False} and flags("RCQ", 3) == {True, False}          # unit_alpha
    assert {k[4] for k in cf.COVERAGE if k[0] == "RCQ" and k[2] == 4} == {True, False}    # rcq_zero0, 4 levels
    assert {k[4] for k in cf.COVERAGE if k[0] == "RCQ" and k[2] == 0} == {True, False}    # rcq_zero0, run-time levels
    assert flags("OMS", 5) == {True, False}                                               # oms_alpha


def test_capped_and_final_iterations_run_a_quantiser_with_distinct_levels():
    """the GPU file reads the per-edge codes of an RCQ decode back from the reconstructed values of its last iteration"""
    from rcq_decoder import NonUniformQuantizer, _quantizer_schedule, _threshold_table
    for c in cf.default_cases():
        f = cf.FAMILIES[c.family]
        if f.qp is None:
            continue
        thr = _threshold_table([NonUniformQuantizer(f.bc, C, g) for C, g in f.qp])
        tau = thr[_quantizer_schedule(len(f.qp), c.T)[(c.cap or c.T) - 1]]
        assert len(np.unique(tau)) == len(tau), cf.case_id(c)


def _one_beta_slot_per_check(family, code):
    """what the plan derives from the decoder's beta_slot table (csrc/ldpc_plan.h, resident_layout: per_check)"""
    from weight_sharing import SharingLayout
    g = code.tanner_graph()
    f = cf.FAMILIES[family]
    if f.kind in ("edge", "edge-offset"):
        slot = np.arange(g.E)
    elif f.kind == "rcq":
        slot = np.zeros(g.E, np.int64)
    else:
        slot = SharingLayout(g, f.arg).beta_slot
    first = np.repeat(slot[np.minimum(g.check_ptr[:-1], max(g.E - 1, 0))], np.diff(g.check_ptr))
    return bool(np.all(slot == first))


def test_the_codes_give_every_family_the_beta_slots_its_instantiation_needs():
    """BPC follows from the graph as well as from the sharing type (type 1 on a graph of one variable degree has one slot per
    check): the matrix codes and the property graphs give every family the instantiation its row of the table names"""
    pairs = {(c.family, c.code, c.T) for c in cf.default_cases()}
    for family, codename, T in sorted(pairs):
        assert _one_beta_slot_per_check(family, cf.make_code(codename, T)) == cf.FAMILIES[family].kernel[1], (family, codename)
    for seed in cf.property_seeds():
        code, family, _, _, _ = cf.property_case(seed)
        assert _one_beta_slot_per_check(family, code) == cf.FAMILIES[family].kernel[1], (family, seed)


def test_the_property_graphs_mostly_qualify():
    from test_compact_layout import layout
    seeds = cf.property_seeds()
    refused = 0
    for seed in seeds:
        _, cp, vi, n = cf.property_graph(seed)
        refused += layout(cp, vi, n)[0] != 0
    print(f"{refused} of {len(seeds)} property graphs refused by the compact planner")
    assert 3 * refused <= len(seeds)


def test_property_graphs_span_several_waves_and_rounds():
    sizes = [cf.property_graph(seed)[0].shape for seed in cf.property_seeds()]
    assert any(m > 128 for m, n in sizes) and any(n > 1024 for m, n in sizes)      # > 2 check waves, > 2 variable rounds
    assert all(m <= 495 and n <= 2048 for m, n in sizes)


def test_resident_kernel_hook_rejects_bad_arguments():
    import _native
    lib = _native.load()
    out = np.zeros(12, np.int32)
    assert lib.ldpc_debug_resident_kernel(None, 0, _native.ptr(out)) == -1        # LDPC_ERR_ARG (_native.check)
    assert lib.ldpc_debug_resident_kernel(None, 0, None) == -1
    assert not out.any()
    # with a live decoder (NULL output, a decoder off the resident engine, a layered schedule): tests/test_gpu_compact_forms.py
