"""
GPU tests (-m gpu) of every RCQ kernel form at the quantiser widths no other test reaches: 2, 32, 64 and 128 levels through
RCQMinSumDecoder / WeightedRCQDecoder (bc 2, 6, 7, 8) and 1, 9, 62, 63, 127 and 128 levels on engines built directly.  A code is
one byte, (w < 0) * L + level: at L = 128 the negative codes use bit 7 and the saturated negative code is 255.  The cases,
weights and inputs are those of tests/quantiser_width_cases.py; tests/test_quantiser_widths.py holds, on the oracle alone,
that part of every batch decodes, both signs of the top level occur and at least 95 % of the code values are written.

Every flooding case runs with early stop on and off in every engine form that admits its decoder -- resident, sweeps, gather,
code pair, and whatever `stream` picks, which must be the form include/ldpc_hip.h promises -- and must equal the CPU oracle
exactly: bits, posterior, iterations, success and the per-edge codes of every codeword's last executed iteration.  The
code-pair form must be refused above 62 levels and for a per-edge beta.  The layered decoders run on the LDS and the streaming
kernel against oracle.rcq_layered and the restatement of tests/test_gpu_layered_weighted.py.
"""
import numpy as np
import pytest
import torch

import _native as nat
import quantiser_width_cases as qw
from test_gpu_parity import assert_codes

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def inference_mode(monkeypatch):
    monkeypatch.setenv("LDPC_ENGINE_MODE", "auto")
    with torch.no_grad():
        yield


def codes_of_values(vals, tau):
    """quantiser codes of the resident engine's reconstructed values (1 - 2*sign) * tau[level]; tau strictly increasing"""
    L = len(tau)
    assert L == 1 or np.all(np.diff(tau) > 0)
    level = np.minimum(np.searchsorted(tau, np.abs(vals)), L - 1)
    assert np.array_equal(tau[level], np.abs(vals)), "a resident C2V value is not a reconstruction level"
    return np.where(np.signbit(vals), L, 0) + level


def last_codes(eng, x, early_stop, thr, q_of_iter):
    """per-edge codes [B, E] of every codeword's last executed iteration, from the engine form that is set: the streaming
    forms keep the bytes in HBM (state of the decode that just ran), the resident kernel's values are mapped back"""
    if eng.info()["engine"] == "stream":
        return eng.debug_c2v(x.shape[0]).cpu().numpy()
    vals, _, iters = eng.debug_resident_c2v(x, early_stop=early_stop)
    vals, iters = vals.cpu().numpy(), iters.cpu().numpy()
    out = np.empty(vals.shape, np.int64)
    for q in np.unique(q_of_iter):
        rows = np.flatnonzero(q_of_iter[iters - 1] == q)
        out[rows] = codes_of_values(vals[rows], thr[q])
    return out


def modes_of(c, resident=True):
    """(mode, stream form it must report or None for the resident engine) for every form that admits the case's decoder"""
    modes = [("sweeps", "two-sweeps")]
    if resident:
        modes += [("resident", None), ("gather", "fused-rcq-iteration")]
    if qw.pair_admitted(c):
        modes.append(("pair", "rcq-code-pair"))
    if resident:          # what `stream` takes by the header: the code-pair form when admitted, else the fused gather iteration
        modes.append(("stream", "rcq-code-pair" if qw.pair_admitted(c) else "fused-rcq-iteration"))
    return modes


def run_case(eng, c, oracle_mod, early_stop, thr, q_of_iter, resident=True):
    L = qw.n_levels(c)
    llr = qw.case_inputs(c)
    ob, op, oi, os_, oc = qw.expected(oracle_mod, c, early_stop)
    ran = []
    for mode, form in modes_of(c, resident):
        eng.set_mode(mode)
        info = eng.info()
        assert info["stream_form"] == form and info["engine"] == ("stream" if form else "resident"), (mode, info)
        ran.append(info["kernel"])
        for r0 in range(0, c.B, c.chunk):
            x = torch.from_numpy(llr[r0:r0 + c.chunk]).to(eng.device)
            res = eng.decode(x, early_stop=early_stop)
            what = f"{qw.case_id(c)} {mode} rows {r0}.. early_stop={early_stop}"
            got = last_codes(eng, x, early_stop, thr, q_of_iter)
            sl = slice(r0, r0 + c.chunk)
            np.testing.assert_array_equal(res.iterations.cpu().numpy(), oi[sl], err_msg=what)
            np.testing.assert_array_equal(res.success.cpu().numpy(), os_[sl], err_msg=what)
            np.testing.assert_array_equal(res.bits.cpu().numpy(), ob[sl], err_msg=what)
            np.testing.assert_array_equal(res.posterior.cpu().numpy(), op[sl], err_msg=what)
            assert_codes(got, oc[sl], L)
    if not qw.pair_admitted(c):
        with pytest.raises(NotImplementedError):
            eng.set_mode("pair")
    print(f"{qw.case_id(c)} early_stop={early_stop}: ran {sorted(set(ran))}")
    return ran


# ---------------------------------------------------------------------------------------------------- through the classes
@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("case", qw.flood_cases(), ids=qw.case_id)
def test_classes_every_form_vs_oracle(case, early_stop, gpu_device, oracle_mod):
    from rcq_decoder import _quantizer_schedule, _threshold_table
    dec, _, T = qw.build_flood(case)
    eng = dec._get_engine(gpu_device)
    thr, qoi = _threshold_table(dec.quantizers), _quantizer_schedule(len(dec.quantizers), T)
    assert thr.shape == (3, 2 ** (case.bc - 1))
    ran = run_case(eng, case, oracle_mod, early_stop, thr, qoi, resident=case.code == "small")
    if case.code == "small":
        assert set(ran) == {"sweeps", "resident", "cn_gather"} | ({"code_pair"} if qw.pair_admitted(case) else set())
    else:                                       # dc > 32, dv > 8: neither the resident engine nor the gather form
        assert set(ran) == {"sweeps"} | ({"code_pair"} if qw.pair_admitted(case) else set())
        for mode in ("resident", "gather"):
            with pytest.raises(NotImplementedError):
                eng.set_mode(mode)


# ---------------------------------------------------------------------------------------------------- level counts of the C ABI
def level_engine(oracle_mod, c, gpu_device):
    from engine import DecodeEngine
    code, T, kw = qw.level_tables(oracle_mod, c)
    eng = DecodeEngine(code.tanner_graph(), dtype=torch.float32, c2v_form=nat.C2V_RCQ, iters=T, device=gpu_device, **kw)
    return eng, kw


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("case", qw.level_cases(), ids=qw.case_id)
def test_level_counts_every_form_vs_oracle(case, early_stop, gpu_device, oracle_mod):
    """1 level (all eight threshold registers of the dword kernels are padding; with tau = 1.5 level 0 reconstructs a non-zero
    value), 9 (the first count on the threshold loop), 62 and 63 (either side of the code-pair gate), 127 and 128"""
    eng, kw = level_engine(oracle_mod, case, gpu_device)
    ran = run_case(eng, case, oracle_mod, early_stop, kw["thresholds"], kw["q_of_iter"])
    assert ("code_pair" in ran) == (case.L <= 62)


def test_level_counts_outside_the_abi_are_refused(gpu_device, oracle_mod):
    """ldpc_decoder_create: n_levels 1..128; 0 and 129 return LDPC_ERR_UNSUPPORTED"""
    from engine import DecodeEngine
    code, T, kw = qw.level_tables(oracle_mod, qw.Level(9, 0.0, 40, 40))
    for L in (0, 129):
        kw["thresholds"] = np.zeros((3, L), np.float32)
        with pytest.raises(NotImplementedError, match="n_levels"):
            DecodeEngine(code.tanner_graph(), dtype=torch.float32, c2v_form=nat.C2V_RCQ, iters=T, device=gpu_device, **kw)


# ---------------------------------------------------------------------------------------------------- layered
@pytest.mark.parametrize("mode", ["auto", "stream"])
@pytest.mark.parametrize("case", qw.layered_cases(), ids=qw.case_id)
def test_layered_widths_vs_reference(case, mode, gpu_device, oracle_mod):
    """RCQMinSumDecoder(layered=True / "paper") and WeightedRCQDecoder(layered="paper") at 2, 32 and 128 levels on the LDS
    kernel (auto) and the streaming kernel: early stop equals the reference exactly; a fixed-T decode equals the weighted
    restatement exactly, and for the unweighted decoders -- whose oracle has no fixed-T form -- on the rows that never stop"""
    llr, ob, op, oi, os_, fixed, _ = qw.layered_expected(oracle_mod, case)
    dec, _, T = qw.build_flood(case, layered=True if case.dec == "ref" else "paper")
    eng = dec._get_engine(gpu_device)
    eng.set_mode(mode)
    lds, stream = {"ref": ("layered_lds", "layered_rcq<ref>")}.get(case.dec, ("layered_paper_lds", "layered_rcq<paper>"))
    assert eng.info()["kernel"] == (lds if mode == "auto" else stream)
    x = torch.from_numpy(llr).to(gpu_device)
    res = eng.decode(x, early_stop=True)
    np.testing.assert_array_equal(res.iterations.cpu().numpy(), oi)
    np.testing.assert_array_equal(res.success.cpu().numpy(), os_)
    np.testing.assert_array_equal(res.bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(res.posterior.cpu().numpy(), op)
    fix = eng.decode(x, early_stop=False)
    assert np.all(fix.iterations.cpu().numpy() == T)
    if fixed is not None:
        fb, fp, _, fs = fixed
        np.testing.assert_array_equal(fix.bits.cpu().numpy(), fb)
        np.testing.assert_array_equal(fix.posterior.cpu().numpy(), fp)
        np.testing.assert_array_equal(fix.success.cpu().numpy(), fs)
    else:
        keep = ~os_
        np.testing.assert_array_equal(fix.bits.cpu().numpy()[keep], ob[keep])
        np.testing.assert_array_equal(fix.posterior.cpu().numpy()[keep], op[keep])
        syn = dec.code.tanner_graph().syndrome(fix.bits.cpu().numpy()).any(axis=-1)
        np.testing.assert_array_equal(fix.success.cpu().numpy(), ~syn)
    print(f"{qw.case_id(case)} {mode}: ran {eng.info()['kernel']}")
