"""
The fp64 engine with weight tables (-m gpu): ``DecodeEngine(dtype=torch.float64)`` built directly on NMS / OMS descriptors with
many beta slots, per-variable alpha slots and a check-side alpha table -- what ``ldpc_decoder_create`` accepts and the decoder
classes never build (they hand fp64 beta = 0.7 in one slot and alpha = 1).  Cases, seeded float64 tables, inputs and the
oracle's expectations are those of tests/fp64_cases.py; tests/test_fp64_cases_host.py holds the conditions on them.

Every decode is compared with ``oracle.decode`` in float64 / SUM_NUMPY: bits, iterations and success exactly, the packed bits
against the bits, and the posterior EQUAL AS VALUES (``np.array_equal``).  Where a case runs on both engines the
LDS-resident and the streaming results are bit-identical in all five outputs.  ``info()`` says which engine and which
``resident_decode`` instantiation ran.
"""
import numpy as np
import pytest
import torch

import fp64_cases as fc

pytestmark = pytest.mark.gpu

STOPS = (True, False)


# ---- engines --------------------------------------------------------------------------------------------------------------
def build_engine(oracle_mod, case, device, **override):
    import _native as nat
    from engine import DecodeEngine
    t = fc.tables(oracle_mod, case)
    kw = dict(dtype=torch.float64, c2v_form=nat.C2V_OMS if case.form == "oms" else nat.C2V_NMS, iters=fc.T_of(case.code),
              beta=t.beta, beta_slot=t.beta_slot, alpha=t.alpha, alpha_slot=t.alpha_slot, device=device)
    if case.form == "oms":
        kw.update(oms_alpha=t.oms_alpha, oms_alpha_slot=t.oms_alpha_slot)
    kw.update(override)
    return DecodeEngine(fc.load_code(case.code).tanner_graph(), **kw)


_engines = {}


def engine(oracle_mod, case, device, mode):
    """the case's engine (one per case and process) in `mode`"""
    if case not in _engines:
        if case.form == "basic":
            from ldpc_decoder import BasicMinSumDecoder
            dec = BasicMinSumDecoder(fc.load_code(case.code), 0.7)
            _engines[case] = (dec, dec._engine(torch.float64, device))
        else:
            _engines[case] = (None, build_engine(oracle_mod, case, device))
    return _engines[case][1].set_mode(mode)


def resident_cases():
    return fc.NMS_RESIDENT + fc.BASIC


def modes_of(case):
    """(mode, engine info() must report; None: whichever the planner chose)"""
    if case == fc.WIDE:
        return [("auto", None), ("stream", "stream")]
    if case in resident_cases():
        return [("auto", "resident"), ("stream", "stream")]
    return [("auto", "stream"), ("stream", "stream")]


def assert_form(eng, case, want_engine):
    """the engine that runs, and for a resident decode the instantiation the launcher selects in both stop modes"""
    info = eng.info()
    assert info["form"] == ("OMS" if case.form == "oms" else "NMS")
    if want_engine is not None:
        assert info["engine"] == want_engine, info
    if info["engine"] == "stream":
        assert info["stream_form"] == "two-sweeps" and info["resident_kernel"] is None
        return "stream"
    assert case.form != "oms" and case.wtype != 1            # the planner takes fp64 NMS with one beta per check only
    assert info["codewords_per_workgroup"] == 1
    for stop, k in info["resident_kernel"].items():
        what = (fc.case_id(case), stop, k)
        assert k["unit_alpha"] == (case.form == "basic"), what
        assert k["alpha_in_lds"] is False and k["form"] == "NMS" and k["bpc"] is True and k["G"] == 1, what
        assert k["oms_alpha"] is False and k["nl"] == 0, what
        if case.code in fc.PLAIN:
            assert k["plan"] == ("register-state" if stop == "fixed_T" else "general") and k["split"] is False, what
        else:
            assert k["split"] is True and k["plan"] == "general", what   # split checks keep the streaming variable loop
    return "resident"


# ---- comparison -----------------------------------------------------------------------------------------------------------
def assert_decode(res, want, what):
    bits = res.bits.cpu().numpy()
    np.testing.assert_array_equal(res.iterations.cpu().numpy(), want.iterations, err_msg=what)
    np.testing.assert_array_equal(res.success.cpu().numpy(), want.success, err_msg=what)
    np.testing.assert_array_equal(bits, want.bits, err_msg=what)
    unpacked = np.unpackbits(res.packed_bits.cpu().numpy(), axis=1, bitorder="little")[:, :bits.shape[1]]
    np.testing.assert_array_equal(unpacked, bits, err_msg=what + ": packed bits")
    got = res.posterior.cpu().numpy()
    assert got.dtype == np.float64 and np.isfinite(got).all(), what
    if not np.array_equal(got, want.posterior):
        bad = got != want.posterior
        rel = np.abs(got - want.posterior)[bad] / np.maximum(1.0, np.abs(want.posterior[bad]))
        raise AssertionError(f"{what}: posterior differs as a value at {int(bad.sum())} of {bad.size} entries, "
                             f"{int(bad.any(axis=1).sum())} of {len(bad)} codewords; largest relative difference {rel.max():.3e}")


def assert_identical(a, b, what):
    """two engines' results, bit for bit in all five outputs"""
    assert torch.equal(a.bits, b.bits) and torch.equal(a.packed_bits, b.packed_bits), what
    assert torch.equal(a.iterations, b.iterations) and torch.equal(a.success, b.success), what
    assert torch.equal(a.posterior.view(torch.int64), b.posterior.view(torch.int64)), what


def run_case(oracle_mod, device, case, batch=fc.B, caps=(None,)):
    x = torch.from_numpy(fc.llrs(case.code, batch).copy()).to(device)        # the shared array is read-only
    ran, results = [], {}
    for mode, want_engine in modes_of(case):
        eng = engine(oracle_mod, case, device, mode)
        form = assert_form(eng, case, want_engine)
        if form in ran:                                        # 'auto' of a streaming-only case: the same kernels as 'stream'
            continue
        ran.append(form)
        for early in STOPS:
            for cap in caps:
                want = fc.expected(oracle_mod, case, early_stop=early, cap=cap, batch=batch)
                what = f"{fc.case_id(case)} B={batch} {form} early_stop={early} max_iters={cap}"
                res = eng.decode(x, early_stop=early, want_packed=True, max_iters=cap)
                assert_decode(res, want, what)
                results.setdefault((early, cap), {})[form] = res
                if early:
                    # decisions only: the resident kernel then takes the stop rule from its variable phase (the mode that
                    # reads alpha while it forms the hard decisions)
                    hard = eng.decode(x, early_stop=True, want_posterior=False, want_packed=True, max_iters=cap)
                    assert hard.posterior is None
                    np.testing.assert_array_equal(hard.bits.cpu().numpy(), want.bits, err_msg=what + " (no posterior)")
                    np.testing.assert_array_equal(hard.iterations.cpu().numpy(), want.iterations, err_msg=what + " (no posterior)")
                    np.testing.assert_array_equal(hard.success.cpu().numpy(), want.success, err_msg=what + " (no posterior)")
                    assert torch.equal(hard.packed_bits, res.packed_bits), what + " (no posterior)"
    for key, by_form in results.items():
        if len(by_form) == 2:
            assert_identical(by_form["resident"], by_form["stream"], f"{fc.case_id(case)} B={batch} {key}: resident vs stream")
    return ran


# ---- decodes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.WEIGHTED, ids=fc.case_id)
def test_weighted_fp64_decode_equals_the_oracle(case, gpu_device, oracle_mod):
    """every sharing type of the normalised form, the offset form with its check-side alpha and the wide-check code at batch
    37, both stop modes, on every engine the case has"""
    ran = run_case(oracle_mod, gpu_device, case)
    if case in fc.NMS_RESIDENT:
        assert ran == ["resident", "stream"]
    elif case != fc.WIDE:
        assert ran == ["stream"]
    assert "stream" in ran


@pytest.mark.parametrize("case", fc.BASIC, ids=fc.case_id)
def test_basic_fp64_posterior_equals_the_oracle_as_values(case, gpu_device, oracle_mod):
    """BasicMinSumDecoder's own fp64 engine (beta = 0.7, alpha = 1: the unit_alpha shortcut) -- its posterior too is equal as
    values, on both engines and in both stop modes"""
    assert run_case(oracle_mod, gpu_device, case) == ["resident", "stream"]


@pytest.mark.parametrize("batch", fc.TILE_BATCHES)
@pytest.mark.parametrize("case", fc.TILE_CASES, ids=fc.case_id)
def test_tile_edges_of_the_fp64_layout(case, batch, gpu_device, oracle_mod):
    """64-codeword tiles up to batch 64, 128-codeword tiles (two codewords per lane) above: one row, a full tile, one row
    past it, and the same around 128"""
    eng = engine(oracle_mod, case, gpu_device, "stream")
    assert eng.boundary_kernels(batch)["vec"] == (1 if batch <= 64 else 2)
    run_case(oracle_mod, gpu_device, case, batch=batch)


def test_capped_decodes_read_each_iterations_table_row(gpu_device, oracle_mod):
    """max_iters 1, 2 and T - 1 on the (1998,1512) code with type-2 tables: the oracle run for that many iterations with the
    T-row tables -- the beta / alpha row of each iteration in double, on both engines (the resident fixed-T kernel then loops
    fewer times than the decoder's T)"""
    case = fc.CAP_CASE
    assert run_case(oracle_mod, gpu_device, case, caps=fc.caps(case)) == ["resident", "stream"]


# ---- weight updates ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.SET_WEIGHTS_CASES, ids=fc.case_id)
def test_set_weights_on_an_fp64_engine(case, gpu_device, oracle_mod):
    """ldpc_decoder_set_weights with double tables on a live engine: non-unit tables, alpha = 1 (the resident kernel's
    unit_alpha shortcut switches on), the first tables again (and off), then another draw of every table; each decode equals
    the oracle under the tables in force and the third equals the first bit for bit"""
    resident = case.form == "nms"
    eng = build_engine(oracle_mod, case, gpu_device).set_mode("auto")
    assert eng.info()["engine"] == ("resident" if resident else "stream")
    x = torch.from_numpy(fc.llrs(case.code).copy()).to(gpu_device)
    t0, t1 = fc.tables(oracle_mod, case), fc.tables(oracle_mod, case, variant=1)

    def flags():
        return [k["unit_alpha"] for k in eng.info()["resident_kernel"].values()] if resident else None

    def decode(what, **expect):
        out = {}
        for early in STOPS:
            out[early] = eng.decode(x, early_stop=early, want_packed=True)
            assert_decode(out[early], fc.expected(oracle_mod, case, early_stop=early, **expect), f"{fc.case_id(case)} {what} early_stop={early}")
        return out

    assert flags() in (None, [False, False])
    first = decode("first tables")
    eng.set_weights(None, np.ones_like(t0.alpha))
    assert flags() in (None, [True, True])
    decode("alpha = 1", unit=True)
    eng.set_weights(None, t0.alpha)
    assert flags() in (None, [False, False])
    third = decode("first tables again")
    for early in STOPS:
        assert_identical(first[early], third[early], f"{fc.case_id(case)}: third decode vs first, early_stop={early}")
    eng.set_weights(t1.beta, t1.alpha, t1.oms_alpha)
    assert flags() in (None, [False, False])
    decode("second draw", variant=1)
    for a, b in zip(eng.current_tables(), (t1.beta, t1.alpha, t1.oms_alpha)):
        assert (a is None and b is None) or np.array_equal(a, b)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_what_an_fp64_engine_refuses(gpu_device, oracle_mod):
    import _native as nat
    for case in fc.NMS_STREAM_ONLY + fc.OMS:
        eng = engine(oracle_mod, case, gpu_device, "stream")
        with pytest.raises(NotImplementedError, match="does not qualify for the LDS-resident engine"):
            eng.set_mode("resident")
        assert eng.info()["engine"] == "stream"
    for case in (fc.NMS_RESIDENT[0], fc.OMS[0], fc.BASIC[0]):
        eng = engine(oracle_mod, case, gpu_device, "stream")
        with pytest.raises(NotImplementedError, match="fused RCQ iteration needs an fp32"):
            eng.set_mode("gather")
        with pytest.raises(NotImplementedError, match="code-pair form needs an fp32"):
            eng.set_mode("pair")
        assert eng.info()["engine"] == "stream"
    case = fc.NMS_RESIDENT[0]
    engine(oracle_mod, case, gpu_device, "resident")         # a qualifying case takes the forced mode
    T = fc.T_of(case.code)
    thr = np.asarray([oracle_mod.quantizer_thresholds(3, 5.0, 1.3)], dtype=np.float32)
    with pytest.raises(NotImplementedError, match="RCQ messages are fp32 only"):
        build_engine(oracle_mod, case, gpu_device, c2v_form=nat.C2V_RCQ, thresholds=thr, q_of_iter=np.zeros(T, np.int32))
    for schedule in (nat.SCHED_LAYERED, nat.SCHED_LAYERED_REF):
        with pytest.raises(NotImplementedError, match="layered schedule is fp32 only"):
            build_engine(oracle_mod, case, gpu_device, schedule=schedule)
