"""
The association order of the variable sums on the device (-m gpu).  DESIGN 4: sums follow ``np.sum`` (fp64) / ``torch.sum``
(fp32) order and posteriors are equal as values; tests/test_oracle.py pins the ORACLE's two orders bit for bit for
N = 0..575.  Here the kernels' restatements -- ``sum_ct`` up to eight operands, ``sum_rt`` above (csrc/ldpc_kernels.hip) -- are
held to the oracle on the two graphs of tests/fp64_cases.py, which carry one variable of every degree at which an order
changes block, up to the degrees the engine admits.  A tolerance cannot see the order (on these inputs the two differ by at
most 1.6e-15 resp. 3.4e-6 relative and flip no bit: tests/test_fp64_cases_host.py), so the posterior is compared with
``np.array_equal``, and a failure names the degrees of the variables that differ: at T = 1 a posterior depends on its own sum
only, T = 3 puts the leave-one-out sums on the path.
"""
import numpy as np
import pytest
import torch

import fp64_cases as fc

pytestmark = pytest.mark.gpu

TORCH = {fc.F64: torch.float64, fc.F32: torch.float32}
RUNS = [(T, fc.SUM_BATCH) for T in fc.SUM_T] + [(1, None)]          # None: the graph's wide batch
CASES = [(n, d, T, b) for n in sorted(fc.SUM_GRAPHS) for d in fc.SUM_DECODERS[n] for T, b in RUNS]


def make_engine(oracle_mod, graph, dtype, form, t, T, device):
    import _native as nat
    from engine import DecodeEngine
    kw = dict(oms_alpha=t.oms_alpha, oms_alpha_slot=t.oms_alpha_slot) if form == "oms" else {}
    return DecodeEngine(graph, dtype=TORCH[dtype], c2v_form=nat.C2V_OMS if form == "oms" else nat.C2V_NMS, iters=T,
                        beta=t.beta, beta_slot=t.beta_slot, alpha=t.alpha, alpha_slot=t.alpha_slot, device=device, **kw)


@pytest.mark.parametrize("name,decoder,T,batch", CASES,
                         ids=[f"{n}-{d}-T{T}-B{b or fc.SUM_WIDE_BATCH[n]}" for n, d, T, b in CASES])
def test_variable_sums_follow_the_reference_order(name, decoder, T, batch, gpu_device, oracle_mod):
    dtype = fc.SUM_GRAPHS[name][0]
    batch = batch or fc.SUM_WIDE_BATCH[name]
    graph = fc.sum_graph(name)
    eng = make_engine(oracle_mod, graph, dtype, decoder[:3], fc.sum_tables(oracle_mod, name, decoder, T), T, gpu_device)
    with pytest.raises(NotImplementedError):                       # dv > 8: no LDS-resident plan
        eng.set_mode("resident")
    want = fc.sum_expected(oracle_mod, name, decoder, T, batch=batch)
    x = torch.from_numpy(fc.sum_llrs(name, batch).copy()).to(gpu_device)        # the shared array is read-only
    vec = 1 if batch <= 64 else 2 if dtype is fc.F64 else 4
    for mode in ("auto", "sweeps") if dtype is fc.F32 else ("auto",):
        eng.set_mode(mode)
        info = eng.info()
        assert info["engine"] == "stream" and info["stream_form"] == "two-sweeps", info
        assert eng.boundary_kernels(batch)["vec"] == vec
        res = eng.decode(x, early_stop=False)
        got = res.posterior.cpu().numpy()
        assert got.dtype == dtype and np.isfinite(got).all()
        what = f"{name} {decoder} T={T} B={batch} mode={mode}"
        if not np.array_equal(got, want.posterior):
            rel = np.abs(got.astype(np.float64) - want.posterior) / np.maximum(1.0, np.abs(want.posterior))
            raise AssertionError(f"{what}: the posterior differs from the oracle's at the variables of degree "
                                 f"{fc.differing_degrees(name, got, want.posterior)}; largest relative difference {rel.max():.3e}")
        np.testing.assert_array_equal(res.bits.cpu().numpy(), want.bits, err_msg=what)
        assert bool((res.iterations == T).all()), what
        np.testing.assert_array_equal(res.success.cpu().numpy(), want.success, err_msg=what)


def test_degrees_past_the_restated_orders_are_refused(gpu_device, oracle_mod):
    """np.sum's pairwise recursion starts above 128 operands and torch.sum's cascade above 575: the engine restates neither
    and refuses the graph for that arithmetic when the decoder is created (no decode runs here)"""
    def create(graph, dtype):
        og = fc.oracle_graph(oracle_mod, graph)
        t = fc.draw_tables(oracle_mod, og, "nms", None, 1, 5)
        return make_engine(oracle_mod, graph, dtype, "nms", t, 1, gpu_device)

    g129, g576 = fc.refused_graph(129), fc.refused_graph(576)
    with pytest.raises(NotImplementedError, match=r"variable degree 129 > 128 \(fp64 sum order\)"):
        create(g129, fc.F64)
    assert create(g129, fc.F32).info()["engine"] == "stream"
    with pytest.raises(NotImplementedError, match=r"variable degree 576 > 575 \(fp32 sum order\)"):
        create(g576, fc.F32)
    with pytest.raises(NotImplementedError, match=r"variable degree 576 > 128 \(fp64 sum order\)"):
        create(g576, fc.F64)
    for name in sorted(fc.SUM_GRAPHS):                                # the limits themselves are admitted (and decoded above)
        assert fc.sum_graph(name).max_dv == (128 if name == "f64" else 575)
