"""
Block-parallel layered decode (-m gpu): layered_block_lds (csrc/ldpc_layered_block.hip, LDPC_MODE_BLOCK /
LDPC_ENGINE_MODE=block) on graphs that declare layers -- quasi-cyclic codes, a ragged layer-ordered graph, the degenerate
one-check-per-layer partition, the layer-ordered (1998,1512) code and the committed (1944,972) QC code.

The checks of a layer share no variable and every step of the layered update is one rounded operation, so the kernel
must return, bit for bit, what the sequential walk over the same graph returns.  The yardsticks are the numpy
restatements (tests/layered_minsum_reference.py; the ``restate`` of tests/test_gpu_layered_weighted.py), and the existing
kernels on the same graph under ``resident`` and ``stream``.  Every comparison is ``np.array_equal`` on decisions, fp32
posteriors, iterations, success and the unpacked packed bits.  Inputs come from tests/block_layered_cases.py; the host
test shows that frozen rows sit beside live ones in every input set.
"""
import numpy as np
import pytest
import torch

import block_layered_cases as bc

pytestmark = pytest.mark.gpu

MODES = ("block", "resident", "stream", "auto")
BLOCK = "layered_block_lds"


@pytest.fixture(autouse=True)
def inference_mode():
    with torch.no_grad():
        yield


def engine_of(dec, device):
    from simulation_framework import _engine_of
    return _engine_of(dec, device)


def outputs(res, n):
    return (res.bits.cpu().numpy(), res.posterior.cpu().numpy(), res.iterations.cpu().numpy(), res.success.cpu().numpy(),
            np.unpackbits(res.packed_bits.cpu().numpy(), axis=1, bitorder="little")[:, :n])


def assert_equals(res, want, n, tag):
    bits, post, iters, succ, unpacked = outputs(res, n)
    np.testing.assert_array_equal(iters, want[2], err_msg=tag)
    np.testing.assert_array_equal(succ, want[3], err_msg=tag)
    np.testing.assert_array_equal(bits, want[0], err_msg=tag)
    np.testing.assert_array_equal(post, want[1], err_msg=tag)
    np.testing.assert_array_equal(unpacked, want[0], err_msg=tag)


def check(kind, name, form, device, *, T=bc.T, modes=MODES, stops=(True, False), max_iters=None, rows=None):
    """decode the input set of `name` under every mode and stop rule: everything equals the restatement (and so each other)"""
    dec = (bc.make_minsum if kind == "ms" else bc.make_rcq)(form, name, T)
    ref = bc.reference_minsum if kind == "ms" else bc.reference_rcq
    llr = bc.input_llr(name) if rows is None else bc.input_llr(name)[:rows]
    x = torch.from_numpy(np.array(llr)).to(device)
    eng = engine_of(dec, device)
    for mode in modes:
        try:
            eng.set_mode(mode)
        except NotImplementedError:
            # the sequential LDS kernels want four one-wave workgroups per CU: a code they leave to the streaming
            # walk has no `resident` form to compare with; every other mode must exist
            assert mode == "resident"
            continue
        info = eng.info()
        assert info["layers"] == bc.graph(name).n_layers
        if mode == "block":
            assert info["kernel"] == BLOCK and info["engine"] == "resident", info
            assert info["codewords_per_workgroup"] >= 1 and info["threads_per_workgroup"] % 64 == 0 and \
                0 < info["lds_bytes"] <= 160 * 1024, info
        elif mode == "stream":
            assert info["engine"] == "stream", info
        elif mode == "resident":
            assert info["kernel"] in ("layered_minsum_lds", "layered_paper_lds"), info
        else:       # auto: whatever it picked, info() is self-consistent
            assert (info["engine"] == "resident") == (info["lds_bytes"] > 0 and info["workgroups_per_cu"] >= 1), info
            assert (info["kernel"] == BLOCK) <= (info["engine"] == "resident"), info
        for es in stops:
            want = ref(name, form, T, early_stop=es, max_iters=max_iters, rows=rows)
            res = eng.decode(x, early_stop=es, want_packed=True, max_iters=max_iters)
            assert_equals(res, want, llr.shape[1], f"{name} {form} T={T} es={es} cap={max_iters} rows={rows} {mode}")
    return eng


# ---- every family and form on every small case graph -------------------------------------------------------------------------
@pytest.mark.parametrize("family", bc.FAMILIES)
@pytest.mark.parametrize("name", bc.SMALL_GRAPHS)
def test_minsum_families(name, family, gpu_device):
    """basic; per-degree betas with a zero and a negative slot; the offset form with a check-side alpha; per-edge offset"""
    check("ms", name, family, gpu_device)


@pytest.mark.parametrize("form", tuple(bc.RCQ_FORMS))
@pytest.mark.parametrize("name", bc.SMALL_GRAPHS)
def test_weighted_rcq_forms(name, form, gpu_device):
    """W-RCQ layered="paper" at sharing types 1 and 2 with 4, 8 and 16 levels, a gamma = 0 table, and beta == 1"""
    check("rcq", name, form, gpu_device)


@pytest.mark.parametrize("kind,form", [("ms", "basic"), ("ms", "n2d_oms"), ("rcq", "t2_l8")])
@pytest.mark.parametrize("name", ["ira_lo", "qc_1944"])
def test_full_size_codes(name, kind, form, gpu_device):
    """layered_order(ira_1998_1512), 128 rows, and qc_1944_972, 64 rows, T = 10"""
    check(kind, name, form, gpu_device)


# ---- iteration counts, caps, batches -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,form", [("ms", "n2d_oms"), ("ms", "n2d1"), ("rcq", "t1_l4")])
@pytest.mark.parametrize("name", ["qc_4_8_65", "ragged"])
def test_caps_and_short_decodes(name, kind, form, gpu_device):
    """max_iters 1 and 3 below T = 10 (iteration t keeps the tables of iteration t; an open codeword reports the cap and no
    success); T = 0 returns the LLRs, T = 1 runs no previous message"""
    for cap in (1, 3):
        check(kind, name, form, gpu_device, max_iters=cap, modes=("block", "stream"))
    for T in (0, 1):
        check(kind, name, form, gpu_device, T=T, modes=("block", "stream"))
    ref = bc.reference_minsum if kind == "ms" else bc.reference_rcq
    assert (ref(name, form, max_iters=3)[2] == 3).any()


@pytest.mark.parametrize("kind,form", [("ms", "n2d1"), ("rcq", "t2_l8")])
@pytest.mark.parametrize("name", ["qc_3_6_5", "qc_4_8_65", "qc_2_5_130", "ragged"])
def test_batches_that_leave_partly_filled_workgroups(name, kind, form, gpu_device):
    """batches of 1, G + 1, 3G - 1 (G codewords per workgroup, from info()) and the whole pool; pool rows repeat where a
    batch is larger than the pool"""
    dec = (bc.make_minsum if kind == "ms" else bc.make_rcq)(form, name)
    ref = bc.reference_minsum if kind == "ms" else bc.reference_rcq
    eng = engine_of(dec, gpu_device).set_mode("block")
    G = eng.info()["codewords_per_workgroup"]
    llr = bc.input_llr(name)
    pool = llr.shape[0]
    for B in (1, G + 1, 3 * G - 1, pool):
        idx = np.arange(B) % pool
        x = torch.from_numpy(np.ascontiguousarray(llr[idx])).to(gpu_device)
        for es in (True, False):
            want = tuple(a[idx] for a in ref(name, form, early_stop=es))
            assert_equals(eng.decode(x, early_stop=es, want_packed=True), want, llr.shape[1], f"{name} {form} B={B} G={G} es={es}")


def test_a_decode_does_not_depend_on_what_ran_before(gpu_device):
    name = "qc_4_8_64"
    eng = engine_of(bc.make_minsum("n2d_oms", name), gpu_device).set_mode("block")
    llr = bc.input_llr(name)
    x = torch.from_numpy(np.array(llr)).to(gpu_device)
    first = outputs(eng.decode(x, want_packed=True), llr.shape[1])
    other = torch.from_numpy(np.ascontiguousarray(-3.0 * llr[::-1][:29])).to(gpu_device)      # another batch, another size
    eng.decode(other, early_stop=False)
    again = outputs(eng.decode(x, want_packed=True), llr.shape[1])
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)
    assert_equals(eng.decode(x, want_packed=True), bc.reference_minsum(name, "n2d_oms"), llr.shape[1], "third")


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.GRAPHS)
def test_info_reports_the_planners_geometry(name, gpu_device):
    import _native as nat
    g = bc.graph(name)
    cp, vi, lp = (np.ascontiguousarray(a, dtype=np.int32) for a in (g.check_ptr, g.var_idx, g.layer_ptr))
    for kind, dec in ((0, bc.make_minsum("basic", name)), (1, bc.make_rcq("t2_l8", name))):
        out = np.zeros(8, dtype=np.int64)
        assert nat.load().ldpc_debug_layer_plan(g.n, g.m, g.E, nat.ptr(cp), nat.ptr(vi), len(lp) - 1, nat.ptr(lp), kind,
                                                nat.ptr(out)) == 0 and out[0] == 1
        info = engine_of(dec, gpu_device).set_mode("block").info()
        assert (info["codewords_per_workgroup"], info["threads_per_workgroup"], info["lds_bytes"]) == tuple(out[[1, 3, 4]]), info
        assert info["kernel"] == BLOCK and info["layers"] == g.n_layers


def test_engine_mode_block_from_the_environment(gpu_device, monkeypatch):
    monkeypatch.setenv("LDPC_ENGINE_MODE", "block")
    name = "qc_4_8_65"
    dec = bc.make_minsum("basic", name)
    eng = engine_of(dec, gpu_device)
    assert eng.info()["kernel"] == BLOCK
    x = torch.from_numpy(np.array(bc.input_llr(name))).to(gpu_device)
    assert_equals(eng.decode(x, want_packed=True), bc.reference_minsum(name, "basic"), x.shape[1], "env")
    bits, succ, iters = dec.decode(x)                                  # the host class returns the engine's result
    np.testing.assert_array_equal(bits.cpu().numpy(), bc.reference_minsum(name, "basic")[0])


# ---- weight and quantiser updates on a cached engine ----------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["n2d1", "n2d_oms"])
def test_weight_update_reaches_the_cached_engine_in_block_mode(family, gpu_device):
    """an optimiser-style in-place update of the parameters: same engine, new plan-ordered tables"""
    import layered_minsum_cases as ms
    import layered_minsum_reference as ref
    name = "qc_4_8_65"
    dec = bc.make_minsum(family, name)
    eng = engine_of(dec, gpu_device).set_mode("block")
    llr = bc.input_llr(name)
    x = torch.from_numpy(np.array(llr)).to(gpu_device)
    first = eng.decode(x)
    with torch.no_grad():
        for p in list(dec.beta_weights.values()) + list(getattr(dec, "alpha_weights", {}).values()):
            p.add_(-0.05 * torch.sign(p))                                # what an optimiser step does: p.data changes in place
    assert engine_of(dec, gpu_device) is eng and eng.info()["kernel"] == BLOCK
    beta_e, a_e = ms.edge_tables(dec, family, bc.T)
    want = ref.restate(bc.graph(name), llr, bc.T, ms.form_of(family), beta_e, a_e)
    res = eng.decode(x, want_packed=True)
    assert_equals(res, want, llr.shape[1], family)
    assert not torch.equal(first.posterior, res.posterior)


def test_set_quantizers_and_betas_reach_the_cached_engine_in_block_mode(gpu_device):
    import test_gpu_layered_weighted as wl
    name, form = "qc_4_8_64", "t2_l8"
    bcw, qp, _, _ = bc.RCQ_FORMS[form]
    dec = bc.make_rcq(form, name)
    eng = engine_of(dec, gpu_device).set_mode("block")
    llr = bc.input_llr(name)
    x = torch.from_numpy(np.array(llr)).to(gpu_device)
    first = eng.decode(x)
    with torch.no_grad():
        for p in dec.beta_weights.values():
            p.mul_(0.93)
    assert engine_of(dec, gpu_device) is eng
    qp2 = [(c * 1.25, g) for c, g in qp]
    eng.set_quantizers(wl.thresholds(bcw, qp2))
    assert eng.info()["kernel"] == BLOCK
    want = wl.restate(bc.code(name), llr, bcw, qp2, bc.T, bc.rcq_edge_betas(dec, bc.T))
    res = eng.decode(x, want_packed=True)
    assert_equals(res, want, llr.shape[1], "set_quantizers")
    assert not torch.equal(first.posterior, res.posterior)


# ---- training and the simulator ---------------------------------------------------------------------------------------------------------
def test_joint_training_forward_is_the_block_decode(gpu_device):
    """the training entry points keep their streaming one-iteration walk; on a layered graph their forward is the same
    decode: the posterior joint_posterior_loss returns is the block decode's at fixed T"""
    name = "qc_4_8_65"
    llr = bc.input_llr(name)
    x = torch.from_numpy(np.array(llr)).to(gpu_device)
    for family in ("n2d1", "n2d_oms"):
        dec = bc.make_minsum(family, name)
        with torch.enable_grad():
            loss, per_iter, bits, post = dec.joint_posterior_loss(x, layered_gradient="posterior_local")
        res = engine_of(dec, gpu_device).set_mode("block").decode(x, early_stop=False)
        np.testing.assert_array_equal(post.detach().cpu().numpy(), res.posterior.cpu().numpy(), err_msg=family)
        np.testing.assert_array_equal(bits.cpu().numpy(), res.bits.cpu().numpy(), err_msg=family)
        np.testing.assert_array_equal(res.posterior.cpu().numpy(), bc.reference_minsum(name, family, early_stop=False)[1])


def test_simulator_counters_equal_under_block_and_stream(gpu_device, monkeypatch, tmp_path):
    from simulation_framework import LDPSimulator, SimulationConfig
    name = "qc_4_8_64"
    got = {}
    for mode in ("block", "stream"):
        monkeypatch.setenv("LDPC_ENGINE_MODE", mode)
        dec = bc.make_minsum("basic", name)
        assert engine_of(dec, gpu_device).info()["kernel"] == (BLOCK if mode == "block" else "layered_minsum")
        cfg = SimulationConfig(max_frames=600, max_errors=40, batch_frames=256, seed=13, results_dir=str(tmp_path),
                               save_results=False)
        fer, ber, avg_it, _t, frames, errs = LDPSimulator(cfg).simulate_single_snr(dec, dec.code, 2.5, 600, 40)
        got[mode] = (fer, ber, avg_it, frames, errs)
    assert got["block"] == got["stream"] and got["block"][4] > 0


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_what_mode_block_refuses(gpu_device, monkeypatch):
    import _native as nat
    import codes
    import layered_minsum_cases as ms
    from engine import DecodeEngine
    monkeypatch.setenv("LDPC_ENGINE_MODE", "auto")
    plain = ms.make("basic", codes.load_code("small_96_48", 10), 10, 0)            # a layered decoder on a graph without layers
    eng = engine_of(plain, gpu_device)
    assert eng.info()["layers"] == 0
    with pytest.raises(NotImplementedError, match="no layers"):
        eng.set_mode("block")
    assert eng.info()["kernel"] == "layered_minsum_lds"                              # the refusal changed nothing
    g = bc.graph("qc_4_8_65")
    tables = dict(beta=np.full((10, 1), 0.7, np.float32), beta_slot=np.zeros(g.E, np.int32),
                  alpha=np.ones((10, 1), np.float32), alpha_slot=np.zeros(g.n, np.int32))
    flooding = DecodeEngine(g, dtype=torch.float32, c2v_form=nat.C2V_NMS, iters=10, device=gpu_device, **tables)
    assert flooding.info()["layers"] == 4
    with pytest.raises(NotImplementedError, match="LDPC_SCHED_LAYERED"):
        flooding.set_mode("block")
    f64 = DecodeEngine(g, dtype=torch.float64, c2v_form=nat.C2V_NMS, iters=10, device=gpu_device,
                       **{k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in tables.items()})
    with pytest.raises(NotImplementedError, match="fp32"):
        f64.set_mode("block")
    # a flooding decode on a graph that declares layers is the flooding decode of the bare graph
    x = torch.from_numpy(np.array(bc.input_llr("qc_4_8_65"))).to(gpu_device)
    from tanner_graph import TannerGraph
    bare = DecodeEngine(TannerGraph.from_csr(g.n, g.check_ptr, g.var_idx), dtype=torch.float32, c2v_form=nat.C2V_NMS, iters=10,
                        device=gpu_device, **tables)
    a, b = flooding.decode(x), bare.decode(x)
    assert torch.equal(a.posterior, b.posterior) and torch.equal(a.iterations, b.iterations)
    # the C ABI refuses a partition with a shared variable, naming the layer
    cp, vi = np.ascontiguousarray(g.check_ptr, np.int32), np.ascontiguousarray(g.var_idx, np.int32)
    bad = np.array([0, 66, 130, 195, 260], dtype=np.int32)
    import ctypes as C
    handle = C.c_void_p()
    rc = nat.load().ldpc_graph_create_layered(C.byref(handle), g.n, g.m, g.E, nat.ptr(cp), nat.ptr(vi), 4, nat.ptr(bad))
    assert rc == -1 and not handle.value and b"layer 0 " in nat.load().ldpc_last_error()
