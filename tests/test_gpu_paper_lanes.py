"""
layered_paper_lds<LW, NL, ES, WB> (csrc/ldpc_layered.hip) at every lane width (-m gpu): RCQMinSumDecoder(layered="paper") and
WeightedRCQDecoder(layered="paper") on the cases of tests/paper_lane_cases.py -- a graph per lane width 1..64 with a check
that fills the row, a degree-1 and a degree-0 check; 4, 8 and 16 levels and a quantiser whose level 0 is not zero at lane
widths 8 and 64; and a graph per outcome of the host's codewords-per-wave search (full wave, a count that is no power of two,
one codeword with shadow groups, the refusal).  Rows alternate between two SNRs, so the lane groups of a wave stop at
different iterations (tests/test_paper_lanes_host.py holds the conditions; they are asserted again here under the
codewords-per-wave count the engine reports).

Every comparison is ``np.array_equal``: against oracle.rcq_layered(paper=True) (plain) and the restatement of
tests/test_gpu_layered_weighted.py (weighted; at fixed T both), and between the LDS kernel and the streaming kernel
layered_rcq<VEC, true>.
"""
import numpy as np
import pytest
import torch

import paper_lane_cases as pc

pytestmark = pytest.mark.gpu

LDS, STREAM = "layered_paper_lds", "layered_rcq<paper>"


@pytest.fixture(autouse=True)
def inference_mode():
    with torch.no_grad():
        yield


def syndrome_ok(g, bits):
    """rows of ``bits`` that satisfy every check"""
    par = np.zeros(bits.shape[0], dtype=np.int64)
    for i in range(g.m):
        par |= bits[:, g.var_idx[g.check_ptr[i]:g.check_ptr[i + 1]]].sum(axis=1) & 1
    return par == 0


def fresh_engine(dec, device, mode, monkeypatch):
    monkeypatch.setenv("LDPC_ENGINE_MODE", mode)
    dec._engine = None                                          # a fresh engine reads the mode
    if hasattr(dec, "_engines"):
        dec._engines = {}
    from simulation_framework import _engine_of
    return _engine_of(dec, device)


def outputs(res, n):
    return (res.bits.cpu().numpy(), res.posterior.cpu().numpy(), res.iterations.cpu().numpy(),
            res.success.cpu().numpy().astype(bool),
            np.unpackbits(res.packed_bits.cpu().numpy(), axis=1, bitorder="little")[:, :n].astype(np.int32))


@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_paper_lds_kernel_vs_references_and_streaming_kernel(name, gpu_device, oracle_mod, monkeypatch):
    c, code = pc.BY_NAME[name], pc.code_of(name)
    g = code.tanner_graph()
    plain, weighted, _ = pc.decoders(name)
    llr = pc.inputs(name)
    for is_w, dec in ((False, plain), (True, weighted)):
        ref_es = pc.reference(oracle_mod, name, is_w, early_stop=True)
        ref_fx = pc.reference(oracle_mod, name, is_w, early_stop=False)
        open_ = ~ref_es[3]
        got = {}
        # batches of 1, cw + 1 and 3 cw - 1 rows and the whole pool, under the LDS kernel's own count for both kernels
        # (the refused geometry has no such count: 8)
        cw_auto = fresh_engine(dec, gpu_device, "auto", monkeypatch).info()["codewords_per_workgroup"]
        sizes = pc.batches(cw_auto if c.klass != pc.STREAM else 8)
        for mode in ("auto", "stream"):
            eng = fresh_engine(dec, gpu_device, mode, monkeypatch)
            info = eng.info()
            tag = f"{name} {'weighted' if is_w else 'plain'} {mode}"
            # ---- which kernel, and what the codewords-per-wave search gave it
            lds = mode == "auto" and c.klass != pc.STREAM
            assert info["kernel"] == (LDS if lds else STREAM), (tag, info)
            cw = info["codewords_per_workgroup"]
            if lds:
                assert info["lds_bytes"] == cw * pc.row_bytes(g.n, g.m, c.lw), (tag, info)
                assert info["workgroups_per_cu"] >= pc.MIN_WORKGROUPS, (tag, info)
                assert 1 <= cw <= 64 // c.lw, (tag, info)
                if c.kind == "geom":
                    assert pc.class_of(cw, c.lw) == c.klass, \
                        (f"{tag}: {cw} of {64 // c.lw} codewords per wave is not '{c.klass}': if the host's rule "
                         f"(build_layered_plan) changed, pick another (n, m, max dc) for this class", info)
                # the wave's lane groups stop at different iterations under THIS count too
                assert pc.degeneracy(name, ref_es[2], ref_es[3], cw) == [], (tag, cw)
            for B in sizes:
                x = torch.from_numpy(np.array(llr[:B])).to(gpu_device)     # a copy: the pool is read-only
                # ---- early stop: everything equals the reference
                bits, post, iters, succ, unpacked = outputs(eng.decode(x, early_stop=True, want_packed=True), g.n)
                np.testing.assert_array_equal(iters, ref_es[2][:B], err_msg=f"{tag} B={B} iterations")
                np.testing.assert_array_equal(succ, ref_es[3][:B], err_msg=f"{tag} B={B} success")
                np.testing.assert_array_equal(bits, ref_es[0][:B], err_msg=f"{tag} B={B} bits")
                np.testing.assert_array_equal(post, ref_es[1][:B], err_msg=f"{tag} B={B} posterior")
                np.testing.assert_array_equal(unpacked, ref_es[0][:B], err_msg=f"{tag} B={B} packed bits")
                got[(mode, B, True)] = (bits, post, iters, succ, unpacked)
                # ---- fixed T
                fbits, fpost, fiters, fsucc, funpacked = outputs(eng.decode(x, early_stop=False, want_packed=True), g.n)
                assert (fiters == pc.T).all(), f"{tag} B={B}"
                keep = open_[:B]                                 # rows the early-stop decode never froze: the same walk
                np.testing.assert_array_equal(fbits[keep], ref_es[0][:B][keep], err_msg=f"{tag} B={B} fixed-T open bits")
                np.testing.assert_array_equal(fpost[keep], ref_es[1][:B][keep], err_msg=f"{tag} B={B} fixed-T open posterior")
                np.testing.assert_array_equal(fsucc, syndrome_ok(g, fbits), err_msg=f"{tag} B={B} fixed-T success")
                np.testing.assert_array_equal(funpacked, fbits, err_msg=f"{tag} B={B} fixed-T packed bits")
                np.testing.assert_array_equal(fpost, ref_fx[1][:B], err_msg=f"{tag} B={B} fixed-T posterior")
                np.testing.assert_array_equal(fbits, ref_fx[0][:B], err_msg=f"{tag} B={B} fixed-T bits")
                np.testing.assert_array_equal(fsucc, ref_fx[3][:B], err_msg=f"{tag} B={B} fixed-T success vs reference")
                got[(mode, B, False)] = (fbits, fpost, fiters, fsucc, funpacked)
        # ---- the two kernels agree bit for bit in both stop modes
        for B in sizes:
            for es in (True, False):
                for a, s in zip(got[("auto", B, es)], got[("stream", B, es)]):
                    np.testing.assert_array_equal(a, s, err_msg=f"{name} B={B} es={es} auto vs stream")
