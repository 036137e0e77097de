"""
A decode does not depend on where the caller's rows lie: the streaming engine picks the kernels that change layout at its two
ends from the row length and from the address of llr, posterior and bits (csrc/ldpc_hip.hip, boundary_kernels), and every
choice must give the same bytes.  tests/row_alignment_cases.py has the codes (4n mod 16 = 0, 8, and n odd), the families,
batches and placements; tests/test_row_alignment_host.py what the oracle does with them.

Every pointer sits at its own byte offset behind a 256-byte guard inside a buffer filled with 0xA5.  Each run is compared
with the CPU restatement of its family, as tests/test_gpu_dirty_state.py compares, bit for bit with the all-aligned run, and
ldpc_debug_boundary_kernels is asked first which kernels the run launches: the answer must be what the placement was built
for, and over the case list every family must take every width its engine can reach.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import row_alignment_cases as ra
from row_alignment_cases import ds
from test_gpu_dirty_state import GUARD, OUTPUTS, GuardedDecode, host, unpack
from test_gpu_parity import assert_post

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def inference_mode():
    with torch.no_grad():
        yield


class PlacedDecode(GuardedDecode):
    """ldpc_decode / ldpc_decode_capped / ldpc_decode_saving through the raw entry points with llr, posterior and bits each
    GUARD + its placement's offset bytes into a buffer of its own filled with 0xA5 (the other outputs at GUARD)"""

    def place(self, x, pl, packed=True):
        """-> the buffers of one run: the LLRs copied to their offset, every requested output's buffer poisoned"""
        eng, (B, n) = self.eng, x.shape
        es = x.element_size()
        self.shape, self.pl = (B, n), pl
        self.sizes = {"llr": B * n * es, "bits": B * n * 4, "posterior": B * n * es, "iterations": B * 4, "success": B,
                      "packed_bits": B * ((n + 7) // 8)}
        self.off = {"llr": pl.llr, "bits": pl.bits, "posterior": pl.posterior, "iterations": 0, "success": 0,
                    "packed_bits": 0 if packed else None}
        self.bufs = {k: torch.full((v + 2 * GUARD + ra.MAX_OFFSET,), 0xA5, dtype=torch.uint8, device=eng.device)
                     for k, v in self.sizes.items() if self.off[k] is not None}
        assert all(b.data_ptr() % 256 == 0 for b in self.bufs.values())
        lo = GUARD + pl.llr
        self.bufs["llr"][lo:lo + self.sizes["llr"]].view(x.dtype).copy_(x.reshape(-1))
        return self

    def addr(self, k):
        return self.bufs[k].data_ptr() + GUARD + self.off[k] if k in self.bufs else 0

    def kernels(self, cap=None, saving=False):
        """what ldpc_debug_boundary_kernels says this run launches"""
        k = self.eng.boundary_kernels(self.shape[0], llr=self.addr("llr"), posterior=self.addr("posterior"),
                                      bits=self.addr("bits"), max_iters=cap, saving=saving)
        return ra.Kernels(**k)

    def decode(self, early_stop, cap=None, saved=None):
        """-> {output: numpy array | None}; every byte of every buffer outside its body must still be 0xA5"""
        eng, (B, n) = self.eng, self.shape
        p = lambda k: C.c_void_p(self.addr(k)) if k in self.bufs else None
        outs = [p(k) for k in OUTPUTS]
        with torch.cuda.device(eng.device):
            stream = C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
            if saved is not None:
                ws = eng._train_workspace(B)
                rc, what = self.lib.ldpc_decode_saving(eng.handle, p("llr"), B, int(early_stop), *outs[:4], C.c_void_p(saved.data_ptr()),
                                                       saved.numel(), C.c_void_p(ws.data_ptr()), ws.numel(), stream), "ldpc_decode_saving"
            elif cap is None:
                ws = eng._workspace(B)
                rc, what = self.lib.ldpc_decode(eng.handle, p("llr"), B, int(early_stop), *outs, C.c_void_p(ws.data_ptr()),
                                                ws.numel(), stream), "ldpc_decode"
            else:
                ws = eng._workspace(B)
                rc, what = self.lib.ldpc_decode_capped(eng.handle, p("llr"), B, int(early_stop), int(cap), *outs,
                                                       C.c_void_p(ws.data_ptr()), ws.numel(), stream), "ldpc_decode_capped"
            self.nat.check(rc, what)
        out = dict.fromkeys(OUTPUTS)
        dtypes = {"llr": eng.np_dtype, "bits": np.int32, "posterior": eng.np_dtype, "iterations": np.int32, "success": np.uint8,
                  "packed_bits": np.uint8}
        for k, buf in self.bufs.items():
            raw = buf.cpu().numpy()
            lo, hi = GUARD + self.off[k], GUARD + self.off[k] + self.sizes[k]
            assert (raw[:lo] == 0xA5).all() and (raw[hi:] == 0xA5).all(), f"{k} at +{self.off[k]}: bytes around the rows were written"
            if k == "llr":
                continue
            body = np.frombuffer(raw[lo:hi].tobytes(), dtype=dtypes[k])
            out[k] = body.reshape(B, -1) if k in ("bits", "posterior", "packed_bits") else body
        return out


def check(out, want, kind, graph, tag):
    """the outputs a run asked for against ds.Expected, as tests/test_gpu_dirty_state.py compares them; the hard decisions are
    taken from the packed rows where there are any (their pad bits zero), and wherever success is 1 they satisfy every check"""
    n = graph.n
    assert want.rows is None and want.success is not None
    np.testing.assert_array_equal(out["iterations"], want.iterations, err_msg=tag)
    np.testing.assert_array_equal(out["success"].astype(bool), want.success, err_msg=tag)
    decided = out["bits"]
    if out["packed_bits"] is not None:
        expanded = np.unpackbits(out["packed_bits"], axis=1, bitorder="little")
        assert not expanded[:, n:].any(), f"{tag}: the pad bits of a packed row are zero"
        decided = expanded[:, :n]
        np.testing.assert_array_equal(decided, want.bits, err_msg=f"{tag}: packed bits")
    if out["bits"] is not None:
        np.testing.assert_array_equal(out["bits"], want.bits, err_msg=f"{tag}: bits")
    if out["posterior"] is not None:
        if kind in ds.EXACT_POSTERIOR:
            np.testing.assert_array_equal(out["posterior"], want.posterior, err_msg=f"{tag}: posterior")
        else:
            assert_post(out["posterior"], want.posterior, tag)
    ok = out["success"].astype(bool)
    assert not graph.syndrome(decided[ok]).any(), f"{tag}: a row reported as a success fails a check"


def same(out, base, tag):
    for k in OUTPUTS:
        if out[k] is not None:
            np.testing.assert_array_equal(out[k], base[k], err_msg=f"{tag}: {k} differs from the aligned run")


def device_llrs(case, device):
    return torch.from_numpy(np.array(ds.llrs(*case))).to(device)


# ---- a. the raw entry points at every placement ----------------------------------------------------------------------------
@pytest.mark.parametrize("family,code", ra.FAMILY_CODES)
def test_a_streaming_decode_does_not_depend_on_where_the_rows_lie(family, code, gpu_device, oracle_mod):
    fam = ds.FAMILIES[family]
    eng = ds.engine(family, code, gpu_device)
    info = eng.info()
    assert info["engine"] == "stream" and fam.where in (info["stream_form"], info["kernel"]), info
    graph = ds.load_code(code).tanner_graph()
    run = PlacedDecode(eng)
    for case in ra.cases(family, code):
        x = device_llrs(case, gpu_device)
        for early_stop, cap in ra.STOPS:
            want = ra.expected(oracle_mod, case, early_stop, cap)
            base = None
            for pl in ra.placements(family):
                tag = f"{ds.case_id(case)} early_stop={early_stop} cap={cap} {pl.name}"
                run.place(x, pl)
                assert run.kernels(cap) == ra.kernels(family, graph.n, case.B, pl), tag
                out = run.decode(early_stop, cap)
                assert (out["bits"] is None) == (pl.bits is None) and (out["posterior"] is None) == (pl.posterior is None)
                check(out, want, fam.kind, graph, tag)
                if base is None:
                    assert pl.name == "aligned"
                    base = out
                same(out, base, tag)


# ---- b. every family takes every width its engine can reach --------------------------------------------------------------
@pytest.mark.parametrize("family", ra.FAMILIES)
def test_the_case_list_takes_every_boundary_kernel_the_family_can_reach(family, gpu_device):
    """what test (a) launches, asked of the launcher's own selection (no decode here: the hook compares addresses only)"""
    seen = set()
    for code in ra.CODES:
        eng = ds.engine(family, code, gpu_device)
        for B in ra.BATCHES[ra.dtype_of(family)]:
            for _, cap in ra.STOPS:
                for pl in ra.placements(family):
                    a = lambda off: 0 if off is None else (1 << 20) + GUARD + off
                    k = ra.Kernels(**eng.boundary_kernels(B, llr=a(pl.llr), posterior=a(pl.posterior), bits=a(pl.bits), max_iters=cap))
                    assert k == ra.kernels(family, eng.graph.n, B, pl), (code, B, cap, pl)
                    seen.add(k)
    ins, outs = ra.reachable(family)
    assert {(k.vec, k.in_bytes) for k in seen} == ins
    assert {(k.vec, k.out_path, k.out_bytes) for k in seen} == outs
    if family in ra.PAIR_Q4:        # the fused entrance pass: on for 16-byte rows on 256-codeword tiles, off everywhere else
        assert {(k.vec, k.in_bytes) for k in seen if k.fused_in} == {(4, 16)}
        assert {(k.vec, k.in_bytes) for k in seen if not k.fused_in} == ins - {(4, 16)}
    else:
        assert not any(k.fused_in for k in seen)
    assert eng._lib.ldpc_debug_boundary_kernels(eng.handle, 65, 0, 0, None, None, None, None) == -1     # NULL output: LDPC_ERR_ARG
    with pytest.raises(ValueError):
        eng.boundary_kernels(0)


# ---- c. ldpc_decode_saving: the layout pass on 256-codeword tiles, then the backward -----------------------------------------
@pytest.mark.parametrize("family", ["n2d2", "offset2"])
def test_decode_saving_and_backward_with_every_pointer_at_4_bytes(family, gpu_device, oracle_mod):
    fam = ds.FAMILIES[family]
    eng = ds.engine(family, ra.ODD, gpu_device)
    graph = ds.load_code(ra.ODD).tanner_graph()
    run = PlacedDecode(eng)
    skewed = ra.Placement("all+4", 4, 4, 4)
    for B in (65, 257):
        case = ra.Case(family, ra.ODD, B)
        x = device_llrs(case, gpu_device)
        gpost = torch.from_numpy(np.random.default_rng(ra.seed_of("gpost", family, B)).standard_normal((B, graph.n)).astype(np.float32))
        for early_stop in (True, False):
            want = ra.expected(oracle_mod, case, early_stop)
            got = {}
            for pl in (ra.PLACEMENTS[ra.F32][0], skewed):
                tag = f"{ds.case_id(case)} saving early_stop={early_stop} {pl.name}"
                run.place(x, pl, packed=False)
                launched = run.kernels(saving=True)
                assert launched == ra.kernels(family, graph.n, B, pl, saving=True), tag
                assert launched == ra.Kernels(4, 4, False, "layout", 4), tag          # the 4-byte layout pass at both ends
                saved = torch.full((eng.train_saved_bytes(B),), 0xA5, dtype=torch.uint8, device=gpu_device)
                out = run.decode(early_stop, saved=saved)
                check(out, want, fam.kind, graph, tag)
                grads = eng.backward(saved, x, torch.from_numpy(out["iterations"].copy()), gpost, want_grad_llr=True)
                got[pl.name] = (out, [None if g is None else host(g) for g in grads])
            (out, grads), (base, base_grads) = got["all+4"], got["aligned"]
            same(out, base, tag)
            assert any(g is not None and np.any(g != 0) for g in base_grads)
            for g, b, what in zip(grads, base_grads, ("beta", "alpha", "oms_alpha", "llr")):
                assert (g is None) == (b is None)
                if g is not None:
                    np.testing.assert_array_equal(g, b, err_msg=f"{tag}: grad {what} differs from the aligned run")


# ---- d. the public API -------------------------------------------------------------------------------------------------------
def view_at(x, k):
    """x's rows as a contiguous view k elements into a flat buffer (what DecodeEngine.decode's .contiguous() keeps)"""
    flat = torch.full((x.numel() + 8,), float("nan"), dtype=x.dtype, device=x.device)
    v = flat[k:k + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and flat.data_ptr() % 16 == 0 and v.data_ptr() == flat.data_ptr() + k * x.element_size()
    return v


FIELDS = ("bits", "posterior", "iterations", "success", "packed_bits")


@pytest.mark.parametrize("mode", ["stream", "pair", "gather", "auto"])
@pytest.mark.parametrize("code", ["small96", ra.ODD])
def test_decode_of_a_view_into_a_flat_buffer(code, mode, gpu_device, oracle_mod):
    family = "rcq-pair"
    eng = ds.engine(family, code, gpu_device, mode)
    info = eng.info()
    assert info["engine"] == ("resident" if mode == "auto" else "stream"), info
    assert mode in ("auto", "stream") or info["stream_form"] == {"pair": "rcq-code-pair", "gather": "fused-rcq-iteration"}[mode]
    graph = ds.load_code(code).tanner_graph()
    for B in (65, 257):
        case = ra.Case(family, code, B)
        x = device_llrs(case, gpu_device)
        for early_stop in (True, False):
            want = ra.expected(oracle_mod, case, early_stop)
            ref = eng.decode(x.clone(), early_stop=early_stop, want_packed=True)
            tag = f"{ds.case_id(case)} {mode} early_stop={early_stop}"
            check({"bits": host(ref.bits), "posterior": host(ref.posterior), "iterations": host(ref.iterations),
                   "success": host(ref.success), "packed_bits": host(ref.packed_bits)}, want, "rcq", graph, tag)
            for k in (1, 2, 3):
                v = view_at(x, k)
                if mode != "auto":
                    took = eng.boundary_kernels(B, llr=v.data_ptr())
                    assert took["in_bytes"] == ra.width(4, graph.n, 4 * k) and took["fused_in"] == (mode != "gather" and took["in_bytes"] == 16)
                for how, res in (("decode", eng.decode(v, early_stop=early_stop, want_packed=True)),
                                 ("torch.ops.ldpc.decode", eng.decode_op(v, early_stop=early_stop, want_packed=True))):
                    for f in FIELDS:
                        assert torch.equal(getattr(res, f), getattr(ref, f)), f"{tag}: {f} of {how} at +{k} floats"


@pytest.mark.parametrize("family", ["basic32", "n2d2", "rcq-pair"])
@pytest.mark.parametrize("mode", ["auto", "stream"])
def test_the_host_decoder_classes_on_the_odd_code(family, mode, gpu_device, oracle_mod):
    """a CPU batch of 5 rows (decode_host staging) and a device batch of 130, each a view one element into a flat buffer"""
    fam, dec = ds.FAMILIES[family], ds.decoder(family, ra.ODD)
    ds.engine(family, ra.ODD, gpu_device, mode)
    for B, dev in ((5, torch.device("cpu")), (130, gpu_device)):
        case = ra.Case(family, ra.ODD, B)
        v = view_at(torch.from_numpy(np.array(ds.llrs(*case))).to(dev), 1)
        for early_stop in (True, False):
            want = ra.expected(oracle_mod, case, early_stop)
            tag = f"{ds.case_id(case)} {mode} {dev.type} early_stop={early_stop}"
            if fam.kind == "neural2d":
                bits, post, iters = dec(v, early_stop=early_stop)
                assert_post(host(post), want.posterior, tag)
            else:
                arg = v.numpy() if dev.type == "cpu" and fam.kind == "basic" else v
                bits, succ, iters = dec.decode(arg, early_stop=early_stop)
                np.testing.assert_array_equal(np.asarray(host(succ) if torch.is_tensor(succ) else succ, dtype=bool), want.success, err_msg=tag)
            as_np = lambda t: host(t) if torch.is_tensor(t) else np.asarray(t)
            np.testing.assert_array_equal(as_np(bits), want.bits, err_msg=tag)
            np.testing.assert_array_equal(as_np(iters), want.iterations, err_msg=tag)
    ds.engine(family, ra.ODD, gpu_device)


# ---- e. the LDS-resident engines as the control: rows are read and written element by element -------------------------------
@pytest.mark.parametrize("code", ["small96", ra.ODD])
def test_the_resident_engine_takes_no_layout_pass(code, gpu_device, oracle_mod):
    family = "basic32"
    eng = ds.engine(family, code, gpu_device, "auto")
    info = eng.info()
    assert info["engine"] == "resident", info
    assert info["resident_kernel"]["early_stop"]["plan"] == "general", info
    assert info["resident_kernel"]["fixed_T"]["plan"] in ("general", "register-state", "compact"), info
    graph = ds.load_code(code).tanner_graph()
    run = PlacedDecode(eng)
    for B in (1, 3, 130):
        case = ra.Case(family, code, B)
        x = device_llrs(case, gpu_device)
        for early_stop in (True, False):
            want = ra.expected(oracle_mod, case, early_stop)
            base = None
            for pl in ra.placements(family):
                tag = f"{ds.case_id(case)} resident early_stop={early_stop} {pl.name}"
                run.place(x, pl)
                with pytest.raises(NotImplementedError):                     # LDPC_ERR_UNSUPPORTED
                    run.kernels()
                out = run.decode(early_stop)
                check(out, want, "basic", graph, tag)
                base = base or out
                same(out, base, tag)
    ds.engine(family, code, gpu_device)
