"""
A result is a function of the inputs only: decode, training and Monte-Carlo results must not depend on what the caller's
scratch, the `saved` block or the output buffers held before the call (tests/dirty_state_cases.py has the families, codes,
batches and inputs; tests/test_dirty_state_host.py what the oracle does with them).

Every scratch buffer is filled byte-wise before the call under test -- 0x00 (what a fresh allocation usually holds), 0xFF
(fp32 NaN, every latch bit set, ticket -1, code 255), 0x7F (3.39e38, code 127) -- or left as a decode of 300 saturated rows
in the opposite stop mode wrote it ("history").  Each run is compared with the CPU restatement of its family, as that
family's own tests compare, and bit for bit with the 0x00 run.  Outputs are handed over inside larger 0xA5 buffers: every
element of a non-NULL output must be written, nothing around it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import dirty_state_cases as ds
from test_gpu_parity import assert_post

pytestmark = pytest.mark.gpu

BYTE_POISONS = ("0x00", "0xFF", "0x7F")
POISONS = BYTE_POISONS + ("history",)


@pytest.fixture(autouse=True)
def inference_mode():
    with torch.no_grad():
        yield


def host(t):
    return t.detach().cpu().numpy()


def unpack(packed, n):
    return np.unpackbits(np.asarray(packed), axis=1, bitorder="little")[:, :n]


def compare(got, want, kind, graph, tag):
    """got: (bits, posterior, iterations, success, packed | None) as numpy arrays against ds.Expected"""
    bits, post, iters, succ, packed = got
    np.testing.assert_array_equal(iters, want.iterations, err_msg=tag)
    if want.success is None:                      # fixed T without a fixed-T oracle: success is the syndrome of the decisions
        np.testing.assert_array_equal(succ.astype(bool), ~graph.syndrome(bits).any(axis=-1), err_msg=tag)
    else:
        np.testing.assert_array_equal(succ.astype(bool), want.success, err_msg=tag)
    rows = slice(None) if want.rows is None else want.rows
    np.testing.assert_array_equal(bits[rows], want.bits[rows], err_msg=tag)
    if kind in ds.EXACT_POSTERIOR:
        np.testing.assert_array_equal(post[rows], want.posterior[rows], err_msg=tag)
    else:
        assert_post(post[rows], want.posterior[rows], tag)
    if packed is not None:
        np.testing.assert_array_equal(unpack(packed, bits.shape[1]), bits, err_msg=tag)


# ---- a. the streaming engine's workspace -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ds.DECODE_CASES, ids=ds.case_id)
def test_streaming_decode_does_not_read_what_the_workspace_held(case, gpu_device, oracle_mod):
    fam = ds.FAMILIES[case.family]
    eng = ds.engine(case.family, case.code, gpu_device)
    info = eng.info()
    assert info["engine"] == "stream" and fam.where in (info["stream_form"], info["kernel"]), info
    graph = ds.load_code(case.code).tanner_graph()
    x = torch.from_numpy(np.array(ds.llrs(case.family, case.code, case.B))).to(gpu_device)
    history = torch.from_numpy(ds.saturated_llrs(case.code, fam.dtype)).to(gpu_device)
    for early_stop, cap in ds.STOPS:
        want = ds.expected(oracle_mod, case, early_stop, cap)
        base = None
        for poison in POISONS:
            if poison == "history":
                eng.decode(history, early_stop=not early_stop)          # same engine, same stream, same buffer
                assert eng._workspace(case.B).numel() >= eng.workspace_bytes(300)
            else:
                eng._workspace(case.B).fill_(int(poison, 16))
            res = eng.decode(x, early_stop=early_stop, want_packed=True, max_iters=cap)
            tag = f"{ds.case_id(case)} early_stop={early_stop} cap={cap} workspace {poison}"
            compare((host(res.bits), host(res.posterior), host(res.iterations), host(res.success), host(res.packed_bits)),
                    want, fam.kind, graph, tag)
            if base is None:
                base = res
            for name in ("bits", "posterior", "iterations", "success", "packed_bits"):
                assert torch.equal(getattr(res, name), getattr(base, name)), f"{tag}: {name} differs from the 0x00 run"


# ---- b. outputs, every engine ----------------------------------------------------------------------------------------------
GUARD = 256
OUTPUTS = ("bits", "posterior", "iterations", "success", "packed_bits")


class GuardedDecode:
    """ldpc_decode through the raw entry point, every output inside a larger buffer filled with 0xA5"""

    def __init__(self, eng):
        import _native
        self.nat, self.lib, self.eng = _native, _native.load(), eng

    def __call__(self, x, early_stop, null=None):
        """-> {output: numpy array | None}; the 256 bytes before and after every output are checked"""
        eng, (B, n) = self.eng, x.shape
        es = 4 if eng.dtype == torch.float32 else 8
        sizes = {"bits": B * n * 4, "posterior": B * n * es, "iterations": B * 4, "success": B, "packed_bits": B * ((n + 7) // 8)}
        bufs = {k: torch.full((v + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=eng.device) for k, v in sizes.items() if k != null}
        p = lambda k: C.c_void_p(bufs[k].data_ptr() + GUARD) if k in bufs else None
        ws = eng._workspace(B)
        with torch.cuda.device(eng.device):
            stream = torch.cuda.current_stream(eng.device).cuda_stream
            self.nat.check(self.lib.ldpc_decode(eng.handle, C.c_void_p(x.data_ptr()), B, int(early_stop), p("bits"), p("posterior"),
                                                p("iterations"), p("success"), p("packed_bits"), C.c_void_p(ws.data_ptr()),
                                                ws.numel(), C.c_void_p(stream)), "ldpc_decode")
        out = dict.fromkeys(OUTPUTS)
        for k, buf in bufs.items():
            raw = buf.cpu().numpy()
            assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + sizes[k]:] == 0xA5).all(), f"{k}: bytes around the output were written"
            body = raw[GUARD:GUARD + sizes[k]]
            out[k] = {"bits": lambda: body.view(np.int32).reshape(B, n), "posterior": lambda: body.view(eng.np_dtype).reshape(B, n),
                      "iterations": lambda: body.view(np.int32), "success": lambda: body.copy(),
                      "packed_bits": lambda: body.reshape(B, (n + 7) // 8)}[k]()
        return out


def _regstate_case(oracle_mod, B, early_stop):
    """Basic on the `mixed_stride` code of tests/test_gpu_resident_regstate.py -> (decoder, kind, llr, Expected)"""
    import test_gpu_resident_regstate as rr
    from ldpc_decoder import BasicMinSumDecoder
    code = _cached("regstate-code", rr.code_mixed_stride)
    llr = rr.llrs(np.random.default_rng(ds.seed_of("regstate", B)), B, code.n)
    out = oracle_mod.basic_minsum(oracle_mod.OracleGraph(code.H), llr, 0.7, 8, early_stop=early_stop, dtype=np.float32)
    return _cached("regstate-dec", lambda: BasicMinSumDecoder(code, 0.7)), "basic", llr, ds.Expected(*out, None)


def _compact_case(oracle_mod, B, early_stop):
    """family n2d-4 on the `tails` code of tests/compact_forms_cases.py (the compact fixed-T plan)"""
    import compact_forms_cases as cf
    from test_gpu_parity import oracle_capped
    code = _cached("compact-code", lambda: cf.make_code("tails", cf.T_FULL))
    dec, wkw = _cached("compact-dec", lambda: cf.build_decoder("n2d-4", code, cf.T_FULL, cf.seed_of("w", "n2d-4", "tails", cf.T_FULL)))
    llr = cf.llrs_mix(cf.seed_of("dirty", B), B, code.n, cf.snr_of("n2d-4", "tails"))
    out = oracle_capped(oracle_mod, cf.oracle_graph(oracle_mod, code), llr, "neural2d", cf.T_FULL, cf.T_FULL, early_stop=early_stop, **wkw)
    return dec, "neural2d", llr, ds.Expected(*out, None)


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# name -> (engine mode, what info() must report: engine, and the kernel / fixed-T resident plan where it matters, source)
OUTPUT_CASES = {
    "stream-basic-ira": ("stream", "stream", None, ("basic32", "ira")),
    "stream-wrcq-small": ("pair", "stream", None, ("wrcq-q4", "small")),
    "resident-general": ("auto", "resident", "general", ("basic32", "small")),          # early stop: always the general plan
    "resident-register-state": ("auto", "resident", "register-state", _regstate_case),
    "resident-compact": ("auto", "resident", "compact", _compact_case),
    "layered-lds": ("auto", "resident", "layered_lds", ("lay-ref", "small")),
    "layered-paper-lds": ("auto", "resident", "layered_paper_lds", ("lay-paper", "small")),
    "layered-minsum-lds": ("auto", "resident", "layered_minsum_lds", ("lay-nms", "small")),
}


def _output_case(name, oracle_mod, device, B, early_stop):
    """-> (engine, kind, llr, Expected)"""
    from simulation_framework import _engine_of
    mode, _, _, src = OUTPUT_CASES[name]
    if callable(src):
        dec, kind, llr, want = src(oracle_mod, B, early_stop)
        return _engine_of(dec, device).set_mode(mode), kind, llr, want
    case = ds.Case(*src, B)
    return (ds.engine(case.family, case.code, device, mode), ds.FAMILIES[case.family].kind, ds.llrs(*case),
            ds.expected(oracle_mod, case, early_stop))


@pytest.mark.parametrize("name", list(OUTPUT_CASES))
def test_every_element_of_every_output_is_written_and_nothing_else(name, gpu_device, oracle_mod):
    _, engine_kind, where, _ = OUTPUT_CASES[name]
    eng = _output_case(name, oracle_mod, gpu_device, 1, True)[0]
    info = eng.info()
    assert info["engine"] == engine_kind, info
    if where in ("general", "register-state", "compact"):
        assert info["resident_kernel"]["early_stop"]["plan"] == "general", info
        assert where == "general" or info["resident_kernel"]["fixed_T"]["plan"] == where, info
    elif where is not None:
        assert info["kernel"] == where, info
    cpw = info["codewords_per_workgroup"]
    for B in sorted({1, 3, 130} | ({cpw - 1, cpw + 1} if cpw > 1 else set())):
        for early_stop in (True, False):
            eng, kind, llr, want = _output_case(name, oracle_mod, gpu_device, B, early_stop)
            graph = eng.graph
            x = torch.from_numpy(np.array(llr)).to(gpu_device)
            run = GuardedDecode(eng)
            full = run(x, early_stop)
            tag = f"{name} B={B} early_stop={early_stop}"
            compare([full[k] for k in OUTPUTS], want, kind, graph, tag)
            pad = np.unpackbits(full["packed_bits"], axis=1, bitorder="little")[:, graph.n:]
            assert not pad.any(), f"{tag}: the pad bits of a packed row are zero"
            for null in OUTPUTS:                                          # each output pointer NULL in turn: the others unchanged
                part = run(x, early_stop, null=null)
                assert part[null] is None
                for k in OUTPUTS:
                    if k != null:
                        np.testing.assert_array_equal(part[k], full[k], err_msg=f"{tag}: {k} with {null} = NULL")


# ---- c. training: saved, the backward workspace -----------------------------------------------------------------------------
def _decode_saving_into(eng, x, early_stop, saved, poison):
    """DecodeEngine.decode_saving with the caller's `saved` block and a poisoned workspace"""
    import _native as nat
    B, n = x.shape
    out = [torch.empty((B, n), dtype=torch.int32, device=eng.device), torch.empty((B, n), dtype=torch.float32, device=eng.device),
           torch.empty((B,), dtype=torch.int32, device=eng.device), torch.empty((B,), dtype=torch.uint8, device=eng.device)]
    ws = eng._train_workspace(B)
    ws.fill_(poison)
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(eng.device):
        stream = torch.cuda.current_stream(eng.device).cuda_stream
        nat.check(eng._lib.ldpc_decode_saving(eng.handle, p(x), B, int(early_stop), *map(p, out), p(saved), saved.numel(), p(ws),
                                              ws.numel(), C.c_void_p(stream)), "ldpc_decode_saving")
    return out


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("form", ["nms", "oms"])
def test_backward_does_not_read_what_saved_and_the_workspace_held(form, early_stop, gpu_device, oracle_mod):
    """decode_saving + backward (table gradients and d loss / d llr) of the normalised form and of the offset form with its
    check-side alpha, on the 48 x 96 code at B = 70 (VEC = 4, 186 padding codewords): against the gradient oracle within the
    tolerances of tests/test_gpu_training.py, whatever `saved` and the workspace held"""
    import codes
    import grad_oracle
    from neural_2d_decoder import Neural2DMinSumDecoder, Neural2DOffsetMinSumDecoder
    T, B = 4, 70
    code = codes.load_code("small_96_48", T)
    rng = np.random.default_rng(ds.seed_of("backward", form))
    torch.manual_seed(1)
    dec = (Neural2DOffsetMinSumDecoder if form == "oms" else Neural2DMinSumDecoder)(code, 2, T)
    ds.fill(dec.beta_weights, rng, *((0.0, 0.4) if form == "oms" else (0.5, 1.0)))
    ds.fill(dec.alpha_weights, rng, *((0.0, 0.1) if form == "oms" else (0.8, 1.2)))
    llr = np.concatenate([ds.awgn(rng, B - B // 2, code.n, 1.0), ds.awgn(rng, B // 2, code.n, 6.0)])[rng.permutation(B)].astype(np.float32)
    eng = dec._get_engine(gpu_device)
    x = torch.from_numpy(llr).to(gpu_device)
    lay = dec._sharing_layout()
    bt_np, at_np = dec.weight_tables()
    bt, at = torch.tensor(bt_np, requires_grad=True), torch.tensor(at_np, requires_grad=True)
    xt = torch.tensor(llr, requires_grad=True)
    with torch.enable_grad():                                             # the oracle's gradient is torch autograd on the CPU
        post, _, iters = grad_oracle.forward(oracle_mod.OracleGraph(code.H), xt, bt, lay.beta_slot, at,
                                             lay.alpha_edge_slot if form == "oms" else lay.alpha_slot, T, early_stop,
                                             offset=form == "oms")
    post_np = post.detach().numpy()
    saved_bytes = eng.train_saved_bytes(B)
    gpost = None
    for poison in (0x00, 0xFF, 0x7F):
        saved = torch.full((saved_bytes,), poison, dtype=torch.uint8, device=gpu_device)
        bits, gpu_post, gpu_iters, _ = _decode_saving_into(eng, x, early_stop, saved, poison)
        plain = eng.decode(x, early_stop=early_stop)
        assert torch.equal(bits, plain.bits) and torch.equal(gpu_post, plain.posterior) and torch.equal(gpu_iters, plain.iterations)
        if gpost is None:
            # a different summation order may flip a near-tie; those codewords are left out, as tests/test_gpu_training.py does
            agree = (iters.numpy() == host(gpu_iters)) & np.all(np.abs(post_np - host(gpu_post)) <= 1e-4 * np.maximum(1, np.abs(post_np)), axis=1)
            assert agree.mean() > 0.95
            gpost = rng.standard_normal((B, code.n)).astype(np.float32) * agree[:, None]
            with torch.enable_grad():
                (post * torch.from_numpy(gpost)).sum().backward()
            if early_stop:
                assert len(np.unique(host(gpu_iters))) >= 2
        eng._train_workspace(B).fill_(poison)
        gb, ga, goa, gl = eng.backward(saved, x, gpu_iters, torch.from_numpy(gpost).to(gpu_device), want_grad_llr=True)
        got_alpha = goa if form == "oms" else ga
        for got, want, what in ((gb, bt.grad, "beta"), (got_alpha, at.grad, "alpha"), (gl, xt.grad, "llr")):
            want = want.numpy()
            np.testing.assert_allclose(host(got), want, rtol=2e-3, atol=2e-4 * np.abs(want).max(), err_msg=f"{what}, poison {poison:#x}")


# the four posterior-joint-training entry points, each on the first (smallest) case of its own test file, through that file's
# own comparison with its restatement (its `close` helper and tolerances): engine kind -> (test module, test function)
JOINT = {"minsum": ("test_gpu_joint_training", "test_gradients_match_the_restatement"),
         "ste": ("test_gpu_joint_training_rcq", "test_gradients_match_the_restatement"),
         "layered": ("test_gpu_layered_joint_training", "test_forward_loss_and_gradients_match_the_restatement"),
         "layered_ste": ("test_gpu_layered_joint_training_rcq", "test_gradients_match_the_restatement")}


@pytest.mark.parametrize("poison", [0x00, 0xFF, 0x7F], ids=hex)
@pytest.mark.parametrize("kind", list(JOINT))
def test_train_joint_does_not_read_what_its_workspace_held(kind, poison, gpu_device, oracle_mod, monkeypatch):
    import importlib
    import inspect
    from engine import DecodeEngine
    plain, kinds = DecodeEngine._train_joint, []

    def poisoned(self, llr, targets, iteration_weights, want_grads, want_grad_llr, kind):
        need = int(getattr(self._lib, self._JOINT_ENTRY[kind][1])(self.handle, llr.shape[0]))
        ws = getattr(self, "_joint_ws", None)
        if ws is None or ws.numel() < need:
            self._joint_ws = ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        ws.fill_(poison)                                                  # _train_joint finds the buffer and keeps it
        kinds.append(kind)
        return plain(self, llr, targets, iteration_weights, want_grads, want_grad_llr, kind)

    monkeypatch.setattr(DecodeEngine, "_train_joint", poisoned)
    module, name = JOINT[kind]
    test = getattr(importlib.import_module(module), name)
    kw = {"gpu_device": gpu_device, "case": 0, "oracle_mod": oracle_mod}
    with torch.enable_grad():
        test(**{k: kw[k] for k in inspect.signature(test).parameters})
    assert kind in kinds, kinds


# ---- d. Monte-Carlo -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["auto", "stream"])
def test_simulate_does_not_read_what_its_workspace_held(mode, gpu_device, oracle_mod):
    """one regime of tests/test_gpu_simulate.py (3.0 dB, 2500 frames, 30 errors) at block 257, plain and with diagnostics"""
    import codes
    import test_gpu_sim_diag as sd
    import test_gpu_simulate as sim
    from simulation_framework import _engine_of
    snr_db, max_frames, max_errors = sim.REGIMES[0]
    assert (snr_db, max_frames, max_errors) == (3.0, 2500, 30) and sim.SEED == sd.SEED
    code = codes.load_code("small_96_48", sd.T)
    dec, oracle_decode = sd.make_decoder("basic", code, oracle_mod)
    frames = _cached("sim-frames", lambda: sd.decoded_frames(oracle_decode, code.n, gpu_device, snr_db, max_frames))
    want = sd.fold(frames, 4, max_frames, max_errors)
    assert 0 < want["frame_errors"] < want["frames"] and want["done"] == 1 and want["captured"] == 4
    eng = _engine_of(dec, gpu_device).set_mode(mode)
    kw = dict(snr_db=snr_db, max_frames=max_frames, max_errors=max_errors, block=257)
    sd.native_point(eng, diagnostics=True, capture=4, **kw)                 # the workspace exists from here on
    for poison in (0x00, 0xFF, 0x7F):
        eng._sim_ws.fill_(poison)
        plain = sd.native_point(eng, **kw)
        assert {k: plain[k] for k in sd.COUNTERS} == {k: want[k] for k in sd.COUNTERS}, hex(poison)
        eng._sim_ws.fill_(poison)
        sd.same(sd.native_point(eng, diagnostics=True, capture=4, **kw), want)
    eng.set_mode("auto")


# ---- e. decode_host -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["basic32", "rcq-pair"])
def test_decode_host_does_not_read_what_its_staging_buffers_held(family, gpu_device, oracle_mod):
    fam = ds.FAMILIES[family]
    graph = ds.load_code("small").tanner_graph()
    for mode in ("auto", fam.mode):
        eng = ds.engine(family, "small", gpu_device, mode)
        eng.decode_host(torch.from_numpy(ds.saturated_llrs("small", fam.dtype, rows=64)), early_stop=False)
        for poison, B in ((0x00, 1), (0xFF, 3), (0x7F, 64), (0xFF, 1)):
            st = eng._host_stage
            for k in ("d_out", "h_out", "ws"):
                st[k].fill_(poison)
            case = ds.Case(family, "small", B)
            for early_stop in (True, False):
                bits, post, iters, succ = eng.decode_host(torch.from_numpy(np.array(ds.llrs(*case))), early_stop=early_stop)
                compare((bits.numpy(), post.numpy(), iters.numpy(), succ.numpy(), None), ds.expected(oracle_mod, case, early_stop),
                        fam.kind, graph, f"{family} {mode} B={B} early_stop={early_stop} poison {poison:#x}")
