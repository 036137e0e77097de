"""
GPU parity tests (-m gpu): the HIP engine, called through the C ABI by the host classes,
against (1) the golden vectors captured from the real reference (tests/golden, made by
oracle/make_golden.py) and (2) the CPU restatement (oracle/) on fresh seeded inputs.

Bars: bits / success / iterations / RCQ codes bit-exact; fp32 posteriors within 1e-5
(BASELINE.json north_star) -- in practice they are equal as values because the kernels
reproduce torch.sum's association order.
"""
import numpy as np
import pytest
import torch

from conftest import golden_sub, load_golden, weights_dict

pytestmark = pytest.mark.gpu

QP = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]
POST_TOL = 1e-5


@pytest.fixture(autouse=True)
def inference_mode():
    """These are decode (inference) tests: with autograd enabled the trainable decoders keep their messages for
    backward and run the saving streaming path, which tests/test_gpu_training.py covers.  Here grad is off so that
    LDPC_ENGINE_MODE really selects the engine under test; check_neural re-enables it for one comparison."""
    with torch.no_grad():
        yield


@pytest.fixture(autouse=True, params=["auto", "stream", "sweeps", "gather"])
def engine_mode(request, monkeypatch):
    """every test runs on every engine form: 'auto' picks the LDS-resident fused kernel for codes that qualify
    (all the fp32 fixtures here), 'stream' the HBM-streaming engine (RCQ decoders: its fused one-kernel-per-
    iteration form), 'sweeps' the streaming engine with one kernel per sweep for every decoder"""
    monkeypatch.setenv("LDPC_ENGINE_MODE", request.param)
    return request.param


def codes_of(dec, llr_gpu, early_stop=True, max_iters=None):
    """per-edge quantiser codes [B, E] (CSR order) of every codeword's last executed iteration, on BOTH engines:
    the streaming engine keeps the 1-byte codes in HBM (state of the last decode, which must have run with this
    max_iters); the LDS-resident engine holds reconstructed values (1 - 2*sign) * tau[level], dumped by
    ldpc_debug_resident_c2v (its own decode, capped at max_iters) and mapped back to codes here (the sign bit of a
    reconstructed zero tells code L, "-0", from code 0)."""
    eng = dec._engine
    B = llr_gpu.shape[0]
    if eng.info()["engine"] == "stream":
        return eng.debug_c2v(B, max_iters=max_iters).detach().cpu().numpy()
    from rcq_decoder import _quantizer_schedule, _threshold_table
    vals, _, iters = eng.debug_resident_c2v(llr_gpu.to(torch.float32), early_stop=early_stop, max_iters=max_iters)
    vals, iters = vals.cpu().numpy(), iters.cpu().numpy()
    thr = _threshold_table(dec.quantizers)                       # [Q, L] float32(tau)
    T = int(dec.max_iterations)
    if T == 0:
        return np.zeros(vals.shape, np.uint8)
    q_of_iter = _quantizer_schedule(len(dec.quantizers), T)
    L = thr.shape[1]
    out = np.empty(vals.shape, np.uint8)
    for r in range(B):
        tau = thr[q_of_iter[max(int(iters[r]), 1) - 1]]
        mag = np.abs(vals[r])
        level = np.array([np.flatnonzero(tau == m)[-1] if np.any(tau == m) else 255 for m in mag])
        assert np.all(level != 255), "a resident C2V value is not a reconstruction level"
        out[r] = np.where(np.signbit(vals[r]), L, 0) + level
    return out


def assert_codes(got, want, n_levels):
    """Codes must be equal, with ONE licence for the value-based read-out of the resident engine: the reference
    gives code 0 to w = -0.0 (sign(-0.0) is not < 0) where the reconstructed value there is -0.0, read back as code L;
    both reconstruct to a zero.  Anything else, including a reference code L read as 0, is a failure."""
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    bad = got != want
    licence = (want == 0) & (got == n_levels)
    assert not np.any(bad & ~licence), f"{int(np.sum(bad & ~licence))} per-edge quantiser codes differ"


# --------------------------------------------------------------------------------- helpers
def make_code(gold, max_iterations):
    from ldpc_decoder import LDPCCode
    import codes
    if "H" in gold:
        H = gold["H"].astype(np.int64)
        return LDPCCode(n=H.shape[1], k=H.shape[1] - H.shape[0], H=H, max_iterations=int(max_iterations))
    return codes.load_code(str(gold["graph"]), max_iterations=int(max_iterations))


def load_weights(dec, sub):
    beta = weights_dict(sub["beta_keys"], sub["beta_vals"])
    alpha = weights_dict(sub["alpha_keys"], sub["alpha_vals"])
    assert set(beta) == set(dec.beta_weights.keys()) and set(alpha) == set(dec.alpha_weights.keys())
    sd = {f"beta_weights.{k}": torch.tensor([v], dtype=torch.float32) for k, v in beta.items()}
    sd.update({f"alpha_weights.{k}": torch.tensor([v], dtype=torch.float32) for k, v in alpha.items()})
    dec.load_state_dict(sd)           # the reference's state_dict key scheme
    return beta, alpha


def assert_post(a, b, what=""):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    err = np.abs(a - b)
    tol = POST_TOL * np.maximum(1.0, np.abs(b))
    assert np.all(err <= tol), f"{what}: posterior max err {err.max()}"


def check_neural(dec, sub, gpu):
    """batched + single-vector forward against a golden block"""
    llr = torch.from_numpy(sub["llr"])
    with torch.no_grad():                       # inference: the engine LDPC_ENGINE_MODE selects
        bits, post, iters = dec(llr.to(gpu))
    assert bits.dtype == torch.int32 and post.dtype == torch.float32 and iters.dtype == torch.int32
    if any(p.requires_grad for p in dec.parameters()):
        # grad enabled (the reference's default call): same numbers; the normalised min-sum decoders attach a grad_fn
        with torch.enable_grad():
            b2, p2, i2 = dec(llr.to(gpu))
        assert torch.equal(b2, bits) and torch.equal(i2, iters) and torch.equal(p2.detach(), post)
        assert p2.requires_grad == (type(dec).__name__ in ("Neural2DMinSumDecoder", "Neural2DOffsetMinSumDecoder",
                                                           "NeuralMinSumDecoder", "NeuralOffsetMinSumDecoder"))
    np.testing.assert_array_equal(iters.detach().cpu().numpy(), sub["iters"])
    np.testing.assert_array_equal(bits.detach().cpu().numpy(), sub["bits"].astype(np.int32))
    assert_post(post.detach().cpu().numpy(), sub["posterior"])
    # the reference's own call shape: one CPU vector in, CPU tensors + python int out
    b1, p1, i1 = dec(llr[0])
    assert b1.device.type == "cpu" and b1.shape == (dec.code.n,) and isinstance(i1, int)
    assert i1 == int(sub["iters"][0])
    np.testing.assert_array_equal(b1.numpy(), sub["bits"][0].astype(np.int32))
    assert_post(p1.detach().numpy(), sub["posterior"][0])


def final_codes(golden_codes, iters):
    """code trace [B,T,E] -> codes of the last executed iteration of every codeword"""
    return np.stack([golden_codes[r, iters[r] - 1] for r in range(len(iters))])


def oracle_capped(oracle_mod, og, llr, kind, t, T, *, early_stop=True, trace_codes=False, factor=0.7, bc=3, qp=QP,
                  wtype=None, beta=None, alpha=None):
    """Expected outputs of a decode capped at t (ldpc_decode_capped, max_iters=t) by a decoder built for T iterations: the
    oracle run for t iterations with the T-iteration decoder's tables -- beta / alpha rows 0..t-1 and the quantiser
    schedule of T (oracle.quantizer_schedule, restated independently of rcq_decoder._quantizer_index).
    kind: "basic" (fp32 or fp64 as llr), "neural2d", "offset" (Neural2DOffsetMinSumDecoder), "rcq", "wrcq".
    -> (bits, posterior, iterations, success[, codes [B, t, E]])"""
    assert 1 <= t <= T
    o = oracle_mod
    kw = dict(T=t, early_stop=early_stop, trace_codes=trace_codes)
    no_beta = dict(beta=np.ones((T, 1), np.float32), beta_slot=np.zeros(og.E, np.int32))
    no_alpha = dict(alpha=np.ones((T, 1), np.float32), alpha_slot=np.zeros(og.n, np.int32))
    if kind == "basic":
        dt = np.float64 if np.asarray(llr).dtype == np.float64 else np.float32
        return o.decode(og, np.asarray(llr, dt), c2v_form=o.C2V_NMS, sum_order=o.SUM_NUMPY if dt == np.float64 else o.SUM_TORCH,
                        beta=np.full((T, 1), factor, dt), beta_slot=np.zeros(og.E, np.int32),
                        alpha=np.ones((T, 1), dt), alpha_slot=np.zeros(og.n, np.int32), **kw)
    x = np.asarray(llr, np.float32)
    if kind == "offset":
        bt, bs, at, as_ = o.weight_tables(og, wtype, T, beta, alpha, beta_default=0.0, alpha_default=0.0)
        return o.decode(og, x, c2v_form=o.C2V_OMS, beta=bt, beta_slot=bs, oms_alpha=at, oms_alpha_slot=as_[og.var_idx],
                        **no_alpha, **kw)
    if kind in ("neural2d", "wrcq"):
        bt, bs, at, as_ = o.weight_tables(og, wtype, T, beta, alpha)
        tables = dict(beta=bt, beta_slot=bs, alpha=at, alpha_slot=as_)
    else:
        assert kind == "rcq"
        tables = dict(no_beta, **no_alpha)
    if kind == "neural2d":
        return o.decode(og, x, c2v_form=o.C2V_NMS, **tables, **kw)
    thr = np.asarray([o.quantizer_thresholds(bc, c, gm) for c, gm in qp], dtype=np.float32)
    return o.decode(og, x, c2v_form=o.C2V_RCQ, thresholds=thr, q_of_iter=o.quantizer_schedule(T, len(qp)), **tables, **kw)


# --------------------------------------------------------------------------------- Basic
@pytest.mark.parametrize("name", ["toy_basic", "small_basic", "ira_basic"])
def test_basic_golden_fp64(name, gpu_device):
    from ldpc_decoder import BasicMinSumDecoder
    g = load_golden(name)
    code = make_code(g, g["T"])
    dec = BasicMinSumDecoder(code, factor=float(g["factor"]))
    bits, succ, iters = dec.decode(g["llr"])                      # float64 batch -> fp64 kernels
    assert bits.dtype == np.int64
    np.testing.assert_array_equal(iters, g["iters"])
    np.testing.assert_array_equal(succ, g["success"])
    np.testing.assert_array_equal(bits, g["bits"].astype(np.int64))
    # reference call shape
    b, s, i = dec.decode(g["llr"][0])
    assert isinstance(s, bool) and isinstance(i, int) and b.dtype == np.int64 and b.shape == (code.n,)
    assert (s, i) == (bool(g["success"][0]), int(g["iters"][0]))
    np.testing.assert_array_equal(b, g["bits"][0])


def test_basic_fp32_vs_oracle_and_fp64_reference(gpu_device, oracle_mod):
    """config 2's arithmetic: fp32 Basic.  Bit-exact against the fp32 oracle; against the
    fp64 reference outputs only away from decision boundaries (tolerance statement)."""
    from ldpc_decoder import BasicMinSumDecoder
    g = load_golden("ira_basic")
    code = make_code(g, g["T"])
    dec = BasicMinSumDecoder(code, factor=0.7)
    llr32 = g["llr"].astype(np.float32)
    bits, succ, iters = dec.decode(llr32)
    og = oracle_mod.OracleGraph(code.H)
    ob, op, oi, os_ = oracle_mod.basic_minsum(og, llr32, factor=0.7, T=int(g["T"]), dtype=np.float32)
    np.testing.assert_array_equal(bits, ob)
    np.testing.assert_array_equal(iters, oi)
    np.testing.assert_array_equal(succ, os_)
    # fp32 engine vs the float64 REFERENCE outputs on the reference's own inputs: measured identical (BASELINE.md 6,
    # tools/f32_vs_f64.py) -- every iteration count, success flag and bit of the 16 golden codewords
    np.testing.assert_array_equal(iters, g["iters"])
    np.testing.assert_array_equal(succ, g["success"])
    np.testing.assert_array_equal(bits, g["bits"])


@pytest.mark.parametrize("snr_db,max_cw_frac", [(2.0, 5e-4), (5.0, 1e-4)])
def test_basic_fp32_vs_fp64_mismatch_rate_is_bounded(snr_db, max_cw_frac, gpu_device, engine_mode):
    """The benchmark computes BasicMinSumDecoder in fp32 (BASELINE.json north_star) where the reference computes in
    float64 (ldpc_decoder.py:80-81, 116-120).  Quantified on a fresh 65536-codeword batch with the float64 kernels
    (bit-exact against the reference goldens) as the yardstick -- measured on MI355X: at 2 dB 3 of
    65536 codewords differ in any bit (4.6e-5; 2.3e-8 of the bits) and no iteration count differs; at 5 dB nothing
    differs.  The bounds asserted here are 10x the measurement."""
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    if engine_mode != "auto":
        pytest.skip("one engine suffices: the engines give identical results (every other test checks that)")
    code = codes.load_code("ira_1998_1512", 10)
    dec = BasicMinSumDecoder(code, 0.7)
    s2 = 10.0 ** (-snr_db / 10.0)
    gen = torch.Generator(device=gpu_device)
    gen.manual_seed(1234)
    z = torch.randn((65536, code.n), generator=gen, device=gpu_device, dtype=torch.float32)
    x64 = (2.0 * (1.0 + (s2 ** 0.5) * z) / s2).double()
    for early in (True, False):
        b64, s64, i64 = dec.decode(x64, early_stop=early)
        b32, s32, i32 = dec.decode(x64.float(), early_stop=early)
        cw_differs = (b64 != b32).any(dim=1).float().mean().item()
        assert cw_differs <= max_cw_frac, f"{cw_differs} of the codewords differ in a bit"
        assert (i64 != i32).float().mean().item() <= max_cw_frac
        assert (s64 != s32).float().mean().item() <= max_cw_frac
        assert (b64 != b32).float().mean().item() <= 1e-6


# --------------------------------------------------------------------------------- Neural 2D
@pytest.mark.parametrize("wtype", [1, 2, 3, 4])
def test_neural2d_toy_golden(wtype, gpu_device):
    from neural_2d_decoder import Neural2DMinSumDecoder
    g = load_golden("toy_neural2d")
    for tag in (f"t{wtype}", f"t{wtype}d"):
        sub = golden_sub(g, tag)
        code = make_code({"H": g["H"]}, 10)
        dec = Neural2DMinSumDecoder(code, weight_sharing_type=wtype, max_iterations=int(sub["T"]))
        load_weights(dec, sub)
        check_neural(dec, sub, gpu_device)


@pytest.mark.parametrize("wtype", [1, 2, 3, 4])
def test_neural2d_small_golden(wtype, gpu_device):
    from neural_2d_decoder import Neural2DMinSumDecoder
    g = load_golden("small_neural2d")
    sub = golden_sub(g, f"t{wtype}")
    dec = Neural2DMinSumDecoder(make_code(g, 10), weight_sharing_type=wtype, max_iterations=int(sub["T"]))
    load_weights(dec, sub)
    check_neural(dec, sub, gpu_device)


def test_neural2d_ira_golden(gpu_device):
    from neural_2d_decoder import Neural2DMinSumDecoder
    g = load_golden("ira_neural2d")
    dec = Neural2DMinSumDecoder(make_code(g, 10), weight_sharing_type=int(g["wtype"]), max_iterations=int(g["T"]))
    load_weights(dec, g)
    check_neural(dec, g, gpu_device)


# --------------------------------------------------------------------------------- RCQ
def check_rcq(code, sub, gpu, bc=3, qp=QP):
    from rcq_decoder import RCQMinSumDecoder
    dec = RCQMinSumDecoder(code, bc=bc, bv=8, quantizer_params=qp, max_iterations=int(sub["T"]))
    llr = torch.from_numpy(sub["llr"])
    bits, succ, iters = dec.decode(llr.to(gpu))
    np.testing.assert_array_equal(iters.detach().cpu().numpy(), sub["iters"])
    np.testing.assert_array_equal(succ.detach().cpu().numpy(), sub["success"])
    np.testing.assert_array_equal(bits.detach().cpu().numpy(), sub["bits"].astype(np.int32))
    # per-edge quantiser codes (CSR order) of every codeword's last executed iteration
    assert_codes(codes_of(dec, llr.to(gpu)), final_codes(sub["codes"], sub["iters"]), 2 ** (bc - 1))
    b1, s1, i1 = dec.decode(llr[1])
    assert isinstance(s1, bool) and isinstance(i1, int) and b1.dtype == torch.int32 and b1.device.type == "cpu"
    assert (s1, i1) == (bool(sub["success"][1]), int(sub["iters"][1]))
    np.testing.assert_array_equal(b1.numpy(), sub["bits"][1].astype(np.int32))


def check_wrcq(code, sub, gpu, wtype, bc=3, qp=QP):
    from rcq_decoder import WeightedRCQDecoder
    dec = WeightedRCQDecoder(code, bc=bc, bv=8, quantizer_params=qp, weight_sharing_type=wtype,
                             max_iterations=int(sub["T"]))
    load_weights(dec, sub)
    check_neural(dec, sub, gpu)
    dec(torch.from_numpy(sub["llr"]).to(gpu))
    assert_codes(codes_of(dec, torch.from_numpy(sub["llr"]).to(gpu)), final_codes(sub["codes"], sub["iters"]), 2 ** (bc - 1))
    # RCQ posteriors are sums of a handful of table values: must be equal as values
    b, p, i = dec(torch.from_numpy(sub["llr"]).to(gpu))
    np.testing.assert_array_equal(p.detach().cpu().numpy(), sub["posterior"])


def test_rcq_toy_golden(gpu_device):
    g = load_golden("toy_rcq")
    code = make_code({"H": g["H"]}, 10)
    check_rcq(code, golden_sub(g, "rcq"), gpu_device)
    sub4 = golden_sub(g, "rcq4")
    check_rcq(code, sub4, gpu_device, bc=4, qp=[tuple(x) for x in sub4["qp"]])
    for wtype in (1, 2, 3, 4):
        check_wrcq(code, golden_sub(g, f"w{wtype}"), gpu_device, wtype)
    check_wrcq(code, golden_sub(g, "w2d"), gpu_device, 2)


def test_rcq_small_golden(gpu_device):
    g = load_golden("small_rcq")
    code = make_code(g, 10)
    check_rcq(code, golden_sub(g, "rcq"), gpu_device)
    check_wrcq(code, golden_sub(g, "w2"), gpu_device, 2)
    check_wrcq(code, golden_sub(g, "w1"), gpu_device, 1)


def test_rcq_ira_golden(gpu_device):
    g = load_golden("ira_rcq")
    check_rcq(make_code(g, 10), g, gpu_device)
    g = load_golden("ira_wrcq")
    check_wrcq(make_code(g, 10), g, gpu_device, int(g["wtype"]))


def test_wrcq_dvbs2_golden(gpu_device):
    """config 5's decoder on the (16200,7200) graph, T=20, one reference codeword"""
    import os
    from conftest import GOLDEN
    if not os.path.exists(os.path.join(GOLDEN, "dvbs2_wrcq.npz")):
        pytest.skip("dvbs2 golden not generated")
    g = load_golden("dvbs2_wrcq")
    check_wrcq(make_code(g, 20), g, gpu_device, int(g["wtype"]))


# --------------------------------------------------------------------------------- RCQ, every iteration
# every golden block with a per-iteration code trace: (file, prefix of the block or None)
RCQ_TRACE_BLOCKS = [("toy_rcq", "rcq"), ("toy_rcq", "rcq4"), ("toy_rcq", "w1"), ("toy_rcq", "w2"), ("toy_rcq", "w3"),
                    ("toy_rcq", "w4"), ("toy_rcq", "w2d"), ("small_rcq", "rcq"), ("small_rcq", "w1"), ("small_rcq", "w2"),
                    ("ira_rcq", None), ("ira_wrcq", None), ("dvbs2_wrcq", None),
                    # 2, 32, 64 and 128 levels (bc 2, 6, 7, 8): codes with bit 7 set, level 127
                    ("rcq_widths", "rcq2"), ("rcq_widths", "rcq6"), ("rcq_widths", "rcq7"), ("rcq_widths", "rcq8"),
                    ("rcq_widths", "w2b6"), ("rcq_widths", "w2b8"), ("rcq_widths", "w1b8")]


def rcq_trace_block(name, tag):
    """-> (golden file dict, block dict, oracle_capped keyword arguments of the block's decoder)"""
    g = load_golden(name)
    sub = golden_sub(g, tag) if tag else g
    kw = dict(kind="wrcq" if "wtype" in sub else "rcq", bc=int(sub["bc"]), qp=[tuple(x) for x in sub["qp"]])
    if kw["kind"] == "wrcq":
        kw.update(wtype=int(sub["wtype"]), beta=weights_dict(sub["beta_keys"], sub["beta_vals"]),
                  alpha=weights_dict(sub["alpha_keys"], sub["alpha_vals"]))
    return g, sub, kw


@pytest.mark.parametrize("name,tag", RCQ_TRACE_BLOCKS, ids=[f"{n}-{t}" if t else n for n, t in RCQ_TRACE_BLOCKS])
def test_rcq_golden_every_iteration(name, tag, gpu_device, oracle_mod, engine_mode):
    """ldpc_decode_capped at every t in 1..T on every golden block with a code trace, both stop modes, every engine form:
    the per-edge codes of the last executed iteration equal the reference's codes of iteration min(t, iters) (early stop)
    and the oracle's (fixed T); bits, iterations, success and the posterior (equal as values) equal the oracle run for t
    iterations with the T-iteration tables.  Pins the quantiser schedule and the beta / alpha row of EVERY iteration, not
    only the last -- a schedule one iteration off can leave the final codes right when the codeword converges early."""
    from rcq_decoder import RCQMinSumDecoder, WeightedRCQDecoder
    g, sub, kw = rcq_trace_block(name, tag)
    T, L = int(sub["T"]), 2 ** (int(sub["bc"]) - 1)
    code = make_code(g, T)
    og = oracle_mod.OracleGraph(n=code.n, check_ptr=code.tanner_graph().check_ptr, var_idx=code.tanner_graph().var_idx)
    if kw["kind"] == "wrcq":
        dec = WeightedRCQDecoder(code, kw["bc"], 8, kw["qp"], weight_sharing_type=kw["wtype"], max_iterations=T)
        load_weights(dec, sub)
    else:
        dec = RCQMinSumDecoder(code, kw["bc"], 8, kw["qp"], max_iterations=T)
    eng = dec._get_engine(gpu_device)
    llr = sub["llr"]
    x = torch.from_numpy(llr).to(gpu_device)
    gi = sub["iters"].astype(np.int64)
    full = eng.decode(x, early_stop=True)
    np.testing.assert_array_equal(full.iterations.cpu().numpy(), gi)
    for early in (True, False):
        for t in range(1, T + 1):
            res = eng.decode(x, early_stop=early, max_iters=t)
            got = codes_of(dec, x, early, max_iters=t)
            ob, op, oi, os_, oc = oracle_capped(oracle_mod, og, llr, t=t, T=T, early_stop=early, trace_codes=True, **kw)
            what = f"t={t} early_stop={early}"
            np.testing.assert_array_equal(res.iterations.cpu().numpy(), oi, err_msg=what)
            np.testing.assert_array_equal(res.success.cpu().numpy(), os_, err_msg=what)
            np.testing.assert_array_equal(res.bits.cpu().numpy(), ob, err_msg=what)
            np.testing.assert_array_equal(res.posterior.cpu().numpy(), op, err_msg=what)
            assert_codes(got, np.stack([oc[r, oi[r] - 1] for r in range(len(oi))]), L)
            if early:
                assert_codes(got, np.stack([sub["codes"][r, min(t, gi[r]) - 1] for r in range(len(gi))]), L)
                done = gi <= t
                it, sc = res.iterations.cpu().numpy(), res.success.cpu().numpy()
                np.testing.assert_array_equal(it[done], gi[done], err_msg=what)
                np.testing.assert_array_equal(res.bits.cpu().numpy()[done], sub["bits"][done].astype(np.int32), err_msg=what)
                np.testing.assert_array_equal(sc[done], full.success.cpu().numpy()[done], err_msg=what)
                assert np.all(it[~done] == t) and not sc[~done].any(), what
            else:
                assert bool((res.iterations == t).all()), what


# --------------------------------------------------------------------------------- oracle, fresh inputs
def awgn(rng, B, n, snr_db):
    s2 = 10.0 ** (-snr_db / 10.0)
    return (2.0 * (1.0 + np.sqrt(s2) * rng.standard_normal((B, n))) / s2).astype(np.float32)


def rand_weights(dec, rng):
    with torch.no_grad():
        for p in dec.beta_weights.values():
            p.fill_(float(np.float32(rng.uniform(0.5, 1.0))))
        for p in dec.alpha_weights.values():
            p.fill_(float(np.float32(rng.uniform(0.8, 1.2))))
    return ({k: float(v.item()) for k, v in dec.beta_weights.items()},
            {k: float(v.item()) for k, v in dec.alpha_weights.items()})


@pytest.mark.parametrize("B", [1, 3, 64, 65, 256, 300, 1000])
@pytest.mark.parametrize("early_stop", [True, False])
def test_batch_sizes_vs_oracle_neural2d(B, early_stop, gpu_device, oracle_mod):
    """ragged batches (tile padding, VEC=1 latency tile) on the 48x96 code, mixed SNR so that
    codewords of one wave stop at different iterations"""
    import codes
    from neural_2d_decoder import Neural2DMinSumDecoder
    rng = np.random.default_rng(1000 + B)
    code = codes.load_code("small_96_48", 10)
    dec = Neural2DMinSumDecoder(code, weight_sharing_type=2, max_iterations=8)
    beta, alpha = rand_weights(dec, rng)
    llr = np.concatenate([awgn(rng, B - B // 2, 96, 1.0), awgn(rng, B // 2, 96, 6.0)])[rng.permutation(B)]
    bits, post, iters = dec(torch.from_numpy(llr).to(gpu_device), early_stop=early_stop)
    og = oracle_mod.OracleGraph(code.H)
    ob, op, oi, _ = oracle_mod.neural2d(og, llr, 2, 8, beta, alpha, early_stop=early_stop)
    np.testing.assert_array_equal(iters.detach().cpu().numpy(), oi)
    np.testing.assert_array_equal(bits.detach().cpu().numpy(), ob)
    assert_post(post.detach().cpu().numpy(), op)


@pytest.mark.parametrize("early_stop", [True, False])
def test_ira_batch_vs_oracle_all_decoders(early_stop, gpu_device, oracle_mod):
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    from neural_2d_decoder import Neural2DMinSumDecoder
    from rcq_decoder import RCQMinSumDecoder, WeightedRCQDecoder
    rng = np.random.default_rng(77)
    B = 300
    code = codes.load_code("ira_1998_1512", 10)
    og = oracle_mod.OracleGraph(n=code.n, check_ptr=code.tanner_graph().check_ptr, var_idx=code.tanner_graph().var_idx)
    llr = np.concatenate([awgn(rng, 150, code.n, 2.0), awgn(rng, 150, code.n, 4.5)])[rng.permutation(B)]
    x = torch.from_numpy(llr).to(gpu_device)

    bits, succ, iters = BasicMinSumDecoder(code).decode(x, early_stop=early_stop)
    ob, op, oi, os_ = oracle_mod.basic_minsum(og, llr, 0.7, 10, early_stop=early_stop, dtype=np.float32)
    np.testing.assert_array_equal(iters.detach().cpu().numpy(), oi)
    np.testing.assert_array_equal(succ.detach().cpu().numpy(), os_)
    np.testing.assert_array_equal(bits.detach().cpu().numpy(), ob)

    for wtype in (1, 2, 4):
        dec = Neural2DMinSumDecoder(code, weight_sharing_type=wtype, max_iterations=10)
        beta, alpha = rand_weights(dec, rng)
        bits, post, iters = dec(x, early_stop=early_stop)
        ob, op, oi, _ = oracle_mod.neural2d(og, llr, wtype, 10, beta, alpha, early_stop=early_stop)
        np.testing.assert_array_equal(iters.detach().cpu().numpy(), oi)
        np.testing.assert_array_equal(bits.detach().cpu().numpy(), ob)
        assert_post(post.detach().cpu().numpy(), op)

    dec = RCQMinSumDecoder(code, 3, 8, QP, max_iterations=10)
    bits, succ, iters = dec.decode(x, early_stop=early_stop)
    ob, op, oi, os_, oc = oracle_mod.rcq(og, llr, 3, QP, 10, early_stop=early_stop, trace_codes=True)
    np.testing.assert_array_equal(iters.detach().cpu().numpy(), oi)
    np.testing.assert_array_equal(succ.detach().cpu().numpy(), os_)
    np.testing.assert_array_equal(bits.detach().cpu().numpy(), ob)
    assert_codes(codes_of(dec, x, early_stop), final_codes(oc, oi), 4)

    dec = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=2, max_iterations=10)
    beta, alpha = rand_weights(dec, rng)
    bits, post, iters = dec(x, early_stop=early_stop)
    ob, op, oi, _, oc = oracle_mod.weighted_rcq(og, llr, 3, QP, 2, 10, beta, alpha, early_stop=early_stop, trace_codes=True)
    np.testing.assert_array_equal(iters.detach().cpu().numpy(), oi)
    np.testing.assert_array_equal(bits.detach().cpu().numpy(), ob)
    np.testing.assert_array_equal(post.detach().cpu().numpy(), op)
    assert_codes(codes_of(dec, x, early_stop), final_codes(oc, oi), 4)


IRA_CAPS = (1, 2, 3, 5, 9)
IRA_FLOAT_CASES = ["basic-f32", "basic-f64", "neural2d-1", "neural2d-2", "neural2d-3", "neural2d-4", "offset-2"]


def ira_float_case(case):
    """(1998,1512), T = 10: the decoder of `case` with seeded random weights, 300 codewords (a third each at 2.5, 5 and
    7 dB: with this channel convention only the last two thirds converge within the caps, at 1 to 9 iterations)"""
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    from neural_2d_decoder import Neural2DMinSumDecoder, Neural2DOffsetMinSumDecoder
    kind, arg = case.split("-")
    code = codes.load_code("ira_1998_1512", 10)
    rng = np.random.default_rng(sum(map(ord, case)))
    llr = np.concatenate([awgn(rng, 100, code.n, 2.5), awgn(rng, 100, code.n, 5.0), awgn(rng, 100, code.n, 7.0)])
    llr = llr[rng.permutation(len(llr))]
    if kind == "basic":
        return code, BasicMinSumDecoder(code, 0.7), (llr.astype(np.float64) if arg == "f64" else llr), {}
    dec = (Neural2DOffsetMinSumDecoder if kind == "offset" else Neural2DMinSumDecoder)(code, weight_sharing_type=int(arg),
                                                                                       max_iterations=10)
    with torch.no_grad():
        for p in dec.beta_weights.values():
            p.fill_(float(np.float32(rng.uniform(0.0, 0.6) if kind == "offset" else rng.uniform(0.5, 1.0))))
        for p in dec.alpha_weights.values():
            p.fill_(float(np.float32(rng.uniform(0.0, 0.3) if kind == "offset" else rng.uniform(0.8, 1.2))))
    beta = {k: float(v.item()) for k, v in dec.beta_weights.items()}
    alpha = {k: float(v.item()) for k, v in dec.alpha_weights.items()}
    return code, dec, llr, dict(wtype=int(arg), beta=beta, alpha=alpha)


_ira_expect = {}


@pytest.mark.parametrize("case", IRA_FLOAT_CASES)
def test_float_decoders_every_cap_vs_oracle_ira(case, gpu_device, oracle_mod, engine_mode):
    """Capped decodes (t = 1, 2, 3, 5, 9 of T = 10) of Basic fp32 / fp64, Neural-2D types 1-4 and Neural-2D offset on the
    (1998,1512) code against the oracle run for t iterations with the T-iteration tables, both stop modes, every engine form:
    bits, iterations, success exact, posterior within 1e-5.  Pins the beta / alpha row of every iteration; under auto the
    fixed-T decodes run the register-state resident kernel with a loop count below the decoder's T."""
    code, dec, llr, wkw = ira_float_case(case)
    kind = case.split("-")[0]
    tg = code.tanner_graph()
    og = oracle_mod.OracleGraph(n=tg.n, check_ptr=tg.check_ptr, var_idx=tg.var_idx)
    eng = dec._engine(torch.from_numpy(llr).dtype, gpu_device) if kind == "basic" else dec._get_engine(gpu_device)
    if engine_mode == "auto":
        assert eng.info()["engine"] == "resident"
    x = torch.from_numpy(llr).to(gpu_device)
    stopped = set()
    for early in (True, False):
        for t in IRA_CAPS:
            key = (case, early, t)
            if key not in _ira_expect:                        # the same for every engine form
                _ira_expect[key] = oracle_capped(oracle_mod, og, llr, kind, t, 10, early_stop=early, **wkw)
            ob, op, oi, os_ = _ira_expect[key]
            res = eng.decode(x, early_stop=early, max_iters=t)
            what = f"t={t} early_stop={early}"
            np.testing.assert_array_equal(res.iterations.cpu().numpy(), oi, err_msg=what)
            np.testing.assert_array_equal(res.success.cpu().numpy(), os_, err_msg=what)
            np.testing.assert_array_equal(res.bits.cpu().numpy(), ob, err_msg=what)
            assert_post(res.posterior.cpu().numpy(), op, what)
            if early:
                stopped |= set(np.unique(oi[os_]).tolist())
    assert {1, 2, 3, 5} <= stopped                          # codewords stop inside the caps, at each of them


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_saturated_llrs_basic_and_neural2d(dtype, gpu_device, oracle_mod, engine_mode):
    """Clipped channels hand over +-inf: |inf| takes part in min1 / min2 like any value, inf + finite = inf in the sums and
    the posterior, a check whose other inputs are all infinite sends +-inf.  Basic (fp32 and the reference's float64) and
    Neural-2D against the CPU restatement, every engine form (LDPC_ENGINE_MODE), both stop rules.  The inputs keep a
    variable's infinite LLR and its infinite messages of one sign, so no inf - inf arises: a NaN is outside the path's domain
    (the reference's sign product np.sign(nan) = nan floods the codeword; documented in DESIGN.md 4)."""
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    from neural_2d_decoder import Neural2DMinSumDecoder
    rng = np.random.default_rng(41)
    for name, T in (("small_96_48", 8), ("ira_1998_1512", 6)):
        code = codes.load_code(name, T)
        g = code.tanner_graph()
        og = oracle_mod.OracleGraph(n=g.n, check_ptr=g.check_ptr, var_idx=g.var_idx)
        B = 70
        llr = awgn(rng, B, code.n, 3.0).astype(np.float64)
        sat = rng.random(llr.shape) < 0.02
        llr[sat] = np.where(llr[sat] >= 0, np.inf, -np.inf)               # saturate in the direction of the sample
        llr[0, : code.n // 3] = np.inf                                     # a third of a codeword clipped
        for early_stop in (True, False):
            if dtype == "f64":
                x = torch.from_numpy(llr).to(gpu_device)
                bits, succ, iters = BasicMinSumDecoder(code).decode(x, early_stop=early_stop)
                ob, op, oi, os_ = oracle_mod.basic_minsum(og, llr, 0.7, T, early_stop=early_stop, dtype=np.float64)
            else:
                x = torch.from_numpy(llr.astype(np.float32)).to(gpu_device)
                bits, succ, iters = BasicMinSumDecoder(code).decode(x, early_stop=early_stop)
                ob, op, oi, os_ = oracle_mod.basic_minsum(og, llr.astype(np.float32), 0.7, T, early_stop=early_stop, dtype=np.float32)
            np.testing.assert_array_equal(iters.cpu().numpy(), oi)
            np.testing.assert_array_equal(succ.cpu().numpy(), os_)
            np.testing.assert_array_equal(bits.cpu().numpy(), ob)
            if dtype == "f32":
                dec = Neural2DMinSumDecoder(code, weight_sharing_type=2, max_iterations=T)
                beta, alpha = rand_weights(dec, rng)
                with torch.no_grad():
                    bits, post, iters = dec(x, early_stop=early_stop)
                ob, op, oi, _ = oracle_mod.neural2d(og, llr.astype(np.float32), 2, T, beta, alpha, early_stop=early_stop)
                np.testing.assert_array_equal(iters.cpu().numpy(), oi)
                np.testing.assert_array_equal(bits.cpu().numpy(), ob)
                got, want = post.cpu().numpy(), op
                assert np.array_equal(np.isinf(got), np.isinf(want)) and not np.isnan(got).any()
                fin = np.isfinite(want)
                np.testing.assert_array_equal(np.sign(got[~fin]), np.sign(want[~fin]))
                assert_post(got[fin], want[fin])


def test_offset_minsum_vs_oracle(gpu_device, oracle_mod):
    """Neural2DOffsetMinSumDecoder (zero-aware sign product), incl. exact-zero inputs"""
    import codes
    from neural_2d_decoder import Neural2DOffsetMinSumDecoder
    from weight_sharing import SharingLayout
    rng = np.random.default_rng(5)
    code = codes.load_code("small_96_48", 10)
    og = oracle_mod.OracleGraph(code.H)
    llr = awgn(rng, 200, 96, 3.0)
    llr[::3, rng.integers(0, 96, 67)] = 0.0
    llr[1::5] = np.round(llr[1::5])
    for wtype in (1, 2, 3, 4):
        dec = Neural2DOffsetMinSumDecoder(code, weight_sharing_type=wtype, max_iterations=7)
        with torch.no_grad():
            for p in dec.beta_weights.values():
                p.fill_(float(np.float32(rng.uniform(0.0, 0.6))))
            for p in dec.alpha_weights.values():
                p.fill_(float(np.float32(rng.uniform(0.0, 0.3))))
        bits, post, iters = dec(torch.from_numpy(llr).to(gpu_device))
        lay = SharingLayout(code.tanner_graph(), wtype)
        bt, at = dec.weight_tables()
        ob, op, oi, _ = oracle_mod.decode(og, llr, T=7, c2v_form=oracle_mod.C2V_OMS, beta=bt, beta_slot=lay.beta_slot,
                                          alpha=np.ones((7, 1), np.float32), alpha_slot=np.zeros(96, np.int32),
                                          oms_alpha=at, oms_alpha_slot=lay.alpha_edge_slot)
        np.testing.assert_array_equal(iters.detach().cpu().numpy(), oi)
        np.testing.assert_array_equal(bits.detach().cpu().numpy(), ob)
        assert_post(post.detach().cpu().numpy(), op)


@pytest.mark.parametrize("name", ["toy_offset_edge", "small_offset_edge"])
def test_offset_and_edge_weight_golden(name, gpu_device):
    """SURVEY 8f-2 rows against the reference's own outputs: Neural2DOffsetMinSumDecoder types 1-4,
    NeuralMinSumDecoder, NeuralOffsetMinSumDecoder (per-edge weights)"""
    from neural_2d_decoder import Neural2DOffsetMinSumDecoder
    from neural_minsum_decoder import NeuralMinSumDecoder, NeuralOffsetMinSumDecoder
    g = load_golden(name)
    for w in (1, 2, 3, 4):
        sub = golden_sub(g, f"o{w}")
        dec = Neural2DOffsetMinSumDecoder(make_code(g, 10), weight_sharing_type=w, max_iterations=int(sub["T"]))
        load_weights(dec, sub)
        check_neural(dec, sub, gpu_device)
    for tag, cls in (("nms", NeuralMinSumDecoder), ("oms", NeuralOffsetMinSumDecoder)):
        sub = golden_sub(g, tag)
        dec = cls(make_code(g, 10), max_iterations=int(sub["T"]))
        beta = weights_dict(sub["beta_keys"], sub["beta_vals"])
        assert set(beta) == set(dec.beta_weights.keys())
        dec.load_state_dict({f"beta_weights.{k}": torch.tensor([v], dtype=torch.float32) for k, v in beta.items()})
        check_neural(dec, sub, gpu_device)


# --------------------------------------------------------------------------------- edge cases
def odd_code():
    """dense-ish 12x40 code: check degrees > 32 (wide path), variable degrees > 8 (generic
    sums), plus a degree-1 check, an isolated variable and an empty check"""
    from ldpc_decoder import LDPCCode
    rng = np.random.default_rng(12)
    H = (rng.random((12, 40)) < 0.9).astype(np.int64)
    H[10, :] = 0; H[10, 5] = 1          # degree-1 check
    H[11, :] = 0                        # empty check
    H[:, 39] = 0                        # isolated variable
    H[:, 38] = 0; H[0, 38] = 1          # degree-1 variable
    return LDPCCode(n=40, k=28, H=H, max_iterations=6)


@pytest.mark.parametrize("T", [0, 1, 6])
def test_odd_degrees_and_iteration_counts(T, gpu_device, oracle_mod):
    from ldpc_decoder import BasicMinSumDecoder
    from neural_2d_decoder import Neural2DMinSumDecoder
    from rcq_decoder import RCQMinSumDecoder
    code = odd_code()
    code.max_iterations = T
    og = oracle_mod.OracleGraph(code.H)
    assert og.dc.max() > 32 and og.dv.max() > 8
    rng = np.random.default_rng(T)
    llr64 = rng.standard_normal((130, 40)) * 3
    llr64[7, 3] = 0.0
    llr64[9] = np.round(llr64[9])
    # fp64 Basic (np.sum order incl. the 8-accumulator branch)
    bits, succ, iters = BasicMinSumDecoder(code).decode(llr64)
    ob, op, oi, os_ = oracle_mod.basic_minsum(og, llr64, 0.7, T)
    np.testing.assert_array_equal(iters, oi)
    np.testing.assert_array_equal(succ, os_)
    np.testing.assert_array_equal(bits, ob)
    llr = llr64.astype(np.float32)
    x = torch.from_numpy(llr).to(gpu_device)
    dec = Neural2DMinSumDecoder(code, weight_sharing_type=1, max_iterations=T)
    beta, alpha = rand_weights(dec, rng)
    bits, post, iters = dec(x)
    ob, op, oi, _ = oracle_mod.neural2d(og, llr, 1, T, beta, alpha)
    np.testing.assert_array_equal(iters.detach().cpu().numpy(), oi)
    np.testing.assert_array_equal(bits.detach().cpu().numpy(), ob)
    assert_post(post.detach().cpu().numpy(), op)
    dec = RCQMinSumDecoder(code, 3, 8, QP, max_iterations=T)
    bits, succ, iters = dec.decode(x)
    ob, op, oi, os_ = oracle_mod.rcq(og, llr, 3, QP, T)
    np.testing.assert_array_equal(iters.detach().cpu().numpy(), oi)
    np.testing.assert_array_equal(succ.detach().cpu().numpy(), os_)
    np.testing.assert_array_equal(bits.detach().cpu().numpy(), ob)


@pytest.mark.parametrize("bc,B", [(3, 300), (3, 40), (4, 300), (5, 130), (5, 7)])
@pytest.mark.parametrize("early_stop", [True, False])
def test_rcq_code_pair_form_edge_cases(bc, B, early_stop, gpu_device, oracle_mod, engine_mode):
    """The streaming form that sends BOTH directions as 1-byte codes (vn_sweep_q / cn_sweep_q: the variable side applies
    the next iteration's beta and quantiser) against the CPU restatement and against the fp32-V2C sweeps, on inputs that
    hit its special cases: negative and zero betas (sign of beta * min, all-zero magnitudes), exact-zero and tied
    messages, 4 / 8 / 16 levels (compile-time compare chain, register thresholds, threshold loop), 256- and
    64-codeword tiles, odd degrees (dc > 32, dv > 8) next to the (96,48) code."""
    if engine_mode != "stream":
        pytest.skip("sets the engine forms itself")
    import codes
    from rcq_decoder import WeightedRCQDecoder
    rng = np.random.default_rng(100 * bc + B)
    qp = QP if bc == 3 else [(4.0, 1.2), (6.0, 1.0), (9.0, 0.8)]
    for code, T in ((codes.load_code("small_96_48", 10), 7), (odd_code(), 5)):
        og = oracle_mod.OracleGraph(code.H)
        llr = (rng.standard_normal((B, code.n)) * 2.5 + 1.0).astype(np.float32)
        llr[0] = np.round(llr[0])                                    # ties and exact zeros
        llr[1 % B, ::3] = 0.0
        if B > 3:                                                    # saturated inputs: |beta * inf| = inf, 0 * inf = NaN -> code 0
            llr[2, ::5] = np.inf
            llr[3, 1::4] = -np.inf
        x = torch.from_numpy(llr).to(gpu_device)
        dec = WeightedRCQDecoder(code, bc, 8, qp, weight_sharing_type=2, max_iterations=T)
        with torch.no_grad():
            for i, p_ in enumerate(dec.beta_weights.values()):
                p_.fill_(float(np.float32([0.8, -0.6, 0.0, 1.3][i % 4] if i % 5 else rng.uniform(0.4, 1.1))))
            for p_ in dec.alpha_weights.values():
                p_.fill_(float(np.float32(rng.uniform(0.7, 1.2))))
        beta = {k: float(v.item()) for k, v in dec.beta_weights.items()}
        alpha = {k: float(v.item()) for k, v in dec.alpha_weights.items()}
        eng = dec._get_engine(gpu_device)
        eng.set_mode("pair")
        assert eng.info()["stream_form"] == "rcq-code-pair"
        a = eng.decode(x, early_stop=early_stop)
        ca = eng.debug_c2v(B).cpu().numpy()
        eng.set_mode("sweeps")
        b = eng.decode(x, early_stop=early_stop)
        cb = eng.debug_c2v(B).cpu().numpy()
        ob, op, oi, osucc = oracle_mod.weighted_rcq(og, llr, bc, qp, 2, T, beta, alpha, early_stop=early_stop)
        np.testing.assert_array_equal(a.bits.cpu().numpy(), ob)
        np.testing.assert_array_equal(a.iterations.cpu().numpy(), oi)
        np.testing.assert_array_equal(a.success.cpu().numpy(), osucc)
        np.testing.assert_array_equal(a.posterior.cpu().numpy(), op)
        assert torch.equal(a.posterior, b.posterior) and torch.equal(a.bits, b.bits)
        np.testing.assert_array_equal(ca, cb)                        # per-edge codes of the last executed iteration


@pytest.mark.parametrize("scale", [1e-17, 3e16])
def test_code_pair_thresholds_outside_the_float_key_range(scale, gpu_device, oracle_mod):
    """The float form of the key (key_pair4) is admitted only for thresholds within [2^-50, 2^50]; a 4-level decoder with
    smaller or larger thresholds keeps the integer compare chain.  Same decode, LLRs and quantisers scaled together (tiny: the
    products are near the subnormal range; huge: beyond 2^50), code-pair form against the CPU restatement and the fp32 sweeps."""
    import codes
    from rcq_decoder import WeightedRCQDecoder
    rng = np.random.default_rng(5)
    code = codes.load_code("small_96_48", 10)
    og = oracle_mod.OracleGraph(code.H)
    qp = [(3.0 * scale, 1.3), (5.0 * scale, 1.3), (7.0 * scale, 1.3)]
    B, T = 300, 6
    llr = ((rng.standard_normal((B, code.n)) * 2.5 + 1.0) * scale).astype(np.float32)
    llr[0, ::4] = 0.0
    x = torch.from_numpy(llr).to(gpu_device)
    dec = WeightedRCQDecoder(code, 3, 8, qp, weight_sharing_type=2, max_iterations=T)
    with torch.no_grad():
        for i, p_ in enumerate(dec.beta_weights.values()):
            p_.fill_(float(np.float32([0.8, -0.6, 1.3][i % 3])))
        for p_ in dec.alpha_weights.values():
            p_.fill_(float(np.float32(rng.uniform(0.7, 1.2))))
    beta = {k: float(v.item()) for k, v in dec.beta_weights.items()}
    alpha = {k: float(v.item()) for k, v in dec.alpha_weights.items()}
    eng = dec._get_engine(gpu_device)
    for early_stop in (False, True):
        eng.set_mode("pair")
        assert eng.info()["stream_form"] == "rcq-code-pair"
        a = eng.decode(x, early_stop=early_stop)
        ca = eng.debug_c2v(B).cpu().numpy()
        eng.set_mode("sweeps")
        b = eng.decode(x, early_stop=early_stop)
        cb = eng.debug_c2v(B).cpu().numpy()
        ob, op, oi, osucc = oracle_mod.weighted_rcq(og, llr, 3, qp, 2, T, beta, alpha, early_stop=early_stop)
        np.testing.assert_array_equal(a.bits.cpu().numpy(), ob)
        np.testing.assert_array_equal(a.iterations.cpu().numpy(), oi)
        np.testing.assert_array_equal(a.posterior.cpu().numpy(), op)
        assert torch.equal(a.posterior, b.posterior) and torch.equal(a.bits, b.bits)
        np.testing.assert_array_equal(ca, cb)


def test_code_pair_key_float_form_is_exact(gpu_device):
    """The 4-level variable sweep counts thresholds with clamped float differences (key_pair4: fast VALU instructions)
    instead of integer compares.  Both device forms against numpy on values that sit ON, one ulp below and one ulp above
    every threshold (after the multiplication by beta), subnormals, zeros of both signs, NaN, infinities, products that
    overflow or underflow, plus two million random bit patterns -- for thresholds at the limits the host admits to the
    form (2^-50, 2^50), tied thresholds, and betas of both signs."""
    import ctypes as C
    import _native
    lib = _native.load()
    rng = np.random.default_rng(17)
    f32 = np.float32
    def neighbours(x, span=3):
        b = np.float32(x).view(np.uint32).astype(np.int64)
        return (b + np.arange(-span, span + 1)).clip(0, 0x7f7fffff).astype(np.uint32).view(np.float32)
    cases = [([0.0, 0.9, 1.9, 3.1], [1.0, 0.7, -0.6, 1.3, 1e-3, 3e4]),
             ([0.0, 2.0 ** -50, 1.0, 2.0 ** 50], [1.0, 0.5, -2.0]),
             ([0.0, 0.37, 0.37, 5.5], [0.8, -1.0]),
             ([0.0, 1.1754944e-38 * 2 ** 76, 2.5, 2.5], [1.0, 0.3])]
    for thr, betas in cases:
        thr = np.asarray(thr, f32)
        for beta in betas:
            beta = f32(beta)
            special = [np.asarray([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1.1754944e-38, 3e-39, 3.4e38, -3.4e38,
                                   2.0 ** -149 / 1, 2.0 ** 53, 2.0 ** 52.5, 2.0 ** -75, 2.0 ** -76], f32)]
            for t in thr[1:]:
                target = neighbours(t)                                  # values whose product with beta lands around t
                with np.errstate(all="ignore"):
                    v = (target / beta).astype(f32)
                special += [np.concatenate([neighbours(x, 4) for x in v]), -np.concatenate([neighbours(x, 2) for x in v]), target]
            rnd_bits = rng.integers(0, 2 ** 32, 2_000_000, dtype=np.uint64).astype(np.uint32).view(f32)
            near = (thr[1 + rng.integers(0, 3, 200_000)] / beta * (1 + rng.standard_normal(200_000) * 1e-6)).astype(f32)
            vals = np.concatenate(special + [rnd_bits, near, (rng.standard_normal(300_001) * 3).astype(f32)])
            x = torch.from_numpy(vals).to(gpu_device)
            t_dev = torch.from_numpy(thr).to(gpu_device)
            kf = torch.full((len(vals),), 255, dtype=torch.uint8, device=gpu_device)
            kc = torch.full_like(kf, 255)
            rc = lib.ldpc_debug_key4(C.c_void_p(x.data_ptr()), len(vals), C.c_float(float(beta)), C.c_void_p(t_dev.data_ptr()),
                                     C.c_void_p(kf.data_ptr()), C.c_void_p(kc.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0
            torch.cuda.synchronize()
            with np.errstate(all="ignore"):
                m = np.abs((beta * vals).astype(f32))                   # float32 product, as rcq_decoder.py:236-241 forms it
                want = (m > 0).astype(np.uint8) + (m >= thr[1]) + (m >= thr[2]) + (m >= thr[3])
            np.testing.assert_array_equal(kc.cpu().numpy(), want)
            np.testing.assert_array_equal(kf.cpu().numpy(), want)


def test_layered_rcq_golden_and_oracle(gpu_device, oracle_mod):
    """RCQMinSumDecoder(layered=True): the reference's own outputs (toy, 48x96), then fresh batches on the
    (1998,1512) code against the oracle in both stop modes"""
    import codes
    from ldpc_decoder import LDPCCode
    from rcq_decoder import RCQMinSumDecoder
    g = load_golden("layered_rcq")
    H = g["toy_H"].astype(np.int64)
    cases = [("toy", LDPCCode(n=7, k=4, H=H, max_iterations=10)), ("small", codes.load_code("small_96_48", 10))]
    for tag, code in cases:
        dec = RCQMinSumDecoder(code, 3, 8, QP, max_iterations=int(g[f"{tag}_T"]), layered=True)
        llr = torch.from_numpy(g[f"{tag}_llr"])
        bits, succ, iters = dec.decode(llr.to(gpu_device))
        np.testing.assert_array_equal(iters.detach().cpu().numpy(), g[f"{tag}_iters"])
        np.testing.assert_array_equal(succ.detach().cpu().numpy(), g[f"{tag}_success"])
        np.testing.assert_array_equal(bits.detach().cpu().numpy(), g[f"{tag}_bits"].astype(np.int32))
        b1, s1, i1 = dec.decode(llr[3])
        assert isinstance(s1, bool) and (s1, i1) == (bool(g[f"{tag}_success"][3]), int(g[f"{tag}_iters"][3]))
        np.testing.assert_array_equal(b1.numpy(), g[f"{tag}_bits"][3].astype(np.int32))
    code = codes.load_code("ira_1998_1512", 10)
    tg = code.tanner_graph()
    og = oracle_mod.OracleGraph(n=tg.n, check_ptr=tg.check_ptr, var_idx=tg.var_idx)
    rng = np.random.default_rng(9)
    llr = np.concatenate([awgn(rng, 100, tg.n, 2.0), awgn(rng, 100, tg.n, 6.5)])[rng.permutation(200)]
    dec = RCQMinSumDecoder(code, 3, 8, QP, max_iterations=10, layered=True)
    bits, succ, iters = dec.decode(torch.from_numpy(llr).to(gpu_device))
    ob, op, oi, os_ = oracle_mod.rcq_layered(og, llr, 3, QP, 10)
    np.testing.assert_array_equal(iters.detach().cpu().numpy(), oi)
    np.testing.assert_array_equal(succ.detach().cpu().numpy(), os_)
    np.testing.assert_array_equal(bits.detach().cpu().numpy(), ob)
    res = dec._engine.decode(torch.from_numpy(llr).to(gpu_device), early_stop=True)
    np.testing.assert_array_equal(res.posterior.detach().cpu().numpy(), op)          # latched posteriors, value-equal
    assert len(np.unique(oi)) >= 2                                          # early stop was exercised


@pytest.mark.parametrize("bc", [2, 8])
def test_layered_rcq_widths_golden(bc, gpu_device, engine_mode):
    """RCQMinSumDecoder(layered=True) against the reference's own outputs at 2 and 128 levels (tests/golden/rcq_widths.npz),
    on the LDS-resident kernel (auto) and the streaming kernel (every other engine mode)"""
    from rcq_decoder import RCQMinSumDecoder
    g = load_golden("rcq_widths")
    sub = golden_sub(g, f"lay{bc}")
    dec = RCQMinSumDecoder(make_code(g, 10), bc, 8, [tuple(x) for x in sub["qp"]], max_iterations=int(sub["T"]), layered=True)
    x = torch.from_numpy(sub["llr"]).to(gpu_device)
    eng = dec._get_engine(gpu_device)
    assert eng.info()["kernel"] == ("layered_lds" if engine_mode == "auto" else "layered_rcq<ref>")
    bits, succ, iters = dec.decode(x)
    np.testing.assert_array_equal(iters.cpu().numpy(), sub["iters"])
    np.testing.assert_array_equal(succ.cpu().numpy(), sub["success"])
    np.testing.assert_array_equal(bits.cpu().numpy(), sub["bits"].astype(np.int32))
    res = eng.decode(x, early_stop=True)
    np.testing.assert_array_equal(res.posterior.cpu().numpy(), sub["oracle_posterior"])
    b1, s1, i1 = dec.decode(torch.from_numpy(sub["llr"])[3])
    assert (s1, i1) == (bool(sub["success"][3]), int(sub["iters"][3]))
    np.testing.assert_array_equal(b1.numpy(), sub["bits"][3].astype(np.int32))


@pytest.mark.parametrize("early_stop", [True, False])
def test_layered_paper_schedule_vs_cpu_restatement(early_stop, gpu_device, oracle_mod):
    """RCQMinSumDecoder(layered="paper"): the layered schedule the reference's _decode_layered sets out to implement
    (rcq_decoder.py:281-350 with its message matrix kept across checks).  PARITY UNPINNED -- nothing in the reference
    executes it; the check is against the independent CPU restatement (oracle.rcq_layered(paper=True)) on the toy code,
    the 48x96 code, the (1998,1512) code and a code with checks wider than the kernel's register-held path."""
    import codes
    from ldpc_decoder import create_test_ldpc_code
    from rcq_decoder import RCQMinSumDecoder
    rng = np.random.default_rng(31)
    cases = [(create_test_ldpc_code(), 40, 10, 2.5), (codes.load_code("small_96_48", 10), 130, 10, 2.0),
             (codes.load_code("ira_1998_1512", 10), 100, 10, 4.0), (wide_check_code(), 70, 6, 3.0)]
    for code, B, T, snr in cases:
        tg = code.tanner_graph()
        og = oracle_mod.OracleGraph(n=tg.n, check_ptr=tg.check_ptr, var_idx=tg.var_idx)
        llr = awgn(rng, B, tg.n, snr)
        llr[0, :3] = 0.0
        dec = RCQMinSumDecoder(code, 3, 8, QP, max_iterations=T, layered="paper")
        x = torch.from_numpy(llr).to(gpu_device)
        bits, succ, iters = dec.decode(x, early_stop=early_stop)
        ob, op, oi, os_ = oracle_mod.rcq_layered(og, llr, 3, QP, T, paper=True)
        if early_stop:
            np.testing.assert_array_equal(iters.cpu().numpy(), oi)
            np.testing.assert_array_equal(succ.cpu().numpy(), os_)
            np.testing.assert_array_equal(bits.cpu().numpy(), ob)
            res = dec._engine.decode(x, early_stop=True)
            np.testing.assert_array_equal(res.posterior.cpu().numpy(), op)
        else:
            # fixed T: rows that never converged agree with the early-stop restatement bit for bit
            keep = ~os_
            assert np.all(iters.cpu().numpy() == T)
            np.testing.assert_array_equal(bits.cpu().numpy()[keep], ob[keep])
    # the paper's schedule converges in fewer iterations than flooding on the same inputs (sanity of the algorithm itself)
    code = codes.load_code("small_96_48", 10)
    llr = awgn(rng, 256, code.n, 2.0)
    x = torch.from_numpy(llr).to(gpu_device)
    it_lay = RCQMinSumDecoder(code, 3, 8, QP, max_iterations=10, layered="paper").decode(x)[2].float().mean()
    it_flo = RCQMinSumDecoder(code, 3, 8, QP, max_iterations=10).decode(x)[2].float().mean()
    assert it_lay < it_flo


def _layered_case_code(rng, n, m, dc_lo, dc_hi, deg1=False):
    """random code whose check degrees lie in [dc_lo, dc_hi] (deg1: check 0 has one edge)"""
    from ldpc_decoder import LDPCCode
    H = np.zeros((m, n), dtype=np.int64)
    for i in range(m):
        dc = 1 if (deg1 and i == 0) else int(rng.integers(dc_lo, dc_hi + 1))
        H[i, rng.choice(n, size=dc, replace=False)] = 1
    return LDPCCode(n=n, k=max(n - m, 1), H=H, max_iterations=6)     # some variables may be in no check at all


@pytest.mark.parametrize("case", ["lw1", "lw2", "lw4", "lw8", "lw16", "lw32", "lw64", "deg1", "gamma0", "bc4", "bc5", "bign",
                                  "bc2", "bc6", "bc8"])
def test_layered_lds_kernel_every_lane_width_vs_oracle_and_streaming_kernel(case, gpu_device, oracle_mod, engine_mode):
    """RCQMinSumDecoder(layered=True) on the LDS-resident kernel (lanes over the edges of a check, ldpc_layered.hip): every
    lane width 1..64, a degree-1 check, a quantiser whose zero level is not zero (gamma = 0: general sign rule), 8 and 16
    levels, 2, 32 and 128 levels (bc 8: the negative codes use bit 7, level 127 fills the low seven), a code whose posteriors leave room for fewer codewords per wave than lane groups, ragged batches, both stop
    modes, packed bits -- against the oracle's restatement of rcq_decoder.py:281-350 and, bit for bit, against the
    streaming kernel (engine modes other than auto run that one)."""
    from rcq_decoder import RCQMinSumDecoder
    rng = np.random.default_rng(sum(map(ord, case)))
    qp, bc, T = QP, 3, 6
    if case.startswith("lw"):
        lw = int(case[2:])
        lo, hi = (1, 1) if lw == 1 else (lw // 2 + 1, lw)
        code = _layered_case_code(rng, 90 if lw < 64 else 130, 30, lo, hi)
    elif case == "deg1":
        code = _layered_case_code(rng, 80, 28, 3, 7, deg1=True)
    elif case == "gamma0":
        code, qp = _layered_case_code(rng, 80, 28, 3, 8), [(1.5, 0.0), (3.0, 1.3), (2.0, 0.0)]
    elif case == "bc4":
        code, bc = _layered_case_code(rng, 80, 28, 3, 8), 4
    elif case in ("bc5", "bc2", "bc6", "bc8"):                  # 16 levels; 2, 32 and 128 (bit 7 of a code, level 127)
        code, bc = _layered_case_code(rng, 80, 28, 3, 8), int(case[2:])
    else:                                                       # 4n bytes per codeword: only 2 of the 8 lane groups hold one
        code = _layered_case_code(rng, 16000, 40, 5, 8)
    tg = code.tanner_graph()
    og = oracle_mod.OracleGraph(n=tg.n, check_ptr=tg.check_ptr, var_idx=tg.var_idx)
    dec = RCQMinSumDecoder(code, bc, 8, qp, max_iterations=T, layered=True)
    for B, snr in ((1, 3.0), (37, 2.0), (130, 5.0)):
        llr = awgn(rng, B, tg.n, snr)
        llr[0, :3] = 0.0                                         # exact zeros
        if B > 2:
            llr[1] = np.round(llr[1])                            # ties
            llr[2] = np.abs(llr[2]) + 4.0                        # a codeword: stops after the first iteration
        x = torch.from_numpy(llr).to(gpu_device)
        eng = dec._get_engine(gpu_device)
        if engine_mode == "auto":
            assert eng.info()["engine"] == "resident" and eng.info()["threads_per_workgroup"] == 64
        else:
            assert eng.info()["engine"] == "stream"
        ob, op, oi, os_ = oracle_mod.rcq_layered(og, llr, bc, qp, T)
        res = eng.decode(x, early_stop=True, want_packed=True)
        np.testing.assert_array_equal(res.iterations.cpu().numpy(), oi)
        np.testing.assert_array_equal(res.success.cpu().numpy(), os_)
        np.testing.assert_array_equal(res.bits.cpu().numpy(), ob)
        np.testing.assert_array_equal(res.posterior.cpu().numpy(), op)
        packed = res.packed_bits.cpu().numpy()
        np.testing.assert_array_equal(((packed[:, :, None] >> np.arange(8)) & 1).reshape(B, -1)[:, :tg.n], ob)
        fix = eng.decode(x, early_stop=False)
        keep = ~os_                                              # never converged: the fixed-T walk is the same walk
        assert np.all(fix.iterations.cpu().numpy() == T)
        np.testing.assert_array_equal(fix.bits.cpu().numpy()[keep], ob[keep])
        np.testing.assert_array_equal(fix.posterior.cpu().numpy()[keep], op[keep])
        syn = (tg.syndrome(fix.bits.cpu().numpy()).any(axis=-1))
        np.testing.assert_array_equal(fix.success.cpu().numpy(), ~syn)
        if engine_mode == "auto":                                # bit for bit against the streaming kernel
            eng.set_mode("stream")
            try:
                ref = eng.decode(x, early_stop=True)
                ref_fix = eng.decode(x, early_stop=False)
            finally:
                eng.set_mode("auto")
            for a_, b_ in ((res, ref), (fix, ref_fix)):
                assert torch.equal(a_.bits, b_.bits) and torch.equal(a_.iterations, b_.iterations)
                assert torch.equal(a_.success, b_.success) and torch.equal(a_.posterior, b_.posterior)


def wide_check_code():
    """Checks far wider than a lane's slot row (degree 40, 64, 100, 33, 129) beside ordinary ones, variable degrees <= 8:
    the resident engine splits each wide check over a group of adjacent lanes (wavefront exchanges between the two
    passes), the streaming engine over the four waves of a block (partials through LDS).  Reference loop: any degree,
    ldpc_decoder.py:91-120."""
    from ldpc_decoder import LDPCCode
    rng = np.random.default_rng(2024)
    n, degs = 420, [129, 100, 64, 40, 33, 6, 6, 5, 7, 6, 6, 3, 1, 6, 6, 6, 16, 17, 32, 6, 6, 6, 6, 2]
    H = np.zeros((len(degs), n), dtype=np.int64)
    load = np.zeros(n, dtype=np.int64)
    for i, dc in enumerate(degs):
        free = np.flatnonzero(load < 8)
        pick = rng.choice(free, size=dc, replace=False)
        H[i, pick] = 1
        load[pick] += 1
    return LDPCCode(n=n, k=n - len(degs), H=H, max_iterations=8)


@pytest.mark.parametrize("early_stop", [True, False])
def test_wide_checks_split_over_lanes_and_waves(early_stop, gpu_device, oracle_mod, engine_mode):
    from ldpc_decoder import BasicMinSumDecoder
    from neural_2d_decoder import Neural2DMinSumDecoder, Neural2DOffsetMinSumDecoder
    from rcq_decoder import RCQMinSumDecoder, WeightedRCQDecoder
    code = wide_check_code()
    og = oracle_mod.OracleGraph(code.H)
    assert og.dc.max() == 129 and og.dv.max() <= 8
    rng = np.random.default_rng(5)
    B, T = 150, 8
    llr64 = rng.standard_normal((B, code.n)) * 2.5 + 1.2
    llr64[3, 7] = 0.0                                     # an exact zero inside a wide check (zero-aware OMS sign rule)
    llr64[5] = np.round(llr64[5])                         # ties
    llr = llr64.astype(np.float32)
    x = torch.from_numpy(llr).to(gpu_device)

    dec = BasicMinSumDecoder(code)
    if engine_mode == "auto":
        assert dec._engine(torch.float32, gpu_device).info()["engine"] == "resident"      # wide checks are admitted now
    for arr, dt in ((llr64, np.float64), (llr, np.float32)):
        bits, succ, iters = dec.decode(arr, early_stop=early_stop)
        ob, op, oi, os_ = oracle_mod.basic_minsum(og, arr, 0.7, T, early_stop=early_stop, dtype=dt)
        np.testing.assert_array_equal(iters, oi)
        np.testing.assert_array_equal(succ, os_)
        np.testing.assert_array_equal(bits, ob)

    for wtype in (1, 2):
        dec = Neural2DMinSumDecoder(code, weight_sharing_type=wtype, max_iterations=T)
        beta, alpha = rand_weights(dec, rng)
        bits, post, iters = dec(x, early_stop=early_stop)
        ob, op, oi, _ = oracle_mod.neural2d(og, llr, wtype, T, beta, alpha, early_stop=early_stop)
        np.testing.assert_array_equal(iters.cpu().numpy(), oi)
        np.testing.assert_array_equal(bits.cpu().numpy(), ob)
        assert_post(post.cpu().numpy(), op)

    dec = Neural2DOffsetMinSumDecoder(code, weight_sharing_type=2, max_iterations=T)
    with torch.no_grad():
        for p_ in dec.beta_weights.values():
            p_.fill_(float(np.float32(rng.uniform(0.0, 0.4))))
        for p_ in dec.alpha_weights.values():
            p_.fill_(float(np.float32(rng.uniform(0.0, 0.1))))
    beta = {k: float(v.item()) for k, v in dec.beta_weights.items()}
    alpha = {k: float(v.item()) for k, v in dec.alpha_weights.items()}
    bits, post, iters = dec(x, early_stop=early_stop)
    ob, op, oi, _ = oracle_mod.neural2d_offset(og, llr, 2, T, beta, alpha, early_stop=early_stop)
    np.testing.assert_array_equal(iters.cpu().numpy(), oi)
    np.testing.assert_array_equal(bits.cpu().numpy(), ob)
    assert_post(post.cpu().numpy(), op)

    dec = RCQMinSumDecoder(code, 3, 8, QP, max_iterations=T)
    bits, succ, iters = dec.decode(x, early_stop=early_stop)
    ob, op, oi, os_, oc = oracle_mod.rcq(og, llr, 3, QP, T, early_stop=early_stop, trace_codes=True)
    np.testing.assert_array_equal(iters.cpu().numpy(), oi)
    np.testing.assert_array_equal(succ.cpu().numpy(), os_)
    np.testing.assert_array_equal(bits.cpu().numpy(), ob)
    assert_codes(codes_of(dec, x, early_stop), final_codes(oc, oi), 4)

    dec = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=1, max_iterations=T)      # per-(dc,dv) beta: per-edge path
    beta, alpha = rand_weights(dec, rng)
    bits, post, iters = dec(x, early_stop=early_stop)
    ob, op, oi, _, oc = oracle_mod.weighted_rcq(og, llr, 3, QP, 1, T, beta, alpha, early_stop=early_stop, trace_codes=True)
    np.testing.assert_array_equal(iters.cpu().numpy(), oi)
    np.testing.assert_array_equal(bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(post.cpu().numpy(), op)
    assert_codes(codes_of(dec, x, early_stop), final_codes(oc, oi), 4)


@pytest.mark.parametrize("B", [1, 3, 64, 65])
def test_host_batches_take_the_staged_path_with_identical_results(B, gpu_device):
    """CPU inputs of at most 64 codewords (the reference's call shape) go through torch.ops.ldpc.decode_host -- one staged
    copy each way -- and give exactly what the device-resident path gives; larger host batches take the ordinary path"""
    import codes
    import torch_ops
    from ldpc_decoder import BasicMinSumDecoder
    from neural_2d_decoder import Neural2DMinSumDecoder
    from rcq_decoder import RCQMinSumDecoder
    code = codes.load_code("small_96_48", 8)
    rng = np.random.default_rng(B)
    llr = (rng.standard_normal((B, code.n)) * 2.0 + 1.5).astype(np.float32)
    x = torch.from_numpy(llr)
    n2d = Neural2DMinSumDecoder(code, 2, 8)
    rand_weights(n2d, rng)
    b_h, p_h, i_h = n2d(x)
    b_d, p_d, i_d = n2d(x.to(gpu_device))
    assert b_h.device.type == "cpu" and p_h.device.type == "cpu"
    assert torch.equal(b_h, b_d.cpu()) and torch.equal(p_h, p_d.cpu()) and torch.equal(i_h, i_d.cpu())
    rcq = RCQMinSumDecoder(code, 3, 8, QP, max_iterations=8)
    b_h, s_h, i_h = rcq.decode(x)
    b_d, s_d, i_d = rcq.decode(x.to(gpu_device))
    assert torch.equal(b_h, b_d.cpu()) and torch.equal(s_h, s_d.cpu()) and torch.equal(i_h, i_d.cpu())
    bas = BasicMinSumDecoder(code)
    for arr in (llr, llr.astype(np.float64)):
        b_h, s_h, i_h = bas.decode(arr)
        b_d, s_d, i_d = bas.decode(torch.from_numpy(arr).to(gpu_device))
        np.testing.assert_array_equal(b_h, b_d.cpu().numpy())
        np.testing.assert_array_equal(s_h, s_d.cpu().numpy())
        np.testing.assert_array_equal(i_h, i_d.cpu().numpy())
    if B <= 64:
        h = torch_ops.engine_handle(n2d._get_engine(gpu_device))
        torch.library.opcheck(torch.ops.ldpc.decode_host, (x, h, True, True))


def test_workspace_cache_is_bounded_and_host_staging_moves_only_the_batch(gpu_device, oracle_mod):
    """(1) the per-stream workspace cache of an engine is a small LRU -- a caller cycling through short-lived
    torch streams does not pile up one multi-GB buffer per stream; (2) decode_host lays its device block out for the ACTUAL
    batch (a one-codeword call copies ~2n words back, not the 64-row block) and still equals the device path; its staging
    lock is not the workspace lock."""
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    code = codes.load_code("small_96_48", 10)
    dec = BasicMinSumDecoder(code, 0.7)
    eng = dec._engine(torch.float32, gpu_device)
    eng.set_mode("stream")                               # the streaming engine is the one with a real workspace
    rng = np.random.default_rng(3)
    llr = awgn(rng, 70, code.n, 3.0)
    x = torch.from_numpy(llr).to(gpu_device)
    want = eng.decode(x)
    keep = []
    for _ in range(3 * eng._WS_MAX):
        st = torch.cuda.Stream(device=gpu_device)
        keep.append(st)
        st.wait_stream(torch.cuda.current_stream(gpu_device))
        with torch.cuda.stream(st):
            got = eng.decode(x)
        st.synchronize()
        assert torch.equal(got.bits, want.bits) and torch.equal(got.iterations, want.iterations)
        assert len(eng._ws) <= eng._WS_MAX
    assert len(eng._ws) == eng._WS_MAX
    eng.set_mode("auto")
    assert eng._host_lock is not eng._ws_lock
    for B in (1, 5, 64):
        bits, post, iters, succ = eng.decode_host(torch.from_numpy(llr[:B]), want_posterior=True)
        dev = eng.decode(x[:B])
        assert torch.equal(bits, dev.bits.cpu()) and torch.equal(iters, dev.iterations.cpu()) and torch.equal(succ, dev.success.cpu())
        assert torch.equal(post, dev.posterior.cpu())
        bits2, post2, iters2, _ = eng.decode_host(torch.from_numpy(llr[:B]), want_posterior=False)
        assert post2 is None and torch.equal(bits2, bits) and torch.equal(iters2, iters)


def sparse_odd_code():
    """14x40 sparse code that QUALIFIES for the LDS-resident engine (dc <= 32, dv <= 8) and still has a
    degree-1 check, an empty check, an isolated variable and a degree-1 variable"""
    from ldpc_decoder import LDPCCode
    rng = np.random.default_rng(21)
    H = (rng.random((14, 40)) < 0.12).astype(np.int64)
    H[12, :] = 0; H[12, 7] = 1          # degree-1 check
    H[13, :] = 0                        # empty check
    H[:, 39] = 0                        # isolated variable
    H[:, 38] = 0; H[3, 38] = 1          # degree-1 variable
    assert H.sum(axis=0).max() <= 8
    return LDPCCode(n=40, k=26, H=H, max_iterations=5)


@pytest.mark.parametrize("T", [0, 1, 2, 5])
@pytest.mark.parametrize("B", [1, 2, 3, 130])
def test_resident_engine_edge_cases(T, B, gpu_device, oracle_mod, engine_mode):
    """iteration counts 0/1/2, odd batches (padding codeword inside a workgroup), degenerate nodes --
    on a code the resident engine accepts (so 'auto' really exercises it)"""
    from neural_2d_decoder import Neural2DMinSumDecoder, Neural2DOffsetMinSumDecoder
    from rcq_decoder import WeightedRCQDecoder
    from weight_sharing import SharingLayout
    code = sparse_odd_code()
    og = oracle_mod.OracleGraph(code.H)
    rng = np.random.default_rng(100 * T + B)
    llr = (rng.standard_normal((B, 40)) * 3).astype(np.float32)
    llr[0, 5] = 0.0
    if B > 2:
        llr[2] = np.round(llr[2])
        llr[1] = np.abs(llr[1]) + 4.0                    # converges at once: early-stop emit at iteration 1
    x = torch.from_numpy(llr).to(gpu_device)
    for early in (True, False):
        dec = Neural2DMinSumDecoder(code, weight_sharing_type=1, max_iterations=T)
        beta, alpha = rand_weights(dec, rng)
        bits, post, iters = dec(x, early_stop=early)
        if engine_mode == "auto":
            assert dec._engine.info()["engine"] == "resident"
        ob, op, oi, _ = oracle_mod.neural2d(og, llr, 1, T, beta, alpha, early_stop=early)
        np.testing.assert_array_equal(iters.detach().cpu().numpy(), oi)
        np.testing.assert_array_equal(bits.detach().cpu().numpy(), ob)
        assert_post(post.detach().cpu().numpy(), op)
        res = dec._engine.decode(x, early_stop=early, want_packed=True)
        osucc = oracle_mod.neural2d(og, llr, 1, T, beta, alpha, early_stop=early)[3]
        np.testing.assert_array_equal(res.success.detach().cpu().numpy(), osucc)
        unpacked = ((res.packed_bits.detach().cpu().numpy()[:, :, None] >> np.arange(8)) & 1).reshape(B, -1)[:, :40]
        np.testing.assert_array_equal(unpacked, ob)

        w = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=2, max_iterations=T)
        beta, alpha = rand_weights(w, rng)
        bits, post, iters = w(x, early_stop=early)
        ob, op, oi, _ = oracle_mod.weighted_rcq(og, llr, 3, QP, 2, T, beta, alpha, early_stop=early)
        np.testing.assert_array_equal(iters.detach().cpu().numpy(), oi)
        np.testing.assert_array_equal(bits.detach().cpu().numpy(), ob)
        np.testing.assert_array_equal(post.detach().cpu().numpy(), op)

        o = Neural2DOffsetMinSumDecoder(code, weight_sharing_type=2, max_iterations=T)
        with torch.no_grad():
            for p in o.beta_weights.values():
                p.fill_(float(np.float32(rng.uniform(0.0, 0.6))))
            for p in o.alpha_weights.values():
                p.fill_(float(np.float32(rng.uniform(0.0, 0.3))))
        bits, post, iters = o(x, early_stop=early)
        ob, op, oi, _ = oracle_mod.neural2d_offset(og, llr, 2, T, {k: float(v.item()) for k, v in o.beta_weights.items()},
                                                   {k: float(v.item()) for k, v in o.alpha_weights.items()}, early_stop=early)
        np.testing.assert_array_equal(iters.detach().cpu().numpy(), oi)
        np.testing.assert_array_equal(bits.detach().cpu().numpy(), ob)
        assert_post(post.detach().cpu().numpy(), op)


def test_error_behaviour(gpu_device):
    from ldpc_decoder import BasicMinSumDecoder, create_test_ldpc_code
    from neural_2d_decoder import Neural2DMinSumDecoder
    from rcq_decoder import RCQMinSumDecoder
    code = create_test_ldpc_code()
    with pytest.raises(ValueError):
        Neural2DMinSumDecoder(code, weight_sharing_type=5, max_iterations=3)      # neural_2d_decoder.py:82
    with pytest.raises(ValueError):
        BasicMinSumDecoder(code).decode(np.zeros(6))
    from ldpc_decoder import LDPCCode
    one_check = LDPCCode(n=4, k=3, H=np.ones((1, 4), dtype=int), max_iterations=3)
    with pytest.raises(NotImplementedError):         # the only case where the reference's layered subtraction is real
        RCQMinSumDecoder(one_check, 3, 8, QP, 3, layered=True).decode(torch.zeros(4))
    with pytest.raises(TypeError):
        RCQMinSumDecoder(code, 3, 8, QP, 10).decode(np.zeros(7))
    # empty batch
    b, s, i = BasicMinSumDecoder(code).decode(np.zeros((0, 7)))
    assert b.shape == (0, 7) and s.shape == (0,) and i.shape == (0,)


@pytest.mark.parametrize("which", ["neural2d", "wrcq", "offset", "edge"])
def test_weight_update_is_picked_up(which, gpu_device, oracle_mod):
    """parameters changed after the first forward reach the GPU tables, whichever way they were changed: the cases of
    tests/test_host_logic.py (in-place updates, the four writes through `.data`, replaced storage -- twice, so that the
    first address can come back --, a replaced Parameter, load_state_dict, an optimizer step), each decoded and compared
    with the oracle run on the new values; a decode with nothing changed uploads nothing"""
    import codes
    from test_host_logic import WEIGHT_CHANGES, weight_change_decoders
    rng = np.random.default_rng(3)
    T = 6
    code = codes.load_code("small_96_48", 10)
    og = oracle_mod.OracleGraph(code.H)
    dec = weight_change_decoders(code, T)[which]()
    llr = awgn(rng, 70, 96, 2.5)
    x = torch.from_numpy(llr).to(gpu_device)
    items = lambda d: {k: float(v.item()) for k, v in d.items()}

    def check():
        bits, post, iters = dec(x)
        if which == "neural2d":
            ob, op, oi, _ = oracle_mod.neural2d(og, llr, 2, T, items(dec.beta_weights), items(dec.alpha_weights))
        elif which == "wrcq":
            ob, op, oi, _ = oracle_mod.weighted_rcq(og, llr, 3, QP, 3, T, items(dec.beta_weights), items(dec.alpha_weights))
        elif which == "offset":
            ob, op, oi, _ = oracle_mod.neural2d_offset(og, llr, 2, T, items(dec.beta_weights), items(dec.alpha_weights))
        else:
            ob, op, oi, _ = oracle_mod.neural_minsum(og, llr, T, items(dec.beta_weights))
        np.testing.assert_array_equal(bits.detach().cpu().numpy(), ob)
        np.testing.assert_array_equal(iters.detach().cpu().numpy(), oi)
        if which == "wrcq":
            np.testing.assert_array_equal(post.detach().cpu().numpy(), op)
        else:
            assert_post(post.detach().cpu().numpy(), op)
        return op

    ranges = {"offset": ((0.0, 0.4), (0.0, 0.1))}.get(which, ((0.5, 1.0), (0.8, 1.2)))   # as rand_weights / the offset tests draw them
    for _ in range(2):
        with torch.no_grad():                                             # in-place fill_ (version counter)
            for params, (lo, hi) in zip((dec.beta_weights, getattr(dec, "alpha_weights", {})), ranges):
                for p in params.values():
                    p.fill_(float(np.float32(rng.uniform(lo, hi))))
        check()
    k0 = sorted(dec.beta_weights.keys())[0]
    eng = dec._engine
    uploads = []
    upload = eng.set_weights
    eng.set_weights = lambda *a, **kw: (uploads.append(1), upload(*a, **kw))[1]
    check()
    assert not uploads
    for n_changes, (name, change) in enumerate(WEIGHT_CHANGES, 1):
        change(dec, k0)
        check()                                                           # the oracle with the new values
        assert dec._engine is eng and len(uploads) == n_changes, name
    check()                                                               # nothing changed: no upload, same results
    assert len(uploads) == len(WEIGHT_CHANGES)


def test_packed_bits_and_threads(gpu_device):
    """packed wire format == bits; decoder instances driven from worker threads (the
    reference's ThreadPoolExecutor usage, simulation_framework.py:194-198)"""
    import codes
    from concurrent.futures import ThreadPoolExecutor
    from rcq_decoder import RCQMinSumDecoder
    rng = np.random.default_rng(8)
    code = codes.load_code("small_96_48", 10)
    llr = torch.from_numpy(awgn(rng, 500, 96, 3.0)).to(gpu_device)
    dec = RCQMinSumDecoder(code, 3, 8, QP, 10)
    ref_bits, _, _ = dec.decode(llr)
    res = dec._engine.decode(llr, want_packed=True, want_posterior=False)
    unpacked = ((res.packed_bits.detach().cpu().numpy()[:, :, None] >> np.arange(8)) & 1).reshape(500, -1)[:, :96]
    np.testing.assert_array_equal(unpacked, ref_bits.detach().cpu().numpy())

    def work(seed):
        d = RCQMinSumDecoder(code, 3, 8, QP, 10)
        return d.decode(llr)[0].detach().cpu().numpy()
    with ThreadPoolExecutor(4) as ex:
        outs = list(ex.map(work, range(4)))
    for o in outs:
        np.testing.assert_array_equal(o, ref_bits.detach().cpu().numpy())


@pytest.mark.parametrize("early_stop", [True, False])
def test_capped_decode(early_stop, gpu_device, oracle_mod, engine_mode):
    """ldpc_decode_capped: at most c of the decoder's iterations, iteration t with the decoder's own tables of iteration t.
    Basic (no per-iteration tables) equals the CPU restatement run with T = c; for every decoder a codeword that stops within
    the cap has the full decode's outputs, one still open reports iterations = c, success = False, and the posterior after c
    iterations (fixed T: equal to the first c iterations of the full schedule, checked through Basic).  Every engine form."""
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    from neural_2d_decoder import Neural2DMinSumDecoder
    from rcq_decoder import RCQMinSumDecoder
    rng = np.random.default_rng(12)
    code = codes.load_code("small_96_48", 10)
    g = code.tanner_graph()
    og = oracle_mod.OracleGraph(n=g.n, check_ptr=g.check_ptr, var_idx=g.var_idx)
    llr = awgn(rng, 300, code.n, 3.0)
    x = torch.from_numpy(llr).to(gpu_device)
    n2d = Neural2DMinSumDecoder(code, 2, 10)
    rand_weights(n2d, rng)
    engines = {"basic": BasicMinSumDecoder(code, 0.7)._engine(torch.float32, gpu_device),
               "rcq": RCQMinSumDecoder(code, 3, 8, QP, 10)._get_engine(gpu_device) if hasattr(RCQMinSumDecoder, "_get_engine") else None,
               "neural2d": n2d._get_engine(gpu_device)}
    if engines["rcq"] is None:
        dec = RCQMinSumDecoder(code, 3, 8, QP, 10)
        dec.decode(x[:2])
        engines["rcq"] = dec._engine
    for name, eng in engines.items():
        full = eng.decode(x, early_stop=early_stop)
        for c in (1, 3, 10, 25):
            part = eng.decode(x, early_stop=early_stop, max_iters=c)
            if c >= 10:                                               # a cap at or above T changes nothing
                assert torch.equal(part.bits, full.bits) and torch.equal(part.iterations, full.iterations)
                assert torch.equal(part.success, full.success) and torch.equal(part.posterior, full.posterior)
                continue
            if early_stop:
                inside = full.success & (full.iterations <= c)
                assert torch.equal(part.success, inside)
                assert torch.equal(part.bits[inside], full.bits[inside]) and torch.equal(part.posterior[inside], full.posterior[inside])
                assert torch.equal(part.iterations[inside], full.iterations[inside])
                assert bool((part.iterations[~inside] == c).all())
            else:
                assert bool((part.iterations == c).all())
            if name == "basic":
                ob, op, oi, os_ = oracle_mod.basic_minsum(og, llr, 0.7, c, early_stop=early_stop, dtype=np.float32)
                np.testing.assert_array_equal(part.bits.cpu().numpy(), ob)
                np.testing.assert_array_equal(part.iterations.cpu().numpy(), oi)
                np.testing.assert_array_equal(part.success.cpu().numpy(), os_)
                assert_post(part.posterior.cpu().numpy(), op)
        # packed decisions only (what the Monte-Carlo driver asks for): no int32 rows, no posterior rows, same decisions
        only = eng.decode(x, early_stop=early_stop, want_bits=False, want_posterior=False, want_packed=True)
        both = eng.decode(x, early_stop=early_stop, want_packed=True)
        assert only.bits is None and only.posterior is None
        assert torch.equal(only.packed_bits, both.packed_bits) and torch.equal(only.iterations, full.iterations)
        assert torch.equal(only.success, full.success)
        unpacked = ((only.packed_bits.cpu().numpy()[:, :, None] >> np.arange(8)) & 1).reshape(len(llr), -1)[:, :code.n]
        np.testing.assert_array_equal(unpacked, full.bits.cpu().numpy())
    with pytest.raises(Exception):
        engines["basic"].decode(x, max_iters=0)


def test_decode_is_capturable_in_a_hip_graph(gpu_device, engine_mode):
    """ldpc_decode only enqueues work on the caller's stream (no allocation, no synchronisation), so a launch-bound
    caller can capture it once and replay it: replays on new inputs equal eager decodes"""
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    code = codes.load_code("small_96_48", max_iterations=6)
    eng = BasicMinSumDecoder(code, 0.7)._engine(torch.float32, gpu_device)
    gen = torch.Generator(device=gpu_device).manual_seed(77)
    x_static = torch.randn(200, code.n, device=gpu_device, generator=gen) * 2 + 1.5
    eng.decode(x_static)                                   # warm-up: workspace allocation, kernel attributes
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        eng.decode(x_static)
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = eng.decode(x_static, early_stop=True)
    for trial in range(3):
        x_new = torch.randn(200, code.n, device=gpu_device, generator=gen) * 2 + 1.0 + 0.3 * trial
        x_static.copy_(x_new)
        graph.replay()
        torch.cuda.synchronize()
        got = (res.bits.clone(), res.posterior.clone(), res.iterations.clone(), res.success.clone())
        ref = eng.decode(x_new, early_stop=True)
        assert torch.equal(got[0], ref.bits) and torch.equal(got[1], ref.posterior)
        assert torch.equal(got[2], ref.iterations)


def test_fp64_basic_runs_on_the_resident_engine_with_identical_results(gpu_device, monkeypatch):
    """BasicMinSumDecoder with the reference's own float64 LLRs: one fp64 codeword per workgroup in the slots of a
    float pair; bits / iterations / success equal the golden vectors, posteriors equal the streaming engine's bit for bit"""
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    monkeypatch.setenv("LDPC_ENGINE_MODE", "auto")
    gold = load_golden("ira_basic")
    code = codes.load_code("ira_1998_1512", max_iterations=int(gold["T"]) if "T" in gold else 10)
    dec = BasicMinSumDecoder(code, 0.7)
    eng = dec._engine(torch.float64, gpu_device)
    assert eng.info()["engine"] == "resident" and eng.info()["codewords_per_workgroup"] == 1
    llr = torch.from_numpy(np.asarray(gold["llr"], dtype=np.float64)).to(gpu_device)
    for early in (True, False):
        eng.set_mode("auto")
        a = eng.decode(llr, early_stop=early, want_packed=True)
        eng.set_mode("stream")
        b = eng.decode(llr, early_stop=early, want_packed=True)
        assert torch.equal(a.bits, b.bits) and torch.equal(a.iterations, b.iterations) and torch.equal(a.success, b.success)
        assert torch.equal(a.posterior, b.posterior) and torch.equal(a.packed_bits, b.packed_bits)
        if early:
            np.testing.assert_array_equal(a.bits.cpu().numpy(), gold["bits"].astype(np.int32))
            np.testing.assert_array_equal(a.iterations.cpu().numpy(), gold["iters"])


def _random_code(rng, T):
    """random sparse graph the resident engine accepts: check degrees 1..20, variable degrees <= 8, now and then a
    degree-0 check or variable -- and in a third of the graphs a few WIDE checks (33..150 edges: lane-group split in the
    resident engine, wave split in the streaming engine)"""
    from ldpc_decoder import LDPCCode
    m = int(rng.integers(4, 60))
    n = int(rng.integers(m + 3, 160))
    H = np.zeros((m, n), dtype=np.int64)
    room = np.full(n, 8)
    wide = set(rng.choice(m, size=int(rng.integers(1, 4)), replace=False).tolist()) if (n > 40 and rng.random() < 0.33) else set()
    for i in range(m):
        if i in wide:
            dc = int(rng.integers(33, min(150, n) + 1))
        else:
            dc = int(rng.integers(0 if rng.random() < 0.05 else 1, min(20, n) + 1))
        cand = np.flatnonzero(room > 0)
        pick = rng.choice(cand, size=min(dc, len(cand)), replace=False)
        H[i, pick] = 1
        room[pick] -= 1
    return LDPCCode(n=n, k=max(n - m, 1), H=H, max_iterations=T)


import os as _os
_FUZZ_SEEDS = int(_os.environ.get("LDPC_FUZZ_SEEDS", "12"))     # LDPC_FUZZ_SEEDS widens the campaign


@pytest.mark.parametrize("seed", range(_FUZZ_SEEDS))
def test_random_graphs_engines_agree_with_the_oracle(seed, gpu_device, oracle_mod):
    """property test over random Tanner graphs: for every decoder form the resident engine, the streaming engine and the
    CPU oracle give the same bits / iterations / success (and the two engines bit-identical posteriors)"""
    from ldpc_decoder import BasicMinSumDecoder
    from neural_2d_decoder import Neural2DMinSumDecoder, Neural2DOffsetMinSumDecoder
    from rcq_decoder import WeightedRCQDecoder
    rng = np.random.default_rng(1000 + seed)
    T = int(rng.integers(1, 7))
    code = _random_code(rng, T)
    og = oracle_mod.OracleGraph(code.H)
    B = int(rng.integers(1, 150))
    llr = (rng.standard_normal((B, code.n)) * 2.5 + 1.0).astype(np.float32)
    llr[rng.random(llr.shape) < 0.01] = 0.0                     # exact zeros
    if B > 3:
        llr[1] = np.round(llr[1])                               # ties
        llr[2] = np.abs(llr[2]) + 3.0                           # stops at once
    x = torch.from_numpy(llr).to(gpu_device)
    early = bool(seed % 2 == 0)

    def both_engines(eng, inp):
        eng.set_mode("auto")
        assert eng.info()["engine"] == "resident"
        a = eng.decode(inp, early_stop=early, want_packed=True)
        for mode in ("stream", "sweeps", "gather", "pair"):
            try:
                eng.set_mode(mode)
            except NotImplementedError:
                assert mode in ("gather", "pair")               # the RCQ-only forms
                continue
            b = eng.decode(inp, early_stop=early, want_packed=True)
            assert torch.equal(a.bits, b.bits) and torch.equal(a.iterations, b.iterations) and torch.equal(a.success, b.success)
            assert torch.equal(a.posterior, b.posterior) and torch.equal(a.packed_bits, b.packed_bits)
        return a

    wtype = int(rng.integers(1, 5))
    dec = Neural2DMinSumDecoder(code, weight_sharing_type=wtype, max_iterations=T)
    beta, alpha = rand_weights(dec, rng)
    a = both_engines(dec._get_engine(gpu_device), x)
    ob, op, oi, osucc = oracle_mod.neural2d(og, llr, wtype, T, beta, alpha, early_stop=early)
    np.testing.assert_array_equal(a.bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(a.iterations.cpu().numpy(), oi)
    np.testing.assert_array_equal(a.success.cpu().numpy(), osucc)
    assert_post(a.posterior.cpu().numpy(), op)

    w = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=2, max_iterations=T)
    beta, alpha = rand_weights(w, rng)
    a = both_engines(w._get_engine(gpu_device), x)
    ob, op, oi, osucc = oracle_mod.weighted_rcq(og, llr, 3, QP, 2, T, beta, alpha, early_stop=early)
    np.testing.assert_array_equal(a.bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(a.iterations.cpu().numpy(), oi)
    np.testing.assert_array_equal(a.posterior.cpu().numpy(), op)

    o = Neural2DOffsetMinSumDecoder(code, weight_sharing_type=2, max_iterations=T)
    with torch.no_grad():
        for p in o.beta_weights.values():
            p.fill_(float(np.float32(rng.uniform(0.0, 0.6))))
        for p in o.alpha_weights.values():
            p.fill_(float(np.float32(rng.uniform(0.0, 0.3))))
    a = both_engines(o._get_engine(gpu_device), x)
    ob, op, oi, _ = oracle_mod.neural2d_offset(og, llr, 2, T, {k: float(v.item()) for k, v in o.beta_weights.items()},
                                               {k: float(v.item()) for k, v in o.alpha_weights.items()}, early_stop=early)
    np.testing.assert_array_equal(a.bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(a.iterations.cpu().numpy(), oi)

    # the reference's layered schedule: LDS-resident layered kernel == streaming kernel == oracle (which restates the early-stop
    # form; a fixed-T run is compared between the two kernels only)
    if code.H.shape[0] > 1 and int(code.H.sum(axis=1).max()) >= 1:
        from rcq_decoder import RCQMinSumDecoder
        lay = RCQMinSumDecoder(code, 3, 8, QP, max_iterations=T, layered=True)
        le = lay._get_engine(gpu_device)
        le.set_mode("auto")
        a = le.decode(x, early_stop=early, want_packed=True)
        le.set_mode("stream")
        b = le.decode(x, early_stop=early, want_packed=True)
        assert torch.equal(a.bits, b.bits) and torch.equal(a.iterations, b.iterations) and torch.equal(a.success, b.success)
        assert torch.equal(a.posterior, b.posterior) and torch.equal(a.packed_bits, b.packed_bits)
        if early:
            ob, op, oi, osucc = oracle_mod.rcq_layered(og, llr, 3, QP, T)
            np.testing.assert_array_equal(a.bits.cpu().numpy(), ob)
            np.testing.assert_array_equal(a.iterations.cpu().numpy(), oi)
            np.testing.assert_array_equal(a.success.cpu().numpy(), osucc)
            np.testing.assert_array_equal(a.posterior.cpu().numpy(), op)

    basic = BasicMinSumDecoder(code, 0.7)                       # the reference's float64 decoder, resident fp64 kernel
    x64 = torch.from_numpy(llr.astype(np.float64)).to(gpu_device)
    a = both_engines(basic._engine(torch.float64, gpu_device), x64)
    ob, op, oi, osucc = oracle_mod.basic_minsum(og, llr.astype(np.float64), 0.7, T, early_stop=early)
    np.testing.assert_array_equal(a.bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(a.iterations.cpu().numpy(), oi)
    np.testing.assert_array_equal(a.success.cpu().numpy(), osucc)
