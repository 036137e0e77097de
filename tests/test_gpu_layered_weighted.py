"""
WeightedRCQDecoder(layered="paper") (-m gpu): the weighted layered RCQ decode of the paper (rcq_decoder.py module
docstring), on the LDS-resident kernel (layered_paper_lds, ldpc_layered.hip) and the HBM-streaming one
(layered_rcq<VEC, true>, LDPC_ENGINE_MODE=stream).  Nothing in the reference executes this schedule: the yardstick is
the numpy restatement below, vectorised over the batch, one check at a time, in the fp32 order of the flooding W-RCQ
check update (oracle/ldpc_oracle_impl.h: w = (beta * prod(sign(others))) * min_others, sign(0) = 0, first minimum is
the arg-min, ties keep min2 == min1) and the subtraction order of oracle.rcq_layered(paper=True).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

QP = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]


@pytest.fixture(autouse=True)
def inference_mode():
    with torch.no_grad():
        yield


def awgn(rng, B, n, snr_db):
    s2 = 10.0 ** (-snr_db / 10.0)
    return (2.0 * (1.0 + np.sqrt(s2) * rng.standard_normal((B, n))) / s2).astype(np.float32)


def wide_check_code():
    """checks of degree 129, 100, 64, ... beside ordinary ones: wider than a wavefront, so the streaming kernel runs"""
    from ldpc_decoder import LDPCCode
    rng = np.random.default_rng(2024)
    n, degs = 420, [129, 100, 64, 40, 33, 6, 6, 5, 7, 6, 6, 3, 1, 6, 6, 6, 16, 17, 32, 6, 6, 6, 6, 2]
    H = np.zeros((len(degs), n), dtype=np.int64)
    load = np.zeros(n, dtype=np.int64)
    for i, dc in enumerate(degs):
        pick = rng.choice(np.flatnonzero(load < 8), size=dc, replace=False)
        H[i, pick] = 1
        load[pick] += 1
    return LDPCCode(n=n, k=n - len(degs), H=H, max_iterations=8)


def load(name, T):
    import codes
    from ldpc_decoder import create_test_ldpc_code
    if name == "toy":
        return create_test_ldpc_code()
    if name == "wide":
        return wide_check_code()
    return codes.load_code(name, T)


def thresholds(bc, qp):
    top = 2 ** (bc - 1) - 1
    return np.asarray([[c * (j / top) ** g for j in range(top + 1)] for c, g in qp], dtype=np.float32)


def q_schedule(nq, T):
    if nq == 1:
        return [0] * T
    return [0 if t < T // 3 else (1 if t < 2 * T // 3 else nq - 1) for t in range(T)]


def edge_betas(dec, T):
    """beta_t of every CSR edge straight from the parameter dict by the reference's key names (default 0.7)"""
    g = dec.code.tanner_graph()
    dc = g.dc[g.check_of_edge]
    dv = g.dv[g.var_idx]
    typ = dec.weight_sharing_type
    out = np.full((T, g.E), 0.7, dtype=np.float32)
    for t in range(T):
        for e in range(g.E):
            key = (f"iter_{t}_dc{dc[e]}_dv{dv[e]}" if typ == 1 else f"iter_{t}_dc{dc[e]}" if typ in (2, 3) else None)
            if key is not None and key in dec.beta_weights:
                out[t, e] = np.float32(dec.beta_weights[key].item())
    return out


def restate(code, llr, bc, qp, T, beta_e, early_stop=True, want_messages=False, max_iters=None):
    """the paper's layered W-RCQ decode (module docstring of rcq_decoder.py): -> bits, posteriors, iterations, success
    (want_messages: and the code (w < 0) * L + level every edge holds when its codeword's decode ends, 255 = no message;
    max_iters: run at most that many of the T iterations, an open codeword then reports iterations = max_iters)"""
    g = code.tanner_graph()
    thr = thresholds(bc, qp)
    sched = q_schedule(len(qp), T)
    L = thr.shape[1]
    P = np.array(llr, dtype=np.float32, copy=True)
    B = P.shape[0]
    R = np.zeros((B, g.E), dtype=np.float32)          # reconstructed previous message of every edge ("none" = 0)
    K = np.full((B, g.E), 255, dtype=np.int64)
    open_ = np.ones(B, dtype=bool)
    T_run = T if max_iters is None else min(T, int(max_iters))
    iters = np.full(B, T_run, dtype=np.int32)
    succ = np.zeros(B, dtype=bool)
    cp, vi = g.check_ptr, g.var_idx

    def unsat(P_):
        hard = (P_ < 0).astype(np.int64)
        par = np.zeros(P_.shape[0], dtype=np.int64)
        for i in range(g.m):
            par |= hard[:, vi[cp[i]:cp[i + 1]]].sum(axis=1) & 1
        return par.astype(bool)

    for t in range(T_run):
        rows = np.flatnonzero(open_)
        if rows.size == 0:
            break
        th = thr[sched[t]]
        for i in range(g.m):
            e0, e1 = int(cp[i]), int(cp[i + 1])
            dc = e1 - e0
            if dc == 0:
                continue
            V = vi[e0:e1]
            u = P[np.ix_(rows, V)] - R[rows, e0:e1]
            sg = np.sign(u).astype(np.float32)
            mg = np.abs(u)
            k = np.argmin(mg, axis=1)
            m1 = mg[np.arange(rows.size), k]
            if dc > 1:
                other = mg.copy()
                other[np.arange(rows.size), k] = np.inf
                m2 = other.min(axis=1)
            else:
                m2 = m1
            zeros = (sg == 0).sum(axis=1, keepdims=True) - (sg == 0)
            negs = (sg < 0).sum(axis=1, keepdims=True) - (sg < 0)
            prod = np.where(zeros > 0, np.float32(0), np.where(negs % 2 == 1, np.float32(-1), np.float32(1))).astype(np.float32)
            raw = np.where(np.arange(dc)[None, :] == k[:, None], m2[:, None], m1[:, None]).astype(np.float32)
            w = (beta_e[t, e0:e1][None, :] * prod) * raw
            mag = np.abs(w)
            lvl = np.zeros(w.shape, dtype=np.int64)
            for q in range(L):
                lvl = np.where(mag >= th[q], q, lvl)
            rec = (np.float32(1) - np.float32(2) * (w < 0).astype(np.float32)) * th[lvl]
            P[np.ix_(rows, V)] = u + rec
            R[rows, e0:e1] = rec
            K[rows, e0:e1] = (w < 0) * L + lvl
        bad = unsat(P)
        if early_stop:
            done = open_ & ~bad
            iters[done] = t + 1
            succ[done] = True
            open_ &= bad
    if not early_stop:
        succ = ~unsat(P)
    out = (P < 0).astype(np.int32), P, iters, succ
    return out + (K,) if want_messages else out


def randomise_betas(dec, rng, zero_neg=True):
    """seeded init plus a perturbation; some zero and some negative entries"""
    with torch.no_grad():
        for k, p in dec.beta_weights.items():
            v = float(p.item()) + rng.uniform(-0.3, 0.3)
            r = rng.uniform()
            if zero_neg and r < 0.08:
                v = 0.0
            elif zero_neg and r < 0.16:
                v = -abs(v)
            p.fill_(float(np.float32(v)))


def run(dec, x, early_stop, mode, monkeypatch):
    monkeypatch.setenv("LDPC_ENGINE_MODE", mode)
    dec._engine = None                                  # a fresh engine reads the mode
    bits, post, iters = dec(x, early_stop=early_stop)
    return dec._engine, bits.cpu().numpy(), post.cpu().numpy(), iters.cpu().numpy()


CODES = [("toy", 40, 10, 2.5), ("small_96_48", 130, 10, 2.0), ("ira_1998_1512", 100, 10, 5.0), ("wide", 70, 6, 3.0)]


@pytest.mark.parametrize("wtype", [1, 2, 3, 4])
@pytest.mark.parametrize("mode", ["auto", "stream"])
def test_weighted_layered_vs_restatement(wtype, mode, gpu_device, monkeypatch):
    """every sharing type, random betas with zeros and negatives, every code form (the wide code runs the streaming
    kernel under both modes): bits, iterations, success, posteriors equal; fixed-T rows that never converge equal"""
    from rcq_decoder import WeightedRCQDecoder
    rng = np.random.default_rng(100 + wtype)
    for name, B, T, snr in CODES:
        code = load(name, T)
        dec = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=wtype, max_iterations=T, layered="paper")
        randomise_betas(dec, rng)
        llr = awgn(rng, B, code.n, snr)
        llr[0, :3] = 0.0                                 # exact zeros: sign(0)
        llr[1] = np.round(llr[1])                        # ties
        x = torch.from_numpy(llr).to(gpu_device)
        eng, bits, post, iters = run(dec, x, True, mode, monkeypatch)
        lds = eng.info()["kernel"] == "layered_paper_lds"
        assert lds == (mode == "auto" and name != "wide"), (name, mode, eng.info())
        beta_e = edge_betas(dec, T)
        ob, op, oi, os_ = restate(code, llr, 3, QP, T, beta_e)
        np.testing.assert_array_equal(iters, oi, err_msg=name)
        np.testing.assert_array_equal(bits, ob, err_msg=name)
        np.testing.assert_array_equal(post, op, err_msg=name)
        res = eng.decode(x, early_stop=True)
        np.testing.assert_array_equal(res.success.cpu().numpy(), os_, err_msg=name)
        _, fbits, fpost, fiters = run(dec, x, False, mode, monkeypatch)
        keep = ~os_
        assert np.all(fiters == T)
        np.testing.assert_array_equal(fbits[keep], ob[keep], err_msg=name)
        np.testing.assert_array_equal(fpost[keep], op[keep], err_msg=name)


@pytest.mark.parametrize("mode", ["auto", "stream"])
def test_unit_beta_equals_unweighted_paper_schedule_and_oracle(mode, gpu_device, oracle_mod, monkeypatch):
    """beta == 1 everywhere: bit-identical to RCQMinSumDecoder(layered="paper") and oracle.rcq_layered(paper=True)"""
    from rcq_decoder import RCQMinSumDecoder, WeightedRCQDecoder
    rng = np.random.default_rng(7)
    monkeypatch.setenv("LDPC_ENGINE_MODE", mode)
    for name, B, T, snr in CODES:
        code = load(name, T)
        tg = code.tanner_graph()
        og = oracle_mod.OracleGraph(n=tg.n, check_ptr=tg.check_ptr, var_idx=tg.var_idx)
        w = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=2, max_iterations=T, layered="paper")
        with torch.no_grad():
            for p in w.beta_weights.values():
                p.fill_(1.0)
        llr = awgn(rng, B, tg.n, snr)
        llr[0, :3] = 0.0
        x = torch.from_numpy(llr).to(gpu_device)
        bits, post, iters = w(x)
        u = RCQMinSumDecoder(code, 3, 8, QP, max_iterations=T, layered="paper")
        ub, us, ui = u.decode(x)
        ures = u._engine.decode(x, early_stop=True)
        ob, op, oi, os_ = oracle_mod.rcq_layered(og, llr, 3, QP, T, paper=True)
        for got, want in ((bits, ub), (iters, ui), (post, ures.posterior)):
            np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy(), err_msg=name)
        np.testing.assert_array_equal(bits.cpu().numpy(), ob, err_msg=name)
        np.testing.assert_array_equal(iters.cpu().numpy(), oi, err_msg=name)
        np.testing.assert_array_equal(post.cpu().numpy(), op, err_msg=name)
        np.testing.assert_array_equal(us.cpu().numpy(), os_, err_msg=name)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 4097])
def test_lds_and_streaming_kernels_agree(B, gpu_device, monkeypatch):
    """both decoders, stream vs auto, bit for bit, both stop modes, ragged batches on (1998,1512)"""
    from rcq_decoder import RCQMinSumDecoder, WeightedRCQDecoder
    rng = np.random.default_rng(B)
    code = load("ira_1998_1512", 10)
    llr = np.concatenate([awgn(rng, B - B // 2, code.n, 4.5), awgn(rng, B // 2, code.n, 6.0)])
    x = torch.from_numpy(llr).to(gpu_device)
    w = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=1, max_iterations=10, layered="paper")
    randomise_betas(w, rng)
    u = RCQMinSumDecoder(code, 3, 8, QP, max_iterations=10, layered="paper")
    for es in (True, False):
        outs = {}
        for mode in ("auto", "stream"):
            monkeypatch.setenv("LDPC_ENGINE_MODE", mode)
            w._engine = None
            u._engine = None
            wb, wp, wi = w(x, early_stop=es)
            ub, us, ui = u.decode(x, early_stop=es)
            assert w._engine.info()["kernel"] == ("layered_paper_lds" if mode == "auto" else "layered_rcq<paper>")
            assert u._engine.info()["kernel"] == ("layered_paper_lds" if mode == "auto" else "layered_rcq<paper>")
            outs[mode] = [a.cpu().numpy() for a in (wb, wp, wi, ub, us, ui)]
        for a, s in zip(outs["auto"], outs["stream"]):
            np.testing.assert_array_equal(a, s)


def test_full_batch_against_restatement(gpu_device, monkeypatch):
    """65536 codewords on (1998,1512): LDS kernel == streaming kernel, 128 rows == the restatement"""
    from rcq_decoder import WeightedRCQDecoder
    rng = np.random.default_rng(65536)
    code = load("ira_1998_1512", 10)
    B = 65536
    gen = torch.Generator(device=gpu_device)
    gen.manual_seed(5)
    s2 = 10.0 ** (-5.0 / 10.0)
    x = (2.0 * (1.0 + (s2 ** 0.5) * torch.randn((B, code.n), generator=gen, device=gpu_device)) / s2).float()
    w = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=2, max_iterations=10, layered="paper")
    randomise_betas(w, rng, zero_neg=False)
    outs = {}
    for mode in ("auto", "stream"):
        monkeypatch.setenv("LDPC_ENGINE_MODE", mode)
        w._engine = None
        outs[mode] = [a.cpu().numpy() for a in w(x)]
    for a, s in zip(outs["auto"], outs["stream"]):
        np.testing.assert_array_equal(a, s)
    pick = np.sort(rng.choice(B, size=128, replace=False))
    ob, op, oi, _ = restate(code, x[pick].cpu().numpy(), 3, QP, 10, edge_betas(w, 10))
    bits, post, iters = outs["auto"]
    np.testing.assert_array_equal(iters[pick], oi)
    np.testing.assert_array_equal(bits[pick], ob)
    np.testing.assert_array_equal(post[pick], op)


def test_alpha_has_no_effect(gpu_device):
    from rcq_decoder import WeightedRCQDecoder
    rng = np.random.default_rng(3)
    code = load("small_96_48", 10)
    x = torch.from_numpy(awgn(rng, 200, code.n, 2.0)).to(gpu_device)
    w = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=2, max_iterations=10, layered="paper")
    randomise_betas(w, rng)
    before = [a.cpu().numpy() for a in w(x)]
    with torch.no_grad():
        for p in w.alpha_weights.values():
            p.fill_(float(rng.uniform(0.2, 1.8)))
    after = [a.cpu().numpy() for a in w(x)]
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("mode", ["auto", "stream"])
def test_weight_update_reaches_cached_engine(mode, gpu_device, monkeypatch):
    from rcq_decoder import WeightedRCQDecoder
    monkeypatch.setenv("LDPC_ENGINE_MODE", mode)
    rng = np.random.default_rng(11)
    code = load("small_96_48", 10)
    llr = awgn(rng, 150, code.n, 2.0)
    x = torch.from_numpy(llr).to(gpu_device)
    w = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=3, max_iterations=10, layered="paper")
    w(x)
    eng = w._engine
    randomise_betas(w, rng)
    bits, post, iters = w(x)
    assert w._engine is eng                              # same engine, new tables
    ob, op, oi, _ = restate(code, llr, 3, QP, 10, edge_betas(w, 10))
    np.testing.assert_array_equal(iters.cpu().numpy(), oi)
    np.testing.assert_array_equal(bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(post.cpu().numpy(), op)


def test_layered_needs_fewer_iterations_than_flooding(gpu_device):
    from rcq_decoder import WeightedRCQDecoder
    rng = np.random.default_rng(12)
    code = load("small_96_48", 10)
    x = torch.from_numpy(awgn(rng, 256, code.n, 2.0)).to(gpu_device)
    lay = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=2, max_iterations=10, layered="paper")
    with torch.no_grad():
        for p in lay.beta_weights.values():
            p.fill_(0.8)
    flo = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=2, max_iterations=10)
    flo.load_state_dict(lay.state_dict())
    assert lay(x)[2].float().mean() < flo(x)[2].float().mean()


def test_layered_true_still_runs_flooding(gpu_device):
    """the reference ignores WeightedRCQDecoder's `layered`; every value but "paper" keeps doing so"""
    from rcq_decoder import WeightedRCQDecoder
    rng = np.random.default_rng(13)
    code = load("small_96_48", 10)
    x = torch.from_numpy(awgn(rng, 200, code.n, 2.0)).to(gpu_device)
    flo = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=2, max_iterations=10)
    randomise_betas(flo, rng)
    want = [a.cpu().numpy() for a in flo(x)]
    for layered in (True, "other"):
        dec = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=2, max_iterations=10, layered=layered)
        dec.load_state_dict(flo.state_dict())
        for a, b in zip([a.cpu().numpy() for a in dec(x)], want):
            np.testing.assert_array_equal(a, b)
