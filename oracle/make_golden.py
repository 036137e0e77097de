#!/usr/bin/env python3
"""
Generate tests/golden/*.npz by running the REAL reference (imported from
/root/reference, build container only) on seeded inputs, and check the CPU
restatement (oracle/ldpc_oracle.c) against it while doing so.

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python oracle/make_golden.py [--only NAME ...] [--slow]

The fixtures are data only: graphs (dense H for the small codes, the name of a
committed edge list for the large ones), input LLRs, weight values, and the
reference's outputs (bits, success/posterior, iterations, per-iteration
quantiser codes, one byte each).  Nothing of the reference's source text is stored.

Sets:
  quantizer      NonUniformQuantizer known answers + threshold-boundary sweep
  sums           torch.sum / np.sum association-order known answers
  toy_basic      BasicMinSumDecoder on create_test_ldpc_code(), 256 vectors
  toy_neural2d   Neural2DMinSumDecoder types 1-4 (+ default randn*0.1 init)
  toy_rcq        RCQMinSumDecoder / WeightedRCQDecoder with code traces
  small_*        the same on the 48x96 code (variable degrees 1,2,3,8)
  ira_*          (1998,1512) code: Basic x16, Neural2D x2, RCQ x4, W-RCQ x2
  dvbs2_wrcq     (16200,7200) W-RCQ T=20, 1 codeword              (--slow, ~15 min)
  grad_toy/small d loss/d beta, d loss/d alpha of the reference under torch autograd (the loss of
                 training_framework.py:101), Neural2D types 1-4 and the per-edge NeuralMinSumDecoder
  rcq_widths     the RCQ decoders on the 48x96 code at 2, 32, 64 and 128 quantiser levels (bc 2, 6, 7, 8: codes that use
                 bit 7), flooding with code traces and layered, plus a threshold-boundary sweep at bc 6, 7 and 8
  grad_ties      the same plus d loss/d llr on half-integer LLRs: exact ties for the second minimum (autograd splits evenly)
"""
import argparse
import os
import sys
import time

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden")
PKG_DATA = os.path.join(ROOT, "implementation-of-neural-ldpc-decoders-with-degree-specific-weight-sharing-and-rcq-quantization_amd", "data")
sys.path.insert(0, REF)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import logging  # noqa: E402

import ldpc_decoder as ref_ldpc  # noqa: E402  (the reference's)
import neural_2d_decoder as ref_n2d  # noqa: E402
import rcq_decoder as ref_rcq  # noqa: E402
import neural_minsum_decoder as ref_nms  # noqa: E402
import oracle  # noqa: E402  (oracle/oracle.py)

logging.getLogger().setLevel(logging.WARNING)
assert ref_ldpc.__file__.startswith(REF)

QP = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]       # rcq_decoder.py:619


class CachedCode(ref_ldpc.LDPCCode):
    """LDPCCode whose degree dicts are computed once.  The reference recomputes
    them with an O(m*n) Python loop on every property access (ldpc_decoder.py:38-54),
    which the neural decoders do per edge; the decoders only read the dicts."""

    def _cache(self):
        if "_cn" not in self.__dict__:
            self.__dict__["_cn"] = {i: int(d) for i, d in enumerate(np.sum(self.H, axis=1))}
            self.__dict__["_vn"] = {j: int(d) for j, d in enumerate(np.sum(self.H, axis=0))}

    @property
    def check_node_degrees(self):
        self._cache()
        return self.__dict__["_cn"]

    @property
    def variable_node_degrees(self):
        self._cache()
        return self.__dict__["_vn"]


def load_edge_list(name):
    z = np.load(os.path.join(PKG_DATA, name + ".npz"))
    n = int(z["n"])
    cp = z["check_ptr"].astype(np.int64)
    m = len(cp) - 1
    H = np.zeros((m, n), dtype=np.int64)
    H[np.repeat(np.arange(m), np.diff(cp)), z["var_idx"].astype(np.int64)] = 1
    return H


def awgn_llr_decoder_convention(rng, B, n, snr_db, dtype):
    """all-zero codeword, decoder convention (+LLR = bit 0): llr = 2(1+sigma z)/sigma^2"""
    s2 = 10.0 ** (-snr_db / 10.0)
    z = rng.standard_normal((B, n))
    return (2.0 * (1.0 + np.sqrt(s2) * z) / s2).astype(dtype)


def set_weights(dec, rng, lo_b=0.5, hi_b=1.0, lo_a=0.8, hi_a=1.2):
    beta, alpha = {}, {}
    with torch.no_grad():
        for k in dec.beta_weights.keys():
            v = np.float32(rng.uniform(lo_b, hi_b))
            dec.beta_weights[k].fill_(float(v))
            beta[k] = float(v)
        for k in dec.alpha_weights.keys():
            v = np.float32(rng.uniform(lo_a, hi_a))
            dec.alpha_weights[k].fill_(float(v))
            alpha[k] = float(v)
    return beta, alpha


def get_weights(dec):
    beta = {k: float(v.detach().item()) for k, v in dec.beta_weights.items()}
    alpha = {k: float(v.detach().item()) for k, v in dec.alpha_weights.items()}
    return beta, alpha


def pack_weights(d):
    keys = sorted(d)
    return np.asarray(keys, dtype="U64"), np.asarray([d[k] for k in keys], dtype=np.float32)


class CodeLogger:
    """Wraps quantizer.quantize of every quantiser of a decoder (instance attribute,
    no reference edit) and records the integer code of every call, in call order."""

    def __init__(self, dec):
        self.codes = []
        for q in dec.quantizers:
            orig = q.quantize

            def wrapped(x, _orig=orig):
                out = _orig(x)
                self.codes.append(int(out.reshape(-1)[0].item()))
                return out
            q.quantize = wrapped

    def take(self, E, T):
        c = np.asarray(self.codes, dtype=np.int64)
        self.codes = []
        assert c.size % E == 0, (c.size, E)
        out = np.full((T, E), 255, dtype=np.uint8)
        out[: c.size // E] = c.reshape(-1, E)
        return out


def special_llrs(rng, n, count, scale=3.0):
    """random LLRs with injected exact zeros, exact ties and tiny values"""
    x = rng.standard_normal((count, n)) * scale
    for r in range(count):
        mode = r % 8
        if mode == 1:
            x[r, rng.integers(0, n)] = 0.0
        elif mode == 2:
            j = rng.choice(n, 2, replace=False)
            x[r, j[1]] = x[r, j[0]]
        elif mode == 3:
            j = rng.choice(n, 2, replace=False)
            x[r, j[1]] = -x[r, j[0]]
        elif mode == 4:
            x[r, rng.choice(n, 2, replace=False)] = 0.0
        elif mode == 5:
            x[r] = np.round(x[r])          # many ties / zeros
        elif mode == 6:
            x[r, rng.integers(0, n)] = -0.0
        elif mode == 7:
            x[r] *= 0.05
    return x


def check_equal(name, a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(a, b):
        bad = np.argwhere(a != b)[:5] if a.shape == b.shape else "shape"
        raise SystemExit(f"ORACLE MISMATCH in {name}: {bad}")


def check_bits_exact(name, a, b):
    """float arrays equal bit for bit (sign of zero included)"""
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    if a.shape != b.shape or a.tobytes() != b.tobytes():
        d = np.abs(a.astype(np.float64) - b.astype(np.float64)).max() if a.shape == b.shape else -1
        raise SystemExit(f"ORACLE MISMATCH (bitwise) in {name}: max abs diff {d}")


# =============================================================================== sets
def gen_quantizer():
    out = {}
    q = ref_rcq.NonUniformQuantizer(bc=3, C=5.0, gamma=1.5)
    x = torch.tensor([-3.2, -1.1, 0.5, 2.8, 4.1])           # rcq_decoder.py:609, comprehensive_test.py:259
    out["kat_thresholds"] = np.asarray(q.thresholds, dtype=np.float64)
    out["kat_x"] = x.numpy()
    out["kat_codes"] = q.quantize(x).numpy()
    out["kat_deq"] = q.dequantize(q.quantize(x)).numpy()
    check_equal("kat thr", np.asarray(oracle.quantizer_thresholds(3, 5.0, 1.5)), out["kat_thresholds"])
    check_equal("kat codes", oracle.quantize(out["kat_x"], out["kat_thresholds"]), out["kat_codes"])
    check_bits_exact("kat deq", oracle.dequantize(out["kat_codes"], out["kat_thresholds"]), out["kat_deq"])
    cfgs = [(3, 3.0, 1.3), (3, 5.0, 1.3), (3, 7.0, 1.3), (4, 6.0, 1.7), (2, 2.0, 1.0), (5, 8.0, 0.7)]
    quantizer_sweep(out, "sweep", cfgs, np.random.default_rng(7))
    return out


def gen_sums():
    """Association order of torch.sum (fp32) and np.sum (fp64) on 1-D contiguous
    arrays produced by fancy indexing, as the reference calls them."""
    rng = np.random.default_rng(11)
    Ns = list(range(0, 41)) + [47, 48, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256, 300, 511, 512, 575]
    xs32, ys32, xs64, ys64, lens = [], [], [], [], []
    for N in Ns:
        for rep in range(6):
            x = (rng.standard_normal(N) * 10.0 ** rng.uniform(-3, 3, N))
            x32 = x.astype(np.float32)
            t = torch.from_numpy(x32)[torch.arange(N)]
            y32 = np.float32(torch.sum(t).item())
            y64 = np.float64(np.sum(x[np.arange(N)]))
            check_bits_exact(f"torch.sum N={N}", oracle.sum_f32(x32), y32)
            check_bits_exact(f"np.sum N={N}", oracle.sum_f64(x), y64)
            pad32 = np.zeros(600, np.float32); pad32[:N] = x32
            pad64 = np.zeros(600, np.float64); pad64[:N] = x
            xs32.append(pad32); ys32.append(y32); xs64.append(pad64); ys64.append(y64); lens.append(N)
    # values drawn from a dequantiser alphabet (what RCQ actually sums)
    thr = np.asarray(oracle.quantizer_thresholds(3, 7.0, 1.3), dtype=np.float32)
    alphabet = np.concatenate([thr, -thr]).astype(np.float32)
    for N in range(0, 33):
        for rep in range(6):
            x32 = alphabet[rng.integers(0, alphabet.size, N)]
            t = torch.from_numpy(x32)[torch.arange(N)]
            y32 = np.float32(torch.sum(t).item())
            check_bits_exact(f"torch.sum alphabet N={N}", oracle.sum_f32(x32), y32)
            pad32 = np.zeros(600, np.float32); pad32[:N] = x32
            xs32.append(pad32); ys32.append(y32)
            xs64.append(np.zeros(600)); ys64.append(np.float64(0)); lens.append(-N - 1)  # negative: fp32-only row
    return dict(x32=np.stack(xs32), y32=np.asarray(ys32, np.float32), x64=np.stack(xs64),
                y64=np.asarray(ys64, np.float64), n=np.asarray(lens, np.int32),
                torch_version=np.asarray(torch.__version__), numpy_version=np.asarray(np.__version__))


def run_basic(code, H, llrs, factor=0.7):
    g = oracle.OracleGraph(H)
    dec = ref_ldpc.BasicMinSumDecoder(code, factor=factor)
    bits, succ, its = [], [], []
    for x in llrs:
        b, s, i = dec.decode(x.copy())
        bits.append(np.asarray(b, dtype=np.int64)); succ.append(bool(s)); its.append(int(i))
    bits, succ, its = np.stack(bits), np.asarray(succ), np.asarray(its, np.int32)
    ob, op, oi, os_ = oracle.basic_minsum(g, llrs, factor=factor, T=code.max_iterations)
    check_equal("basic bits", ob, bits); check_equal("basic iters", oi, its); check_equal("basic success", os_, succ)
    return dict(llr=llrs, bits=bits.astype(np.uint8), success=succ, iters=its, factor=np.float64(factor),
                T=np.int32(code.max_iterations), oracle_posterior=op)


def run_neural2d(code, H, llrs, wtype, T, rng=None, default_init_seed=None):
    g = oracle.OracleGraph(H)
    if default_init_seed is not None:
        torch.manual_seed(default_init_seed)
    dec = ref_n2d.Neural2DMinSumDecoder(code, weight_sharing_type=wtype, max_iterations=T)
    if default_init_seed is None:
        beta, alpha = set_weights(dec, rng)
    else:
        beta, alpha = get_weights(dec)
    bits, post, its = [], [], []
    with torch.no_grad():
        for x in llrs:
            b, p, i = dec(torch.from_numpy(x.copy()))
            bits.append(b.numpy().copy()); post.append(p.detach().numpy().reshape(-1).copy()); its.append(int(i))
    bits, post, its = np.stack(bits), np.stack(post), np.asarray(its, np.int32)
    ob, op, oi, _ = oracle.neural2d(g, llrs, wtype, T, beta, alpha)
    check_equal("n2d bits", ob, bits); check_equal("n2d iters", oi, its); check_bits_exact("n2d posterior", op, post)
    bk, bv = pack_weights(beta); ak, av = pack_weights(alpha)
    return dict(llr=llrs, bits=bits.astype(np.uint8), posterior=post, iters=its, wtype=np.int32(wtype), T=np.int32(T),
                beta_keys=bk, beta_vals=bv, alpha_keys=ak, alpha_vals=av)


def run_rcq(code, H, llrs, T, bc=3, qp=QP):
    g = oracle.OracleGraph(H)
    dec = ref_rcq.RCQMinSumDecoder(code, bc=bc, bv=8, quantizer_params=qp, max_iterations=T)
    log = CodeLogger(dec)
    bits, succ, its, codes = [], [], [], []
    for x in llrs:
        b, s, i = dec.decode(torch.from_numpy(x.copy()))
        bits.append(b.numpy().copy()); succ.append(bool(s)); its.append(int(i)); codes.append(log.take(g.E, T))
    bits, succ, its, codes = np.stack(bits), np.asarray(succ), np.asarray(its, np.int32), np.stack(codes)
    ob, op, oi, os_, oc = oracle.rcq(g, llrs, bc, qp, T, trace_codes=True)
    check_equal("rcq bits", ob, bits); check_equal("rcq iters", oi, its); check_equal("rcq success", os_, succ)
    for r in range(len(llrs)):
        check_equal("rcq codes", oc[r, : its[r]], codes[r, : its[r]])
    return dict(llr=llrs, bits=bits.astype(np.uint8), success=succ, iters=its, codes=codes, T=np.int32(T),
                bc=np.int32(bc), qp=np.asarray(qp, np.float64), oracle_posterior=op)


def run_wrcq(code, H, llrs, wtype, T, rng=None, default_init_seed=None, bc=3, qp=QP):
    g = oracle.OracleGraph(H)
    if default_init_seed is not None:
        torch.manual_seed(default_init_seed)
    dec = ref_rcq.WeightedRCQDecoder(code, bc=bc, bv=8, quantizer_params=qp, weight_sharing_type=wtype, max_iterations=T)
    if default_init_seed is None:
        beta, alpha = set_weights(dec, rng)
    else:
        beta, alpha = get_weights(dec)
    log = CodeLogger(dec)
    bits, post, its, codes = [], [], [], []
    with torch.no_grad():
        for x in llrs:
            b, p, i = dec(torch.from_numpy(x.copy()))
            bits.append(b.numpy().copy()); post.append(p.detach().numpy().reshape(-1).copy()); its.append(int(i))
            codes.append(log.take(g.E, T))
    bits, post, its, codes = np.stack(bits), np.stack(post), np.asarray(its, np.int32), np.stack(codes)
    ob, op, oi, _, oc = oracle.weighted_rcq(g, llrs, bc, qp, wtype, T, beta, alpha, trace_codes=True)
    check_equal("wrcq bits", ob, bits); check_equal("wrcq iters", oi, its); check_bits_exact("wrcq posterior", op, post)
    for r in range(len(llrs)):
        check_equal("wrcq codes", oc[r, : its[r]], codes[r, : its[r]])
    bk, bv = pack_weights(beta); ak, av = pack_weights(alpha)
    return dict(llr=llrs, bits=bits.astype(np.uint8), posterior=post, iters=its, codes=codes, wtype=np.int32(wtype),
                T=np.int32(T), bc=np.int32(bc), qp=np.asarray(qp, np.float64),
                beta_keys=bk, beta_vals=bv, alpha_keys=ak, alpha_vals=av)


def run_offset2d(code, H, llrs, wtype, T, rng):
    g = oracle.OracleGraph(H)
    dec = ref_n2d.Neural2DOffsetMinSumDecoder(code, weight_sharing_type=wtype, max_iterations=T)
    beta, alpha = set_weights(dec, rng, 0.0, 0.6, 0.0, 0.3)
    bits, post, its = [], [], []
    with torch.no_grad():
        for x in llrs:
            b, p, i = dec(torch.from_numpy(x.copy()))
            bits.append(b.numpy().copy()); post.append(p.detach().numpy().reshape(-1).copy()); its.append(int(i))
    bits, post, its = np.stack(bits), np.stack(post), np.asarray(its, np.int32)
    ob, op, oi, _ = oracle.neural2d_offset(g, llrs, wtype, T, beta, alpha)
    check_equal("oms2d bits", ob, bits); check_equal("oms2d iters", oi, its)
    if not np.array_equal(op, post):                       # value equality (the product with a zero sign gives -0.0)
        raise SystemExit("ORACLE MISMATCH in oms2d posterior")
    bk, bv = pack_weights(beta); ak, av = pack_weights(alpha)
    return dict(llr=llrs, bits=bits.astype(np.uint8), posterior=post, iters=its, wtype=np.int32(wtype), T=np.int32(T),
                beta_keys=bk, beta_vals=bv, alpha_keys=ak, alpha_vals=av)


def run_edge(code, H, llrs, T, offset, seed):
    """NeuralMinSumDecoder / NeuralOffsetMinSumDecoder with the constructor's own seeded init"""
    g = oracle.OracleGraph(H)
    torch.manual_seed(seed)
    dec = (ref_nms.NeuralOffsetMinSumDecoder if offset else ref_nms.NeuralMinSumDecoder)(code, max_iterations=T)
    if offset:                                             # spread the offsets so relu() actually clips
        with torch.no_grad():
            for p in dec.beta_weights.values():
                p.mul_(3.0).abs_()
    beta = {k: float(v.detach().item()) for k, v in dec.beta_weights.items()}
    bits, post, its = [], [], []
    with torch.no_grad():
        for x in llrs:
            b, p, i = dec(torch.from_numpy(x.copy()))
            bits.append(b.numpy().copy()); post.append(p.detach().numpy().reshape(-1).copy()); its.append(int(i))
    bits, post, its = np.stack(bits), np.stack(post), np.asarray(its, np.int32)
    ob, op, oi, _ = oracle.neural_minsum(g, llrs, T, beta, offset=offset)
    check_equal("edge bits", ob, bits); check_equal("edge iters", oi, its)
    if not np.array_equal(op, post):
        raise SystemExit("ORACLE MISMATCH in edge-weight posterior")
    bk, bv = pack_weights(beta)
    return dict(llr=llrs, bits=bits.astype(np.uint8), posterior=post, iters=its, T=np.int32(T), seed=np.int32(seed),
                offset=np.int32(offset), beta_keys=bk, beta_vals=bv)


def gen_offset_and_edge(which):
    """'next' rows of SURVEY 8f-2: offset forms and per-edge weights, toy + 48x96 codes"""
    if which == "toy":
        code = ref_ldpc.create_test_ldpc_code()
        H = code.H
        llrs = toy_inputs_fp64(48).astype(np.float32)
        T = 10
    else:
        H = load_edge_list("small_96_48")
        code = CachedCode(n=96, k=48, H=H, max_iterations=10)
        rng0 = np.random.default_rng(77)
        llrs = np.concatenate([awgn_llr_decoder_convention(rng0, 5, 96, 2.0, np.float32),
                               awgn_llr_decoder_convention(rng0, 5, 96, 5.0, np.float32),
                               special_llrs(rng0, 96, 4).astype(np.float32)])
        T = 6
    rng = np.random.default_rng(2025)
    out = {"H": np.asarray(H).astype(np.uint8)} if which == "toy" else {"graph": np.asarray("small_96_48")}
    for wtype in (1, 2, 3, 4):
        for k, v in run_offset2d(code, H, llrs, wtype, T, rng).items():
            out[f"o{wtype}_{k}"] = v
    for k, v in run_edge(code, H, llrs, T, False, 11).items():
        out[f"nms_{k}"] = v
    for k, v in run_edge(code, H, llrs, T, True, 12).items():
        out[f"oms_{k}"] = v
    return out


def gen_layered():
    """RCQMinSumDecoder(layered=True) (rcq_decoder.py:281-350) on the toy and 48x96 codes"""
    out = {}
    for tag in ("toy", "small"):
        if tag == "toy":
            code = ref_ldpc.create_test_ldpc_code(); H = code.H
            llrs = toy_inputs_fp64(64).astype(np.float32); T = 10
            out["toy_H"] = np.asarray(H).astype(np.uint8)
        else:
            H = load_edge_list("small_96_48")
            code = CachedCode(n=96, k=48, H=H, max_iterations=10)
            rng = np.random.default_rng(31)
            llrs = np.concatenate([awgn_llr_decoder_convention(rng, 8, 96, 2.0, np.float32),
                                   awgn_llr_decoder_convention(rng, 8, 96, 5.0, np.float32),
                                   special_llrs(rng, 96, 4).astype(np.float32)]); T = 9
        g = oracle.OracleGraph(H)
        dec = ref_rcq.RCQMinSumDecoder(code, bc=3, bv=8, quantizer_params=QP, max_iterations=T, layered=True)
        bits, succ, its = [], [], []
        for x in llrs:
            b, s_, i = dec.decode(torch.from_numpy(x.copy()))
            bits.append(b.numpy().copy()); succ.append(bool(s_)); its.append(int(i))
        bits, succ, its = np.stack(bits), np.asarray(succ), np.asarray(its, np.int32)
        ob, op, oi, os_ = oracle.rcq_layered(g, llrs, 3, QP, T)
        check_equal("layered bits", ob, bits); check_equal("layered iters", oi, its); check_equal("layered success", os_, succ)
        out.update({f"{tag}_llr": llrs, f"{tag}_bits": bits.astype(np.uint8), f"{tag}_success": succ, f"{tag}_iters": its,
                    f"{tag}_T": np.int32(T), f"{tag}_oracle_posterior": op})
    return out


def toy_inputs_fp64(count):
    """config 1 inputs: np.random.seed(s); simulate_awgn_channel(zeros(7), 2.0) literally
    (ldpc_decoder.py:286-302), then a block of special vectors, then the flipped sign
    convention so that a good share converges."""
    rows = []
    for s in range(count // 4):
        np.random.seed(s)
        rows.append(ref_ldpc.simulate_awgn_channel(np.zeros(7, dtype=int), 2.0))
    for s in range(count // 4):
        np.random.seed(10_000 + s)
        rows.append(-ref_ldpc.simulate_awgn_channel(np.zeros(7, dtype=int), 2.0))
    rng = np.random.default_rng(3)
    rows += list(special_llrs(rng, 7, count - len(rows)))
    return np.asarray(rows, dtype=np.float64)


def gen_toy_basic():
    code = ref_ldpc.create_test_ldpc_code()
    out = run_basic(code, code.H, toy_inputs_fp64(256))
    out["H"] = code.H.astype(np.uint8)
    return out


def gen_toy_neural2d():
    code = ref_ldpc.create_test_ldpc_code()
    llrs = toy_inputs_fp64(64).astype(np.float32)
    rng = np.random.default_rng(4321)
    out = {"H": code.H.astype(np.uint8)}
    for wtype in (1, 2, 3, 4):
        for k, v in run_neural2d(code, code.H, llrs, wtype, 10, rng=rng).items():
            out[f"t{wtype}_{k}"] = v
        # the constructor's own init (randn * 0.1: negative / tiny betas)
        for k, v in run_neural2d(code, code.H, llrs[:24], wtype, 10, default_init_seed=100 + wtype).items():
            out[f"t{wtype}d_{k}"] = v
    return out


def gen_toy_rcq():
    code = ref_ldpc.create_test_ldpc_code()
    llrs = toy_inputs_fp64(64).astype(np.float32)
    rng = np.random.default_rng(99)
    out = {"H": code.H.astype(np.uint8)}
    for k, v in run_rcq(code, code.H, llrs, 10).items():
        out[f"rcq_{k}"] = v
    for k, v in run_rcq(code, code.H, llrs[:16], 7, bc=4, qp=[(6.0, 1.7)]).items():
        out[f"rcq4_{k}"] = v
    for wtype in (1, 2, 3, 4):
        for k, v in run_wrcq(code, code.H, llrs[:32], wtype, 10, rng=rng).items():
            out[f"w{wtype}_{k}"] = v
    for k, v in run_wrcq(code, code.H, llrs[:16], 2, 10, default_init_seed=7).items():
        out[f"w2d_{k}"] = v
    return out


def gen_small(kind):
    H = load_edge_list("small_96_48")
    rng = np.random.default_rng(4848)
    if kind == "basic":
        code = CachedCode(n=96, k=48, H=H, max_iterations=12)
        llrs = np.concatenate([awgn_llr_decoder_convention(rng, 12, 96, 2.0, np.float64),
                               awgn_llr_decoder_convention(rng, 12, 96, 5.0, np.float64),
                               special_llrs(rng, 96, 8)])
        out = run_basic(code, H, llrs)
    elif kind == "neural2d":
        code = CachedCode(n=96, k=48, H=H, max_iterations=10)
        llrs = np.concatenate([awgn_llr_decoder_convention(rng, 6, 96, 2.0, np.float32),
                               awgn_llr_decoder_convention(rng, 6, 96, 5.0, np.float32),
                               special_llrs(rng, 96, 4).astype(np.float32)])
        out = {}
        for wtype in (1, 2, 3, 4):
            for k, v in run_neural2d(code, H, llrs, wtype, 8, rng=rng).items():
                out[f"t{wtype}_{k}"] = v
    elif kind == "rcq":
        code = CachedCode(n=96, k=48, H=H, max_iterations=10)
        llrs = np.concatenate([awgn_llr_decoder_convention(rng, 8, 96, 2.0, np.float32),
                               awgn_llr_decoder_convention(rng, 6, 96, 5.0, np.float32),
                               special_llrs(rng, 96, 4).astype(np.float32)])
        out = {}
        for k, v in run_rcq(code, H, llrs, 10).items():
            out[f"rcq_{k}"] = v
        for k, v in run_wrcq(code, H, llrs[:12], 2, 10, rng=rng).items():
            out[f"w2_{k}"] = v
        for k, v in run_wrcq(code, H, llrs[:6], 1, 9, rng=rng).items():
            out[f"w1_{k}"] = v
    out["graph"] = np.asarray("small_96_48")
    return out


def gen_ira(kind):
    H = load_edge_list("ira_1998_1512")
    n = 1998
    rng = np.random.default_rng(1998)
    t0 = time.time()
    if kind == "basic":
        code = CachedCode(n=n, k=1512, H=H, max_iterations=10)
        llrs = np.concatenate([awgn_llr_decoder_convention(rng, 8, n, 2.0, np.float64),
                               awgn_llr_decoder_convention(rng, 8, n, 5.0, np.float64)])
        out = run_basic(code, H, llrs)
    elif kind == "neural2d":
        code = CachedCode(n=n, k=1512, H=H, max_iterations=10)
        llrs = np.concatenate([awgn_llr_decoder_convention(rng, 1, n, 2.0, np.float32),
                               awgn_llr_decoder_convention(rng, 1, n, 5.0, np.float32)])
        out = run_neural2d(code, H, llrs, 2, 10, rng=rng)
    elif kind == "rcq":
        code = CachedCode(n=n, k=1512, H=H, max_iterations=10)
        llrs = np.concatenate([awgn_llr_decoder_convention(rng, 2, n, 2.0, np.float32),
                               awgn_llr_decoder_convention(rng, 2, n, 5.0, np.float32)])
        out = run_rcq(code, H, llrs, 10)
    elif kind == "wrcq":
        code = CachedCode(n=n, k=1512, H=H, max_iterations=10)
        llrs = np.concatenate([awgn_llr_decoder_convention(rng, 1, n, 2.0, np.float32),
                               awgn_llr_decoder_convention(rng, 1, n, 5.0, np.float32)])
        out = run_wrcq(code, H, llrs, 2, 10, rng=rng)
    out["graph"] = np.asarray("ira_1998_1512")
    print(f"   ira {kind}: {time.time() - t0:.1f}s")
    return out


def gen_dvbs2_wrcq():
    H = load_edge_list("dvbs2_like_16200_7200")
    n = 16200
    rng = np.random.default_rng(16200)
    code = CachedCode(n=n, k=7200, H=H, max_iterations=20)
    llrs = awgn_llr_decoder_convention(rng, 1, n, 2.0, np.float32)
    t0 = time.time()
    out = run_wrcq(code, H, llrs, 2, 20, rng=rng)
    out["graph"] = np.asarray("dvbs2_like_16200_7200")
    print(f"   dvbs2 wrcq: {time.time() - t0:.1f}s")
    return out


def _ref_grads(dec, llrs, targets=None):
    """The REAL reference under autograd: per codeword loss = binary_cross_entropy_with_logits(-posterior, target)
    (training_framework.py:101), backward, gradients summed over the codewords.  Parameters autograd leaves
    without a gradient (None) count as 0; a posterior without grad_fn (no parameter on its path) adds nothing."""
    import torch.nn.functional as F
    gb = {k: 0.0 for k in dec.beta_weights.keys()}
    ga = {k: 0.0 for k in getattr(dec, "alpha_weights", {}).keys()}
    post, its, losses = [], [], []
    for b, x in enumerate(llrs):
        dec.zero_grad()
        _, p, i = dec(torch.from_numpy(x.copy()))
        tgt = torch.zeros_like(p) if targets is None else torch.from_numpy(targets[b].astype(np.float32))
        loss = F.binary_cross_entropy_with_logits(-p, tgt)
        if p.requires_grad:
            loss.backward()
        for k, w in dec.beta_weights.items():
            if w.grad is not None:
                gb[k] += float(w.grad.item())
        for k, w in getattr(dec, "alpha_weights", {}).items():
            if w.grad is not None:
                ga[k] += float(w.grad.item())
        post.append(p.detach().numpy().reshape(-1).copy()); its.append(int(i)); losses.append(float(loss.item()))
    return gb, ga, np.stack(post), np.asarray(its, np.int32), np.asarray(losses, np.float64)


def _check_grad_oracle(name, g, llrs, bt, bs, at, as_, T, gb_ref, ga_ref, post, its, offset=False):
    import grad_oracle
    ogb, oga, opost, oit = grad_oracle.table_grads(g, llrs, bt, bs, at, as_, T, offset=offset)
    check_equal(name + " iters", oit.astype(np.int32), its)
    if not np.allclose(opost, post, rtol=1e-5, atol=1e-5):
        raise SystemExit(f"GRAD ORACLE MISMATCH ({name}): posterior")
    # a table column that is a constant of the sharing type (no reference parameter behind it) has no reference gradient
    for tag, a, b in (("beta", ogb, gb_ref), ("alpha", oga, ga_ref)):
        if b is not None and not np.allclose(a, b, rtol=2e-4, atol=2e-6):
            raise SystemExit(f"GRAD ORACLE MISMATCH ({name}): d loss/d {tag}: max |diff| {np.abs(a - b).max()}")


def run_grad_neural2d(code, H, llrs, wtype, T, rng):
    g = oracle.OracleGraph(H)
    dec = ref_n2d.Neural2DMinSumDecoder(code, weight_sharing_type=wtype, max_iterations=T)
    beta, alpha = set_weights(dec, rng)
    gb, ga, post, its, losses = _ref_grads(dec, llrs)
    bt, bs, at, as_ = oracle.weight_tables(g, wtype, T, beta, alpha)
    # reference per-key gradients -> the [T][slots] tables of the engines (independent flattening: oracle.weight_tables)
    gbt, _, gat, _ = oracle.weight_tables(g, wtype, T, gb, ga, beta_default=0.0, alpha_default=0.0)
    _check_grad_oracle(f"n2d type {wtype}", g, llrs, bt, bs, at, as_, T, gbt if gb else None, gat if ga else None, post, its)
    bk, bv = pack_weights(beta); ak, av = pack_weights(alpha)
    return dict(llr=llrs, posterior=post, iters=its, loss=losses, wtype=np.int32(wtype), T=np.int32(T),
                beta_keys=bk, beta_vals=bv, alpha_keys=ak, alpha_vals=av,
                grad_beta_keys=pack_weights(gb)[0], grad_beta_vals=np.asarray([gb[k] for k in sorted(gb)], np.float64),
                grad_alpha_keys=pack_weights(ga)[0], grad_alpha_vals=np.asarray([ga[k] for k in sorted(ga)], np.float64),
                grad_beta_table=gbt.astype(np.float64), grad_alpha_table=gat.astype(np.float64))


def run_grad_edge(code, H, llrs, T, seed):
    """NeuralMinSumDecoder (one beta per edge and iteration, neural_minsum_decoder.py:58-150) under autograd"""
    g = oracle.OracleGraph(H)
    torch.manual_seed(seed)
    dec = ref_nms.NeuralMinSumDecoder(code, max_iterations=T)
    with torch.no_grad():                                   # randn * 0.1 init -> useful decoding range
        for w in dec.beta_weights.values():
            w.mul_(1.5).add_(0.75)
    beta = {k: float(v.detach().item()) for k, v in dec.beta_weights.items()}
    gb, _, post, its, losses = _ref_grads(dec, llrs)
    bt = oracle.edge_weight_table(g, T, beta)
    gbt = oracle.edge_weight_table(g, T, gb).astype(np.float64)
    ones, zslot = np.ones((max(T, 1), 1), np.float32), np.zeros(g.n, np.int32)
    _check_grad_oracle("edge", g, llrs, bt, np.arange(g.E, dtype=np.int32), ones, zslot, T, gbt, None, post, its)
    bk, bv = pack_weights(beta)
    return dict(llr=llrs, posterior=post, iters=its, loss=losses, T=np.int32(T), seed=np.int32(seed),
                beta_keys=bk, beta_vals=bv, grad_beta_table=gbt)


def run_grad_offset2d(code, H, llrs, wtype, T, rng):
    """Neural2DOffsetMinSumDecoder (relu(min - beta) - alpha, neural_2d_decoder.py:389-401) under autograd"""
    g = oracle.OracleGraph(H)
    dec = ref_n2d.Neural2DOffsetMinSumDecoder(code, weight_sharing_type=wtype, max_iterations=T)
    beta, alpha = set_weights(dec, rng, 0.0, 0.6, 0.0, 0.3)
    gb, ga, post, its, losses = _ref_grads(dec, llrs)
    bt, bs, at, as_ = oracle.weight_tables(g, wtype, T, beta, alpha, beta_default=0.0, alpha_default=0.0)
    gbt, _, gat, _ = oracle.weight_tables(g, wtype, T, gb, ga, beta_default=0.0, alpha_default=0.0)
    _check_grad_oracle(f"oms2d type {wtype}", g, llrs, bt, bs, at, as_[g.var_idx], T, gbt if gb else None,
                       gat if ga else None, post, its, offset=True)
    bk, bv = pack_weights(beta); ak, av = pack_weights(alpha)
    return dict(llr=llrs, posterior=post, iters=its, loss=losses, wtype=np.int32(wtype), T=np.int32(T),
                beta_keys=bk, beta_vals=bv, alpha_keys=ak, alpha_vals=av,
                grad_beta_keys=pack_weights(gb)[0], grad_beta_vals=np.asarray([gb[k] for k in sorted(gb)], np.float64),
                grad_alpha_keys=pack_weights(ga)[0], grad_alpha_vals=np.asarray([ga[k] for k in sorted(ga)], np.float64),
                grad_beta_table=gbt.astype(np.float64), grad_alpha_table=gat.astype(np.float64))


def run_grad_edge_offset(code, H, llrs, T, seed):
    """NeuralOffsetMinSumDecoder (relu(min - beta) per edge, neural_minsum_decoder.py:245-253) under autograd"""
    g = oracle.OracleGraph(H)
    torch.manual_seed(seed)
    dec = ref_nms.NeuralOffsetMinSumDecoder(code, max_iterations=T)
    with torch.no_grad():                                   # spread the offsets so relu() actually clips
        for w in dec.beta_weights.values():
            w.mul_(3.0).abs_()
    beta = {k: float(v.detach().item()) for k, v in dec.beta_weights.items()}
    gb, _, post, its, losses = _ref_grads(dec, llrs)
    bt = oracle.edge_weight_table(g, T, beta)
    gbt = oracle.edge_weight_table(g, T, gb).astype(np.float64)
    zeros = np.zeros((max(T, 1), 1), np.float32)
    _check_grad_oracle("edge offset", g, llrs, bt, np.arange(g.E, dtype=np.int32), zeros, np.zeros(g.E, np.int32), T,
                       gbt, None, post, its, offset=True)
    bk, bv = pack_weights(beta)
    return dict(llr=llrs, posterior=post, iters=its, loss=losses, T=np.int32(T), seed=np.int32(seed),
                beta_keys=bk, beta_vals=bv, grad_beta_table=gbt)


def gen_grad(which):
    rng = np.random.default_rng(8642)
    if which == "toy":
        code = ref_ldpc.create_test_ldpc_code()
        H = code.H
        llrs = np.concatenate([toy_inputs_fp64(32)[8:24].astype(np.float32),          # both sign conventions
                               rng.normal(0.8, 1.6, (8, 7)).astype(np.float32)])
        out = {"H": H.astype(np.uint8)}
        for wtype in (1, 2, 3, 4):
            for T in (3, 6):
                for k, v in run_grad_neural2d(code, H, llrs, wtype, T, rng).items():
                    out[f"t{wtype}_T{T}_{k}"] = v
        for k, v in run_grad_edge(code, H, llrs, 4, seed=77).items():
            out[f"edge_{k}"] = v
        for wtype in (1, 2, 3, 4):
            for k, v in run_grad_offset2d(code, H, llrs, wtype, 4, rng).items():
                out[f"o{wtype}_T4_{k}"] = v
        for k, v in run_grad_edge_offset(code, H, llrs, 4, seed=78).items():
            out[f"edgeoff_{k}"] = v
    elif which == "ira":
        H = load_edge_list("ira_1998_1512")
        code = CachedCode(n=1998, k=1512, H=H, max_iterations=10)
        llrs = np.concatenate([awgn_llr_decoder_convention(rng, 1, 1998, 2.0, np.float32),
                               awgn_llr_decoder_convention(rng, 1, 1998, 5.5, np.float32)])
        out = {"graph": np.asarray("ira_1998_1512")}
        for k, v in run_grad_neural2d(code, H, llrs, 2, 3, rng).items():
            out[f"t2_T3_{k}"] = v
    else:
        H = load_edge_list("small_96_48")
        code = CachedCode(n=96, k=48, H=H, max_iterations=10)
        llrs = np.concatenate([awgn_llr_decoder_convention(rng, 4, 96, 2.0, np.float32),
                               awgn_llr_decoder_convention(rng, 3, 96, 4.5, np.float32)])
        out = {"graph": np.asarray("small_96_48")}
        for wtype, T in ((2, 4), (1, 3)):
            for k, v in run_grad_neural2d(code, H, llrs, wtype, T, rng).items():
                out[f"t{wtype}_T{T}_{k}"] = v
        for k, v in run_grad_offset2d(code, H, llrs, 2, 4, rng).items():
            out[f"o2_T4_{k}"] = v
    return out


def gen_grad_llr():
    """d loss/d llr of the reference (its forward is differentiable in the input too): Neural2D type 2, the offset
    decoder type 2 and the per-edge decoder on the toy code"""
    import torch.nn.functional as F
    import grad_oracle
    rng = np.random.default_rng(9753)
    code = ref_ldpc.create_test_ldpc_code()
    H = code.H
    g = oracle.OracleGraph(H)
    llrs = np.concatenate([toy_inputs_fp64(32)[10:18].astype(np.float32), rng.normal(0.8, 1.6, (6, 7)).astype(np.float32)])
    out = {"H": H.astype(np.uint8), "llr": llrs}

    def run(dec):
        gl, its = [], []
        for x in llrs:
            dec.zero_grad()
            t = torch.from_numpy(x.copy()).requires_grad_(True)
            _, p, i = dec(t)
            F.binary_cross_entropy_with_logits(-p, torch.zeros_like(p)).backward()
            gl.append(t.grad.numpy().copy()); its.append(int(i))
        return np.stack(gl), np.asarray(its, np.int32)

    T = 4
    dec = ref_n2d.Neural2DMinSumDecoder(code, weight_sharing_type=2, max_iterations=T)
    beta, alpha = set_weights(dec, rng)
    gl, its = run(dec)
    bt, bs, at, as_ = oracle.weight_tables(g, 2, T, beta, alpha)
    og = grad_oracle.table_grads(g, llrs, bt, bs, at, as_, T, want_llr=True)
    check_equal("grad llr iters", og[3].astype(np.int32), its)
    if not np.allclose(og[4], gl, rtol=2e-4, atol=2e-6):
        raise SystemExit("GRAD ORACLE MISMATCH: d loss/d llr (n2d)")
    bk, bv = pack_weights(beta); ak, av = pack_weights(alpha)
    out.update(n2d_T=np.int32(T), n2d_iters=its, n2d_grad_llr=gl, n2d_beta_keys=bk, n2d_beta_vals=bv, n2d_alpha_keys=ak, n2d_alpha_vals=av)

    dec = ref_n2d.Neural2DOffsetMinSumDecoder(code, weight_sharing_type=2, max_iterations=T)
    beta, alpha = set_weights(dec, rng, 0.0, 0.6, 0.0, 0.3)
    gl, its = run(dec)
    bt, bs, at, as_ = oracle.weight_tables(g, 2, T, beta, alpha, beta_default=0.0, alpha_default=0.0)
    og = grad_oracle.table_grads(g, llrs, bt, bs, at, as_[g.var_idx], T, offset=True, want_llr=True)
    check_equal("grad llr iters (oms)", og[3].astype(np.int32), its)
    if not np.allclose(og[4], gl, rtol=2e-4, atol=2e-6):
        raise SystemExit("GRAD ORACLE MISMATCH: d loss/d llr (oms2d)")
    bk, bv = pack_weights(beta); ak, av = pack_weights(alpha)
    out.update(oms_T=np.int32(T), oms_iters=its, oms_grad_llr=gl, oms_beta_keys=bk, oms_beta_vals=bv, oms_alpha_keys=ak, oms_alpha_vals=av)
    return out


def gen_grad_ties():
    """Inputs with EXACT ties among the magnitudes a check sees (half-integer LLRs): the reference's `torch.min(temp_mags)`
    (neural_2d_decoder.py:179, a full reduction) splits the gradient of the second minimum evenly among the tied edges,
    `magnitudes[min_idx]` sends the minimum's to the first arg-min.  Visible in d loss/d llr (iteration 0 reads the LLRs)
    and, through later iterations, in the table gradients.  Toy code and the 48x96 code; Neural2D type 2 and the offset form."""
    import torch.nn.functional as F
    import grad_oracle
    rng = np.random.default_rng(2468)
    out = {}
    T = 3
    cases = [("toy", ref_ldpc.create_test_ldpc_code(), 40)]
    Hs = load_edge_list("small_96_48")
    cases.append(("small", CachedCode(n=96, k=48, H=Hs, max_iterations=10), 6))
    for tag, code, count in cases:
        H = code.H
        g = oracle.OracleGraph(H)
        llrs = (np.round(rng.normal(0.9, 1.7, (count, code.n)) * 2) / 2).astype(np.float32)
        llrs[llrs == 0] = 0.5
        # ties the first check sweep sees: per check, edges sharing the second-smallest magnitude (arg-min edge removed)
        ties = 0
        for x in llrs:
            for i in range(g.m):
                a = np.abs(x[g.var_idx[g.check_ptr[i]:g.check_ptr[i + 1]]])
                if len(a) > 1:
                    rest = np.delete(a, int(np.argmin(a)))
                    ties += int(np.sum(rest == rest.min()) > 1)
        assert ties >= 10, ties
        out[f"{tag}_llr"] = llrs
        out[f"{tag}_tied_checks"] = np.int32(ties)
        if tag == "toy":
            out["toy_H"] = H.astype(np.uint8)
        for kind, cls in (("n2d", ref_n2d.Neural2DMinSumDecoder), ("oms", ref_n2d.Neural2DOffsetMinSumDecoder)):
            off = kind == "oms"
            dec = cls(code, weight_sharing_type=2, max_iterations=T)
            beta, alpha = set_weights(dec, rng, *((0.0, 0.6, 0.0, 0.3) if off else ()))
            gb = {k: 0.0 for k in dec.beta_weights.keys()}
            ga = {k: 0.0 for k in dec.alpha_weights.keys()}
            gl, its = [], []
            for x in llrs:
                dec.zero_grad()
                t = torch.from_numpy(x.copy()).requires_grad_(True)
                _, p, i = dec(t)
                F.binary_cross_entropy_with_logits(-p, torch.zeros_like(p)).backward()
                gl.append(t.grad.numpy().copy()); its.append(int(i))
                for k, w in dec.beta_weights.items():
                    gb[k] += 0.0 if w.grad is None else float(w.grad.item())
                for k, w in dec.alpha_weights.items():
                    ga[k] += 0.0 if w.grad is None else float(w.grad.item())
            gl, its = np.stack(gl), np.asarray(its, np.int32)
            dflt = dict(beta_default=0.0, alpha_default=0.0)
            bt, bs, at, as_ = oracle.weight_tables(g, 2, T, beta, alpha, **(dflt if off else {}))
            gbt, _, gat, _ = oracle.weight_tables(g, 2, T, gb, ga, **dflt)
            og = grad_oracle.table_grads(g, llrs, bt, bs, at, as_[g.var_idx] if off else as_, T, want_llr=True, offset=off)
            check_equal(f"grad ties iters ({tag} {kind})", og[3].astype(np.int32), its)
            for what, a, b in (("llr", og[4], gl), ("beta", og[0], gbt), ("alpha", og[1], gat)):
                if not np.allclose(a, b, rtol=2e-4, atol=2e-6):
                    raise SystemExit(f"GRAD ORACLE MISMATCH (ties, {tag} {kind}): d loss/d {what}: {np.abs(a - b).max()}")
            bk, bv = pack_weights(beta); ak, av = pack_weights(alpha)
            out.update({f"{tag}_{kind}_T": np.int32(T), f"{tag}_{kind}_iters": its, f"{tag}_{kind}_grad_llr": gl,
                        f"{tag}_{kind}_beta_keys": bk, f"{tag}_{kind}_beta_vals": bv,
                        f"{tag}_{kind}_alpha_keys": ak, f"{tag}_{kind}_alpha_vals": av,
                        f"{tag}_{kind}_grad_beta_table": gbt.astype(np.float64),
                        f"{tag}_{kind}_grad_alpha_table": gat.astype(np.float64)})
    return out


QP_WIDTHS = [(3.0, 1.3), (5.0, 1.0), (6.0, 0.8)]


def quantizer_sweep(out, prefix, cfgs, rng):
    """threshold-boundary sweep of NonUniformQuantizer, keys {prefix}_cfg and {prefix}{i}_thresholds/_x/_codes/_deq"""
    out[f"{prefix}_cfg"] = np.asarray(cfgs, dtype=np.float64)
    for ci, (bc, C_, gm) in enumerate(cfgs):
        q = ref_rcq.NonUniformQuantizer(bc=bc, C=C_, gamma=gm)
        thr32 = np.asarray(q.thresholds, dtype=np.float32)
        edge = []
        for t in thr32:
            for s in (1.0, -1.0):
                v = np.float32(s * t)
                edge += [v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))]
        # double-rounded neighbours: float32 of the fp64 threshold's neighbours
        edge += [np.float32(np.nextafter(t, np.inf)) for t in q.thresholds]
        edge += [np.float32(np.nextafter(t, -np.inf)) for t in q.thresholds]
        edge += [np.float32(0.0), np.float32(-0.0), np.float32(np.inf), np.float32(-np.inf),
                 np.float32(1e-30), np.float32(-1e-30), np.float32(1e30), np.float32(-1e30)]
        x = np.concatenate([np.asarray(edge, dtype=np.float32),
                            (rng.standard_normal(2000) * C_).astype(np.float32)])
        codes = q.quantize(torch.from_numpy(x)).numpy()
        deq = q.dequantize(torch.from_numpy(codes)).numpy()
        out[f"{prefix}{ci}_thresholds"] = np.asarray(q.thresholds, dtype=np.float64)
        out[f"{prefix}{ci}_x"] = x
        out[f"{prefix}{ci}_codes"] = codes
        out[f"{prefix}{ci}_deq"] = deq
        check_equal(f"{prefix}{ci} thr", np.asarray(oracle.quantizer_thresholds(bc, C_, gm)), out[f"{prefix}{ci}_thresholds"])
        check_equal(f"{prefix}{ci} codes", oracle.quantize(x, q.thresholds), codes)
        check_bits_exact(f"{prefix}{ci} deq", oracle.dequantize(codes, q.thresholds), deq)


def gen_rcq_widths():
    """The RCQ decoders at 2, 32, 64 and 128 levels on the 48x96 code.  A code is one byte, sign * L + level: at bc = 8 the
    negative codes use bit 7.  Flooding blocks carry every iteration's codes; the layered blocks are
    RCQMinSumDecoder(layered=True) as the reference executes it."""
    H = load_edge_list("small_96_48")
    code = CachedCode(n=96, k=48, H=H, max_iterations=10)
    rng = np.random.default_rng(8128)
    llrs = np.concatenate([awgn_llr_decoder_convention(rng, 6, 96, 2.0, np.float32),
                           awgn_llr_decoder_convention(rng, 6, 96, 5.0, np.float32),
                           special_llrs(rng, 96, 4).astype(np.float32)])
    T = 6
    out = {"graph": np.asarray("small_96_48")}
    for bc in (2, 6, 7, 8):
        for k, v in run_rcq(code, H, llrs, T, bc=bc, qp=QP_WIDTHS).items():
            out[f"rcq{bc}_{k}"] = v
    for wtype, bc in ((2, 6), (2, 8), (1, 8)):
        for k, v in run_wrcq(code, H, llrs, wtype, T, rng=rng, bc=bc, qp=QP_WIDTHS).items():
            out[f"w{wtype}b{bc}_{k}"] = v
    g = oracle.OracleGraph(H)
    for bc in (2, 8):
        dec = ref_rcq.RCQMinSumDecoder(code, bc=bc, bv=8, quantizer_params=QP_WIDTHS, max_iterations=T, layered=True)
        bits, succ, its = [], [], []
        for x in llrs:
            b, s_, i = dec.decode(torch.from_numpy(x.copy()))
            bits.append(b.numpy().copy()); succ.append(bool(s_)); its.append(int(i))
        bits, succ, its = np.stack(bits), np.asarray(succ), np.asarray(its, np.int32)
        ob, op, oi, os_ = oracle.rcq_layered(g, llrs, bc, QP_WIDTHS, T)
        check_equal("layered bits", ob, bits); check_equal("layered iters", oi, its); check_equal("layered success", os_, succ)
        out.update({f"lay{bc}_llr": llrs, f"lay{bc}_bits": bits.astype(np.uint8), f"lay{bc}_success": succ,
                    f"lay{bc}_iters": its, f"lay{bc}_T": np.int32(T), f"lay{bc}_bc": np.int32(bc),
                    f"lay{bc}_qp": np.asarray(QP_WIDTHS, np.float64), f"lay{bc}_oracle_posterior": op})
    quantizer_sweep(out, "wsweep", [(6, 5.0, 1.3), (7, 6.0, 0.8), (8, 7.0, 1.0), (8, 3.0, 1.7)], np.random.default_rng(77))
    return out


SETS = {
    "quantizer": gen_quantizer,
    "sums": gen_sums,
    "toy_basic": gen_toy_basic,
    "toy_neural2d": gen_toy_neural2d,
    "toy_rcq": gen_toy_rcq,
    "small_basic": lambda: gen_small("basic"),
    "small_neural2d": lambda: gen_small("neural2d"),
    "small_rcq": lambda: gen_small("rcq"),
    "ira_basic": lambda: gen_ira("basic"),
    "ira_neural2d": lambda: gen_ira("neural2d"),
    "ira_rcq": lambda: gen_ira("rcq"),
    "ira_wrcq": lambda: gen_ira("wrcq"),
    "toy_offset_edge": lambda: gen_offset_and_edge("toy"),
    "small_offset_edge": lambda: gen_offset_and_edge("small"),
    "layered_rcq": gen_layered,
    "grad_toy": lambda: gen_grad("toy"),
    "grad_small": lambda: gen_grad("small"),
    "grad_ira": lambda: gen_grad("ira"),
    "grad_llr_toy": gen_grad_llr,
    "grad_ties": gen_grad_ties,
    "rcq_widths": gen_rcq_widths,
}
SLOW = {"dvbs2_wrcq": gen_dvbs2_wrcq}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--slow", action="store_true")
    args = ap.parse_args()
    oracle.build()
    os.makedirs(GOLD, exist_ok=True)
    todo = dict(SETS)
    if args.slow:
        todo.update(SLOW)
    if args.only:
        allsets = {**SETS, **SLOW}
        todo = {k: allsets[k] for k in args.only}
    for name, fn in todo.items():
        t0 = time.time()
        data = fn()
        path = os.path.join(GOLD, name + ".npz")
        np.savez_compressed(path, **data)
        print(f"{name}: oracle == reference; wrote {os.path.relpath(path, ROOT)} "
              f"({os.path.getsize(path) / 1024:.0f} KiB, {time.time() - t0:.1f}s)")


if __name__ == "__main__":
    main()
