"""
Decoder families, codes, batches and inputs shared by tests/test_dirty_state_host.py (CPU: the oracle alone) and
tests/test_gpu_dirty_state.py (GPU): the property "a result is a function of the inputs only" is checked on inputs of which
the host test establishes that the ORACLE decodes between 20 % and 80 % of every batch of 64 rows or more within T, so that
every tile of the streaming engine holds rows that latch early beside rows that stay open.  One row of every batch above
three is a codeword sent strongly: it stops at iteration 1.  Not a test module: nothing here needs a GPU.

Expected outputs come from the CPU oracle (oracle/), from tests/layered_minsum_reference.py for the layered min-sum forms and
from the restatement of tests/test_gpu_layered_weighted.py for the weighted layered RCQ decoder, as the tests of those
families take them.  The reference's own layered schedule (RCQMinSumDecoder(layered=True)) has an early-stop oracle only;
`expected` says which rows and outputs that oracle pins for the other stop modes.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

import layered_minsum_cases as lm
import layered_minsum_reference as lmref
from test_gpu_layered_weighted import edge_betas
from test_gpu_layered_weighted import restate as layered_wrcq_restate
from test_gpu_parity import QP, oracle_capped, wide_check_code

F32, F64 = np.float32, np.float64
CODES = {"small": "small_96_48", "ira": "ira_1998_1512", "wide": wide_check_code}     # a shipped code's name, or what builds the code
T_OF = {"small": 10, "ira": 10, "wide": 8}
# (precision, B): fp32 1 | 64 (VEC = 1, a full tile) | 65 (VEC = 4, 191 padding codewords) | 257 (the second tile holds one
# live codeword); fp64 129 (VEC = 2).  The layered schedules run VEC = 1 at every B: 65 and 257 end in a tile of one codeword
BATCHES = {F32: (1, 64, 65, 257), F64: (129,)}
STOPS = ((True, None), (False, None), (True, 2))            # (early_stop, max_iters)
CAP = 2

# kind: how the decoder is built and restated; arg: sharing type / layered min-sum family; mode: DecodeEngine.set_mode;
# where: what DecodeEngine.info() must report ("stream_form" of a flooding decoder, "kernel" of a layered one)
Family = namedtuple("Family", "kind arg mode dtype codes where")
FAMILIES = {
    "basic32": Family("basic", None, "stream", F32, ("small", "ira", "wide"), "two-sweeps"),   # cn_sweep_f4 at VEC = 4, cn_sweep at VEC = 1
    "basic64": Family("basic", None, "stream", F64, ("small", "ira"), "two-sweeps"),
    "n2d1": Family("neural2d", 1, "stream", F32, ("small", "ira"), "two-sweeps"),
    "n2d2": Family("neural2d", 2, "stream", F32, ("small", "ira"), "two-sweeps"),
    "offset2": Family("offset", 2, "stream", F32, ("small", "ira"), "two-sweeps"),            # check-side alpha
    "rcq-pair": Family("rcq", None, "pair", F32, ("small", "ira"), "rcq-code-pair"),
    "rcq-gather": Family("rcq", None, "gather", F32, ("small", "ira"), "fused-rcq-iteration"),
    "rcq-sweeps": Family("rcq", None, "sweeps", F32, ("small", "ira", "wide"), "two-sweeps"),
    "wrcq-q4": Family("wrcq", 2, "pair", F32, ("small", "ira"), "rcq-code-pair"),             # fused entrance pass on 16-byte rows
    "lay-ref": Family("lay_ref", None, "stream", F32, ("small", "ira"), "layered_rcq<ref>"),
    "lay-paper": Family("lay_paper", 2, "stream", F32, ("small", "ira"), "layered_rcq<paper>"),
    "lay-nms": Family("lay_minsum", "n2d1", "stream", F32, ("small", "ira"), "layered_minsum"),
    "lay-oms": Family("lay_minsum", "n2d_oms", "stream", F32, ("small", "ira"), "layered_minsum"),
}
EXACT_POSTERIOR = ("rcq", "wrcq", "lay_ref", "lay_paper", "lay_minsum")      # kinds whose tests compare posteriors with array_equal

# (low, high) SNR in dB of the two halves of a batch, chosen on the CPU from the oracle's success counts alone
# (tests/test_dirty_state_host.py holds the condition)
SNR = {"small": (0.0, 6.0), "ira": (2.0, 6.0), "wide": (0.0, 9.0)}

Case = namedtuple("Case", "family code B")
DECODE_CASES = [Case(f, c, B) for f, fam in FAMILIES.items() for c in fam.codes for B in BATCHES[fam.dtype]]


def case_id(c):
    return f"{c.family}-{c.code}-B{c.B}"


def seed_of(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


def register_code(name, make, T, snr):
    """another code for the case lists built on this module (tests/row_alignment_cases.py): make() -> LDPCCode, the
    decoders' T, and the (low, high) SNR of its batches"""
    assert name not in CODES
    CODES[name], T_OF[name], SNR[name] = make, T, snr


@functools.lru_cache(maxsize=None)
def load_code(name):
    import codes
    return CODES[name]() if callable(CODES[name]) else codes.load_code(CODES[name], T_OF[name])


def oracle_graph(oracle_mod, code):
    g = code.tanner_graph()
    return oracle_mod.OracleGraph(n=g.n, check_ptr=g.check_ptr, var_idx=g.var_idx)


def fill(params, rng, lo, hi):
    with torch.no_grad():
        for p in params.values():
            p.fill_(float(np.float32(rng.uniform(lo, hi))))


_decoders = {}


def decoder(family, code_name):
    """the family's decoder on a code, with seeded weights; one object per (family, code) and process"""
    key = (family, code_name)
    if key in _decoders:
        return _decoders[key]
    from ldpc_decoder import BasicMinSumDecoder
    from neural_2d_decoder import Neural2DMinSumDecoder, Neural2DOffsetMinSumDecoder
    from rcq_decoder import RCQMinSumDecoder, WeightedRCQDecoder
    f, code, T = FAMILIES[family], load_code(code_name), T_OF[code_name]
    rng = np.random.default_rng(seed_of("w", family, code_name))
    torch.manual_seed(seed_of("init", family, code_name))
    if f.kind == "basic":
        dec = BasicMinSumDecoder(code, 0.7)
    elif f.kind == "neural2d":
        dec = Neural2DMinSumDecoder(code, f.arg, T)
        fill(dec.beta_weights, rng, 0.5, 1.0)
        fill(dec.alpha_weights, rng, 0.8, 1.2)
    elif f.kind == "offset":
        dec = Neural2DOffsetMinSumDecoder(code, f.arg, T)
        fill(dec.beta_weights, rng, 0.0, 0.4)
        fill(dec.alpha_weights, rng, 0.0, 0.1)
    elif f.kind == "rcq":
        dec = RCQMinSumDecoder(code, 3, 8, QP, T)
    elif f.kind == "wrcq":
        dec = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=f.arg, max_iterations=T)
        fill(dec.beta_weights, rng, 0.5, 1.0)
        fill(dec.alpha_weights, rng, 0.8, 1.2)
    elif f.kind == "lay_ref":
        dec = RCQMinSumDecoder(code, 3, 8, QP, T, layered=True)
    elif f.kind == "lay_paper":
        dec = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=f.arg, max_iterations=T, layered="paper")
        fill(dec.beta_weights, rng, 0.5, 1.0)
        keys = sorted(dec.beta_weights.keys())                 # one negative and one zero beta, as compact_forms_cases gives them
        with torch.no_grad():
            dec.beta_weights[keys[len(keys) // 3]].fill_(-0.6)
            dec.beta_weights[keys[2 * len(keys) // 3]].fill_(0.0)
    else:
        dec = lm.make(f.arg, code, T, seed_of("w", family, code_name) % 2 ** 31)
    _decoders[key] = dec
    return dec


def engine(family, code_name, device, mode=None):
    """the decoder's engine (the family's precision) in the family's mode, or in `mode`"""
    from simulation_framework import _engine_of
    f, dec = FAMILIES[family], decoder(family, code_name)
    eng = dec._engine(torch.float64, device) if f.dtype is F64 else _engine_of(dec, device)
    return eng.set_mode(mode or f.mode)


def awgn(rng, B, n, snr_db):
    s2 = 10.0 ** (-snr_db / 10.0)
    return 2.0 * (1.0 + np.sqrt(s2) * rng.standard_normal((B, n))) / s2


@functools.lru_cache(maxsize=None)
def llrs(family, code_name, B):
    """a permuted mix of a low and a high SNR (the first B - B/2 rows low); row 3 of a batch above three is made a strongly
    sent all-zero codeword, which every decoder here accepts after its first iteration.  Read-only."""
    n = load_code(code_name).n
    lo, hi = SNR[code_name]
    rng = np.random.default_rng(seed_of("llr", code_name, B))
    x = np.concatenate([awgn(rng, B - B // 2, n, lo), awgn(rng, B // 2, n, hi)])[rng.permutation(B)]
    if B > 3:
        x[3] = np.abs(x[3]) + 4.0
    x = np.ascontiguousarray(x.astype(FAMILIES[family].dtype))
    x.setflags(write=False)
    return x


def saturated_llrs(code_name, dtype, rows=300):
    """the "history" decode's input: +-1e30 with random signs -- no codeword, so no row ever latches, every message and
    posterior the decode leaves behind is huge, and every quantiser code is the top level"""
    rng = np.random.default_rng(seed_of("saturated", code_name))
    return (np.where(rng.random((rows, load_code(code_name).n)) < 0.5, -1e30, 1e30)).astype(dtype)


Expected = namedtuple("Expected", "bits posterior iterations success rows")
_expected = {}


def expected(oracle_mod, case, early_stop=True, cap=None):
    """what a decode of the case must return: Expected(bits, posterior, iterations, success, rows).  rows is None where the
    restatement pins every row.  For "lay-ref" outside plain early stop it is a bool mask: under fixed T the rows the
    early-stop oracle never stops run the same walk (bits and posterior pinned there, iterations = T everywhere, success is
    the syndrome of the returned bits); under a cap the rows the oracle stops within the cap are pinned in full, the others
    report iterations = cap and success False.  Computed once per process; the arrays are read-only."""
    key = (case, early_stop, cap)
    if key in _expected:
        return _expected[key]
    f, code, T = FAMILIES[case.family], load_code(case.code), T_OF[case.code]
    dec, llr = decoder(case.family, case.code), llrs(case.family, case.code, case.B)
    rows = None
    if f.kind in ("basic", "neural2d", "offset", "rcq", "wrcq"):
        wkw = {}
        if f.kind in ("neural2d", "offset", "wrcq"):
            wkw = dict(wtype=f.arg, beta={k: float(v.item()) for k, v in dec.beta_weights.items()},
                       alpha={k: float(v.item()) for k, v in dec.alpha_weights.items()})
        out = oracle_capped(oracle_mod, oracle_graph(oracle_mod, code), llr, f.kind, cap or T, T, early_stop=early_stop, **wkw)
    elif f.kind == "lay_minsum":
        beta_e, a_e = lm.edge_tables(dec, f.arg, T)
        out = lmref.restate(code.tanner_graph(), llr, T, lm.form_of(f.arg), beta_e, a_e, early_stop, cap)[:4]
    elif f.kind == "lay_paper":
        out = layered_wrcq_restate(code, llr, 3, QP, T, edge_betas(dec, T), early_stop=early_stop, max_iters=cap)
    else:
        ob, op, oi, os_ = oracle_mod.rcq_layered(oracle_graph(oracle_mod, code), llr, 3, QP, T)
        if early_stop and cap is None:
            out = (ob, op, oi, os_)
        elif not early_stop:
            out, rows = (ob, op, np.full_like(oi, T), None), ~os_
        else:
            rows = os_ & (oi <= cap)
            out = (ob, op, np.where(rows, oi, cap).astype(np.int32), rows.copy())
    out = Expected(*[None if a is None else np.asarray(a) for a in out[:4]], rows)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    _expected[key] = out
    return out
