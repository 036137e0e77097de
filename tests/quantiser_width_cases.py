"""
Case list shared by tests/test_quantiser_widths.py (host: the oracle alone) and tests/test_gpu_quantiser_widths.py (GPU): the
RCQ decoders at the quantiser widths no other test reaches -- 2, 32, 64 and 128 levels through the classes (bc 2, 6, 7, 8) and
1, 9, 62, 63, 127 and 128 levels on engines built directly -- with their seeded weights, codes and inputs.

A code is one byte, (w < 0) * L + level.  At L = 128 the negative codes use bit 7 and level 127 fills the low seven; the
code-pair form is admitted up to 62 levels; the dword kernels pad eight threshold registers below eight levels and L = 9 is the
first count on the threshold loop.

The inputs are the all-zero codeword over an AWGN channel, rows alternating between a low and a high SNR, then four special
rows (ties and zeros, every third LLR zero, +inf and -inf entries).  They are chosen so that the oracle decodes part of every
batch, both signs of the top level occur and nearly every code value is written in the last executed iteration
(tests/test_quantiser_widths.py asserts it).  Not a test module (no test_ prefix): nothing here needs a GPU.
"""
from collections import namedtuple

import numpy as np
import torch

QP_W = [(3.0, 1.3), (5.0, 1.0), (6.0, 0.8)]
T_SMALL = 7                                    # three quantisers: iterations 0-1, 2-3, 4-6
T_ODD = 5
DEFAULT_SNR = (1.0, 4.0)

# dec: "rcq" (RCQMinSumDecoder), "w1" / "w2" (WeightedRCQDecoder, beta per edge class / per check); code: "small" / "odd"
Flood = namedtuple("Flood", "dec bc B code chunk")
# an engine built directly: L levels, thresholds row q = C_q * (j / (L - 1))^g_q, for L = 1 the single threshold tau0
Level = namedtuple("Level", "L tau0 B chunk")
# dec: "ref" (RCQMinSumDecoder(layered=True)), "paper" (layered="paper"), "wpaper" (WeightedRCQDecoder(layered="paper"))
Lay = namedtuple("Lay", "dec bc B")

WIDTHS = (2, 6, 7, 8)
# (rows of the batch, rows per decode call).  300 at once: a 256-codeword tile plus a partial one.  320 decoded 40 rows at a
# time: 64-codeword tiles.  A batch of 40 alone holds about 11 000 codes, too few to meet 95 % of 256 code values -- the negative
# codes of the upper levels are rare on an all-zero codeword -- so the small-tile path decodes a batch of 320 in eight calls.
BATCHES = ((300, 300), (320, 40))


def flood_cases():
    cases = [Flood(d, bc, B, "small", ch) for d in ("rcq", "w1", "w2") for bc in WIDTHS for B, ch in BATCHES]
    return cases + [Flood("w2", bc, 300, "odd", 300) for bc in (6, 8)]


def level_cases():
    cases = [Level(L, 0.0, B, ch) for L in (1, 9, 62, 63, 127, 128) for B, ch in BATCHES]
    return cases + [Level(1, 1.5, B, ch) for B, ch in BATCHES]


def layered_cases():
    return [Lay(d, bc, B) for d in ("ref", "paper", "wpaper") for bc in (2, 6, 8) for B in (63, 130)]


def case_id(c):
    if isinstance(c, Flood):
        return f"{c.dec}-bc{c.bc}-B{c.B}" + (f"x{c.chunk}" if c.chunk != c.B else "") + ("-odd" if c.code == "odd" else "")
    if isinstance(c, Level):
        return f"L{c.L}-B{c.B}" + (f"x{c.chunk}" if c.chunk != c.B else "") + (f"-tau{c.tau0}" if c.tau0 else "")
    return f"{c.dec}-bc{c.bc}-B{c.B}"


# (low, high) SNR in dB of a case's rows; DEFAULT_SNR unless listed.  Chosen on the CPU from the oracle's outputs alone
# (tests/test_quantiser_widths.py holds the conditions).  One level carries no magnitude: the decode is the channel's own
# hard decision (tau = 0), which needs a cleaner channel to decode anything; two levels with weights decode little at 1 dB.
SNR = {}
for _B, _ch in BATCHES:
    for _d in ("w1", "w2"):
        SNR[Flood(_d, 2, _B, "small", _ch)] = (2.0, 5.0)
    SNR[Level(1, 0.0, _B, _ch)] = (5.0, 8.0)
SNR[Level(128, 0.0, 320, 40)] = (2.0, 5.0)


def snr_of(c):
    return SNR.get(c, DEFAULT_SNR)


def seed_of(c):
    """100 * bc + B for the decoders of the classes; the directly built engines have no bc: 100 * (20 + L) + B + (1 for tau0)"""
    if isinstance(c, Level):
        return 100 * (20 + c.L) + c.B + (1 if c.tau0 else 0)
    return 100 * c.bc + c.B


def make_code(c):
    import codes
    if isinstance(c, Flood) and c.code == "odd":
        from test_gpu_parity import odd_code
        code = odd_code()
        code.max_iterations = T_ODD
        return code, T_ODD
    return codes.load_code("small_96_48", T_SMALL), T_SMALL


def llrs(seed, B, n, snr):
    """row r: llr = 2 (1 + sigma z) / sigma^2 at snr[r % 2] dB, z drawn row by row; then the special rows 0..3"""
    rng = np.random.default_rng(seed)
    x = np.empty((B, n), np.float32)
    for r in range(B):
        s2 = 10.0 ** (-snr[r % 2] / 10.0)
        x[r] = (2.0 * (1.0 + np.sqrt(s2) * rng.standard_normal(n)) / s2).astype(np.float32)
    x[0] = np.round(x[0])                                        # ties and exact zeros
    x[1 % B, ::3] = 0.0
    if B > 3:                                                    # saturated inputs: |beta * inf| = inf, 0 * inf = NaN -> code 0
        x[2, ::5] = np.inf
        x[3, 1::4] = -np.inf
    return x


def oracle_graph(oracle_mod, code):
    g = code.tanner_graph()
    return oracle_mod.OracleGraph(n=g.n, check_ptr=g.check_ptr, var_idx=g.var_idx)


def seed_weights(dec, seed):
    """betas in 0.5 .. 1.0, alphas in 0.8 .. 1.2, then one negative and one zero beta slot (sign of beta * min, all-zero
    magnitudes), as test_rcq_code_pair_form_edge_cases and compact_forms_cases.build_decoder give them"""
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for p in dec.beta_weights.values():
            p.fill_(float(np.float32(rng.uniform(0.5, 1.0))))
        for p in dec.alpha_weights.values():
            p.fill_(float(np.float32(rng.uniform(0.8, 1.2))))
        keys = sorted(dec.beta_weights.keys())
        dec.beta_weights[keys[len(keys) // 3]].fill_(-0.6)
        dec.beta_weights[keys[2 * len(keys) // 3]].fill_(0.0)
    return ({k: float(v.item()) for k, v in dec.beta_weights.items()},
            {k: float(v.item()) for k, v in dec.alpha_weights.items()})


def build_flood(c, layered=False):
    """-> (decoder, test_gpu_parity.oracle_capped keyword arguments of it, T)"""
    from rcq_decoder import RCQMinSumDecoder, WeightedRCQDecoder
    code, T = make_code(c)
    if c.dec in ("rcq", "ref", "paper"):
        return RCQMinSumDecoder(code, c.bc, 8, QP_W, T, layered=layered), dict(kind="rcq", bc=c.bc, qp=QP_W), T
    wtype = 1 if c.dec == "w1" else 2
    dec = WeightedRCQDecoder(code, c.bc, 8, QP_W, weight_sharing_type=wtype, max_iterations=T, layered=layered)
    beta, alpha = seed_weights(dec, 7000 + seed_of(c) + wtype)
    return dec, dict(kind="wrcq", bc=c.bc, qp=QP_W, wtype=wtype, beta=beta, alpha=alpha), T


def pair_admitted(c):
    """the header's gate (include/ldpc_hip.h): one beta per check, sorted positive thresholds, at most 62 levels"""
    if isinstance(c, Level):
        return c.L <= 62
    return c.dec != "w1" and 2 ** (c.bc - 1) <= 62


def level_tables(oracle_mod, c):
    """-> (code, T, keyword arguments shared by oracle.decode and engine.DecodeEngine: one beta per check (sharing type 2 with
    seeded weights, one negative and one zero slot), thresholds [3, L], the schedule of T)"""
    code, T = make_code(c)
    og = oracle_graph(oracle_mod, code)
    rng = np.random.default_rng(9000 + seed_of(c))
    dcs, dvs = sorted(set(og.dc.tolist())), sorted(set(og.dv.tolist()))
    beta = {f"iter_{t}_dc{d}": float(np.float32(rng.uniform(0.5, 1.0))) for t in range(T) for d in dcs}
    alpha = {f"iter_{t}_dv{d}": float(np.float32(rng.uniform(0.8, 1.2))) for t in range(T) for d in dvs}
    keys = sorted(beta)
    beta[keys[len(keys) // 3]] = -0.6
    beta[keys[2 * len(keys) // 3]] = 0.0
    bt, bs, at, as_ = oracle_mod.weight_tables(og, 2, T, beta, alpha)
    if c.L == 1:
        thr = np.full((3, 1), c.tau0, np.float32)
    else:
        thr = np.asarray([[C * (j / (c.L - 1)) ** g for j in range(c.L)] for C, g in QP_W], dtype=np.float32)
    return code, T, dict(beta=bt, beta_slot=bs, alpha=at, alpha_slot=as_, thresholds=thr,
                         q_of_iter=oracle_mod.quantizer_schedule(T, 3))


def case_inputs(c):
    code, _ = make_code(c)
    return llrs(seed_of(c), c.B, code.n, snr_of(c))


_expect = {}


def expected(oracle_mod, c, early_stop):
    """oracle outputs of a flooding or level case, once per process
    -> (bits, posterior, iterations, success, codes [B, E] of every codeword's last executed iteration)"""
    key = (c, bool(early_stop))
    if key not in _expect:
        llr = case_inputs(c)
        if isinstance(c, Level):
            code, T, kw = level_tables(oracle_mod, c)
            out = oracle_mod.decode(oracle_graph(oracle_mod, code), llr, T=T, early_stop=early_stop,
                                    c2v_form=oracle_mod.C2V_RCQ, trace_codes=True, **kw)
        else:
            from test_gpu_parity import oracle_capped
            dec, wkw, T = build_flood(c)
            out = oracle_capped(oracle_mod, oracle_graph(oracle_mod, dec.code), llr, t=T, T=T, early_stop=early_stop,
                                trace_codes=True, **wkw)
        b, p, i, s, codes = out
        _expect[key] = (b, p, i, s, np.stack([codes[r, i[r] - 1] for r in range(len(i))]))
    return _expect[key]


def n_levels(c):
    return c.L if isinstance(c, Level) else 2 ** (c.bc - 1)


def figures(c, want):
    """-> (decoded share of the batch, code values seen in the last executed iteration, negative top level seen, positive
    top level seen)"""
    _, _, _, succ, last = want
    L = n_levels(c)
    seen = np.unique(last)
    return float(succ.mean()), len(seen), int(np.sum(last == 2 * L - 1)), int(np.sum(last == L - 1))


# ---- layered ------------------------------------------------------------------------------------------------------------
def layered_expected(oracle_mod, c):
    """early-stop reference of a layered case -> (llr, bits, posterior, iterations, success, fixed-T outputs or None, whether a
    code with the top level and a negative sign is held when the decode ends (None where the reference keeps no messages))"""
    key = ("lay", c)
    if key not in _expect:
        dec, wkw, T = build_flood(c, layered=True if c.dec == "ref" else "paper")
        llr = case_inputs(c)
        if c.dec == "wpaper":
            from test_gpu_layered_weighted import edge_betas, restate
            be = edge_betas(dec, T)
            b, p, i, s, held = restate(dec.code, llr, c.bc, QP_W, T, be, want_messages=True)
            fixed = restate(dec.code, llr, c.bc, QP_W, T, be, early_stop=False)
            neg_top = bool(np.any(held == 2 ** c.bc - 1))
        else:
            b, p, i, s = oracle_mod.rcq_layered(oracle_graph(oracle_mod, dec.code), llr, c.bc, QP_W, T, paper=c.dec == "paper")
            fixed, neg_top = None, None
        _expect[key] = (llr, b, p, i, s, fixed, neg_top)
    return _expect[key]
