"""
Codes, decoders and inputs of the block-parallel layered decode's tests (tests/test_block_layered_host.py and
tests/test_layer_plan_host.py on the CPU, tests/test_gpu_block_layered.py on the GPU).  All files decode the SAME graphs
and input sets, so what the host test establishes about them -- the restatement decodes between 20 % and 80 % of every
set and shows at least two distinct stop iterations, so frozen rows sit beside live ones in a workgroup -- holds for the
GPU comparison.

The yardsticks are imported, not restated: ``layered_minsum_reference.restate`` for the min-sum forms and the
``restate`` of tests/test_gpu_layered_weighted.py for the RCQ forms.  Both walk the checks one by one in CSR order; the
block-parallel kernel must return their bits on the same graph (include/ldpc_hip.h, LDPC_MODE_BLOCK).
"""
import functools

import numpy as np
import torch

import layered_minsum_cases as ms
import layered_minsum_reference as ref
import test_gpu_layered_weighted as wl

MAX_DEG = 64            # the check record's widest check (csrc/ldpc_layer_plan.h kBlkMaxDeg)

# (mb, nb, Z, info_degree_profile, seed): what each shape probes is in the comments
QC_SHAPES = {
    "qc_3_6_5": (3, 6, 5, {2: 2, 3: 1}, 365),          # several codewords and layers inside one wave
    "qc_4_8_64": (4, 8, 64, {3: 3, 4: 1}, 4864),       # a layer is exactly a wave
    "qc_4_8_65": (4, 8, 65, {3: 3, 4: 1}, 4865),       # a layer is one check over a wave
    "qc_2_5_130": (2, 5, 130, {2: 3}, 25130),          # a layer exceeds two waves
}


def ragged_graph():
    """random graph with an odd number of variables and of checks: a degree-0 check, a degree-1 check, a check of degree 33
    and one at the record format's widest degree beside random ones, variable degree <= 6; put through ``layered_order``,
    so layer sizes run from 1 up"""
    import codes
    from tanner_graph import TannerGraph
    rng = np.random.default_rng(777)
    n = 151
    degs = [0, 1, 33, MAX_DEG] + [int(rng.integers(2, 9)) for _ in range(33)]
    degs = [degs[i] for i in rng.permutation(len(degs))]
    assert n % 2 == 1 and len(degs) % 2 == 1
    load = np.zeros(n, dtype=np.int64)
    rows, cols = [], []
    for i, dc in enumerate(degs):
        pick = rng.choice(np.flatnonzero(load < 6), size=dc, replace=False)
        load[pick] += 1
        rows += [i] * dc
        cols += pick.tolist()
    g, _ = codes.layered_order(TannerGraph(n, len(degs), np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64)))
    return g


@functools.lru_cache(maxsize=None)
def graph(name):
    """case graph by name; every one declares layers"""
    import codes
    import tanner_graph
    if name in QC_SHAPES:
        mb, nb, Z, prof, seed = QC_SHAPES[name]
        return codes.generate_qc_code(mb, nb, Z, prof, seed)
    if name == "ragged":
        return ragged_graph()
    if name == "runs_small":                                    # degenerate: every layer is one check
        g = codes.load_graph("small_96_48")
        return g.with_layers(tanner_graph.disjoint_runs(g))
    if name == "ira_lo":
        return codes.layered_order(codes.load_graph("ira_1998_1512"))[0]
    if name == "qc_1944":
        return codes.load_graph("qc_1944_972")
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def code(name):
    from ldpc_decoder import LDPCCode
    g = graph(name)
    return LDPCCode.from_graph(g, k=g.n - g.m, max_iterations=10)


GRAPHS = tuple(QC_SHAPES) + ("ragged", "runs_small", "ira_lo", "qc_1944")
SMALL_GRAPHS = tuple(QC_SHAPES) + ("ragged", "runs_small")          # those every family and form runs on

# input sets: graph -> (rows, (snr_a, snr_b), seed).  Rows alternate between the two SNRs; row 0 starts with exact zeros
# and row 1 is rounded to integers (ties).  Tuned on the restatement (basic, beta 0.7, T = 10): 20-80 % decoded.
INPUTS = {
    "qc_3_6_5": (48, (0.0, 4.0), 1),
    "qc_4_8_64": (48, (2.0, 3.0), 2),
    "qc_4_8_65": (48, (2.0, 3.0), 3),
    "qc_2_5_130": (48, (4.0, 5.5), 4),
    "ragged": (48, (0.0, 6.0), 5),
    "runs_small": (48, (1.0, 2.5), 6),
    "ira_lo": (128, (4.0, 5.0), 7),
    "qc_1944": (64, (1.5, 2.0), 8),
}
T = 10


@functools.lru_cache(maxsize=None)
def input_llr(name):
    rows, (sa, sb), seed = INPUTS[name]
    n = graph(name).n
    rng = np.random.default_rng(5000 + seed)
    llr = np.empty((rows, n), dtype=np.float32)
    llr[0::2] = ms.awgn(rng, len(llr[0::2]), n, sa)
    llr[1::2] = ms.awgn(rng, len(llr[1::2]), n, sb)
    llr[0, :3] = 0.0
    llr[1] = np.round(llr[1])
    llr.setflags(write=False)
    return llr


# ---- min-sum families (the decoders and tables of tests/layered_minsum_cases.py) -----------------------------------------
FAMILIES = ("basic", "n2d1", "n2d_oms", "edge_oms")


def make_minsum(family, name, T_=T, seed=11):
    return ms.make(family, code(name), T_, seed)


_REF = {}


def reference_minsum(name, family, T_=T, early_stop=True, max_iters=None, rows=None, seed=11, reversed_layers=False):
    """restatement of the min-sum family on the case graph (``reversed_layers``: on the graph whose rows are reversed
    inside every layer, with the tables carried along), computed once per argument tuple and read-only;
    -> (bits, P, iterations, success)"""
    key = ("ms", name, family, T_, early_stop, max_iters, rows, seed, reversed_layers)
    if key not in _REF:
        dec = make_minsum(family, name, T_, seed)
        beta_e, a_e = ms.edge_tables(dec, family, T_)
        g = graph(name)
        if reversed_layers:
            g, idx = reversed_inside_layers(name)
            beta_e, a_e = beta_e[:, idx], (None if a_e is None else a_e[:, idx])
        llr = input_llr(name) if rows is None else input_llr(name)[:rows]
        out = ref.restate(g, llr, T_, ms.form_of(family), beta_e, a_e, early_stop, max_iters)[:4]
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


# ---- W-RCQ forms: (bc, quantiser parameters, sharing type, unit beta) -------------------------------------------------------
QP3 = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]
RCQ_FORMS = {
    "t1_l4": (3, QP3, 1, False),
    "t2_l8": (4, QP3, 2, False),
    "t2_l16": (5, [(6.0, 1.2)], 2, False),
    "t1_g0": (3, [(2.5, 0.0), (4.0, 1.3)], 1, False),     # one gamma = 0 table: every threshold of it equals C
    "unit_l4": (3, QP3, 2, True),                         # beta == 1: the unweighted schedule (no product)
}


def make_rcq(form, name, T_=T, seed=21):
    from rcq_decoder import WeightedRCQDecoder
    bc, qp, wtype, unit = RCQ_FORMS[form]
    torch.manual_seed(seed)
    dec = WeightedRCQDecoder(code(name), bc, 8, qp, weight_sharing_type=wtype, max_iterations=T_, layered="paper")
    if unit:
        with torch.no_grad():
            for p in dec.beta_weights.values():
                p.fill_(1.0)
    else:
        rng = np.random.default_rng(seed)
        if wtype == 1:                                        # seeded init plus a perturbation, some zero and negative slots
            wl.randomise_betas(dec, rng)
        else:                                                 # near 1: these forms also decode part of every input set
            with torch.no_grad():
                for p in dec.beta_weights.values():
                    p.fill_(float(np.float32(rng.uniform(0.8, 1.1))))
    return dec


def rcq_edge_betas(dec, T_):
    """beta_t of every CSR edge from the decoder's parameters (the unit form: all ones, the host test asserts it)"""
    return wl.edge_betas(dec, max(T_, 1))


def reference_rcq(name, form, T_=T, early_stop=True, max_iters=None, rows=None, seed=21, reversed_layers=False):
    key = ("rcq", name, form, T_, early_stop, max_iters, rows, seed, reversed_layers)
    if key not in _REF:
        bc, qp, _, _ = RCQ_FORMS[form]
        dec = make_rcq(form, name, T_, seed)
        beta_e = rcq_edge_betas(dec, T_)
        c = code(name)
        if reversed_layers:
            from ldpc_decoder import LDPCCode
            g2, idx = reversed_inside_layers(name)
            beta_e = beta_e[:, idx]
            c = LDPCCode.from_graph(g2, k=g2.n - g2.m, max_iterations=10)
        llr = input_llr(name) if rows is None else input_llr(name)[:rows]
        out = wl.restate(c, llr, bc, qp, T_, beta_e, early_stop=early_stop, max_iters=max_iters)
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


# ---- the legality claim's other check order ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reversed_inside_layers(name):
    """-> (graph, edge_idx): the case graph with its rows reversed inside every layer (same layers, same code); edge e of
    it is edge edge_idx[e] of the case graph (a row keeps its edges in ascending variable order)"""
    from tanner_graph import TannerGraph
    g = graph(name)
    lp = g.layer_ptr
    perm = np.concatenate([np.arange(lp[l + 1] - 1, lp[l] - 1, -1) for l in range(len(lp) - 1)])
    new_row = np.empty(g.m, dtype=np.int64)
    new_row[perm] = np.arange(g.m)
    g2 = TannerGraph(g.n, g.m, new_row[g.check_of_edge], g.var_idx).with_layers(lp)
    edge_idx = np.concatenate([np.arange(g.check_ptr[i], g.check_ptr[i + 1]) for i in perm] + [np.zeros(0, dtype=np.int64)])
    assert np.array_equal(g2.var_idx, g.var_idx[edge_idx])
    return g2, edge_idx.astype(np.int64)
