"""
Decoders, inputs and the shared restatement results of the layered posterior-joint-training tests
(tests/test_layered_joint_training_host.py on the CPU, tests/test_gpu_layered_joint_training.py on the GPU).  Graphs,
decoder families and the AWGN operating points are those of tests/layered_minsum_cases.py, whose host test establishes
that the layered decode answers the syndrome both ways there.
"""
import functools

import numpy as np
import torch

import layered_minsum_cases as lay
import layered_minsum_reference as ref
import layered_pjt_reference as pjt

HOW = "posterior_local"

# graph name -> (name for layered_minsum_cases.load, SNR points of its input set there)
GRAPHS = {"toy": ("toy", (-9.0, 3.0)), "small": ("small_96_48", (1.5,)), "wide": ("wide", (3.0, 9.0)),
          "deg01": ("lw8", (-2.0, 6.0))}       # lw8: 13 checks, one of degree 1 and one of degree 0, widest 8

# (graph, family, T, B, inputs): every family, T = 1 and 4, one lane / a full tile / a tile boundary / three tiles with
# padding, the four graphs; "half" = half-integer LLRs with zeros (exact ties and exact zeros)
CASES = [
    ("toy", "n2d1", 1, 1, "awgn"), ("toy", "n2d2", 4, 64, "awgn"), ("toy", "n2d_oms", 4, 65, "awgn"),
    ("toy", "edge_nms", 1, 130, "awgn"), ("toy", "edge_oms", 4, 130, "half"),
    ("small", "n2d3", 4, 65, "awgn"), ("small", "n2d4", 1, 64, "awgn"), ("small", "n2d_oms", 1, 130, "awgn"),
    ("small", "edge_oms", 4, 1, "awgn"), ("small", "n2d2", 4, 130, "half"),
    ("wide", "n2d1", 4, 65, "awgn"), ("wide", "n2d_oms", 4, 64, "awgn"), ("wide", "edge_nms", 1, 1, "half"),
    ("deg01", "n2d2", 4, 130, "awgn"), ("deg01", "n2d_oms", 1, 65, "half"), ("deg01", "edge_nms", 4, 64, "awgn"),
    ("deg01", "edge_oms", 4, 65, "awgn"),
]


def code_of(graph):
    return lay.load(GRAPHS[graph][0])


def make(graph, family, T, seed):
    """layered decoder with layered_minsum_cases' seeded weights (the normalised forms: one beta exactly 0 and one
    negative), the offset forms additionally with one offset of 2.5 -- large enough to close relus"""
    dec = lay.make(family, code_of(graph), T, seed, schedule="layered")
    if lay.form_of(family) == ref.OMS:
        betas = list(dec.beta_weights.values())
        with torch.no_grad():
            betas[int(np.random.default_rng(seed).integers(len(betas)))].fill_(2.5)
    return dec


def tables_of(dec, family):
    """differentiable tables built from the decoder's parameters the way the decoder builds them
    -> (beta_table [T, Sb], beta_slot [E], oms_table | None, oms_slot | None, offset)"""
    import autograd_bridge as ab
    T = int(dec.max_iterations)
    g = dec.code.tanner_graph()
    offset = lay.form_of(family) == ref.OMS
    if family.startswith("edge"):
        rows, cols = g.check_of_edge.tolist(), g.var_idx.tolist()
        params = [dec.beta_weights[f"iter_{t}_c{i}_v{j}"] for t in range(T) for i, j in zip(rows, cols)]
        bt = ab.table_from_params(params, [(t, e) for t in range(T) for e in range(g.E)], (T, g.E), 0.0)
        return bt, np.arange(g.E), None, None, offset
    layout = dec._sharing_layout()
    bt, at = layout.tables_torch(dec.beta_weights, dec.alpha_weights, T, dec._beta_default, dec._alpha_default)
    if offset:
        return bt, layout.beta_slot, at, layout.alpha_edge_slot, True
    return bt, layout.beta_slot, None, None, False


def grads_of(dec):
    return {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()).cpu() for k, p in dec.named_parameters()}


def llr_of(graph, B, kind, seed):
    code = code_of(graph)
    snrs = GRAPHS[graph][1]
    rng = np.random.default_rng(7000 + seed)
    parts = np.array_split(np.arange(B), len(snrs))
    llr = np.concatenate([lay.awgn(rng, len(p), code.n, snr) for p, snr in zip(parts, snrs) if len(p)])
    llr = llr[rng.permutation(B)]
    if kind == "half":
        llr = (np.round(2.0 * llr) / 2.0).astype(np.float32)
        llr[rng.random(llr.shape) < 0.05] = 0.0
    return np.ascontiguousarray(llr, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> (llr [B, n] float32, targets | None, iteration weights | None): every other case has custom iteration weights
    and soft targets"""
    graph, _, T, B, kind = CASES[case]
    llr = llr_of(graph, B, kind, case)
    rng = np.random.default_rng(50 + case)
    custom = case % 2 == 1
    w = torch.tensor(rng.uniform(0.1, 1.0, T), dtype=torch.float32) if custom else None
    y = (torch.from_numpy(rng.uniform(0, 1, llr.shape).astype(np.float32) * (rng.random(llr.shape) < 0.3))
         if custom else None)
    llr.setflags(write=False)
    return llr, y, w


def decoder_of(case):
    graph, family, T, _, _ = CASES[case]
    return make(graph, family, T, seed=case)


def restate(dec, family, llr, y=None, w=None, want_llr=True):
    """the restatement on the decoder's CURRENT parameters; leaves d J/d parameter in the parameters' .grad
    -> dict(loss, per_iter [T], P [T, B, n] fp32, U [T, B, E] fp32, grad_llr [B, n] | None)"""
    T = int(dec.max_iterations)
    g = dec.code.tanner_graph()
    beta_e, a_e = lay.edge_tables(dec, family, T)
    U, P = pjt.walk(g, llr, T, lay.form_of(family), beta_e, a_e)
    bt, bslot, ot, oslot, offset = tables_of(dec, family)
    x = torch.from_numpy(np.asarray(llr, np.float64)).requires_grad_(want_llr)
    J, per = pjt.forward(g, x, U, P, bt, bslot, ot, oslot, offset, y, w)
    J.backward()
    return {"loss": float(J.detach()), "per_iter": np.array([float(v.detach()) for v in per]), "P": P, "U": U,
            "grad_llr": x.grad.numpy() if want_llr else None}


_RESTATED = {}


def restated(case):
    """the restatement's result for a case, computed once and shared between the tests (arrays read-only)
    -> dict(loss, per_iter, P, U, grad_llr, grads {parameter name: tensor}, tables (beta_e, a_e))"""
    if case not in _RESTATED:
        llr, y, w = inputs(case)
        dec = decoder_of(case)
        r = restate(dec, CASES[case][1], llr, y, w)
        r["grads"] = grads_of(dec)
        r["tables"] = lay.edge_tables(dec, CASES[case][1], CASES[case][2])
        for k in ("per_iter", "P", "U", "grad_llr"):
            r[k].setflags(write=False)
        _RESTATED[case] = r
    return _RESTATED[case]


# ---------------------------------------------------------------------------------------------------- the trainer test
TRAIN = dict(code="small_96_48", T=5, wtype=2, start=0.3, batch_size=64, num_epochs=6, learning_rate=0.05,
             snr_range=(1.0, 4.0), seed=9, torch_seed=5, num_train=512, num_val=128)


def trainer_model():
    """small_96_48 layered N-2D-NMS with every weight at 0.3: a beta far below what min-sum wants"""
    import codes
    from neural_2d_decoder import Neural2DMinSumDecoder
    t = TRAIN
    code = codes.load_code(t["code"], max_iterations=t["T"])
    model = Neural2DMinSumDecoder(code, t["wtype"], t["T"], schedule="layered", layered_gradient=HOW)
    with torch.no_grad():
        for p in model.parameters():
            p.fill_(t["start"])
    return code, model


def trainer_config(device):
    from training_framework import TrainingConfig
    t = TRAIN
    return TrainingConfig(batch_size=t["batch_size"], num_epochs=t["num_epochs"], learning_rate=t["learning_rate"],
                          snr_range=t["snr_range"], device=device, seed=t["seed"], joint_posterior_loss=True)
