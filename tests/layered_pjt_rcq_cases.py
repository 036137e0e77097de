"""
Decoders, inputs and the shared restatement results of the layered W-RCQ posterior-joint-training tests
(tests/test_layered_joint_training_rcq_host.py on the CPU, tests/test_gpu_layered_joint_training_rcq.py on the GPU).
Modelled on tests/pjt_rcq_cases.py: its graphs (the ``wide`` one included), quantiser parameters, weight recipe and channel,
at batches of 1, 3, 37 and 67 codewords (one lane, a few, part of a 64-codeword tile, a tile boundary).
Test infrastructure, not product code.
"""
import functools

import numpy as np
import torch

import pjt_rcq_cases as flood

QP3 = flood.QP3
T_GRAD = flood.T_GRAD                          # three quantisers over four iterations: schedule 0, 1, 2, 2 -- the code an
                                               # iteration subtracts was written with another quantiser than it updates with
HOW = dict(quantizer_gradient="straight_through", layered_gradient="posterior_local")

# (code, sharing type, bc, quantiser parameters, B, SNR range in dB, special)
#   "gamma0"  : gamma = 0, every threshold of a quantiser equals C (two levels in effect, level 0 reconstructs C)
#   "negbeta" : one beta slot of iteration 1 negative, one of iteration 2 exactly zero
#   "saturate": a clean channel, most messages above the top threshold
#   "wide"    : pjt_rcq_cases.wide_code (a degree-40 check: the kernel's two-pass body; a degree-10 variable); every other
#               graph has checks of at most 32 edges and takes the held body
# The SNR ranges are pjt_rcq_cases' where that leaves at least 2 % of the (b, t, e) triples saturated and 2 % not (the host
# test asserts it on the restatement's codes), and higher on the high-rate (1998,1512) code, the negative-beta set and the
# two-level set, whose messages are smaller.
# every set: exact-zero LLRs at the head of row 0 (sign(0)) and, from two rows on, an integer-rounded row 1 (ties)
CASES = [
    ("toy", 1, 3, QP3, 37, (0.5, 4.0), None),
    ("toy", 4, 4, QP3, 3, (0.5, 4.0), None),
    ("small", 2, 3, QP3, 67, (0.5, 4.0), None),
    ("small", 3, 4, QP3, 37, (0.5, 4.0), None),
    ("ira", 2, 3, QP3, 37, (4.0, 7.0), None),
    ("small", 2, 3, [(2.0, 0.0), (3.0, 0.0), (4.0, 0.0)], 67, (0.5, 4.0), "gamma0"),
    ("small", 2, 3, QP3, 37, (3.0, 6.0), "negbeta"),
    ("small", 1, 3, QP3, 67, (4.0, 7.0), "saturate"),
    ("wide", 2, 3, QP3, 67, (0.5, 4.0), "wide"),
    ("wide", 2, 8, QP3, 37, (0.5, 4.0), "wide"),
    # 2 and 128 levels: at bc = 8 the negative codes use bit 7 and reach 255
    ("small", 2, 2, QP3, 1, (5.0, 8.0), None),
    ("small", 2, 8, QP3, 67, (0.5, 4.0), None),
    ("ira", 2, 8, QP3, 3, (3.0, 6.0), None),
]

load = flood.load
quantiser_tables = flood.quantiser_tables


def make_decoder(code, wtype, bc, qp, T, seed, special=None, **kw):
    """``WeightedRCQDecoder(layered="paper")`` with pjt_rcq_cases' seeded weights; keywords: the two gradient options"""
    dec = flood.make_decoder(code, wtype, bc, qp, T, seed, negbeta=special == "negbeta", layered="paper", **kw)
    if special == "negbeta":
        with torch.no_grad():
            dec.beta_weights[sorted(k for k in dec.beta_weights.keys() if k.startswith("iter_2_"))[0]].fill_(0.0)
    return dec


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> (code, llr [B, n] float32, targets | None, iteration weights | None); every other case has custom iteration
    weights and soft targets"""
    name, _, _, _, B, snr, _ = CASES[case]
    code = load(name, T_GRAD)
    rng = np.random.default_rng(150 + case)
    llr = flood.channel(rng, B, code.n, snr)
    llr[0, :3] = 0.0
    if B > 1:
        llr[1] = np.round(llr[1])
    custom = case % 2 == 1
    w = torch.tensor(rng.uniform(0.1, 1.0, T_GRAD), dtype=torch.float32) if custom else None
    y = (torch.from_numpy(rng.uniform(0, 1, (B, code.n)).astype(np.float32) * (rng.random((B, code.n)) < 0.3))
         if custom else None)
    llr.setflags(write=False)
    return code, llr, y, w


def decoder_of(case, **kw):
    _, wtype, bc, qp, _, _, special = CASES[case]
    return make_decoder(inputs(case)[0], wtype, bc, qp, T_GRAD, seed=case, special=special, **kw)


def edge_betas(dec):
    """beta_t of every CSR edge, from the tables the decoder uploads -> fp32 [T, E]"""
    beta, _ = dec.weight_tables()
    return np.ascontiguousarray(beta[:, dec._sharing_layout().beta_slot], dtype=np.float32)


def walk_of(dec, llr):
    import layered_pjt_rcq_reference as ref
    thr, qoi = quantiser_tables(dec)
    return ref.walk(dec.code.tanner_graph(), llr, int(dec.max_iterations), edge_betas(dec), thr, qoi)


def restate(dec, llr, y=None, w=None, want_llr=True):
    """the restatement on the decoder's CURRENT parameters; leaves d J/d parameter in the parameters' .grad
    -> dict(loss, per_iter [T], U, K, P, disagree, grad_llr [B, n] | None, grad_beta [T, Sb]: d J/d the beta TABLE)"""
    import layered_pjt_rcq_reference as ref
    T = int(dec.max_iterations)
    g = dec.code.tanner_graph()
    lay = dec._sharing_layout()
    thr, qoi = quantiser_tables(dec)
    U, K, P = walk_of(dec, llr)
    bt, _ = lay.tables_torch(dec.beta_weights, dec.alpha_weights, T, dec._beta_default, dec._alpha_default)
    bt = bt.to(torch.float64)
    if bt.requires_grad:
        bt.retain_grad()
    else:                                       # sharing type 4 has no beta parameter: the table itself is the leaf
        bt.requires_grad_(True)
    x = torch.from_numpy(np.asarray(llr, np.float64)).requires_grad_(want_llr)
    J, per, disagree = ref.forward(g, x, U, K, P, bt, lay.beta_slot, thr, qoi, y, w)
    J.backward()
    return {"loss": float(J.detach()), "per_iter": np.array([float(v.detach()) for v in per]), "U": U, "K": K, "P": P,
            "disagree": disagree, "grad_llr": x.grad.numpy() if want_llr else None, "grad_beta": bt.grad.numpy()}


def grads_of(dec):
    return {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()).cpu() for k, p in dec.named_parameters()}


_RESTATED = {}


def restated(case):
    """the restatement's result for a case, computed once and shared between the tests (arrays read-only)"""
    if case not in _RESTATED:
        _, llr, y, w = inputs(case)
        dec = decoder_of(case)
        r = restate(dec, llr, y, w)
        r["grads"] = grads_of(dec)
        for k in ("per_iter", "U", "K", "P", "grad_llr", "grad_beta"):
            r[k].setflags(write=False)
        _RESTATED[case] = r
    return _RESTATED[case]


# ---------------------------------------------------------------------------------------------------- the trainer test
TRAIN = flood.TRAIN


def trainer_model():
    """pjt_rcq_cases.trainer_model on the layered schedule: small_96_48 W-RCQ started at beta = 1.0, the plain layered RCQ
    decoder"""
    return flood.trainer_model(layered="paper", **HOW)


trainer_config = flood.trainer_config
