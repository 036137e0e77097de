"""
Input sets of the W-RCQ posterior-joint-training tests, shared by the CPU file (tests/test_joint_training_rcq_host.py: the
restatement's own quantiser agrees with the traced codes on every set) and the GPU file
(tests/test_gpu_joint_training_rcq.py: the kernels' gradients equal the restatement's on the same sets).
Test infrastructure, not product code.
"""
import functools

import numpy as np
import torch

QP3 = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]
T_GRAD = 4                                     # three quantisers over four iterations: schedule 0, 1, 2, 2

# (code, sharing type, bc, quantiser parameters, B, SNR range in dB, special)
#   "gamma0"  : gamma = 0, every threshold of a quantiser equals C (two levels in effect, level 0 reconstructs C)
#   "negbeta" : one beta slot of iteration 1 negative
#   "saturate": a clean channel, most messages above the top threshold
#   "wide"    : the random graph below (a degree-40 check, a degree-10 variable)
CASES = [
    ("toy", 1, 3, QP3, 37, (0.5, 4.0), None),
    ("toy", 4, 4, QP3, 37, (0.5, 4.0), None),
    ("small", 2, 3, QP3, 300, (0.5, 4.0), None),
    ("small", 3, 4, QP3, 64, (0.5, 4.0), None),
    ("ira", 2, 3, QP3, 40, (0.5, 4.0), None),
    ("small", 2, 3, [(2.0, 0.0), (3.0, 0.0), (4.0, 0.0)], 70, (0.5, 4.0), "gamma0"),
    ("small", 2, 3, QP3, 50, (0.5, 4.0), "negbeta"),
    ("small", 1, 3, QP3, 70, (7.0, 10.0), "saturate"),
    ("wide", 2, 3, QP3, 70, (0.5, 4.0), "wide"),
    ("wide", 2, 4, QP3, 33, (0.5, 4.0), "wide"),
    # 2, 32, 64 and 128 levels: at bc = 8 the negative codes use bit 7 and the variable pass's LUT is full (2 * 128 entries)
    ("small", 2, 2, QP3, 70, (0.5, 4.0), None),
    ("small", 1, 6, QP3, 70, (0.5, 4.0), None),
    ("small", 2, 7, QP3, 64, (0.5, 4.0), None),
    ("small", 2, 8, QP3, 300, (0.5, 4.0), None),
    ("wide", 2, 8, QP3, 70, (0.5, 4.0), "wide"),
    ("small", 2, 8, QP3, 50, (0.5, 4.0), "negbeta"),
    ("ira", 2, 8, QP3, 40, (0.5, 4.0), None),
]


def channel(rng, B, n, snr):
    s = np.linspace(snr[0], snr[1], B)
    s2 = 10.0 ** (-s / 10.0)
    return (2.0 * (1.0 + np.sqrt(s2)[:, None] * rng.standard_normal((B, n))) / s2[:, None]).astype(np.float32)


def wide_code(T):
    """n = 60, m = 30: check 0 has degree 40 (the re-read path of the check backward, the one-check-per-block forward
    sweep), variable 59 degree 10 (the loop path of the variable backward); the other checks have degree 3..6"""
    from ldpc_decoder import LDPCCode
    rng = np.random.default_rng(2024)
    n, m = 60, 30
    H = np.zeros((m, n), dtype=np.int64)
    H[0, :40] = 1
    H[1:11, 59] = 1
    for i in range(1, m):
        H[i, rng.choice(59, size=int(rng.integers(3, 7)) - int(H[i, 59]), replace=False)] = 1
    for j in range(n):                          # no isolated variable
        if H[:, j].sum() == 0:
            H[int(rng.integers(1, m)), j] = 1
    assert H[0].sum() == 40 and H[:, 59].sum() == 10
    return LDPCCode(n=n, k=n - m, H=H, max_iterations=T)


def load(name, T):
    import codes
    from ldpc_decoder import create_test_ldpc_code
    if name == "toy":
        return create_test_ldpc_code()
    if name == "wide":
        return wide_code(T)
    return codes.load_code({"small": "small_96_48", "ira": "ira_1998_1512"}[name], max_iterations=T)


def make_decoder(code, wtype, bc, qp, T, seed, negbeta=False, **kw):
    from rcq_decoder import WeightedRCQDecoder
    torch.manual_seed(seed)
    dec = WeightedRCQDecoder(code, bc, 8, qp, wtype, T, **kw)
    rng = np.random.default_rng(seed + 100)
    with torch.no_grad():                       # weights away from the init
        for name, p in dec.named_parameters():
            p.fill_(float(rng.uniform(0.55, 1.0)) if "beta" in name else float(rng.uniform(0.8, 1.2)))
        if negbeta:
            key = sorted(k for k in dec.beta_weights.keys() if k.startswith("iter_1_"))[0]
            dec.beta_weights[key].fill_(-0.6)
    return dec


def oracle_graph(code):
    import oracle
    tg = code.tanner_graph()
    return oracle.OracleGraph(n=tg.n, check_ptr=tg.check_ptr, var_idx=tg.var_idx)


def quantiser_tables(dec):
    from rcq_decoder import _quantizer_schedule, _threshold_table
    return _threshold_table(dec.quantizers), _quantizer_schedule(len(dec.quantizers), int(dec.max_iterations))


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> (code, llr [B, n] float32, targets | None, iteration weights | None); every other case has custom iteration
    weights and soft targets"""
    name, _, _, _, B, snr, _ = CASES[case]
    code = load(name, T_GRAD)
    rng = np.random.default_rng(50 + case)
    llr = channel(rng, B, code.n, snr)
    custom = case % 2 == 1
    w = torch.tensor(rng.uniform(0.1, 1.0, T_GRAD), dtype=torch.float32) if custom else None
    y = (torch.from_numpy(rng.uniform(0, 1, (B, code.n)).astype(np.float32) * (rng.random((B, code.n)) < 0.3))
         if custom else None)
    return code, llr, y, w


def decoder_of(case, **kw):
    _, wtype, bc, qp, _, _, special = CASES[case]
    return make_decoder(inputs(case)[0], wtype, bc, qp, T_GRAD, seed=case, negbeta=special == "negbeta", **kw)


def restate(dec, llr, y=None, w=None, want_llr=True):
    """the restatement on the decoder's CURRENT parameters, teacher-forced by the oracle's fixed-T decode.  Leaves
    d J/d parameter in the parameters' .grad.  -> dict(loss, per_iter, posterior, trace_posterior, trace_bits, disagree,
    grad_llr, codes)"""
    import pjt_rcq_reference as ref
    T = int(dec.max_iterations)
    g = oracle_graph(dec.code)
    lay = dec._sharing_layout()
    thr, qoi = quantiser_tables(dec)
    beta, alpha = dec.weight_tables()
    bits, post, codes = ref.trace(g, llr, beta, lay.beta_slot, alpha, lay.alpha_slot, thr, qoi, T)
    bt, at = lay.tables_torch(dec.beta_weights, dec.alpha_weights, T, dec._beta_default, dec._alpha_default)
    x = torch.from_numpy(np.asarray(llr, np.float32)).requires_grad_(want_llr)
    J, per, post_c, disagree = ref.forward(g, x, codes, bt, lay.beta_slot, at, lay.alpha_slot, thr, qoi, T, y, w)
    J.backward()
    return {"loss": float(J.detach()), "per_iter": np.array([float(v.detach()) for v in per]),
            "posterior": post_c.detach().numpy(), "trace_posterior": post, "trace_bits": bits, "disagree": disagree,
            "grad_llr": x.grad.numpy() if want_llr else None, "codes": codes}


# ---------------------------------------------------------------------------------------------------- the trainer test
TRAIN = dict(code="small_96_48", T=5, wtype=2, bc=3, qp=QP3, batch_size=64, num_epochs=6, learning_rate=0.05,
             snr_range=(1.0, 4.0), seed=9, torch_seed=5, num_train=512, num_val=128)


def trainer_model(**kw):
    """small_96_48 W-RCQ started at beta = alpha = 1.0: the plain RCQ decoder, an over-estimate for min-sum"""
    import codes
    from rcq_decoder import WeightedRCQDecoder
    t = TRAIN
    code = codes.load_code(t["code"], max_iterations=t["T"])
    model = WeightedRCQDecoder(code, t["bc"], 8, t["qp"], t["wtype"], t["T"], **kw)
    with torch.no_grad():
        for p in model.parameters():
            p.fill_(1.0)
    return code, model


def trainer_config(device):
    from training_framework import TrainingConfig
    t = TRAIN
    return TrainingConfig(batch_size=t["batch_size"], num_epochs=t["num_epochs"], learning_rate=t["learning_rate"],
                          snr_range=t["snr_range"], device=device, seed=t["seed"], joint_posterior_loss=True)
