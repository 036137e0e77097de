"""
CPU tests of posterior joint training of the quantised decoder (W-RCQ, straight-through estimator): the new C symbols are
declared, exported and refuse like their siblings; ``WeightedRCQDecoder.joint_posterior_loss`` validates its arguments
before any device work and still refuses without the option; the CPU restatement the GPU tests compare against
(tests/pjt_rcq_reference.py) agrees with a gradient derived by hand, its own quantiser reproduces the traced codes on
every input set of the GPU file, and Adam on its gradients lowers the loss of the trainer test's run.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

QP = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]
STE_SYMBOLS = ("ldpc_train_joint_ste_workspace_bytes", "ldpc_train_joint_ste")


def test_ste_abi_is_declared_exported_and_refuses_without_a_decoder():
    import _native as nat
    header = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    lib = ctypes.CDLL(os.path.join(PKG, "libldpc_hip.so"))
    for sym in STE_SYMBOLS:
        assert sym in nat.PRODUCT_EXPORTS
        assert f"{sym}(" in header
        assert hasattr(lib, sym)
    lib = nat.load()
    assert lib.ldpc_abi_version() == 1                  # an addition, not a new ABI
    assert lib.ldpc_train_joint_ste_workspace_bytes(None, 4) == 0
    args = [None] * 14
    args[3] = 4
    args[12] = 0
    assert lib.ldpc_train_joint_ste(*args) == -1 and b"NULL decoder" in lib.ldpc_last_error()


def test_quantizer_gradient_option_is_validated_before_device_work():
    from ldpc_decoder import create_test_ldpc_code
    from rcq_decoder import WeightedRCQDecoder
    code = create_test_ldpc_code()
    x = torch.zeros(3, 7)
    with pytest.raises(ValueError):
        WeightedRCQDecoder(code, 3, 8, QP, 2, 4, quantizer_gradient="sigmoid")
    plain = WeightedRCQDecoder(code, 3, 8, QP, 2, 4)
    assert plain.quantizer_gradient is None
    with pytest.raises(NotImplementedError):             # the default still refuses
        plain.joint_posterior_loss(x)
    with pytest.raises(ValueError):
        plain.joint_posterior_loss(x, quantizer_gradient="identity")
    ste = WeightedRCQDecoder(code, 3, 8, QP, 2, 4, quantizer_gradient="straight_through")
    assert ste.quantizer_gradient == "straight_through"
    for dec, kw in ((ste, {}), (plain, {"quantizer_gradient": "straight_through"})):
        with pytest.raises(ValueError):
            dec.joint_posterior_loss(x, targets=torch.zeros(3, 6), **kw)
        with pytest.raises(ValueError):
            dec.joint_posterior_loss(x, targets=torch.zeros(7), **kw)
        with pytest.raises(ValueError):
            dec.joint_posterior_loss(x, iteration_weights=torch.ones(3), **kw)
        with pytest.raises(ValueError):
            dec.joint_posterior_loss(torch.zeros(3, 8), **kw)
    with pytest.raises(ValueError):                      # a bad estimator name is an error with the option set as well
        ste.joint_posterior_loss(x, quantizer_gradient="sigmoid")
    paper = WeightedRCQDecoder(code, 3, 8, QP, 2, 4, layered="paper", quantizer_gradient="straight_through")
    with pytest.raises(NotImplementedError):
        paper.joint_posterior_loss(x)
    if not torch.cuda.is_available():                    # still no CPU fallback
        with pytest.raises(Exception) as e:
            ste.joint_posterior_loss(x)
        assert "GPU" in str(e.value) or "HIP" in str(e.value) or "cuda" in str(e.value).lower()


def test_operator_is_registered_with_its_schema():
    import torch_ops  # noqa: F401
    schema = str(torch.ops.ldpc.rcq_joint_loss.default._schema)
    assert "alpha_is_oms" not in schema and "want_grads=True" in schema and "want_grad_llr=False" in schema


# ---------------------------------------------------------------------------------------------------- hand derivation
def _two_check_graph():
    """checks c0 = {v0, v1}, c1 = {v1, v2}; CSR edges e0 = (c0, v0), e1 = (c0, v1), e2 = (c1, v1), e3 = (c1, v2)"""
    import oracle
    return oracle.OracleGraph(n=3, check_ptr=np.array([0, 2, 4], np.int32), var_idx=np.array([0, 1, 1, 2], np.int32))


def test_restatement_matches_a_hand_derived_gradient(oracle_mod):
    """T = 2, quantiser 0 (tau = 0, 1, 2, 3) in iteration 0 and quantiser 1 (tau = 0, 2, 4, 6) in iteration 1, every value
    exact in fp32.  Codeword 0, iteration 0: m = 1.5, 0.375, 3.75, 1.5 on e0..e3 -- e1 sits in the dead zone (level 0,
    gradient passes), e2 saturates (level 3, gradient blocked).  Codeword 1 has negative messages and saturates in
    iteration 1.  A degree-2 check passes the OTHER edge's message: m[e] = beta * v2c[other], d m / d v2c[other] = beta."""
    import pjt_rcq_reference as ref
    g = _two_check_graph()
    thr = np.array([[0.0, 1.0, 2.0, 3.0], [0.0, 2.0, 4.0, 6.0]], np.float32)
    qoi = np.array([0, 1], np.int32)
    L = 4
    x = np.array([[0.5, 2.0, 5.0], [-13.0, 3.0, -1.0]], np.float32)
    y = np.array([[0.0, 0.25, 1.0], [0.5, 0.0, 0.0]])
    b0, b1, a0, a1 = 0.75, 0.5, 1.25, 0.875
    w = np.array([0.3, 0.7])
    B, n = x.shape
    bslot, aslot = np.zeros(4, np.int32), np.zeros(3, np.int32)
    _, post, codes = ref.trace(g, x, [[b0], [b1]], bslot, [[a0], [a1]], aslot, thr, qoi, 2)
    got = ref.joint_grads(g, x, codes, [[b0], [b1]], bslot, [[a0], [a1]], aslot, thr, qoi, 2, targets=y, weights=w,
                          want_llr=True, dtype=torch.float64)
    assert got["disagree"] == 0.0
    np.testing.assert_array_equal(got["posterior"].astype(np.float32), post)

    def quant(m, tau):                                    # -> (reconstruction, straight-through mask), by hand
        lvl = max(q for q in range(L) if abs(m) >= tau[q])
        return (-1.0 if m < 0 else 1.0) * float(tau[lvl]), 1.0 if lvl < L - 1 else 0.0

    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    gb0 = gb1 = ga0 = 0.0
    gx = np.zeros((B, n))
    J = [0.0, 0.0]
    seen = set()
    for b in range(B):
        x0, x1, x2 = (float(v) for v in x[b])
        # iteration 0: v2c = llr
        m0 = [b0 * x1, b0 * x0, b0 * x2, b0 * x1]
        (c0, k0), (c1, k1), (c2, k2), (c3, k3) = (quant(m, thr[0]) for m in m0)
        seen |= {(0, int(max(q for q in range(L) if abs(m) >= thr[0][q]))) for m in m0}
        l0 = np.array([x0 + c0, x1 + c1 + c2, x2 + c3])
        # iteration 1: v2c_1 = llr + alpha_0 * (leave-one-out sum of the RECONSTRUCTED c2v_0, a constant); only v1 has two edges
        s_e1, s_e2 = c2, c1
        u = [x0, x1 + a0 * s_e1, x1 + a0 * s_e2, x2]      # v2c_1 on e0..e3
        m1 = [b1 * u[1], b1 * u[0], b1 * u[3], b1 * u[2]]
        (d0, h0), (d1, h1), (d2, h2), (d3, h3) = (quant(m, thr[1]) for m in m1)
        seen |= {(1, int(max(q for q in range(L) if abs(m) >= thr[1][q]))) for m in m1}
        l1 = np.array([x0 + d0, x1 + d1 + d2, x2 + d3])
        g0 = w[0] * (y[b] - sig(-l0)) / (B * n)            # d J / d l_t
        g1 = w[1] * (y[b] - sig(-l1)) / (B * n)
        for t, l in enumerate((l0, l1)):
            J[t] += float(np.sum(np.maximum(-l, 0) + l * y[b] + np.log1p(np.exp(-np.abs(l))))) / (B * n)
        gb0 += g0[0] * k0 * x1 + g0[1] * (k1 * x0 + k2 * x2) + g0[2] * k3 * x1
        gb1 += g1[0] * h0 * u[1] + g1[1] * (h1 * u[0] + h2 * u[3]) + g1[2] * h3 * u[2]
        ga0 += g1[0] * h0 * b1 * s_e1 + g1[2] * h3 * b1 * s_e2
        M0 = np.array([[1, k0 * b0, 0], [k1 * b0, 1, k2 * b0], [0, k3 * b0, 1]])    # d l_t[v] / d x[u]
        M1 = np.array([[1, h0 * b1, 0], [h1 * b1, 1, h2 * b1], [0, h3 * b1, 1]])
        gx[b] = M0.T @ g0 + M1.T @ g1
    assert {(0, 0), (0, 3), (1, 3)} <= seen                # dead zone and saturation in iteration 0, saturation in iteration 1
    np.testing.assert_allclose(got["loss_per_iter"], J, rtol=1e-12)
    assert got["loss"] == pytest.approx(w @ np.array(J), rel=1e-12)
    np.testing.assert_allclose(got["grad_beta"][:, 0], [gb0, gb1], rtol=1e-12)
    np.testing.assert_allclose(got["grad_alpha"][:, 0], [ga0, 0.0], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(got["grad_llr"], gx, rtol=1e-12, atol=1e-15)
    assert ga0 != 0.0 and gb0 != 0.0 and gb1 != 0.0


# ---------------------------------------------------------------------------------------------------- teacher forcing
def test_restatement_quantiser_agrees_with_the_traced_codes_on_every_gpu_input_set(oracle_mod):
    """the condition that keeps the teacher forcing honest: on every input set of tests/test_gpu_joint_training_rcq.py
    the restatement's own quantiser, on its own m, reproduces the codes it is forced with on all but <= 1e-3 of the
    (b, t, e) triples -- and its posterior is the oracle's fixed-T posterior"""
    import pjt_rcq_cases as cases
    for case in range(len(cases.CASES)):
        _, llr, y, w = cases.inputs(case)
        dec = cases.decoder_of(case)
        r = cases.restate(dec, llr, y, w, want_llr=False)
        assert r["disagree"] <= 1e-3, (cases.CASES[case], r["disagree"])
        np.testing.assert_allclose(r["posterior"], r["trace_posterior"], rtol=1e-5, atol=1e-5)
        grads = [p.grad for p in dec.parameters() if p.grad is not None]
        assert grads and any(float(v.abs().max()) > 0 for v in grads)
        L = 2 ** (cases.CASES[case][2] - 1)
        levels = r["codes"] % L
        assert (levels == L - 1).any() and (levels < L - 1).any()        # both branches of the mask occur
    # the special sets are what they claim to be
    sat = cases.CASES.index(next(c for c in cases.CASES if c[6] == "saturate"))
    r = cases.restate(cases.decoder_of(sat), cases.inputs(sat)[1], want_llr=False)
    assert ((r["codes"] % 4) == 3).mean() > 0.5
    neg = cases.decoder_of(next(i for i, c in enumerate(cases.CASES) if c[6] == "negbeta"))
    assert (neg.weight_tables()[0] < 0).any()
    wide = cases.load("wide", cases.T_GRAD).tanner_graph()
    assert int(wide.dc.max()) == 40 and int(wide.dv.max()) == 10


def test_adam_on_the_restatement_gradients_lowers_the_trainer_loss(oracle_mod):
    """the run of the GPU trainer test, on the CPU: same model, data seed, shuffling seed, optimiser and epochs, with the
    restatement's gradients -- the last epoch's loss lies below the first's"""
    import pjt_rcq_cases as cases
    from torch.utils.data import DataLoader, TensorDataset
    from training_framework import PosteriorJointTrainer
    t = cases.TRAIN
    torch.manual_seed(t["torch_seed"])
    code, model = cases.trainer_model()
    trainer = PosteriorJointTrainer(model, cases.trainer_config("cpu"))
    loader = DataLoader(TensorDataset(*trainer.generate_training_data(code, t["num_train"])), batch_size=t["batch_size"],
                        shuffle=True)
    val = DataLoader(TensorDataset(*trainer.generate_training_data(code, t["num_val"])), batch_size=t["batch_size"])
    losses = []
    for _ in range(t["num_epochs"]):
        tot = 0.0
        for llrs, targets in loader:
            trainer.optimizer.zero_grad()
            tot += cases.restate(model, llrs.numpy(), targets, None, want_llr=False)["loss"]
            trainer.optimizer.step()
        for _ in val:                                     # the trainer validates here: its loader draws a seed as well
            pass
        losses.append(tot / len(loader))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    vals = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    assert float((vals - 1.0).abs().max()) > 0.05
