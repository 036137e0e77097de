"""
CPU tests of posterior joint training (PJT): the C ABI is declared and exported, refuses to run without a GPU, the
host entry points validate their arguments before any device work, the trainer's new switch defaults to off, and the
CPU restatement the GPU tests compare against (tests/pjt_reference.py) agrees with a gradient derived by hand.
"""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

QP = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]
JOINT_SYMBOLS = ("ldpc_train_joint_workspace_bytes", "ldpc_train_joint")


def test_joint_abi_is_declared_and_exported():
    import _native as nat
    header = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    lib = ctypes.CDLL(os.path.join(PKG, "libldpc_hip.so"))
    for sym in JOINT_SYMBOLS:
        assert sym in nat.PRODUCT_EXPORTS
        assert f"{sym}(" in header
        assert hasattr(lib, sym)
    assert nat.load().ldpc_abi_version() == 1          # an addition, not a new ABI


def test_joint_abi_refuses_like_the_other_training_symbols():
    import _native as nat
    lib = nat.load()
    assert lib.ldpc_train_joint_workspace_bytes(None, 4) == 0 == lib.ldpc_train_workspace_bytes(None, 4)
    args = [None] * 15
    args[3] = 4
    args[13] = 0
    assert lib.ldpc_train_joint(*args) == -1 and b"NULL decoder" in lib.ldpc_last_error()
    from ldpc_decoder import create_test_ldpc_code
    from neural_2d_decoder import Neural2DMinSumDecoder
    dec = Neural2DMinSumDecoder(create_test_ldpc_code(), 2, 3)
    if not torch.cuda.is_available():
        with pytest.raises(Exception) as e:                       # still no CPU fallback
            dec.joint_posterior_loss(torch.zeros(2, 7))
        assert "GPU" in str(e.value) or "HIP" in str(e.value) or "cuda" in str(e.value).lower()


def test_joint_loss_validates_arguments_before_device_work():
    from ldpc_decoder import create_test_ldpc_code
    from neural_2d_decoder import Neural2DMinSumDecoder, Neural2DOffsetMinSumDecoder
    from neural_minsum_decoder import NeuralMinSumDecoder, NeuralOffsetMinSumDecoder
    from rcq_decoder import WeightedRCQDecoder
    code = create_test_ldpc_code()
    x = torch.zeros(3, 7)
    for dec in (Neural2DMinSumDecoder(code, 2, 4), Neural2DOffsetMinSumDecoder(code, 1, 4),
                NeuralMinSumDecoder(code, 4), NeuralOffsetMinSumDecoder(code, 4)):
        with pytest.raises(ValueError):
            dec.joint_posterior_loss(x, targets=torch.zeros(3, 6))
        with pytest.raises(ValueError):
            dec.joint_posterior_loss(x, targets=torch.zeros(7))
        with pytest.raises(ValueError):
            dec.joint_posterior_loss(x, iteration_weights=torch.ones(3))
        with pytest.raises(ValueError):
            dec.joint_posterior_loss(torch.zeros(3, 8))
    with pytest.raises(NotImplementedError):             # quantisation passes no gradient
        WeightedRCQDecoder(code, 3, 8, QP, 2, 4).joint_posterior_loss(x)


def test_training_config_joint_switch_defaults_off():
    from training_framework import TrainingConfig
    fields = dataclasses.fields(TrainingConfig)
    assert fields[-1].name == "joint_posterior_loss" and TrainingConfig().joint_posterior_loss is False
    assert TrainingConfig().use_posterior_training is True


def _two_check_graph():
    """checks c0 = {v0, v1}, c1 = {v1, v2}; CSR edges e0 = (c0, v0), e1 = (c0, v1), e2 = (c1, v1), e3 = (c1, v2)"""
    import oracle
    return oracle.OracleGraph(n=3, check_ptr=np.array([0, 2, 4], np.int32), var_idx=np.array([0, 1, 1, 2], np.int32))


def test_restatement_matches_a_hand_derived_gradient(oracle_mod):
    import pjt_reference
    g = _two_check_graph()
    x = np.array([[1.0, 2.0, 3.0], [0.5, 1.5, 2.5]])
    y = np.array([[0.0, 0.25, 1.0], [0.5, 0.0, 0.0]])
    b0, b1, a0, a1 = 0.8, 0.6, 1.3, 0.9
    w = np.array([0.3, 0.7])
    B, n = x.shape
    got = pjt_reference.joint_grads(g, x, [[b0], [b1]], np.zeros(4, np.int64), [[a0], [a1]], np.zeros(3, np.int64), 2,
                                    targets=y, weights=w, want_llr=True, dtype=torch.float64)
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    gb0 = gb1 = ga0 = 0.0
    gx = np.zeros_like(x)
    J = [0.0, 0.0]
    for b in range(B):
        x0, x1, x2 = x[b]
        # iteration 0: every message positive, each degree-2 check passes the other edge's LLR scaled by beta_0
        l0 = np.array([x0 + b0 * x1, x1 + b0 * (x0 + x2), x2 + b0 * x1])
        # iteration 1: v2c_1 = llr + alpha_0 * (leave-one-out c2v_0 sum, a constant): only v1 has two edges
        s_e1, s_e2 = b0 * x2, b0 * x0
        l1 = np.array([x0 + b1 * (x1 + a0 * s_e1), x1 + b1 * (x0 + x2), x2 + b1 * (x1 + a0 * s_e2)])
        g0 = w[0] * (y[b] - sig(-l0)) / (B * n)            # d J / d l_t
        g1 = w[1] * (y[b] - sig(-l1)) / (B * n)
        for t, l in enumerate((l0, l1)):
            J[t] += float(np.sum(np.maximum(-l, 0) + l * y[b] + np.log1p(np.exp(-np.abs(l))))) / (B * n)
        gb0 += g0 @ np.array([x1, x0 + x2, x1])
        gb1 += g1 @ np.array([x1 + a0 * s_e1, x0 + x2, x1 + a0 * s_e2])
        ga0 += g1[0] * b1 * s_e1 + g1[2] * b1 * s_e2
        M0 = np.array([[1, b0, 0], [b0, 1, b0], [0, b0, 1]])      # d l_t[v] / d x[u]: the sums through sg() drop out
        M1 = np.array([[1, b1, 0], [b1, 1, b1], [0, b1, 1]])
        gx[b] = M0.T @ g0 + M1.T @ g1
    np.testing.assert_allclose(got["loss_per_iter"], J, rtol=1e-12)
    assert got["loss"] == pytest.approx(w @ np.array(J), rel=1e-12)
    np.testing.assert_allclose(got["grad_beta"][:, 0], [gb0, gb1], rtol=1e-12)
    np.testing.assert_allclose(got["grad_alpha"][:, 0], [ga0, 0.0], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(got["grad_llr"], gx, rtol=1e-12, atol=1e-15)


def test_restatement_at_one_iteration_is_the_final_posterior_loss(oracle_mod):
    """T = 1: nothing is stopped, so PJT is the ordinary posterior BCE -- the existing gradient oracle's, per codeword mean"""
    import codes
    import grad_oracle
    import oracle
    import pjt_reference
    code = codes.load_code("small_96_48", max_iterations=1)
    tg = code.tanner_graph()
    g = oracle.OracleGraph(n=tg.n, check_ptr=tg.check_ptr, var_idx=tg.var_idx)
    rng = np.random.default_rng(3)
    B = 6
    x = (rng.standard_normal((B, g.n)) * 2 + 1.5).astype(np.float32)
    bt = rng.uniform(0.5, 1.0, (1, 4)).astype(np.float32)
    bslot = rng.integers(0, 4, g.E)
    at = np.ones((1, 1), np.float32)
    aslot = np.zeros(g.n, np.int64)
    got = pjt_reference.joint_grads(g, x, bt, bslot, at, aslot, 1, dtype=torch.float64)
    gb, ga, _, _ = grad_oracle.table_grads(g, x, bt, bslot, at, aslot, 1, early_stop=False, dtype=torch.float64)
    np.testing.assert_allclose(got["grad_beta"] * B, gb, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(got["grad_alpha"], 0.0)
