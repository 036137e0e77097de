"""
Host tests (no GPU) of posterior joint training of ``WeightedRCQDecoder(layered="paper")``: the new C symbols are declared,
exported and refuse like their siblings; the two gradient keywords; the CPU restatement tests/layered_pjt_rcq_reference.py
against the layered decode's restatement (tests/test_gpu_layered_weighted.py), against its own autograd-free closed form and
against a gradient derived by hand; and the condition on the input sets that makes the straight-through mask matter.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import layered_pjt_rcq_cases as cases
import layered_pjt_rcq_reference as ref
from conftest import PKG, ROOT

SYMBOLS = ("ldpc_train_joint_layered_ste_workspace_bytes", "ldpc_train_joint_layered_ste")
QP = cases.QP3


def sig(v):
    return 1.0 / (1.0 + np.exp(-v))


# ---------------------------------------------------------------------------------------------------- symbols, keywords
def test_abi_is_declared_exported_and_refuses_without_a_decoder():
    import _native as nat
    header = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    lib = ctypes.CDLL(os.path.join(PKG, "libldpc_hip.so"))
    for sym in SYMBOLS:
        assert sym in nat.PRODUCT_EXPORTS
        assert f"{sym}(" in header
        assert hasattr(lib, sym)
    lib = nat.load()
    assert lib.ldpc_abi_version() == 1                  # an addition, not a new ABI
    assert lib.ldpc_train_joint_layered_ste_workspace_bytes(None, 4) == 0
    args = [None] * 14
    args[3] = 4
    args[12] = 0
    assert lib.ldpc_train_joint_layered_ste(*args) == -1 and b"NULL decoder" in lib.ldpc_last_error()


def test_operator_is_registered_with_its_schema():
    import torch_ops  # noqa: F401
    schema = str(torch.ops.ldpc.rcq_layered_joint_loss.default._schema)
    assert "alpha_is_oms" not in schema and "want_grads=True" in schema and "want_grad_llr=False" in schema


def test_both_gradient_keywords_are_needed_and_the_call_overrides_the_constructor():
    import _native as nat
    from ldpc_decoder import create_test_ldpc_code
    from rcq_decoder import WeightedRCQDecoder
    code = create_test_ldpc_code()
    x = torch.zeros(3, 7)
    ste, loc = "straight_through", "posterior_local"
    make = lambda **kw: WeightedRCQDecoder(code, 3, 8, QP, 2, 4, **kw)
    # layered="paper": either keyword missing refuses, wherever the other one was given
    plain = make(layered="paper")
    assert plain.layered_gradient is None and plain.quantizer_gradient is None
    for dec, kw in ((plain, {}), (plain, {"quantizer_gradient": ste}), (plain, {"layered_gradient": loc}),
                    (make(layered="paper", quantizer_gradient=ste), {}), (make(layered="paper", layered_gradient=loc), {})):
        with pytest.raises(NotImplementedError):
            dec.joint_posterior_loss(x, **kw)
    both = make(layered="paper", quantizer_gradient=ste, layered_gradient=loc)
    assert both.layered_gradient == loc and both.quantizer_gradient == ste
    # unknown names: ValueError, from the constructor and from the call
    with pytest.raises(ValueError, match="layered_gradient"):
        make(layered="paper", layered_gradient="bptt")
    with pytest.raises(ValueError, match="layered_gradient"):
        both.joint_posterior_loss(x, layered_gradient="bptt")
    with pytest.raises(ValueError, match="quantizer_gradient"):
        both.joint_posterior_loss(x, quantizer_gradient="sigmoid")
    # a flooding W-RCQ decoder has no layered gradient to choose (layered=True is flooding here, as in the reference)
    for kw in ({}, {"layered": True}, {"quantizer_gradient": ste}):
        with pytest.raises(ValueError, match="layered_gradient"):
            make(layered_gradient=loc, **kw)
        with pytest.raises(ValueError, match="layered_gradient"):
            make(**kw).joint_posterior_loss(x, layered_gradient=loc)
    # argument validation comes before any device work, as on the flooding decoder
    with pytest.raises(ValueError):
        both.joint_posterior_loss(x, targets=torch.zeros(3, 6))
    with pytest.raises(ValueError):
        both.joint_posterior_loss(x, iteration_weights=torch.ones(3))
    # the call's values override the constructor's: past both refusals the call goes on to the engine (none here)
    if not torch.cuda.is_available():
        for dec, kw in ((both, {}), (plain, {"quantizer_gradient": ste, "layered_gradient": loc}),
                        (make(layered="paper", quantizer_gradient=ste), {"layered_gradient": loc})):
            with pytest.raises(nat.NativeEngineError):
                dec.joint_posterior_loss(x, **kw)


# ---------------------------------------------------------------------------------------------------- the walk
@pytest.mark.parametrize("case", range(len(cases.CASES)))
def test_walk_is_the_layered_decode_and_the_inputs_exercise_both_branches_of_the_mask(case):
    """walk against the restatement the layered decode is pinned to (tests/test_gpu_layered_weighted.py): bits, posteriors
    and the final codes, exactly.  And a condition on the input set, from the restatement alone: at least 2 % of the
    (b, t, e) triples saturate and at least 2 % do not, so a wrong mask cannot pass"""
    import test_gpu_layered_weighted as lw
    name, wtype, bc, qp, B, _, special = cases.CASES[case]
    code, llr, _, _ = cases.inputs(case)
    dec = cases.decoder_of(case)
    T = cases.T_GRAD
    U, K, P = cases.walk_of(dec, llr)
    beta_e = lw.edge_betas(dec, T)
    assert np.array_equal(beta_e, cases.edge_betas(dec))
    bits, post, iters, _, codes = lw.restate(code, llr, bc, qp, T, beta_e, early_stop=False, want_messages=True)
    assert np.all(iters == T)
    assert np.array_equal(P[T - 1], post) and np.array_equal((P[T - 1] < 0).astype(np.int32), bits)
    assert np.array_equal(K[T - 1].astype(np.int64), codes)
    g = dec.code.tanner_graph()
    e1 = int(g.check_ptr[1])
    assert np.array_equal(U[0][:, :e1], llr[:, g.var_idx[:e1]])            # iteration 0, check 0: u is the LLR itself
    L = 2 ** (bc - 1)
    top = ((K % L) == L - 1).mean()
    assert 0.02 <= top <= 0.98, (cases.CASES[case], top)
    if bc == 8:
        assert int(K.max()) == 255
    if special == "saturate":
        assert top > 0.5
    if special == "negbeta":
        assert (dec.weight_tables()[0] < 0).any() and (dec.weight_tables()[0] == 0).any()
    if special == "wide":
        assert int(g.dc.max()) == 40 and int(g.dv.max()) == 10
    else:
        assert int(g.dc.max()) <= 32


# ---------------------------------------------------------------------------------------------------- the gradient
@pytest.mark.parametrize("case", [0, 1, 2, 5, 6, 10])
def test_autograd_restatement_equals_the_closed_form(case):
    """the two CPU statements of the gradient agree on the toy and small codes: torch autograd teacher-forced on the fp32
    walk, and scalar loops with the formulas written out on a scalar fp32 walk"""
    _, _, _, _, B, _, _ = cases.CASES[case]
    _, llr, y, w = cases.inputs(case)
    rows = slice(0, min(B, 8))
    dec = cases.decoder_of(case)
    r = cases.restate(dec, llr[rows], None if y is None else y[rows], w)
    assert r["disagree"] == 0.0
    thr, qoi = cases.quantiser_tables(dec)
    cf = ref.closed_form(dec.code.tanner_graph(), llr[rows], cases.T_GRAD, cases.edge_betas(dec), thr, qoi,
                         None if y is None else y[rows].numpy(), None if w is None else w.numpy())
    assert np.array_equal(cf["posterior"], r["P"][-1]) and np.array_equal(cf["codes"], r["K"])
    np.testing.assert_allclose(r["per_iter"], cf["per_iter"], rtol=1e-12)
    scale = np.abs(cf["grad_llr"]).max()
    np.testing.assert_allclose(r["grad_llr"], cf["grad_llr"], rtol=1e-9, atol=1e-12 * scale)
    slot = dec._sharing_layout().beta_slot
    want_b = np.zeros_like(r["grad_beta"])
    for t in range(cases.T_GRAD):
        np.add.at(want_b[t], slot, cf["grad_beta_e"][t])
    assert np.abs(want_b).max() > 0
    np.testing.assert_allclose(r["grad_beta"], want_b, rtol=1e-9, atol=1e-12 * np.abs(want_b).max())


def test_restatement_matches_a_hand_derived_gradient():
    """T = 1, tau = 0, 1, 2, 3, per-edge betas, every value exact in fp32.  Check 0 on v0..v3 with u = llr = 1, 2, -2, 8:
    the first minimum on e0, the second minimum TIED on e1, e2.  m = beta * raw * prod:
        e0: 0.75 * 2 * (-)  = -1.5    level 1, passes              e1: 0.5 * 1 * (-) = -0.5   level 0: the DEAD ZONE, passes
        e2: 0.875 * 1 * (+) =  0.875  level 0, passes              e3: 4 * 1 * (-)   = -4     level 3: SATURATED, blocked
    Check 1 on v1 alone (degree 1) runs after check 0 changed P_1: u4 = 2 + (-0) = 2, prod = 1, raw = |u4|, m = 0.25 * 2."""
    from ldpc_decoder import LDPCCode
    H = np.array([[1, 1, 1, 1], [0, 1, 0, 0]], dtype=np.int64)
    g = LDPCCode(n=4, k=2, H=H, max_iterations=1).tanner_graph()
    assert list(g.check_ptr) == [0, 4, 5] and list(g.var_idx) == [0, 1, 2, 3, 1]
    thr = np.array([[0.0, 1.0, 2.0, 3.0]], np.float32)
    b = np.array([0.75, 0.5, 0.875, 4.0, 0.25])
    llr = np.array([[1.0, 2.0, -2.0, 8.0]], np.float32)
    y = np.array([[0.0, 0.25, 1.0, 0.0]])
    U, K, P = ref.walk(g, llr, 1, b[None, :], thr, [0])
    assert K[0, 0].tolist() == [4 + 1, 4 + 0, 0, 4 + 3, 0]
    bt = torch.tensor(b[None, :], dtype=torch.float64, requires_grad=True)
    x = torch.tensor(llr, dtype=torch.float64, requires_grad=True)
    J, per, disagree = ref.forward(g, x, U, K, P, bt, np.arange(5), thr, [0], y)
    J.backward()
    assert disagree == 0.0
    # by hand
    raw, prod = np.array([2.0, 1.0, 1.0, 1.0]), np.array([-1.0, -1.0, 1.0, -1.0])
    passes = np.array([1.0, 1.0, 1.0, 0.0])
    r = np.array([-1.0, -0.0, 0.0, -3.0])                                # the reconstructions
    u4 = 2.0 + r[1]
    r4 = 0.0                                                             # m = 0.5: level 0 reconstructs tau_0 = 0
    Pw = np.array([1.0 + r[0], u4 + r4, -2.0 + r[2], 8.0 + r[3]])
    N = llr.size
    gv = (y[0] - sig(-Pw)) / N                                           # w_0 = 1
    want_J = np.sum(np.maximum(-Pw, 0) + Pw * y[0] + np.log1p(np.exp(-np.abs(Pw)))) / N
    want_b = np.append(gv * passes * raw * prod, gv[1] * abs(u4))
    gm = gv * passes * b[:4] * prod                                      # d J/d raw_e
    acc1, acc2 = gm[1] + gm[2] + gm[3], gm[0]                            # raw = m1 on e1..e3, m2 on e0
    want_x = gv + np.array([acc1 * 1.0, acc2 / 2 * 1.0, acc2 / 2 * -1.0, 0.0])     # m2's split over the two tied edges
    want_x[1] += gv[1] * b[4] * 1.0                                      # the degree-1 check: d|u4|/d llr_1 = sgn(u4)
    np.testing.assert_array_equal(P[0, 0], Pw.astype(np.float32))
    assert float(per[0].detach()) == pytest.approx(want_J, rel=1e-12)
    np.testing.assert_allclose(bt.grad.numpy()[0], want_b, rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(x.grad.numpy()[0], want_x, rtol=1e-12)
    assert want_b[3] == 0.0 and np.all(want_b[[0, 1, 2, 4]] != 0.0)
    cf = ref.closed_form(g, llr, 1, b[None, :], thr, [0], y)
    np.testing.assert_allclose(cf["grad_beta_e"][0], want_b, rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(cf["grad_llr"][0], want_x, rtol=1e-12)


def test_adam_on_the_restatement_gradients_lowers_the_trainer_loss():
    """the run of the GPU trainer test, on the CPU: same model, data seed, shuffling seed, optimiser and epochs, with the
    restatement's gradients -- the last epoch's loss lies below the first's, the betas have moved, the alphas have not"""
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
    betas = torch.cat([p.detach().reshape(-1) for p in model.beta_weights.values()])
    assert float((betas - 1.0).abs().max()) > 0.05
    alphas = torch.cat([p.detach().reshape(-1) for p in model.alpha_weights.values()])
    assert float((alphas - 1.0).abs().max()) == 0.0      # the schedule does not use them: no gradient, no step
