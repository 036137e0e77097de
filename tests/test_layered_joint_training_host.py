"""
Host tests (no GPU) of posterior joint training under the layered schedule: the CPU restatement
tests/layered_pjt_reference.py against a gradient derived by hand and against its own autograd-free closed form, the
``layered_gradient`` keyword of the five trainable decoders, and a rehearsal of the GPU trainer test with the
restatement's gradients.
"""
import numpy as np
import pytest
import torch

import layered_minsum_reference as ref
import layered_pjt_cases as cases
import layered_pjt_reference as pjt


def sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def two_check_graph():
    """check 0 on variables 0..3, check 1 on variable 1 alone (degree 1); edges e0..e3 then e4"""
    from ldpc_decoder import LDPCCode
    H = np.array([[1, 1, 1, 1], [0, 1, 0, 0]], dtype=np.int64)
    g = LDPCCode(n=4, k=2, H=H, max_iterations=1).tanner_graph()
    assert list(g.check_ptr) == [0, 4, 5] and list(g.var_idx) == [0, 1, 2, 3, 1]
    return g


def restatement_grads(g, llr, form, beta_e, a_e=None):
    """T = 1, per-edge tables -> (J_0, d J/d beta_e, d J/d a_e | None, d J/d llr) from walk + forward"""
    U, P = pjt.walk(g, llr, 1, form, beta_e, a_e)
    bt = torch.tensor(beta_e, dtype=torch.float64, requires_grad=True)
    ot = None if a_e is None else torch.tensor(a_e, dtype=torch.float64, requires_grad=True)
    x = torch.tensor(llr, dtype=torch.float64, requires_grad=True)
    slot = np.arange(g.E)
    J, per = pjt.forward(g, x, U, P, bt, slot, ot, None if ot is None else slot, form == ref.OMS)
    J.backward()
    return float(per[0].detach()), bt.grad.numpy()[0], None if ot is None else ot.grad.numpy()[0], x.grad.numpy(), P[0]


# ---------------------------------------------------------------------------------------------------- by hand
def test_normalised_form_on_the_two_check_graph_by_hand():
    """row A: second-minimum tie (|u| = 1, 2, 2, 3); row B: an edge with u = 0 exactly.  Both rows: a degree-1 check that
    runs AFTER check 0 has changed its variable's posterior."""
    g = two_check_graph()
    b = np.array([[0.75, 0.5, -0.625, 0.875, 0.25]])
    llr = np.array([[1.0, 2.0, -2.0, 3.0], [0.0, 2.0, -3.0, 4.0]], dtype=np.float32)
    J, gb, _, gx, P = restatement_grads(g, llr, ref.NMS, b)
    b = b[0]
    N = llr.size                                                        # B * n
    want_b, want_x, want_J = np.zeros(5), np.zeros((2, 4)), 0.0
    # ---- row A.  check 0: u = llr; m1 = 1 on e0, m2 = 2 tied on e1, e2; prod of the OTHER signs: -, -, +, -
    raw, prod = np.array([2.0, 1.0, 1.0, 1.0]), np.array([-1.0, -1.0, 1.0, -1.0])
    r = b[:4] * raw * prod
    u4 = 2.0 + r[1]                                                     # check 1 sees the posterior check 0 left
    r4 = b[4] * abs(u4)                                                 # degree 1: prod = 1, raw = its own |u|
    PA = np.array([1.0 + r[0], u4 + r4, -2.0 + r[2], 3.0 + r[3]])
    gA = -sig(-PA) / N                                                  # w_0 = 1, y = 0
    want_J += np.sum(np.log1p(np.exp(-PA))) / N
    want_b[:4] += gA * raw * prod
    want_b[4] += gA[1] * abs(u4)
    gm = gA * b[:4] * prod                                              # d J/d raw_e
    acc1, acc2 = gm[1] + gm[2] + gm[3], gm[0]                           # raw = m1 on e1..e3, m2 on e0
    want_x[0] = gA + np.array([acc1 * 1.0, acc2 / 2 * 1.0, acc2 / 2 * -1.0, 0.0])     # m2's split over the two tied edges
    want_x[0, 1] += gA[1] * b[4] * np.sign(u4)
    # ---- row B.  check 0: u0 = 0, so prod = 0 on e1..e3 (their messages and gradients vanish); on e0 prod = -, raw = m2 = 2
    r0 = b[0] * 2.0 * -1.0
    r4 = b[4] * 2.0                                                     # u4 = 2 + 0
    PB = np.array([0.0 + r0, 2.0 + r4, -3.0, 4.0])
    gB = -sig(-PB) / N
    want_J += np.sum(np.log1p(np.exp(-PB))) / N
    want_b[0] += gB[0] * 2.0 * -1.0
    want_b[4] += gB[1] * 2.0
    acc2 = gB[0] * b[0] * -1.0                                          # to the second minimum: e1 alone
    want_x[1] = gB + np.array([0.0, acc2 * 1.0, 0.0, 0.0])              # acc1 = 0, and sgn(u0) = 0 anyway
    want_x[1, 1] += gB[1] * b[4] * 1.0
    np.testing.assert_allclose(P, np.stack([PA, PB]), rtol=1e-6)
    assert J == pytest.approx(want_J, rel=1e-6)                          # P is fp32 in the restatement
    np.testing.assert_allclose(gb, want_b, rtol=1e-6)
    np.testing.assert_allclose(gx, want_x, rtol=1e-6, atol=1e-12)
    assert np.all(want_b != 0.0)
    cf = pjt.closed_form(g, llr, 1, ref.NMS, b[None, :])
    np.testing.assert_allclose(cf["grad_beta_e"][0], want_b, rtol=1e-12)
    np.testing.assert_allclose(cf["grad_llr"], want_x, rtol=1e-12, atol=1e-15)


def test_offset_form_on_the_two_check_graph_by_hand():
    """|u| = 1, 2, 2, 3 again; offsets that leave e0 open, close e1 (1 - 1.5 < 0) and e3 (1 - 1 = 0: relu'(0) = 0)"""
    g = two_check_graph()
    b = np.array([[0.5, 1.5, 0.25, 1.0, 0.5]])
    a = np.array([[0.125, 0.25, 0.375, 0.0625, 0.03125]])
    llr = np.array([[1.0, 2.0, -2.0, 3.0]], dtype=np.float32)
    J, gb, ga, gx, P = restatement_grads(g, llr, ref.OMS, b, a)
    b, a = b[0], a[0]
    N = llr.size
    raw, prod = np.array([2.0, 1.0, 1.0, 1.0]), np.array([-1.0, -1.0, 1.0, -1.0])
    is_open = (raw - b[:4] > 0).astype(np.float64)
    assert list(is_open) == [1.0, 0.0, 1.0, 0.0]
    r = prod * (np.maximum(raw - b[:4], 0.0) - a[:4])
    u4 = 2.0 + r[1]
    r4 = (abs(u4) - b[4]) - a[4]                                        # degree 1, open
    Pw = np.array([1.0 + r[0], u4 + r4, -2.0 + r[2], 3.0 + r[3]])
    gv = -sig(-Pw) / N
    want_b = np.append(-gv * prod * is_open, -gv[1])
    want_a = np.append(-gv * prod, -gv[1])
    gm = gv * prod * is_open
    acc1, acc2 = gm[1] + gm[2] + gm[3], gm[0]
    want_x = gv + np.array([acc1, acc2 / 2, -acc2 / 2, 0.0])
    want_x[1] += gv[1] * np.sign(u4)
    np.testing.assert_allclose(P[0], Pw, rtol=1e-6)
    assert J == pytest.approx(np.sum(np.log1p(np.exp(-Pw))) / N, rel=1e-6)
    np.testing.assert_allclose(gb, want_b, rtol=1e-6, atol=1e-15)
    np.testing.assert_allclose(ga, want_a, rtol=1e-6)
    np.testing.assert_allclose(gx[0], want_x, rtol=1e-6)
    assert want_b[1] == 0.0 and want_b[3] == 0.0 and want_b[0] != 0.0
    cf = pjt.closed_form(g, llr, 1, ref.OMS, b[None, :], a[None, :])
    np.testing.assert_allclose(cf["grad_beta_e"][0], want_b, rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(cf["grad_a_e"][0], want_a, rtol=1e-12)
    np.testing.assert_allclose(cf["grad_llr"][0], want_x, rtol=1e-12)


# ---------------------------------------------------------------------------------------------------- the restatement
def test_walk_is_the_layered_decode_with_records():
    """walk's P_t is the layered restatement capped at t + 1 iterations, bit for bit, and U is what the checks consumed"""
    import layered_minsum_cases as lay
    for case in (1, 2, 13):
        graph, family, T, _, _ = cases.CASES[case]
        llr = cases.inputs(case)[0]
        dec = cases.decoder_of(case)
        g = dec.code.tanner_graph()
        beta_e, a_e = lay.edge_tables(dec, family, T)
        U, P = pjt.walk(g, llr, T, lay.form_of(family), beta_e, a_e)
        for t in range(T):
            want = ref.restate(g, llr, T, lay.form_of(family), beta_e, a_e, early_stop=False, max_iters=t + 1)[1]
            assert np.array_equal(P[t], want), (case, t)
        # iteration 0, first non-empty check: u is the LLR itself
        i = next(i for i in range(g.m) if g.check_ptr[i + 1] > g.check_ptr[i])
        e0, e1 = int(g.check_ptr[i]), int(g.check_ptr[i + 1])
        assert np.array_equal(U[0][:, e0:e1], llr[:, g.var_idx[e0:e1]])


@pytest.mark.parametrize("case", [0, 2, 4, 14])
def test_autograd_restatement_equals_the_closed_form(case):
    """the two CPU statements of the gradient agree: torch autograd teacher-forced on the fp32 walk, and scalar loops with
    the formulas written out on a scalar fp32 walk -- the same values, ties and zeros, so they differ by float64 rounding
    of the sums only"""
    import layered_minsum_cases as lay
    graph, family, T, B, _ = cases.CASES[case]
    llr, y, w = cases.inputs(case)
    rows = slice(0, min(B, 12))
    r = cases.restate(cases.decoder_of(case), family, llr[rows], None if y is None else y[rows], w)
    dec = cases.decoder_of(case)
    beta_e, a_e = lay.edge_tables(dec, family, T)
    cf = pjt.closed_form(dec.code.tanner_graph(), llr[rows], T, lay.form_of(family), beta_e, a_e,
                         None if y is None else y[rows].numpy(), None if w is None else w.numpy())
    assert np.array_equal(cf["posterior"], r["P"][-1])
    np.testing.assert_allclose(r["per_iter"], cf["per_iter"], rtol=1e-12)
    scale = np.abs(cf["grad_llr"]).max()
    np.testing.assert_allclose(r["grad_llr"], cf["grad_llr"], rtol=1e-9, atol=1e-12 * scale)


# ---------------------------------------------------------------------------------------------------- the keyword
def _classes():
    import ldpc_decoder
    from neural_2d_decoder import Neural2DMinSumDecoder, Neural2DOffsetMinSumDecoder
    from neural_minsum_decoder import NeuralMinSumDecoder, NeuralOffsetMinSumDecoder
    return [lambda c, **kw: Neural2DMinSumDecoder(c, 2, 2, **kw), lambda c, **kw: Neural2DOffsetMinSumDecoder(c, 2, 2, **kw),
            lambda c, **kw: NeuralMinSumDecoder(c, 2, **kw), lambda c, **kw: NeuralOffsetMinSumDecoder(c, 2, **kw),
            lambda c, **kw: ldpc_decoder.NeuralMinSumDecoder(c, 2, **kw)]


@pytest.mark.parametrize("which", range(5))
def test_layered_gradient_keyword(which):
    import _native as nat
    from ldpc_decoder import create_test_ldpc_code
    code = create_test_ldpc_code()
    make = _classes()[which]
    x = torch.zeros(2, code.n)
    # None: the refusal of before, on the constructor's default and on the call
    dec = make(code, schedule="layered")
    assert dec.layered_gradient is None
    with pytest.raises(NotImplementedError, match="layered"):
        dec.joint_posterior_loss(x)
    with pytest.raises(NotImplementedError, match="layered"):
        dec.joint_posterior_loss(x, layered_gradient=None)
    # unknown names
    with pytest.raises(ValueError, match="layered_gradient"):
        make(code, schedule="layered", layered_gradient="bptt")
    with pytest.raises(ValueError, match="layered_gradient"):
        dec.joint_posterior_loss(x, layered_gradient="bptt")
    # a flooding decoder has nothing to choose
    with pytest.raises(ValueError, match="layered_gradient"):
        make(code, layered_gradient=cases.HOW)
    with pytest.raises(ValueError, match="layered_gradient"):
        make(code).joint_posterior_loss(x, layered_gradient=cases.HOW)
    # the call's value overrides the constructor's: past the refusal, the call goes on to the engine (none here)
    if not torch.cuda.is_available():
        with pytest.raises(nat.NativeEngineError):
            dec.joint_posterior_loss(x, layered_gradient=cases.HOW)
    on = make(code, schedule="layered", layered_gradient=cases.HOW)
    assert on.layered_gradient == cases.HOW
    with pytest.raises(ValueError, match="layered_gradient"):
        on.joint_posterior_loss(x, layered_gradient="bptt")
    # forward under autograd stays refused whatever the keyword says
    with pytest.raises(NotImplementedError, match="layered"):
        on(x)


def test_bridge_validates_the_gradient_name():
    import autograd_bridge as ab
    assert ab.check_layered_gradient(None) is None and ab.check_layered_gradient(None, "flooding") is None
    assert ab.check_layered_gradient("posterior_local") == "posterior_local"
    assert ab.LAYERED_GRADIENTS == ("posterior_local",)
    with pytest.raises(ValueError):
        ab.check_layered_gradient("posterior_local", "flooding")
    with pytest.raises(ValueError):
        ab.check_layered_gradient("straight_through")


def test_native_binding_declares_the_new_entry_points():
    import _native as nat
    assert {"ldpc_train_joint_layered", "ldpc_train_joint_layered_workspace_bytes"} <= set(nat.PRODUCT_EXPORTS)
    header = open(nat.HEADER).read()
    assert "int ldpc_train_joint_layered(" in header and "#define LDPC_HIP_ABI_VERSION 1" in header


# ---------------------------------------------------------------------------------------------------- the trainer, rehearsed
def test_adam_on_the_restatement_gradients_lowers_the_trainer_loss():
    """the run of the GPU trainer test, on the CPU: same model, data seed, shuffling seed, optimiser and epochs, with the
    restatement's gradients -- the last epoch's loss lies below the first's and every beta has moved"""
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
            tot += cases.restate(model, "n2d2", llrs.numpy(), targets, None, want_llr=False)["loss"]
            trainer.optimizer.step()
        for _ in val:                                     # the trainer validates here: its loader draws a seed as well
            pass
        losses.append(tot / len(loader))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    betas = torch.cat([p.detach().reshape(-1) for p in model.beta_weights.values()])
    assert float((betas - t["start"]).abs().min()) > 0.0, betas
    alphas = torch.cat([p.detach().reshape(-1) for p in model.alpha_weights.values()])
    assert float((alphas - t["start"]).abs().max()) == 0.0          # the schedule does not use them: zero gradient, no step
