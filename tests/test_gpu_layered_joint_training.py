"""
GPU tests (-m gpu) of posterior joint training under the layered schedule: ``joint_posterior_loss`` of the five
trainable min-sum decoders with ``schedule="layered"`` and ``layered_gradient="posterior_local"``, the operator
``torch.ops.ldpc.minsum_layered_joint_loss`` and the C function ldpc_train_joint_layered behind them.

What is pinned: the forward is the decoder's own fixed-T layered decode bit for bit (against both decode kernels, and
every iteration's posterior against the decode capped there); loss and gradients equal the CPU restatement
tests/layered_pjt_reference.py, which is teacher-forced on fp32 values the forward reproduces bit for bit -- so no case
and no row is left out; tolerances are those of tests/test_gpu_joint_training.py (the reduction machinery is the same).
"""
import numpy as np
import pytest
import torch

import layered_pjt_cases as cases

pytestmark = pytest.mark.gpu

HOW = cases.HOW


def close(got, want, what, rtol=2e-3, rel_atol=2e-4):
    """``close`` of tests/test_gpu_joint_training.py"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(float(np.abs(want).max()), 1e-30)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=rel_atol * scale, err_msg=what)


def run(dec, llr, y, w, dev):
    x = torch.from_numpy(np.array(llr)).to(dev).requires_grad_(True)
    dec.zero_grad()
    loss, per_iter, bits, post = dec.joint_posterior_loss(x, None if y is None else y.to(dev), w, layered_gradient=HOW)
    loss.backward()
    return x, loss.detach(), per_iter.detach(), bits, post.detach(), cases.grads_of(dec), x.grad.detach().clone()


# ---------------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("case", range(len(cases.CASES)))
def test_forward_loss_and_gradients_match_the_restatement(gpu_device, case):
    graph, family, T, B, kind = cases.CASES[case]
    llr, y, w = cases.inputs(case)
    want = cases.restated(case)
    dec = cases.decoder_of(case)
    x, loss, per_iter, bits, post, got, got_x = run(dec, llr, y, w, gpu_device)
    tag = f"{graph} {family} T={T} B={B} {kind}"
    # forward: the decoder's own fixed-T decode, on the LDS-resident and on the streaming kernel, and the fp32 restatement
    eng = dec._get_engine(gpu_device)
    xd = x.detach()
    try:
        for mode in ("auto", "stream"):
            eng.set_mode(mode)
            res = eng.decode(xd, early_stop=False)
            assert torch.equal(post, res.posterior) and torch.equal(bits, res.bits), (tag, mode, eng.info()["kernel"])
    finally:
        eng.set_mode("auto")
    np.testing.assert_array_equal(post.cpu().numpy(), want["P"][T - 1], err_msg=tag)
    for t in range(T):                              # what the restatement is forced on IS the decode capped at t + 1
        pt = eng.decode(xd, early_stop=False, max_iters=t + 1).posterior
        np.testing.assert_array_equal(pt.cpu().numpy(), want["P"][t], err_msg=f"{tag} P_{t}")
    # loss
    np.testing.assert_allclose(per_iter.cpu().numpy(), want["per_iter"], rtol=1e-4, err_msg=tag)
    assert abs(loss.item() - want["loss"]) <= 1e-4 * abs(want["loss"])
    # gradients: every parameter, the whole LLR gradient, nothing left out
    if family != "n2d4":                            # sharing type 4 has no beta parameter: its table gradients are all 0
        assert any(float(v.abs().max()) > 0 for v in want["grads"].values())
    assert set(got) == set(want["grads"])
    for k in want["grads"]:
        close(got[k], want["grads"][k], f"{tag} {k}")
    close(got_x.cpu().numpy(), want["grad_llr"], f"{tag} d J/d llr")
    # the variable-side alpha of the normalised forms is not used by the schedule: exactly 0
    if family in ("n2d2", "n2d4"):
        alphas = [v for k, v in got.items() if k.startswith("alpha_weights")]
        assert alphas and all(float(v.abs().max()) == 0.0 for v in alphas)


@pytest.mark.parametrize("graph,family", [("toy", "n2d2"), ("small", "n2d_oms")])
def test_every_iterations_posterior_is_the_capped_decode(gpu_device, graph, family):
    """P_t of the training loop itself: a decoder holding the first t + 1 rows of the tables returns, as the posterior of
    its own joint loss, what the full decoder's decode gives when capped at t + 1"""
    from engine import DecodeEngine
    T, B = 4, 65
    dec = cases.make(graph, family, T, seed=77)
    x = torch.from_numpy(cases.llr_of(graph, B, "awgn", 77)).to(gpu_device)
    full = dec._get_engine(gpu_device)
    layout = dec._sharing_layout()
    beta, alpha = dec.weight_tables()
    for t in range(T):
        part = DecodeEngine(dec.code.tanner_graph(), dtype=torch.float32, iters=t + 1, device=gpu_device,
                            **dec._engine_kwargs(layout, beta[:t + 1], alpha[:t + 1]))
        r = part.train_joint_layered(x, want_grads=False)
        capped = full.decode(x, early_stop=False, max_iters=t + 1)
        assert torch.equal(r["posterior"], capped.posterior) and torch.equal(r["bits"], capped.bits), t


# ---------------------------------------------------------------------------------------------------- 2. closed form
def test_one_iteration_on_the_toy_code_in_closed_form(gpu_device):
    """T = 1, per-edge weights: the gradient from the LLRs alone, by the scalar loops of layered_pjt_reference.closed_form
    (no autograd, no records)"""
    import layered_minsum_cases as lay
    import layered_pjt_reference as pjt
    case = cases.CASES.index(("toy", "edge_nms", 1, 130, "awgn"))
    llr, y, w = cases.inputs(case)
    dec = cases.decoder_of(case)
    g = dec.code.tanner_graph()
    beta_e, _ = lay.edge_tables(dec, "edge_nms", 1)
    cf = pjt.closed_form(g, llr, 1, lay.form_of("edge_nms"), beta_e, None, None if y is None else y.numpy(),
                         None if w is None else w.numpy())
    _, loss, per_iter, _, post, got, got_x = run(dec, llr, y, w, gpu_device)
    np.testing.assert_array_equal(post.cpu().numpy(), cf["posterior"])
    np.testing.assert_allclose(per_iter.cpu().numpy(), cf["per_iter"], rtol=1e-4)
    rows, cols = g.check_of_edge.tolist(), g.var_idx.tolist()
    got_e = np.array([float(got[f"beta_weights.iter_0_c{i}_v{j}"]) for i, j in zip(rows, cols)])
    assert np.abs(cf["grad_beta_e"][0]).max() > 0
    close(got_e, cf["grad_beta_e"][0], "d J/d beta per edge")
    close(got_x.cpu().numpy(), cf["grad_llr"], "d J/d llr")


# ---------------------------------------------------------------------------------------------------- 3. plumbing
def test_two_runs_are_bit_identical(gpu_device):
    case = cases.CASES.index(("small", "n2d2", 4, 130, "half"))
    llr, y, w = cases.inputs(case)
    dec = cases.decoder_of(case)
    a = run(dec, llr, y, w, gpu_device)
    b = run(dec, llr, y, w, gpu_device)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[4], b[4]) and torch.equal(a[6], b[6])
    assert all(torch.equal(a[5][k], b[5][k]) for k in a[5])


def test_targets_weights_and_the_loss_only_call(gpu_device):
    import torch.nn.functional as F
    case = cases.CASES.index(("small", "n2d3", 4, 65, "awgn"))
    T = 4
    llr = cases.inputs(case)[0]
    dec = cases.decoder_of(case)
    eng = dec._get_engine(gpu_device)
    x = torch.from_numpy(np.array(llr)).to(gpu_device)
    rng = np.random.default_rng(3)
    y = torch.from_numpy(rng.uniform(0, 1, llr.shape).astype(np.float32)).to(gpu_device)
    w = torch.tensor([0.0, 0.0, 1.5, 0.0], device=gpu_device)
    full = eng.train_joint_layered(x, y, w, want_grads=True, want_grad_llr=True)
    # targets: J_t is the BCE against them, on the capped decode's posterior
    for t in range(T):
        pt = eng.decode(x, early_stop=False, max_iters=t + 1).posterior
        want = F.binary_cross_entropy_with_logits(-pt.double(), y.double()).item()
        assert abs(full["loss_per_iter"][t].item() - want) <= 1e-5 * abs(want), t
    assert abs(full["loss"].item() - 1.5 * full["loss_per_iter"][2].item()) <= 1e-6 * abs(full["loss"].item())
    # weights: only iteration 2 carries a gradient, and it scales with its weight
    gb = full["grad_beta"]
    assert float(gb[2].abs().max()) > 0 and float(gb[[0, 1, 3]].abs().max()) == 0.0
    assert float(full["grad_alpha"].abs().max()) == 0.0 and full["grad_oms_alpha"] is None
    twice = eng.train_joint_layered(x, y, 2.0 * w, want_grads=True, want_grad_llr=True)
    torch.testing.assert_close(twice["grad_beta"], 2.0 * gb, rtol=1e-6, atol=0.0)
    torch.testing.assert_close(twice["grad_llr"], 2.0 * full["grad_llr"], rtol=1e-6, atol=0.0)
    # want_grads False: the loss alone, same numbers, same decode
    only = eng.train_joint_layered(x, y, w, want_grads=False)
    assert only["grad_beta"] is None and only["grad_alpha"] is None and only["grad_llr"] is None
    assert torch.equal(only["loss_per_iter"], full["loss_per_iter"]) and torch.equal(only["posterior"], full["posterior"])
    assert torch.equal(only["bits"], full["bits"])
    with torch.no_grad():
        loss, per_iter, bits, post = dec.joint_posterior_loss(x, y, w, layered_gradient=HOW)
    assert not loss.requires_grad and torch.equal(per_iter, full["loss_per_iter"]) and torch.equal(post, full["posterior"])
    # an empty batch: zero losses and gradients
    empty = eng.train_joint_layered(torch.zeros(0, llr.shape[1], device=gpu_device))
    assert float(empty["loss_per_iter"].abs().sum()) == 0.0 and float(empty["grad_beta"].abs().max()) == 0.0


def test_opcheck(gpu_device):
    import torch_ops
    for case in (cases.CASES.index(("toy", "n2d2", 4, 64, "awgn")), cases.CASES.index(("toy", "n2d_oms", 4, 65, "awgn"))):
        family = cases.CASES[case][1]
        dec = cases.decoder_of(case)
        eng = dec._get_engine(gpu_device)
        offset = family == "n2d_oms"
        bt, at = dec._sharing_layout().tables_torch(dec.beta_weights, dec.alpha_weights, 4, dec._beta_default,
                                                    dec._alpha_default)
        h = torch_ops.engine_handle(eng)
        xs = torch.from_numpy(np.array(cases.inputs(case)[0][:5])).to(gpu_device)
        w = torch.full((4,), 0.25, device=gpu_device)
        utils = ("test_schema", "test_autograd_registration", "test_faketensor")
        torch.library.opcheck(torch.ops.ldpc.minsum_layered_joint_loss,
                              (xs, None, bt.detach().clone().requires_grad_(True), at.detach().clone().requires_grad_(True), w, h,
                               offset, True, False), test_utils=utils)
        torch.library.opcheck(torch.ops.ldpc.minsum_layered_joint_loss,
                              (xs, torch.rand_like(xs), bt.detach().clone(), at.detach().clone(), w, h, offset, False, False),
                              test_utils=utils)


def test_entry_points_refuse_each_others_decoders(gpu_device):
    import layered_minsum_cases as lay
    from ldpc_decoder import BasicMinSumDecoder, create_test_ldpc_code
    from rcq_decoder import RCQMinSumDecoder, WeightedRCQDecoder
    code = create_test_ldpc_code()
    x = torch.randn(5, code.n, device=gpu_device)
    qp = [(3.0, 1.3)]
    # ldpc_train_joint_layered names the entry point a flooding decoder takes ...
    flooding = lay.make("n2d2", code, 3, 1, schedule="flooding")._get_engine(gpu_device)
    with pytest.raises(NotImplementedError, match=r"ldpc_train_joint\b(?!_)"):
        flooding.train_joint_layered(x)
    with pytest.raises(NotImplementedError, match="ldpc_train_joint_ste"):
        WeightedRCQDecoder(code, 3, 8, qp, 2, 4)._get_engine(gpu_device).train_joint_layered(x)
    # ... and has nothing for the layered RCQ decoders and float64
    for dec in (RCQMinSumDecoder(code, 3, 8, qp, 4, layered=True), RCQMinSumDecoder(code, 3, 8, qp, 4, layered="paper"),
                WeightedRCQDecoder(code, 3, 8, qp, 2, 4, layered="paper")):
        with pytest.raises(NotImplementedError):
            dec._get_engine(gpu_device).train_joint_layered(x)
    f64 = BasicMinSumDecoder(lay.with_iterations(code, 3), 0.7)._engine(torch.float64, gpu_device)
    with pytest.raises(NotImplementedError):
        f64.train_joint_layered(x.double())
    # the older entry points keep refusing a layered decoder
    layered = lay.make("n2d2", code, 3, 1)
    eng = layered._get_engine(gpu_device)
    with pytest.raises(NotImplementedError, match="layered"):
        eng.train_joint(x)
    with pytest.raises(NotImplementedError, match="layered"):
        eng.decode_saving(x)
    with pytest.raises(NotImplementedError, match="layered"):
        layered.joint_posterior_loss(x)
    with pytest.raises(NotImplementedError, match="layered"):
        layered(x)


# ---------------------------------------------------------------------------------------------------- 4. trainer
def test_trainer_with_the_joint_loss_trains_a_layered_decoder(gpu_device):
    """the run tests/test_layered_joint_training_host.py rehearses on the CPU"""
    from training_framework import PosteriorJointTrainer
    t = cases.TRAIN
    torch.manual_seed(t["torch_seed"])
    code, model = cases.trainer_model()
    trainer = PosteriorJointTrainer(model, cases.trainer_config("cuda"))
    hist = trainer.train(code, num_train_samples=t["num_train"], num_val_samples=t["num_val"])
    assert len(hist["train_losses"]) >= 2 and hist["train_losses"][-1] < hist["train_losses"][0], hist["train_losses"]
    assert all(np.isfinite(hist["gradient_norms"])) and hist["gradient_norms"][0] > 0
    assert all(len(v) == t["T"] for v in hist["train_iteration_losses"])
    betas = torch.cat([p.detach().reshape(-1) for p in model.beta_weights.values()])
    assert float((betas - t["start"]).abs().min()) > 0.0, betas
