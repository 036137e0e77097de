"""
GPU tests (-m gpu) of posterior joint training of the quantised decoder: ``WeightedRCQDecoder.joint_posterior_loss`` with
``quantizer_gradient="straight_through"``, the registered operator ``torch.ops.ldpc.rcq_joint_loss`` and the C function
ldpc_train_joint_ste behind them.

What is pinned: the forward is the decoder's own fixed-T decode bit for bit, every iteration; the gradients equal torch
autograd on the teacher-forced CPU restatement tests/pjt_rcq_reference.py (tolerances of tests/test_gpu_joint_training.py)
on the input sets of tests/pjt_rcq_cases.py, whose teacher forcing tests/test_joint_training_rcq_host.py keeps honest; at
T = 1 the beta gradient equals a closed form computed in numpy from the LLRs and the codes alone; the result is
bit-identical from run to run; the trainer lowers the loss from the plain-RCQ start.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pjt_rcq_cases as cases

pytestmark = pytest.mark.gpu

STE = {"quantizer_gradient": "straight_through"}


def grads_of(dec):
    return {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()).cpu() for k, p in dec.named_parameters()}


def close(got, want, what, rtol=2e-3, rel_atol=2e-4):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(float(np.abs(want).max()), 1e-30)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=rel_atol * scale, err_msg=what)


# ---------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("name,wtype,bc,B", [("toy", 2, 3, 37), ("small", 1, 4, 300), ("ira", 2, 3, 70),
                                           ("small", 2, 8, 300), ("small", 1, 6, 70)])
def test_forward_is_the_fixed_iteration_decode(gpu_device, name, wtype, bc, B):
    T = 6                                           # three quantisers: the schedule changes twice (0, 0, 1, 1, 2, 2)
    code = cases.load(name, T)
    dec = cases.make_decoder(code, wtype, bc, cases.QP3, T, seed=1, **STE)
    x = torch.from_numpy(cases.channel(np.random.default_rng(1), B, code.n, (1.5, 5.0))).to(gpu_device)
    with torch.no_grad():
        loss, per_iter, bits, post = dec.joint_posterior_loss(x)
    eng = dec._get_engine(gpu_device)
    ref = eng.decode(x, early_stop=False)
    assert torch.equal(post, ref.posterior) and torch.equal(bits, ref.bits)
    assert per_iter.shape == (T,)
    for t in range(T):
        pt = eng.decode(x, early_stop=False, max_iters=t + 1).posterior
        want = F.binary_cross_entropy_with_logits(-pt, torch.zeros_like(pt)).item()
        assert abs(per_iter[t].item() - want) <= 1e-5 * abs(want), (t, per_iter[t].item(), want)
    assert abs(loss.item() - per_iter.mean().item()) <= 1e-6 * abs(loss.item())
    # the keyword form on a decoder built without the option is the same call
    plain = cases.make_decoder(code, wtype, bc, cases.QP3, T, seed=1)
    with torch.no_grad():
        _, per2, bits2, post2 = plain.joint_posterior_loss(x, **STE)
    assert torch.equal(per2, per_iter) and torch.equal(bits2, bits) and torch.equal(post2, post)
    with pytest.raises(NotImplementedError):        # the existing entry points keep refusing the quantised decoder
        eng.train_joint(x)


# ---------------------------------------------------------------------------------------------------- 2. restatement
@pytest.mark.parametrize("case", range(len(cases.CASES)))
def test_gradients_match_the_restatement(gpu_device, case, oracle_mod):
    name = cases.CASES[case][0]
    code, llr, y, w = cases.inputs(case)
    dec = cases.decoder_of(case, **STE)
    x = torch.from_numpy(llr).to(gpu_device).requires_grad_(True)
    loss, per_iter, bits, post = dec.joint_posterior_loss(x, None if y is None else y.to(gpu_device), w)
    loss.backward()
    got, got_x = grads_of(dec), x.grad.cpu().numpy()
    dec.zero_grad()

    r = cases.restate(dec, llr, y, w)
    want = grads_of(dec)
    # the teacher's posterior first: the codes the restatement is forced with are the codes the kernels wrote
    np.testing.assert_array_equal(post.detach().cpu().numpy(), r["trace_posterior"])
    np.testing.assert_array_equal(bits.cpu().numpy(), r["trace_bits"])
    assert r["disagree"] <= 1e-3
    np.testing.assert_allclose(per_iter.detach().cpu().numpy(), r["per_iter"], rtol=1e-4)
    assert any(float(v.abs().max()) > 0 for v in want.values())
    for k in want:
        close(got[k], want[k], f"{cases.CASES[case]} {k}")
    # d J/d llr: element-wise; a min / min2 near-tie may send one check's gradient to another edge -- rows where that
    # happened (rare on the larger codes) are left out, as in test_gpu_joint_training
    gx = r["grad_llr"]
    scale = np.abs(gx).max()
    ok = np.all(np.abs(got_x - gx) <= 2e-3 * np.abs(gx) + 2e-4 * scale, axis=1)
    assert ok.mean() >= (1.0 if name != "ira" else 0.9), ok.mean()


# ---------------------------------------------------------------------------------------------------- 3. T = 1 anchor
@pytest.mark.parametrize("B,bc", [(50, 3), (200, 3), (200, 8)], ids=["50", "200", "200-bc8"])
def test_one_iteration_closed_form(gpu_device, oracle_mod, B, bc):
    """d J/d beta_0[s] = sum over b and the edges e of slot s of g_l[b, v(e)] * mask[b, e] * s_excl[b, e] * minval[b, e],
    g_l = -sigmoid(-l_0) / (B n), l_0 = llr + sum of the reconstructed codes -- numpy, fp64, from the LLRs and the codes"""
    import pjt_rcq_reference as ref
    code = cases.load("small", 1)
    dec = cases.make_decoder(code, 2, bc, [(3.0, 1.3)], 1, seed=11, **STE)
    llr = cases.channel(np.random.default_rng(12), B, code.n, (2.0, 5.0))
    x = torch.from_numpy(llr).to(gpu_device)
    dec.joint_posterior_loss(x)[0].backward()
    lay = dec._sharing_layout()
    beta, alpha = dec.weight_tables()
    thr, qoi = cases.quantiser_tables(dec)
    g = cases.oracle_graph(code)
    _, _, codes = ref.trace(g, llr, beta, lay.beta_slot, alpha, lay.alpha_slot, thr, qoi, 1)
    codes = codes[:, 0, :].astype(np.int64)
    L = thr.shape[1]
    tau = thr[0].astype(np.float64)
    deq = np.where(codes >= L, -1.0, 1.0) * tau[codes % L]
    mask = (codes % L) < L - 1
    l0 = llr.astype(np.float64)
    np.add.at(l0, (slice(None), g.var_idx), deq)
    gl = -1.0 / (1.0 + np.exp(l0)) / (B * g.n)
    want = np.zeros(beta.shape[1])
    for i in range(g.m):
        e0, e1 = int(g.check_ptr[i]), int(g.check_ptr[i + 1])
        v = llr[:, g.var_idx[e0:e1]].astype(np.float64)                     # v2c_0 = llr
        mag, sgn = np.abs(v), np.sign(v)
        order = np.argsort(mag, axis=1, kind="stable")
        k = order[:, 0]
        m1 = mag[np.arange(B), k]
        m2 = mag[np.arange(B), order[:, 1]] if e1 - e0 > 1 else m1
        for u in range(e1 - e0):
            minval = np.where(k == u, m2, m1)
            s_excl = np.prod(np.delete(sgn, u, axis=1), axis=1)
            e = e0 + u
            want[lay.beta_slot[e]] += float(np.sum(gl[:, g.var_idx[e]] * mask[:, e] * s_excl * minval))
    got = grads_of(dec)
    dec.zero_grad()
    # the closed form is per table column; the decoder's own (linear) parameter -> table map carries it to the parameters
    bt, _ = lay.tables_torch(dec.beta_weights, dec.alpha_weights, 1, dec._beta_default, dec._alpha_default)
    (bt[0].double() * torch.from_numpy(want)).sum().backward()
    want_p = grads_of(dec)
    assert np.abs(want).max() > 0 and mask.any() and not mask.all()
    for k in dec.beta_weights.keys():
        np.testing.assert_allclose(got[f"beta_weights.{k}"].numpy(), want_p[f"beta_weights.{k}"].numpy(), rtol=1e-5, atol=1e-7,
                                   err_msg=k)
    assert all(float(got[f"alpha_weights.{k}"].abs().max()) == 0.0 for k in dec.alpha_weights.keys())   # alpha_T-1 gets 0


@pytest.mark.parametrize("tau0", [0.0, 1.5])
def test_one_level_passes_no_gradient_to_the_weights(gpu_device, oracle_mod, tau0):
    """L = 1 (the C ABI's smallest decoder; with tau = 1.5 its one level reconstructs a non-zero value): every code is the top
    level, so the straight-through mask `level < L - 1` is never set and no gradient reaches a beta or an alpha -- exactly
    zero.  The posterior of iteration t is llr + (a constant the codes alone fix), so d J/d llr is the gradient of the loss
    through l_t = llr + const_t: torch autograd on the CPU in fp64, tolerances of test_gradients_match_the_restatement."""
    import _native as nat
    import quantiser_width_cases as qw
    from engine import DecodeEngine
    case = qw.Level(1, tau0, 70, 70)
    code, T, kw = qw.level_tables(oracle_mod, case)
    eng = DecodeEngine(code.tanner_graph(), dtype=torch.float32, c2v_form=nat.C2V_RCQ, iters=T, device=gpu_device, **kw)
    rng = np.random.default_rng(21)
    llr = cases.channel(rng, case.B, code.n, (0.5, 4.0))
    y = torch.from_numpy(rng.uniform(0, 1, llr.shape).astype(np.float32) * (rng.random(llr.shape) < 0.3))
    w = torch.tensor(rng.uniform(0.1, 1.0, T), dtype=torch.float32)
    x = torch.from_numpy(llr).to(gpu_device)
    out = eng.train_joint_ste(x, y.to(gpu_device), w.to(gpu_device), want_grads=True, want_grad_llr=True)
    assert out["grad_beta"].shape == kw["beta"].shape and out["grad_alpha"].shape == kw["alpha"].shape
    assert float(out["grad_beta"].abs().max()) == 0.0 and float(out["grad_alpha"].abs().max()) == 0.0
    xl = torch.from_numpy(llr).double().requires_grad_(True)
    J, per = 0.0, []
    for t in range(T):
        post = eng.decode(x, early_stop=False, max_iters=t + 1).posterior
        const = (post - x).cpu().double()
        if tau0 == 0.0:
            assert float(const.abs().max()) == 0.0
        per.append(F.binary_cross_entropy_with_logits(-(xl + const), y.double()))
        J = J + w[t].double() * per[-1]
    assert tau0 == 0.0 or float(const.abs().max()) > 0.0
    J.backward()
    np.testing.assert_allclose(out["loss_per_iter"].cpu().numpy(), [float(v.detach()) for v in per], rtol=1e-4)
    assert float(xl.grad.abs().max()) > 0
    close(out["grad_llr"].cpu().numpy(), xl.grad.numpy(), f"d J/d llr, one level, tau = {tau0}")


# ---------------------------------------------------------------------------------------------------- 4. plumbing
def test_determinism_empty_batch_and_opcheck(gpu_device):
    import torch_ops
    T = 5
    code = cases.load("ira", T)
    dec = cases.make_decoder(code, 1, 3, cases.QP3, T, seed=7, **STE)
    x = torch.from_numpy(cases.channel(np.random.default_rng(8), 300, code.n, (1.5, 5.0))).to(gpu_device).requires_grad_(True)
    runs = []
    for _ in range(2):
        dec.zero_grad()
        x.grad = None
        loss, per_iter, _, _ = dec.joint_posterior_loss(x)
        loss.backward()
        runs.append((loss.detach().clone(), per_iter.clone(), grads_of(dec), x.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][3], runs[1][3])
    assert all(torch.equal(runs[0][2][k], runs[1][2][k]) for k in runs[0][2])
    assert any(float(v.abs().max()) > 0 for v in runs[0][2].values()) and float(runs[0][3].abs().max()) > 0

    dec.zero_grad()
    loss, per_iter, bits, post = dec.joint_posterior_loss(torch.zeros(0, code.n, device=gpu_device))
    assert bits.shape == (0, code.n) and post.shape == (0, code.n) and per_iter.shape == (T,)
    assert float(loss) == 0.0 and float(per_iter.abs().sum()) == 0.0
    loss.backward()
    assert all(float(v.abs().max()) == 0.0 for v in grads_of(dec).values())

    eng = dec._get_engine(gpu_device)
    lay = dec._sharing_layout()
    bt, at = lay.tables_torch(dec.beta_weights, dec.alpha_weights, T, dec._beta_default, dec._alpha_default)
    h = torch_ops.engine_handle(eng)
    xs = x.detach()[:5].contiguous()
    w = torch.full((T,), 0.2, device=gpu_device)
    torch.library.opcheck(torch.ops.ldpc.rcq_joint_loss,
                          (xs, None, bt.detach().clone().requires_grad_(True), at.detach().clone().requires_grad_(True), w, h,
                           True, False),
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
    torch.library.opcheck(torch.ops.ldpc.rcq_joint_loss,
                          (xs, torch.rand_like(xs), bt.detach().clone(), at.detach().clone(), w, h, False, False),
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
    # the straight-through entry point is for the quantised decoder only
    from neural_2d_decoder import Neural2DMinSumDecoder
    with pytest.raises(NotImplementedError):
        Neural2DMinSumDecoder(code, 2, T)._get_engine(gpu_device).train_joint_ste(xs)
    # its scratch keeps 1-byte C2V rows: smaller than the fp32 forms' on the same code and batch
    assert eng.train_joint_ste_workspace_bytes(300) < eng.train_joint_workspace_bytes(300)


# ---------------------------------------------------------------------------------------------------- 5. trainer
def test_trainer_with_the_straight_through_loss_reduces_the_loss(gpu_device):
    from training_framework import PosteriorJointTrainer
    t = cases.TRAIN
    torch.manual_seed(t["torch_seed"])
    code, model = cases.trainer_model(**STE)
    trainer = PosteriorJointTrainer(model, cases.trainer_config("cuda"))
    hist = trainer.train(code, num_train_samples=t["num_train"], num_val_samples=t["num_val"])
    assert set(hist) >= {"train_losses", "train_accuracies", "gradient_norms", "train_iteration_losses"}
    assert len(hist["train_losses"]) >= 2 and all(np.isfinite(hist["train_losses"]))
    assert hist["train_losses"][-1] < hist["train_losses"][0], hist["train_losses"]
    assert all(np.isfinite(hist["gradient_norms"])) and hist["gradient_norms"][0] > 0
    assert len(hist["train_iteration_losses"]) == len(hist["train_losses"])
    assert all(len(v) == t["T"] for v in hist["train_iteration_losses"])
    vals = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    assert float((vals - 1.0).abs().max()) > 0.05
