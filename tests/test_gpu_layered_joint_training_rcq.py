"""
GPU tests (-m gpu) of posterior joint training of ``WeightedRCQDecoder(layered="paper")``: ``joint_posterior_loss`` with
``quantizer_gradient="straight_through"`` and ``layered_gradient="posterior_local"``, the operator
``torch.ops.ldpc.rcq_layered_joint_loss`` and the C function ldpc_train_joint_layered_ste behind them.

What is pinned: the forward is the decoder's own fixed-T layered decode bit for bit (against both decode kernels, every
iteration's loss against the decode capped there, and the posterior against the free-running fp32 restatement); loss and
gradients equal the CPU restatement tests/layered_pjt_rcq_reference.py, whose records the forward reproduces bit for bit --
so no case and no row is left out; on disjoint checks at T = 1 the path equals ldpc_train_joint_ste on the flooding decoder,
which the reference's goldens pin.  Tolerances are those of tests/test_gpu_joint_training_rcq.py (same reductions).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layered_pjt_rcq_cases as cases
import pjt_rcq_cases as flood

pytestmark = pytest.mark.gpu

HOW = cases.HOW


def close(got, want, what, rtol=2e-3, rel_atol=2e-4):
    """``close`` of tests/test_gpu_joint_training_rcq.py"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(float(np.abs(want).max()), 1e-30)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=rel_atol * scale, err_msg=what)


def run(dec, llr, y, w, dev):
    x = torch.from_numpy(np.array(llr)).to(dev).requires_grad_(True)
    dec.zero_grad()
    loss, per_iter, bits, post = dec.joint_posterior_loss(x, None if y is None else y.to(dev), w)
    loss.backward()
    return loss.detach(), per_iter.detach(), bits, post.detach(), cases.grads_of(dec), x.grad.detach().clone()


# ---------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("name,wtype,bc,B", [("toy", 1, 3, 37), ("small", 2, 4, 67), ("ira", 2, 3, 37), ("wide", 3, 8, 67)])
def test_forward_is_the_fixed_iteration_decode(gpu_device, monkeypatch, name, wtype, bc, B):
    T = 6                                           # three quantisers: the schedule changes twice (0, 0, 1, 1, 2, 2)
    code = cases.load(name, T)
    dec = cases.make_decoder(code, wtype, bc, cases.QP3, T, seed=1, **HOW)
    assert list(cases.quantiser_tables(dec)[1]) == [0, 0, 1, 1, 2, 2]
    llr = flood.channel(np.random.default_rng(1), B, code.n, (1.5, 5.0))
    llr[0, :3] = 0.0
    llr[1] = np.round(llr[1])
    x = torch.from_numpy(llr).to(gpu_device)
    with torch.no_grad():
        loss, per_iter, bits, post = dec.joint_posterior_loss(x)
    assert not loss.requires_grad and per_iter.shape == (T,)
    assert abs(loss.item() - per_iter.mean().item()) <= 1e-6 * abs(loss.item())
    kernels = set()
    for mode in ("auto", "stream"):                 # the LDS-resident kernel (where the code qualifies) and the streaming one
        monkeypatch.setenv("LDPC_ENGINE_MODE", mode)
        dec._engine = None                          # a fresh engine reads the mode
        eng = dec._get_engine(gpu_device)
        ref = eng.decode(x, early_stop=False)
        kernels.add(eng.info()["kernel"])
        assert torch.equal(post, ref.posterior) and torch.equal(bits, ref.bits), (mode, eng.info()["kernel"])
        for t in range(T):
            pt = eng.decode(x, early_stop=False, max_iters=t + 1).posterior
            want = F.binary_cross_entropy_with_logits(-pt, torch.zeros_like(pt)).item()
            assert abs(per_iter[t].item() - want) <= 1e-5 * abs(want), (mode, t, per_iter[t].item(), want)
    assert "layered_paper_lds" in kernels and len(kernels) == 2, kernels
    _, _, P = cases.walk_of(dec, llr)
    np.testing.assert_array_equal(post.cpu().numpy(), P[T - 1])
    np.testing.assert_array_equal(bits.cpu().numpy(), (P[T - 1] < 0).astype(np.int32))
    # the keyword form on a decoder built without the options is the same call
    plain = cases.make_decoder(code, wtype, bc, cases.QP3, T, seed=1)
    with torch.no_grad():
        _, per2, bits2, post2 = plain.joint_posterior_loss(x, **HOW)
    assert torch.equal(per2, per_iter) and torch.equal(bits2, bits) and torch.equal(post2, post)


# ---------------------------------------------------------------------------------------------------- 2. restatement
@pytest.mark.parametrize("case", range(len(cases.CASES)))
def test_gradients_match_the_restatement(gpu_device, case):
    _, wtype, _, _, B, _, _ = cases.CASES[case]
    _, llr, y, w = cases.inputs(case)
    want = cases.restated(case)
    assert want["disagree"] == 0.0
    dec = cases.decoder_of(case, **HOW)
    loss, per_iter, bits, post, got, got_x = run(dec, llr, y, w, gpu_device)
    tag = str(cases.CASES[case])
    T = cases.T_GRAD
    # the forward first: what the restatement is forced on is what the kernels computed
    np.testing.assert_array_equal(post.cpu().numpy(), want["P"][T - 1], err_msg=tag)
    np.testing.assert_array_equal(bits.cpu().numpy(), (want["P"][T - 1] < 0).astype(np.int32), err_msg=tag)
    np.testing.assert_allclose(per_iter.cpu().numpy(), want["per_iter"], rtol=1e-4, err_msg=tag)
    assert abs(loss.item() - want["loss"]) <= 1e-4 * abs(want["loss"])
    # the tables, from the engine: beta against the restatement's table gradient, alpha (unused by the schedule) exactly 0
    eng = dec._get_engine(gpu_device)
    x = torch.from_numpy(np.array(llr)).to(gpu_device)
    out = eng.train_joint_layered_ste(x, None if y is None else y.to(gpu_device), w, want_grads=True, want_grad_llr=True)
    assert float(np.abs(want["grad_beta"]).max()) > 0
    assert out["grad_beta"].shape == want["grad_beta"].shape
    close(out["grad_beta"].cpu().numpy(), want["grad_beta"], f"{tag} d J/d beta table")
    assert out["grad_alpha"].shape[0] == T and float(out["grad_alpha"].abs().max()) == 0.0 and out["grad_oms_alpha"] is None
    assert torch.equal(out["grad_llr"], got_x) and torch.equal(out["posterior"], post)
    # the parameters, through autograd: every one of them
    if wtype != 4:                                  # sharing type 4 has no beta parameter
        assert any(float(v.abs().max()) > 0 for k, v in want["grads"].items() if k.startswith("beta_weights"))
    assert set(got) == set(want["grads"])
    for k in want["grads"]:
        close(got[k], want["grads"][k], f"{tag} {k}")
    assert all(float(v.abs().max()) == 0.0 for k, v in got.items() if k.startswith("alpha_weights"))
    # d J/d llr: the whole array, no row left out -- U is the kernel's bit for bit, so the arg-min edges cannot differ
    close(got_x.cpu().numpy(), want["grad_llr"], f"{tag} d J/d llr")


# ---------------------------------------------------------------------------------------------------- 3. flooding anchor
def disjoint_code(T):
    """every variable in exactly one check: checks of degree 1, 2, 3, 5, 6, 7 on 24 variables, interleaved"""
    from ldpc_decoder import LDPCCode
    degs = [1, 2, 3, 5, 6, 7]
    n = sum(degs)
    order = np.random.default_rng(5).permutation(n)
    H = np.zeros((len(degs), n), dtype=np.int64)
    at = 0
    for i, d in enumerate(degs):
        H[i, order[at:at + d]] = 1
        at += d
    assert np.all(H.sum(axis=0) == 1)
    return LDPCCode(n=n, k=n - len(degs), H=H, max_iterations=T)


@pytest.mark.parametrize("wtype,bc", [(1, 3), (2, 8)])
def test_one_iteration_on_disjoint_checks_is_the_flooding_path(gpu_device, wtype, bc):
    """variables of degree 1, T = 1: the layered walk and the flooding sweeps compute the same thing -- posterior
    llr + the one message, J_0 through the one check update -- so the new path must equal ldpc_train_joint_ste on the
    flooding decoder with the same tables"""
    code = disjoint_code(1)
    B = 67
    lay = cases.make_decoder(code, wtype, bc, cases.QP3, 1, seed=3, **HOW)
    fl = flood.make_decoder(code, wtype, bc, cases.QP3, 1, seed=3, quantizer_gradient="straight_through")
    assert all(torch.equal(a, b) for a, b in zip(lay.parameters(), fl.parameters()))
    rng = np.random.default_rng(4)
    llr = flood.channel(rng, B, code.n, (3.0, 7.0))
    llr[0, :3] = 0.0
    llr[1] = np.round(llr[1])
    x = torch.from_numpy(llr).to(gpu_device)
    y = torch.from_numpy(rng.uniform(0, 1, llr.shape).astype(np.float32)).to(gpu_device)
    w = torch.tensor([0.7], device=gpu_device)
    a = lay._get_engine(gpu_device).train_joint_layered_ste(x, y, w, want_grads=True, want_grad_llr=True)
    b = fl._get_engine(gpu_device).train_joint_ste(x, y, w, want_grads=True, want_grad_llr=True)
    assert float(b["grad_beta"].abs().max()) > 0 and float(b["grad_llr"].abs().max()) > 0
    close(a["loss_per_iter"].cpu().numpy(), b["loss_per_iter"].cpu().numpy(), "J_0")
    close(a["posterior"].cpu().numpy(), b["posterior"].cpu().numpy(), "posterior")
    assert torch.equal(a["bits"], b["bits"])
    close(a["grad_beta"].cpu().numpy(), b["grad_beta"].cpu().numpy(), "d J/d beta")
    close(a["grad_llr"].cpu().numpy(), b["grad_llr"].cpu().numpy(), "d J/d llr")
    assert float(a["grad_alpha"].abs().max()) == 0.0 and float(b["grad_alpha"].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- 4. robustness
def test_determinism_empty_batch_loss_only_live_weights_and_workspace(gpu_device):
    from neural_2d_decoder import Neural2DMinSumDecoder
    case = 2                                        # small_96_48, 67 codewords: two tiles, the second mostly padding
    _, llr, y, w = cases.inputs(case)
    dec = cases.decoder_of(case, **HOW)
    a = run(dec, llr, y, w, gpu_device)
    b = run(dec, llr, y, w, gpu_device)
    assert all(torch.equal(a[i], b[i]) for i in (0, 1, 2, 3, 5))
    assert all(torch.equal(a[4][k], b[4][k]) for k in a[4])
    assert any(float(v.abs().max()) > 0 for v in a[4].values()) and float(a[5].abs().max()) > 0
    # want_grads False: the loss alone, same numbers, same decode, no gradient
    eng = dec._get_engine(gpu_device)
    x = torch.from_numpy(np.array(llr)).to(gpu_device)
    full = eng.train_joint_layered_ste(x, want_grads=True, want_grad_llr=True)
    only = eng.train_joint_layered_ste(x, want_grads=False)
    assert only["grad_beta"] is None and only["grad_alpha"] is None and only["grad_llr"] is None
    assert torch.equal(only["loss_per_iter"], full["loss_per_iter"]) and torch.equal(only["posterior"], full["posterior"])
    assert torch.equal(only["bits"], full["bits"])
    # an empty batch: zero losses and gradients
    dec.zero_grad()
    loss, per_iter, bits, post = dec.joint_posterior_loss(torch.zeros(0, llr.shape[1], device=gpu_device))
    assert bits.shape == (0, llr.shape[1]) and post.shape == (0, llr.shape[1]) and per_iter.shape == (cases.T_GRAD,)
    assert loss.item() == 0.0 and float(per_iter.abs().sum()) == 0.0
    loss.backward()
    assert all(float(v.abs().max()) == 0.0 for v in cases.grads_of(dec).values())
    empty = eng.train_joint_layered_ste(torch.zeros(0, llr.shape[1], device=gpu_device))
    assert float(empty["grad_beta"].abs().max()) == 0.0 and float(empty["grad_alpha"].abs().max()) == 0.0
    # a weight update on the live engine reaches the next call: equal to a decoder built with those weights
    with torch.no_grad():
        for p in dec.beta_weights.values():
            p.mul_(0.5)
    moved = run(dec, llr, y, w, gpu_device)
    assert dec._get_engine(gpu_device) is eng
    fresh = cases.decoder_of(case, **HOW)
    with torch.no_grad():
        for p in fresh.beta_weights.values():
            p.mul_(0.5)
    again = run(fresh, llr, y, w, gpu_device)
    assert not torch.equal(moved[1], a[1])
    assert all(torch.equal(moved[i], again[i]) for i in (0, 1, 2, 3, 5)) and all(torch.equal(moved[4][k], again[4][k]) for k in moved[4])
    # the scratch does not depend on T, and its message rows are bytes: smaller than the layered min-sum scratch
    code4, code50 = cases.load("small", 4), cases.load("small", 50)
    e4 = cases.make_decoder(code4, 2, 3, cases.QP3, 4, seed=1)._get_engine(gpu_device)
    e50 = cases.make_decoder(code50, 2, 3, cases.QP3, 50, seed=1)._get_engine(gpu_device)
    for B in (1, 67, 300):
        assert e4.train_joint_layered_ste_workspace_bytes(B) == e50.train_joint_layered_ste_workspace_bytes(B) > 0
    n2d = Neural2DMinSumDecoder(code4, 2, 4, schedule="layered")._get_engine(gpu_device)
    assert e4.train_joint_layered_ste_workspace_bytes(300) < n2d.train_joint_layered_workspace_bytes(300)
    g = code4.tanner_graph()
    per_codeword = (2 * g.E + 4 * g.n) * 4 + g.E
    assert 320 * per_codeword <= e4.train_joint_layered_ste_workspace_bytes(300) <= 320 * per_codeword + 64 * 1024


# ---------------------------------------------------------------------------------------------------- 5. refusals, op, trainer
def test_entry_points_refuse_each_others_decoders(gpu_device):
    import _native as nat
    import layered_minsum_cases as lms
    from ldpc_decoder import BasicMinSumDecoder, create_test_ldpc_code
    from rcq_decoder import RCQMinSumDecoder, WeightedRCQDecoder
    code = create_test_ldpc_code()
    x = torch.randn(5, code.n, device=gpu_device)
    qp = [(3.0, 1.3)]
    lib = nat.load()

    def c_call(eng):
        """the C entry point itself -> (return code, message)"""
        args = [None] * 14
        args[0], args[3], args[12] = eng.handle, 5, 0
        rc = lib.ldpc_train_joint_layered_ste(*args)
        return rc, lib.ldpc_last_error().decode()

    # the new entry point names the one each other decoder takes ...
    flooding_rcq = WeightedRCQDecoder(code, 3, 8, qp, 2, 4)._get_engine(gpu_device)
    with pytest.raises(NotImplementedError, match="ldpc_train_joint_ste"):
        flooding_rcq.train_joint_layered_ste(x)
    rc, msg = c_call(flooding_rcq)
    assert rc == -3 and "ldpc_train_joint_ste" in msg
    layered_ms = lms.make("n2d2", code, 3, 1)._get_engine(gpu_device)
    with pytest.raises(NotImplementedError, match=r"ldpc_train_joint_layered\b(?!_)"):
        layered_ms.train_joint_layered_ste(x)
    rc, msg = c_call(layered_ms)
    assert rc == -3 and "ldpc_train_joint_layered," in msg
    flooding_ms = lms.make("n2d2", code, 3, 1, schedule="flooding")._get_engine(gpu_device)
    with pytest.raises(NotImplementedError, match=r"ldpc_train_joint\b(?!_)"):
        flooding_ms.train_joint_layered_ste(x)
    # ... and has nothing for the reference's layered schedule and float64
    ref_layered = RCQMinSumDecoder(code, 3, 8, qp, 4, layered=True)._get_engine(gpu_device)
    with pytest.raises(NotImplementedError, match="LDPC_SCHED_LAYERED_REF"):
        ref_layered.train_joint_layered_ste(x)
    assert c_call(ref_layered)[0] == -3
    f64 = BasicMinSumDecoder(lms.with_iterations(code, 3), 0.7)._engine(torch.float64, gpu_device)
    with pytest.raises(NotImplementedError, match="fp32"):
        f64.train_joint_layered_ste(x.double())
    # the three older entry points keep refusing a layered="paper" decoder
    paper = WeightedRCQDecoder(code, 3, 8, qp, 2, 4, layered="paper", **HOW)
    eng = paper._get_engine(gpu_device)
    for call in (eng.train_joint, eng.train_joint_ste, eng.train_joint_layered, eng.decode_saving):
        with pytest.raises(NotImplementedError):
            call(x)
    assert c_call(eng)[0] == -1                     # accepted: the next check is the missing loss_per_iter
    # forward under autograd is unchanged: no grad_fn on the layered decoder
    post = paper(x)[1]
    assert not post.requires_grad


def test_opcheck(gpu_device):
    import torch_ops
    T = cases.T_GRAD
    dec = cases.decoder_of(0, **HOW)
    eng = dec._get_engine(gpu_device)
    bt, at = dec._sharing_layout().tables_torch(dec.beta_weights, dec.alpha_weights, T, dec._beta_default, dec._alpha_default)
    h = torch_ops.engine_handle(eng)
    xs = torch.from_numpy(np.array(cases.inputs(0)[1][:5])).to(gpu_device)
    w = torch.full((T,), 0.25, device=gpu_device)
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    torch.library.opcheck(torch.ops.ldpc.rcq_layered_joint_loss,
                          (xs, None, bt.detach().clone().requires_grad_(True), at.detach().clone().requires_grad_(True), w, h,
                           True, False), test_utils=utils)
    torch.library.opcheck(torch.ops.ldpc.rcq_layered_joint_loss,
                          (xs, torch.rand_like(xs), bt.detach().clone(), at.detach().clone(), w, h, False, False),
                          test_utils=utils)


def test_trainer_with_the_joint_loss_trains_the_layered_quantised_decoder(gpu_device):
    """the run tests/test_layered_joint_training_rcq_host.py rehearses on the CPU; PosteriorJointTrainer is unchanged"""
    from training_framework import PosteriorJointTrainer
    t = cases.TRAIN
    torch.manual_seed(t["torch_seed"])
    code, model = cases.trainer_model()
    trainer = PosteriorJointTrainer(model, cases.trainer_config("cuda"))
    hist = trainer.train(code, num_train_samples=t["num_train"], num_val_samples=t["num_val"])
    til = hist["train_iteration_losses"]
    assert len(til) == len(hist["train_losses"]) >= 2 and all(len(v) == t["T"] for v in til)
    assert np.all(np.isfinite(til)) and np.mean(til[-1]) < np.mean(til[0]), til
    assert hist["train_losses"][-1] < hist["train_losses"][0], hist["train_losses"]
    assert all(np.isfinite(hist["gradient_norms"])) and hist["gradient_norms"][0] > 0
    betas = torch.cat([p.detach().reshape(-1) for p in model.beta_weights.values()])
    assert float((betas - 1.0).abs().max()) > 0.05
    alphas = torch.cat([p.detach().reshape(-1) for p in model.alpha_weights.values()])
    assert float((alphas - 1.0).abs().max()) == 0.0
