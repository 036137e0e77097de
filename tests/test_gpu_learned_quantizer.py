"""
GPU tests (-m gpu) of the learned RCQ quantisers: the level gradient of ldpc_train_joint_ste_levels /
ldpc_train_joint_layered_ste_levels (kernel level_grad), ``DecodeEngine.train_joint_ste(want_levels=True)``, the operators
``torch.ops.ldpc.rcq_joint_loss_levels`` / ``rcq_layered_joint_loss_levels`` and ``WeightedRCQDecoder(learn_quantizer=True)``
through the trainer.

What is pinned: grad_levels, ``quantizer_C.grad`` and ``quantizer_gamma.grad`` equal both CPU restatements of
tests/pjt_rcq_levels_reference.py (autograd with the reconstruction values as a leaf, and the closed-form sum) on every input
set of tests/pjt_rcq_cases.py and tests/layered_pjt_rcq_cases.py, with the tolerances of tests/test_gpu_joint_training_rcq.py;
every other output is bit-identical to the entry point without the level gradient; padding codewords and dirty scratch
change nothing; at T = 1 the gradient equals a numpy formula on the LLRs and the traced codes; two runs are bit-equal; the
trainer moves (C, gamma) inside one native decoder and lowers the loss.
"""
import dataclasses

import numpy as np
import pytest
import torch

import layered_pjt_rcq_cases as lcases
import pjt_rcq_cases as cases
import pjt_rcq_levels_reference as lv
from test_gpu_joint_training_rcq import STE, close

pytestmark = pytest.mark.gpu

SAME = ("loss_per_iter", "bits", "posterior", "grad_beta", "grad_alpha", "grad_llr")


def check_case(gpu_device, dec, llr, y, w, r, special, layered):
    """one input set: the decoder's (C, gamma) gradients and the engine's raw grad_levels against both restatements in `r`,
    every other output against the entry point without the level gradient"""
    x = torch.from_numpy(np.array(llr)).to(gpu_device)
    yd = None if y is None else y.to(gpu_device)
    loss, _, bits, post = dec.joint_posterior_loss(x, yd, w)
    loss.backward()
    eng = dec._get_engine(gpu_device)
    call = eng.train_joint_layered_ste if layered else eng.train_joint_ste
    wd = None if w is None else w.to(gpu_device)
    out = call(x, yd, wd, want_grads=True, want_grad_llr=True, want_levels=True)
    base = call(x, yd, wd, want_grads=True, want_grad_llr=True)
    assert "grad_levels" not in base
    for k in SAME:
        assert torch.equal(out[k], base[k]), k
    assert torch.equal(bits, base["bits"]) and torch.equal(post, base["posterior"])
    got = out["grad_levels"].cpu().numpy()
    T, L = got.shape
    assert got.dtype == np.float32 and (T, L) == r["levels_closed"].shape
    C = dec.quantizer_C.detach().cpu().numpy()
    gamma = dec.quantizer_gamma.detach().cpu().numpy()
    for name in ("levels_closed", "levels_autograd"):
        want = r[name]
        print(name, "max |want|", np.abs(want).max(), "max |got - want| / max", np.abs(got - want).max() / np.abs(want).max())
        assert np.any(np.abs(want) > 0)
        close(got, want, f"grad_levels vs {name}")
        wC, wg = lv.param_grads(C, gamma, lv.per_quantizer(want, r["q_of_iter"], len(C)))
        close(dec.quantizer_C.grad.cpu().numpy(), wC, f"quantizer_C.grad vs {name}")
        close(dec.quantizer_gamma.grad.cpu().numpy(), wg, f"quantizer_gamma.grad vs {name}")
        if special == "saturate":                   # what beta cannot see: the top level carries the largest entry
            assert np.all(np.abs(want).argmax(axis=1) == L - 1) and np.all(np.abs(got).argmax(axis=1) == L - 1)
    return out


# ---------------------------------------------------------------------------------------------------- 1. restatements
@pytest.mark.parametrize("case", range(len(cases.CASES)))
def test_level_gradients_match_the_restatements(gpu_device, oracle_mod, case):
    _, llr, y, w = cases.inputs(case)
    dec = lv.learnable(cases.decoder_of(case))
    r = lv.flooding_expected(case)
    assert r["disagree"] <= 1e-3
    out = check_case(gpu_device, dec, llr, y, w, r, cases.CASES[case][6], layered=False)
    # the teacher: the codes the restatements were given are the codes the kernels wrote
    np.testing.assert_array_equal(out["posterior"].cpu().numpy(), r["trace_posterior"])
    np.testing.assert_array_equal(out["bits"].cpu().numpy(), r["trace_bits"])


@pytest.mark.parametrize("case", range(len(lcases.CASES)))
def test_level_gradients_match_the_restatements_layered(gpu_device, case):
    _, llr, y, w = lcases.inputs(case)
    dec = lv.learnable(lcases.decoder_of(case))
    r = lv.layered_expected(case)
    out = check_case(gpu_device, dec, llr, y, w, r, lcases.CASES[case][6], layered=True)
    np.testing.assert_array_equal(out["posterior"].cpu().numpy(), r["P"][-1])


# ---------------------------------------------------------------------------------------------------- 2. padding, dirty scratch
@pytest.mark.parametrize("layered", [False, "paper"], ids=["flooding", "layered"])
@pytest.mark.parametrize("bc", [3, 8])
@pytest.mark.parametrize("B", [1, 3, 37, 67])
def test_padding_and_dirty_scratch(gpu_device, B, bc, layered):
    T = 4
    code = cases.load("small", T)
    how = dict(lcases.HOW) if layered else dict(STE)
    dec = cases.make_decoder(code, 2, bc, cases.QP3, T, seed=3, layered=layered, **how)
    eng = dec._get_engine(gpu_device)
    call = eng.train_joint_layered_ste if layered else eng.train_joint_ste
    rng = np.random.default_rng(40 + B)
    x = torch.from_numpy(cases.channel(rng, B, code.n, (0.5, 4.0))).to(gpu_device)
    w = torch.tensor(rng.uniform(0.1, 1.0, T), dtype=torch.float32, device=gpu_device)
    runs = [call(x, None, w, want_levels=True)["grad_levels"].clone()]
    ws = eng._joint_ws
    ws.fill_(0xFF)                                                  # every byte a code past 2L - 1, every float a NaN
    runs.append(call(x, None, w, want_levels=True)["grad_levels"].clone())
    ws.view(torch.float32).fill_(float("nan"))
    ws.view(torch.int32)[1::2] = 0x7F800001                         # signalling-NaN pattern on every other word
    runs.append(call(x, None, w, want_levels=True)["grad_levels"].clone())
    assert eng._joint_ws is ws
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    got = runs[0].double().cpu()
    assert torch.isfinite(got).all() and float(got.abs().max()) > 0
    # every (b, e) adds |g_t[b, var(e)]| to one level, once: sum_l |grad_levels[t][l]| <= sum |g_t| * max dv -- a padded
    # codeword leaking in would add to the left side only
    max_dv = int(np.max(code.tanner_graph().dv))
    for t in range(T):
        l = eng.decode(x, early_stop=False, max_iters=t + 1).posterior.double()
        g = w[t].double() * (0.0 - torch.sigmoid(-l)) / (B * code.n)
        bound = float(g.abs().sum()) * max_dv
        assert float(got[t].abs().sum()) <= bound * (1 + 1e-5), (t, float(got[t].abs().sum()), bound)


# ---------------------------------------------------------------------------------------------------- 3. T = 1 anchor
@pytest.mark.parametrize("B,bc", [(50, 3), (200, 3), (50, 8), (200, 8)])
def test_one_iteration_closed_form(gpu_device, oracle_mod, B, bc):
    """grad_levels[0][l] = sum over b and e of [code mod L == l] * s(code) * g[b, v(e)], g = -sigmoid(-l_0) / (B n),
    l_0 = llr + the reconstructed codes at the variable -- numpy, fp64, from the LLRs and the traced codes alone"""
    import pjt_rcq_reference as ref
    code = cases.load("small", 1)
    dec = cases.make_decoder(code, 2, bc, [(3.0, 1.3)], 1, seed=11, **STE)
    llr = cases.channel(np.random.default_rng(12), B, code.n, (2.0, 5.0))
    x = torch.from_numpy(llr).to(gpu_device)
    got = dec._get_engine(gpu_device).train_joint_ste(x, want_levels=True)["grad_levels"].cpu().numpy()
    lay = dec._sharing_layout()
    beta, alpha = dec.weight_tables()
    thr, qoi = cases.quantiser_tables(dec)
    g = cases.oracle_graph(code)
    _, _, codes = ref.trace(g, llr, beta, lay.beta_slot, alpha, lay.alpha_slot, thr, qoi, 1)
    codes = codes[:, 0, :].astype(np.int64)
    L = thr.shape[1]
    tau = thr[0].astype(np.float64)
    sgn = np.where(codes >= L, -1.0, 1.0)
    l0 = llr.astype(np.float64)
    np.add.at(l0, (slice(None), g.var_idx), sgn * tau[codes % L])
    gl = -1.0 / (1.0 + np.exp(l0)) / (B * g.n)
    want = np.zeros(L)
    for e in range(g.E):
        np.add.at(want, codes[:, e] % L, sgn[:, e] * gl[:, g.var_idx[e]])
    assert got.shape == (1, L) and np.abs(want).max() > 0
    np.testing.assert_allclose(got[0], want, rtol=1e-5, atol=1e-7 * np.abs(want).max())


# ---------------------------------------------------------------------------------------------------- 4. plumbing
def test_determinism_empty_batch_null_output_and_opcheck(gpu_device):
    import torch_ops
    T = 5
    code = cases.load("ira", T)
    plain = cases.make_decoder(code, 1, 3, cases.QP3, T, seed=7, **STE)
    dec = lv.learnable(plain)
    eng = dec._get_engine(gpu_device)
    x = torch.from_numpy(cases.channel(np.random.default_rng(8), 300, code.n, (1.5, 5.0))).to(gpu_device)
    a = eng.train_joint_ste(x, want_levels=True)
    b = eng.train_joint_ste(x, want_levels=True)
    assert torch.equal(a["grad_levels"], b["grad_levels"]) and float(a["grad_levels"].abs().max()) > 0
    # the level gradient alone (no table gradient asked for): the same rows
    c = eng.train_joint_ste(x, want_grads=False, want_levels=True)
    assert c["grad_beta"] is None and torch.equal(c["grad_levels"], a["grad_levels"])
    assert torch.equal(c["loss_per_iter"], a["loss_per_iter"]) and torch.equal(c["posterior"], a["posterior"])
    # the existing entry point and its scratch are what they were; the new one needs more
    assert eng.train_joint_ste_workspace_bytes(300) < int(eng._lib.ldpc_train_joint_ste_levels_workspace_bytes(eng.handle, 300))
    e = eng.train_joint_ste(torch.zeros(0, code.n, device=gpu_device), want_levels=True)
    assert e["grad_levels"].shape == (T, 4) and float(e["grad_levels"].abs().max()) == 0.0

    # through the decoder: both quantiser parameters get a gradient, twice the same
    runs = []
    for _ in range(2):
        dec.zero_grad()
        dec.joint_posterior_loss(x)[0].backward()
        runs.append((dec.quantizer_C.grad.clone(), dec.quantizer_gamma.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][0].dtype == torch.float64 and float(runs[0][0].abs().min()) > 0 and float(runs[0][1].abs().min()) > 0
    with torch.no_grad():                           # no autograd: the plain loss, the same numbers
        l0 = dec.joint_posterior_loss(x)[0]
        l1 = plain.joint_posterior_loss(x)[0]
    assert torch.equal(l0.cpu(), l1.cpu())

    lay = dec._sharing_layout()
    bt, at = lay.tables_torch(dec.beta_weights, dec.alpha_weights, T, dec._beta_default, dec._alpha_default)
    h = torch_ops.engine_handle(eng)
    xs = x[:5].contiguous()
    w = torch.full((T,), 0.2, device=gpu_device)
    thr = dec.thresholds_tensor().detach().clone()
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    for op in (torch.ops.ldpc.rcq_joint_loss_levels,):
        torch.library.opcheck(op, (xs, None, bt.detach().clone().requires_grad_(True), at.detach().clone().requires_grad_(True),
                                   thr.clone().requires_grad_(True), w, h, True, False), test_utils=utils)
        torch.library.opcheck(op, (xs, torch.rand_like(xs), bt.detach().clone(), at.detach().clone(), thr.clone(), w, h,
                                   False, False), test_utils=utils)
    # the operator decodes with the table it is given and puts the engine's own back
    held = eng.current_thresholds()
    other = (thr * 1.5).requires_grad_(True)
    out = torch.ops.ldpc.rcq_joint_loss_levels(xs, None, bt.detach(), at.detach(), other, w, h, False, False)
    assert np.array_equal(eng.current_thresholds(), held)
    out[0].backward()
    assert other.grad.shape == thr.shape and other.grad.dtype == torch.float64 and float(other.grad.abs().max()) > 0
    glv = out[7].double().cpu()
    want = torch.zeros_like(thr).index_add(0, torch.as_tensor(np.asarray(eng.q_of_iter[:T], dtype=np.int64)), glv)
    assert torch.equal(other.grad, want)

    paper = lv.learnable(cases.make_decoder(code, 1, 3, cases.QP3, T, seed=7, layered="paper", **lcases.HOW))
    peng = paper._get_engine(gpu_device)
    pbt, pat = paper._sharing_layout().tables_torch(paper.beta_weights, paper.alpha_weights, T, paper._beta_default,
                                                    paper._alpha_default)
    torch.library.opcheck(torch.ops.ldpc.rcq_layered_joint_loss_levels,
                          (xs, None, pbt.detach().clone().requires_grad_(True), pat.detach().clone().requires_grad_(True),
                           thr.clone().requires_grad_(True), w, torch_ops.engine_handle(peng), True, False), test_utils=utils)
    # the level entry points are for the quantised decoders only, each for its schedule
    from neural_2d_decoder import Neural2DMinSumDecoder
    with pytest.raises(NotImplementedError):
        Neural2DMinSumDecoder(code, 2, T)._get_engine(gpu_device).train_joint_ste(xs, want_levels=True)
    with pytest.raises(NotImplementedError):
        peng.train_joint_ste(xs, want_levels=True)
    with pytest.raises(NotImplementedError):
        eng.train_joint_layered_ste(xs, want_levels=True)


# ---------------------------------------------------------------------------------------------------- 5. trainer
def learnable_trainer_model(layered):
    import codes
    from rcq_decoder import WeightedRCQDecoder
    t = cases.TRAIN
    code = codes.load_code(t["code"], max_iterations=t["T"])
    how = dict(lcases.HOW) if layered else dict(STE)
    model = WeightedRCQDecoder(code, t["bc"], 8, t["qp"], t["wtype"], t["T"], layered=layered, learn_quantizer=True, **how)
    with torch.no_grad():                           # the plain RCQ decoder, as pjt_rcq_cases.trainer_model starts
        for p in list(model.beta_weights.values()) + list(model.alpha_weights.values()):
            p.fill_(1.0)
    return code, model


@pytest.mark.parametrize("layered", [False, "paper"], ids=["flooding", "layered"])
def test_trainer_learns_the_quantizer_inside_one_native_decoder(gpu_device, layered):
    from rcq_decoder import WeightedRCQDecoder
    from training_framework import PosteriorJointTrainer
    t = cases.TRAIN
    torch.manual_seed(t["torch_seed"])
    code, model = learnable_trainer_model(layered)
    trainer = PosteriorJointTrainer(model, cases.trainer_config("cuda"))
    eng = model._get_engine(gpu_device)
    handle = eng.handle.value
    C0, g0 = model.quantizer_C.detach().clone(), model.quantizer_gamma.detach().clone()
    hist = trainer.train(code, num_train_samples=t["num_train"], num_val_samples=t["num_val"])
    print("losses", hist["train_losses"], "quantizer", hist["quantizer_params"][-1])
    assert model._get_engine(gpu_device) is eng and eng.handle.value == handle
    assert float((model.quantizer_C.detach() - C0).abs().min()) > 0 and float((model.quantizer_gamma.detach() - g0).abs().min()) > 0
    assert len(hist["train_losses"]) >= 2 and all(np.isfinite(hist["train_losses"]))
    assert all(np.isfinite(v) for row in hist["train_iteration_losses"] for v in row)
    assert hist["train_losses"][-1] < hist["train_losses"][0], hist["train_losses"]
    assert len(hist["quantizer_params"]) == len(hist["train_losses"])
    assert hist["quantizer_params"][-1] == [(float(c), float(g)) for c, g in zip(model.quantizer_C.tolist(),
                                                                                model.quantizer_gamma.tolist())]
    # a plain decoder built from the learned pairs is the trained decoder
    plain = WeightedRCQDecoder(code, t["bc"], 8, hist["quantizer_params"][-1], t["wtype"], t["T"], layered=layered)
    plain.load_state_dict({k: v for k, v in model.state_dict().items() if not k.startswith("quantizer_")})
    x = torch.from_numpy(cases.channel(np.random.default_rng(77), 70, code.n, (1.0, 4.0))).to(gpu_device)
    with torch.no_grad():
        for es in (True, False):
            a, b = model(x, early_stop=es), plain(x, early_stop=es)
            assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert model._get_engine(gpu_device) is eng and eng.handle.value == handle

    # stream training: the same way, two epochs
    trainer2 = PosteriorJointTrainer(model, dataclasses.replace(cases.trainer_config("cuda"), num_epochs=2))
    C1 = model.quantizer_C.detach().clone()
    hist2 = trainer2.train_stream(code, steps_per_epoch=4, val_frames=64)
    assert len(hist2["train_losses"]) == 2 and all(np.isfinite(hist2["train_losses"])) and all(np.isfinite(hist2["val_losses"]))
    assert len(hist2["quantizer_params"]) == 2 and float((model.quantizer_C.detach() - C1).abs().max()) > 0
    assert model._get_engine(gpu_device) is eng and eng.handle.value == handle
