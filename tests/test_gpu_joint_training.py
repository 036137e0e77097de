"""
GPU tests (-m gpu) of posterior joint training (PJT): ``joint_posterior_loss`` on the four trainable decoders, the
registered operator ``torch.ops.ldpc.minsum_joint_loss`` and the C function ldpc_train_joint behind them.

What is pinned: the forward is the decoder's own fixed-T decode bit for bit; the gradients equal torch autograd on the
CPU restatement tests/pjt_reference.py (tolerances of tests/test_gpu_training.py: rtol 2e-3 on random cases); at T = 1
and with the weight on the last iteration only they equal the existing full-backpropagation path, which is itself pinned
to the reference; on the (16200,7200) code at T = 50 the scratch does not grow with T and no saved-state cap applies.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def load(name, T):
    import codes
    from ldpc_decoder import create_test_ldpc_code
    if name == "toy":
        return create_test_ldpc_code()
    return codes.load_code({"small": "small_96_48", "ira": "ira_1998_1512", "dvbs2": "dvbs2_like_16200_7200"}[name],
                           max_iterations=T)


def make_decoder(kind, code, T, wtype=2, seed=0):
    from neural_2d_decoder import Neural2DMinSumDecoder, Neural2DOffsetMinSumDecoder
    from neural_minsum_decoder import NeuralMinSumDecoder, NeuralOffsetMinSumDecoder
    torch.manual_seed(seed)
    dec = {"n2d": lambda: Neural2DMinSumDecoder(code, wtype, T), "oms2d": lambda: Neural2DOffsetMinSumDecoder(code, wtype, T),
           "edge_nms": lambda: NeuralMinSumDecoder(code, T), "edge_oms": lambda: NeuralOffsetMinSumDecoder(code, T)}[kind]()
    rng = np.random.default_rng(seed + 100)
    with torch.no_grad():                           # weights away from the init so that every form is exercised
        for name, p in dec.named_parameters():
            if kind in ("n2d", "edge_nms"):
                p.fill_(float(rng.uniform(0.55, 1.0)) if "beta" in name else float(rng.uniform(0.8, 1.2)))
            else:
                p.fill_(float(rng.uniform(0.0, 0.4)))
    return dec


def tables_of(dec):
    """differentiable (beta table, alpha table, beta slot, alpha slot, offset) on the CPU, built from the parameters
    the way the decoder builds them"""
    import autograd_bridge as ab
    from neural_2d_decoder import _DegreeSharedDecoder
    T = int(dec.max_iterations)
    g = dec.code.tanner_graph()
    if isinstance(dec, _DegreeSharedDecoder):
        lay = dec._sharing_layout()
        bt, at = lay.tables_torch(dec.beta_weights, dec.alpha_weights, T, dec._beta_default, dec._alpha_default)
        return bt, at, lay.beta_slot, (lay.alpha_edge_slot if dec._alpha_is_oms else lay.alpha_slot), dec._alpha_is_oms
    rows, cols = g.check_of_edge.tolist(), g.var_idx.tolist()
    params = [dec.beta_weights[f"iter_{t}_c{i}_v{j}"] for t in range(T) for i, j in zip(rows, cols)]
    bt = ab.table_from_params(params, [(t, e) for t in range(T) for e in range(g.E)], (T, g.E), 0.0)
    oms = dec._c2v_form == "oms"
    if oms:
        return bt, torch.zeros((T, 1)), np.arange(g.E), np.zeros(g.E, np.int64), True
    return bt, torch.ones((T, 1)), np.arange(g.E), np.zeros(g.n, np.int64), False


def oracle_graph(code):
    import oracle
    tg = code.tanner_graph()
    return oracle.OracleGraph(n=tg.n, check_ptr=tg.check_ptr, var_idx=tg.var_idx)


def channel(rng, B, n, snr=(1.5, 5.0)):
    s = np.linspace(snr[0], snr[1], B)
    s2 = 10.0 ** (-s / 10.0)
    return (2.0 * (1.0 + np.sqrt(s2)[:, None] * rng.standard_normal((B, n))) / s2[:, None]).astype(np.float32)


def grads_of(dec):
    return {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()).cpu() for k, p in dec.named_parameters()}


def close(got, want, what, rtol=2e-3, rel_atol=2e-4):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(float(np.abs(want).max()), 1e-30)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=rel_atol * scale, err_msg=what)


# ---------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("name,kind,B", [("small", "n2d", 300), ("ira", "n2d", 37), ("ira", "oms2d", 130),
                                         ("small", "edge_oms", 64)])
def test_forward_is_the_fixed_iteration_decode(gpu_device, name, kind, B):
    T = 6
    code = load(name, T)
    dec = make_decoder(kind, code, T)
    x = torch.from_numpy(channel(np.random.default_rng(1), B, code.n)).to(gpu_device)
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


# ---------------------------------------------------------------------------------------------------- 2. restatement
CASES = [("toy", "n2d", 1, 37), ("toy", "n2d", 4, 37), ("small", "n2d", 2, 300), ("small", "n2d", 3, 64),
         ("ira", "n2d", 1, 40), ("ira", "n2d", 2, 70), ("ira", "n2d", 3, 40), ("ira", "n2d", 4, 40),
         ("toy", "oms2d", 2, 20), ("ira", "oms2d", 1, 40), ("small", "edge_nms", None, 90), ("small", "edge_oms", None, 33)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_gradients_match_the_restatement(gpu_device, case, oracle_mod):
    import pjt_reference
    name, kind, wtype, B = CASES[case]
    T = 4
    code = load(name, T)
    dec = make_decoder(kind, code, T, wtype or 2, seed=case)
    rng = np.random.default_rng(50 + case)
    llr = channel(rng, B, code.n, snr=(0.5, 4.0))
    custom = case % 2 == 1                      # every other case: custom iteration weights and soft targets
    w = torch.tensor(rng.uniform(0.1, 1.0, T), dtype=torch.float32) if custom else None
    y = torch.from_numpy(rng.uniform(0, 1, (B, code.n)).astype(np.float32) * (rng.random((B, code.n)) < 0.3)) if custom else None

    x = torch.from_numpy(llr).to(gpu_device).requires_grad_(True)
    loss, per_iter, _, post = dec.joint_posterior_loss(x, None if y is None else y.to(gpu_device), w)
    loss.backward()
    got, got_x = grads_of(dec), x.grad.cpu().numpy()
    dec.zero_grad()

    bt, at, bslot, aslot, offset = tables_of(dec)
    xc = torch.from_numpy(llr).requires_grad_(True)
    J, per_c, post_c = pjt_reference.forward(oracle_graph(code), xc, bt, bslot, at, aslot, T, y, w, offset)
    J.backward()
    want = grads_of(dec)
    np.testing.assert_allclose(per_iter.detach().cpu().numpy(), [v.item() for v in per_c], rtol=1e-4)
    np.testing.assert_allclose(post.detach().cpu().numpy(), post_c.detach().numpy(), rtol=1e-4, atol=1e-3)
    assert any(float(v.abs().max()) > 0 for v in want.values())
    for k in want:
        close(got[k], want[k], f"{name} {kind} {wtype} {k}")
    # d J/d llr: element-wise; a min / min2 near-tie may send one check's gradient to another edge -- rows where that
    # happened (rare on the larger codes) are left out, as in test_gpu_training
    gx = xc.grad.numpy()
    scale = np.abs(gx).max()
    ok = np.all(np.abs(got_x - gx) <= 2e-3 * np.abs(gx) + 2e-4 * scale, axis=1)
    assert ok.mean() >= (1.0 if name != "ira" else 0.9), ok.mean()


# ---------------------------------------------------------------------------------------------------- 3. anchors
def _bptt_table_grads(eng, bt, at, x, oms):
    """the existing full-backpropagation path at table level: BCE of the final posterior, fixed T"""
    import autograd_bridge as ab
    bt = bt.detach().clone().requires_grad_(True)
    at = at.detach().clone().requires_grad_(True)
    post, _, _ = ab.decode_train(bt, at, eng, x, False, oms)
    F.binary_cross_entropy_with_logits(-post, torch.zeros_like(post)).backward()
    return bt.grad.clone(), at.grad.clone()


def _pjt_table_grads(eng, bt, at, x, oms, w):
    import torch_ops
    bt = bt.detach().clone().requires_grad_(True)
    at = at.detach().clone().requires_grad_(True)
    loss, *_ = torch.ops.ldpc.minsum_joint_loss(x, None, bt, at, w.to(x.device), torch_ops.engine_handle(eng), oms, True, False)
    loss.backward()
    return bt.grad.clone(), at.grad.clone()


@pytest.mark.parametrize("kind", ["n2d", "oms2d"])
def test_one_iteration_equals_the_existing_path(gpu_device, kind):
    code = load("ira", 1)
    dec = make_decoder(kind, code, 1, 2, seed=3)
    x = torch.from_numpy(channel(np.random.default_rng(2), 200, code.n)).to(gpu_device)
    eng = dec._get_engine(gpu_device)
    bt, at, _, _, oms = tables_of(dec)
    gb0, ga0 = _bptt_table_grads(eng, bt, at, x, oms)
    gb1, ga1 = _pjt_table_grads(eng, bt, at, x, oms, torch.ones(1))
    torch.testing.assert_close(gb1, gb0, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(ga1, ga0, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("kind", ["n2d", "oms2d"])
def test_weight_on_the_last_iteration_anchors_to_the_existing_path(gpu_device, kind):
    T = 5
    code = load("ira", T)
    dec = make_decoder(kind, code, T, 2, seed=4)
    x = torch.from_numpy(channel(np.random.default_rng(3), 150, code.n)).to(gpu_device)
    eng = dec._get_engine(gpu_device)
    bt, at, _, _, oms = tables_of(dec)
    gb0, ga0 = _bptt_table_grads(eng, bt, at, x, oms)
    w = torch.zeros(T)
    w[T - 1] = 1.0
    gb1, ga1 = _pjt_table_grads(eng, bt, at, x, oms, w)
    torch.testing.assert_close(gb1[T - 1], gb0[T - 1], rtol=1e-5, atol=1e-7)
    assert float(gb1[:T - 1].abs().max()) == 0.0
    if oms:                                         # check-side offset of the last iteration
        torch.testing.assert_close(ga1[T - 1], ga0[T - 1], rtol=1e-5, atol=1e-7)
        assert float(ga1[:T - 1].abs().max()) == 0.0
    else:                                           # alpha_T-2 shapes v2c_T-1; alpha_T-1 feeds nothing
        torch.testing.assert_close(ga1[T - 2], ga0[T - 2], rtol=1e-5, atol=1e-7)
        assert float(ga1[:T - 2].abs().max()) == 0.0 and float(ga1[T - 1].abs().max()) == 0.0
    assert float(gb1[T - 1].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 4. long code
def test_long_code_at_fifty_iterations(gpu_device, monkeypatch, oracle_mod):
    import autograd_bridge as ab
    import pjt_reference
    T, B = 50, 1024
    code = load("dvbs2", T)
    dec = make_decoder("n2d", code, T, 2, seed=5)
    eng = dec._get_engine(gpu_device)
    assert eng.train_saved_bytes(B) > 19e9                    # what full backpropagation would have to keep
    dec10 = make_decoder("n2d", load("dvbs2", 10), 10, 2, seed=5)
    assert dec10._get_engine(gpu_device).train_joint_workspace_bytes(B) == eng.train_joint_workspace_bytes(B)
    monkeypatch.setattr(ab, "MAX_SAVED_BYTES", 0)
    llr = channel(np.random.default_rng(6), B, code.n, snr=(0.5, 2.0))
    x = torch.from_numpy(llr).to(gpu_device)
    loss, per_iter, _, _ = dec.joint_posterior_loss(x)
    loss.backward()
    full = grads_of(dec)
    assert all(torch.isfinite(v).all() for v in full.values()) and any(float(v.abs().max()) > 0 for v in full.values())
    assert torch.isfinite(per_iter).all()
    halves = []
    for h in (x[:B // 2], x[B // 2:]):
        dec.zero_grad()
        dec.joint_posterior_loss(h.contiguous())[0].backward()
        halves.append(grads_of(dec))
    for k in full:
        close(full[k], (halves[0][k] + halves[1][k]) / 2, f"halves {k}")
    # a 4-codeword slice against the restatement
    dec.zero_grad()
    dec.joint_posterior_loss(x[:4].contiguous())[0].backward()
    got = grads_of(dec)
    dec.zero_grad()
    bt, at, bslot, aslot, offset = tables_of(dec)
    J, _, _ = pjt_reference.forward(oracle_graph(code), torch.from_numpy(llr[:4]), bt, bslot, at, aslot, T)
    J.backward()
    want = grads_of(dec)
    for k in want:
        close(got[k], want[k], f"slice {k}")


# ---------------------------------------------------------------------------------------------------- 5. plumbing
def test_determinism_empty_batch_and_opcheck(gpu_device):
    import torch_ops
    T = 5
    code = load("ira", T)
    dec = make_decoder("n2d", code, T, 1, seed=7)
    x = torch.from_numpy(channel(np.random.default_rng(8), 300, code.n)).to(gpu_device).requires_grad_(True)
    runs = []
    for _ in range(2):
        dec.zero_grad()
        x.grad = None
        loss, per_iter, _, _ = dec.joint_posterior_loss(x)
        loss.backward()
        runs.append((loss.detach().clone(), per_iter.clone(), grads_of(dec), x.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][3], runs[1][3])
    assert all(torch.equal(runs[0][2][k], runs[1][2][k]) for k in runs[0][2])

    dec.zero_grad()
    loss, per_iter, bits, post = dec.joint_posterior_loss(torch.zeros(0, code.n, device=gpu_device))
    assert bits.shape == (0, code.n) and post.shape == (0, code.n) and per_iter.shape == (T,)
    assert float(loss) == 0.0 and float(per_iter.abs().sum()) == 0.0
    loss.backward()
    assert all(float(v.abs().max()) == 0.0 for v in grads_of(dec).values())

    eng = dec._get_engine(gpu_device)
    bt, at, _, _, _ = tables_of(dec)
    h = torch_ops.engine_handle(eng)
    xs = x.detach()[:5].contiguous()
    w = torch.full((T,), 0.2, device=gpu_device)
    torch.library.opcheck(torch.ops.ldpc.minsum_joint_loss,
                          (xs, None, bt.detach().clone().requires_grad_(True), at.detach().clone().requires_grad_(True), w, h,
                           False, True, False),
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
    torch.library.opcheck(torch.ops.ldpc.minsum_joint_loss,
                          (xs, torch.rand_like(xs), bt.detach().clone(), at.detach().clone(), w, h, False, False, False),
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))


def test_forms_without_a_gradient_path_refuse(gpu_device):
    from ldpc_decoder import create_test_ldpc_code
    from rcq_decoder import RCQMinSumDecoder, WeightedRCQDecoder
    code = create_test_ldpc_code()
    x = torch.randn(5, code.n, device=gpu_device)
    with pytest.raises(NotImplementedError):
        WeightedRCQDecoder(code, 3, 8, [(3.0, 1.3)], 2, 4).joint_posterior_loss(x)
    rcq = RCQMinSumDecoder(code, 3, 8, [(3.0, 1.3)], 4)
    with pytest.raises(NotImplementedError):
        rcq._get_engine(gpu_device).train_joint(x)


# ---------------------------------------------------------------------------------------------------- 6. trainer
def test_trainer_with_the_joint_loss_reduces_the_loss(gpu_device):
    import codes
    from neural_2d_decoder import Neural2DMinSumDecoder
    from training_framework import PosteriorJointTrainer, TrainingConfig
    torch.manual_seed(5)
    code = codes.load_code("small_96_48", max_iterations=5)
    model = Neural2DMinSumDecoder(code, 2, 5)
    with torch.no_grad():                     # a deliberately poor start: all weights 0.3
        for p in model.parameters():
            p.fill_(0.3)
    cfg = TrainingConfig(batch_size=64, num_epochs=6, learning_rate=0.05, snr_range=(1.0, 4.0), device="cuda", seed=9,
                         joint_posterior_loss=True)
    trainer = PosteriorJointTrainer(model, cfg)
    hist = trainer.train(code, num_train_samples=512, num_val_samples=128)
    assert len(hist["train_losses"]) >= 2 and hist["train_losses"][-1] < hist["train_losses"][0]
    assert all(np.isfinite(hist["gradient_norms"])) and hist["gradient_norms"][0] > 0
    assert len(hist["train_iteration_losses"]) == len(hist["train_losses"])
    assert all(len(v) == 5 for v in hist["train_iteration_losses"])
    assert abs(np.mean(hist["train_iteration_losses"][0]) - hist["train_losses"][0]) <= 1e-4 * hist["train_losses"][0]
    vals = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    assert float((vals - 0.3).abs().max()) > 0.05
