"""
Host tests (no GPU) of the learned RCQ quantisers: the two restatements of the level gradient agree
(tests/pjt_rcq_levels_reference.py: torch autograd with the reconstruction values as a leaf against the closed-form numpy
sum, flooding and layered), the chain rule to (C, gamma), and the API facts of ``WeightedRCQDecoder(learn_quantizer=True)``
that need no device.
"""
import copy
import os
import re

import numpy as np
import pytest
import torch

import layered_pjt_rcq_cases as lcases
import pjt_rcq_cases as cases
import pjt_rcq_levels_reference as lv

QP3 = cases.QP3


# ---------------------------------------------------------------------------------------------------- 1. the two restatements
@pytest.mark.parametrize("case", [0, 2, 5, 7, 9, 13])
def test_autograd_equals_the_closed_form_flooding(oracle_mod, case):
    r = lv.flooding_expected(case)
    want, got = r["levels_closed"], r["levels_autograd"]
    top = np.abs(want).max()
    print(cases.CASES[case], "max |closed|", top, "max |autograd - closed| / max", np.abs(got - want).max() / top,
          "disagree", r["disagree"])
    assert r["disagree"] <= 1e-3
    assert top > 0
    assert np.abs(got - want).max() <= 1e-4 * top
    if cases.CASES[case][6] == "saturate":          # the part beta cannot see: almost all of it on the top level
        assert np.all(np.abs(want).argmax(axis=1) == want.shape[1] - 1)


@pytest.mark.parametrize("case", [0, 2, 5, 7, 9, 11])
def test_autograd_equals_the_closed_form_layered(case):
    r = lv.layered_expected(case)
    want, got = r["levels_closed"], r["levels_autograd"]
    top = np.abs(want).max()
    print(lcases.CASES[case], "max |closed|", top, "max |autograd - closed| / max", np.abs(got - want).max() / top)
    assert top > 0
    assert np.abs(got - want).max() <= 1e-4 * top


# ---------------------------------------------------------------------------------------------------- 2. chain rule
@pytest.mark.parametrize("bc,qp", [(3, QP3), (4, QP3), (8, QP3), (2, QP3), (3, [(2.0, 0.0), (3.0, 0.0), (4.0, 0.0)]),
                                   (5, [(4.0, 0.7)])])
def test_chain_rule_equals_autograd_through_the_power_law(bc, qp):
    from rcq_decoder import quantizer_param_grads
    L, Q = 2 ** (bc - 1), len(qp)
    table = np.random.default_rng(bc).standard_normal((Q, L))
    C, gamma = [c for c, _ in qp], [g for _, g in qp]
    gC, gg = quantizer_param_grads(C, gamma, table)
    wC, wg = lv.param_grads(C, gamma, table)
    assert gC.dtype == torch.float64 and gg.dtype == torch.float64
    assert np.all(np.isfinite(gC.numpy())) and np.all(np.isfinite(gg.numpy()))      # gamma = 0 included
    np.testing.assert_allclose(gC.numpy(), wC, rtol=1e-12, atol=0)
    np.testing.assert_allclose(gg.numpy(), wg, rtol=1e-12, atol=0)
    # j = 0 and j = L - 1 carry no gamma term: only those two columns non-zero -> d/d gamma is exactly 0
    ends = np.zeros((Q, L))
    ends[:, 0], ends[:, -1] = 3.0, -2.0
    eC, eg = quantizer_param_grads(C, gamma, ends)
    assert np.all(eg.numpy() == 0.0)
    x0 = np.array([1.0 if g == 0 else 0.0 for g in gamma])                          # 0^gamma
    np.testing.assert_allclose(eC.numpy(), 3.0 * x0 - 2.0, rtol=1e-15)


def test_the_decoder_routes_a_table_gradient_to_its_parameters():
    code = cases.load("small", 4)
    dec = cases.make_decoder(code, 2, 4, QP3, 4, seed=3, learn_quantizer=True)
    with torch.no_grad():
        dec.quantizer_C.copy_(torch.tensor([3.0, 5.0, 7.0], dtype=torch.float64))
        dec.quantizer_gamma.copy_(torch.tensor([1.3, 0.8, 2.0], dtype=torch.float64))
    table = np.random.default_rng(1).standard_normal((3, 8))
    thr = dec.thresholds_tensor()
    assert thr.dtype == torch.float64 and thr.shape == (3, 8)
    np.testing.assert_array_equal(thr.detach().numpy(), cases.quantiser_tables(dec)[0].astype(np.float64))
    (thr * torch.from_numpy(table)).sum().backward()
    wC, wg = lv.param_grads([3.0, 5.0, 7.0], [1.3, 0.8, 2.0], table)
    np.testing.assert_allclose(dec.quantizer_C.grad.numpy(), wC, rtol=1e-12)
    np.testing.assert_allclose(dec.quantizer_gamma.grad.numpy(), wg, rtol=1e-12)


# ---------------------------------------------------------------------------------------------------- 3. API facts
def test_header_and_exports_agree():
    import _native as nat
    with open(nat.HEADER) as f:
        declared = set(re.findall(r"^\s*(?:int|size_t|void|const char \*)\s*\*?(ldpc_\w+)\(", f.read(), flags=re.M))
    assert declared == set(nat.PRODUCT_EXPORTS)
    new = {"ldpc_decoder_set_quantizers", "ldpc_train_joint_ste_levels", "ldpc_train_joint_ste_levels_workspace_bytes",
           "ldpc_train_joint_layered_ste_levels", "ldpc_train_joint_layered_ste_levels_workspace_bytes"}
    assert new <= declared
    with open(nat.HEADER) as f:
        assert re.search(r"#define LDPC_HIP_ABI_VERSION 1\b", f.read())
    if os.path.exists(nat.LIB_PATH):                 # the built library exports them
        import ctypes
        lib = ctypes.CDLL(nat.LIB_PATH)
        assert all(hasattr(lib, s) for s in new)


@pytest.mark.parametrize("bc", [2, 3, 4, 8])
@pytest.mark.parametrize("layered", [False, "paper"])
def test_initial_thresholds_are_the_plain_decoders(bc, layered):
    from rcq_decoder import _threshold_table
    code = cases.load("small", 6)
    qp = [(3.0, 1.3), (5.0, 0.0), (7.1, 2.7)]
    plain = cases.make_decoder(code, 2, bc, qp, 6, seed=1, layered=layered)
    learn = lv.learnable(plain)
    a, b = _threshold_table(plain.quantizers), _threshold_table(learn.quantizers)
    assert a.dtype == np.float32 and a.tobytes() == b.tobytes()
    assert learn.quantizer_C.dtype == torch.float64 and learn.quantizer_gamma.dtype == torch.float64
    assert learn.quantizer_C.shape == (3,) and learn.quantizer_C.requires_grad and learn.quantizer_gamma.requires_grad
    # the thresholds are no part of the engine's identity for such a decoder, they are for the plain one
    assert b.tobytes() not in learn._extra_key() and a.tobytes() in plain._extra_key()


def test_data_writes_rebuild_the_quantizers_and_bad_values_are_refused():
    from rcq_decoder import NonUniformQuantizer
    code = cases.load("small", 4)
    dec = cases.make_decoder(code, 2, 3, QP3, 4, seed=1, learn_quantizer=True)
    with torch.no_grad():
        dec.quantizer_C.copy_(torch.tensor([3.0, 5.0, 7.0], dtype=torch.float64))
        dec.quantizer_gamma.copy_(torch.tensor([1.3, 1.3, 1.3], dtype=torch.float64))
    first = dec.quantizers
    assert dec.quantizers is first                                  # unchanged parameters: the same list
    assert [q.thresholds for q in first] == [NonUniformQuantizer(3, C, g).thresholds for C, g in QP3]
    dec.quantizer_C.data[1] = 6.5                                   # leaves no trace on the Parameter's version counter
    dec.quantizer_gamma.data.mul_(2.0)
    assert [q.thresholds for q in dec.quantizers] == [NonUniformQuantizer(3, C, 2.6).thresholds for C in (3.0, 6.5, 7.0)]
    assert dec._get_quantizer(3).C == 7.0
    with pytest.raises(AttributeError):
        dec.quantizers = first
    for name, bad in (("quantizer_C", float("nan")), ("quantizer_C", float("inf")), ("quantizer_gamma", float("nan")),
                      ("quantizer_gamma", -0.5)):
        d2 = copy.deepcopy(dec)
        getattr(d2, name).data[0] = bad
        with pytest.raises(ValueError, match=name):
            d2.quantizers
        with pytest.raises(ValueError, match=name):                 # before any device work: no GPU is asked for
            d2.joint_posterior_loss(torch.zeros(2, code.n), quantizer_gradient="straight_through")
        with pytest.raises(ValueError, match=name):
            d2(torch.zeros(2, code.n))
    with pytest.raises(ValueError, match="bc"):
        cases.make_decoder(code, 2, 1, QP3, 4, seed=1, learn_quantizer=True)
    with pytest.raises(TypeError):                                  # keyword only
        from rcq_decoder import WeightedRCQDecoder
        WeightedRCQDecoder(code, 3, 8, QP3, 2, 4, False, True)
    # gamma = 0 is allowed (every threshold equals C)
    d3 = copy.deepcopy(dec)
    d3.quantizer_gamma.data.zero_()
    assert d3.quantizers[0].thresholds == [3.0, 3.0, 3.0, 3.0]


def test_refusals_without_the_gradient_options_stay():
    code = cases.load("small", 4)
    x = torch.zeros(2, code.n)
    with pytest.raises(NotImplementedError):
        cases.make_decoder(code, 2, 3, QP3, 4, seed=1, learn_quantizer=True).joint_posterior_loss(x)
    with pytest.raises(NotImplementedError):
        cases.make_decoder(code, 2, 3, QP3, 4, seed=1, learn_quantizer=True, layered="paper",
                           quantizer_gradient="straight_through").joint_posterior_loss(x)


def test_state_dict_pickle_and_the_option_off():
    code = cases.load("small", 4)
    plain = cases.make_decoder(code, 2, 3, QP3, 4, seed=1)
    learn = lv.learnable(plain)
    names = [n for n, _ in plain.named_parameters()]
    assert [n for n, _ in learn.named_parameters() if not n.startswith("quantizer_")] == names
    assert not any("quantizer" in n for n in names) and not any("quantizer" in k for k in plain.state_dict())
    assert set(learn.state_dict()) - set(plain.state_dict()) == {"quantizer_C", "quantizer_gamma"}
    assert len(plain.quantizers) == 3
    plain.quantizers = plain.quantizers[:1]                          # still a plain attribute for the plain decoder
    assert len(plain.quantizers) == 1
    # round trip
    with torch.no_grad():
        learn.quantizer_C.copy_(torch.tensor([2.5, 4.5, 6.5], dtype=torch.float64))
        learn.quantizer_gamma.copy_(torch.tensor([1.1, 0.9, 1.7], dtype=torch.float64))
    other = lv.learnable(cases.make_decoder(code, 2, 3, QP3, 4, seed=2))
    other.load_state_dict(learn.state_dict())
    assert torch.equal(other.quantizer_C, learn.quantizer_C) and torch.equal(other.quantizer_gamma, learn.quantizer_gamma)
    assert [q.thresholds for q in other.quantizers] == [q.thresholds for q in learn.quantizers]
    # the cached state never travels
    learn.quantizers
    state = learn.__getstate__()
    assert state["_quantizers"] is None and state["_quantizer_key"] is None and state["_engine"] is None
    clone = copy.deepcopy(learn)
    assert [q.thresholds for q in clone.quantizers] == [q.thresholds for q in learn.quantizers]


def test_optimizer_and_clipping_take_the_float64_pair():
    code = cases.load("small", 4)
    learn = lv.learnable(cases.make_decoder(code, 2, 3, QP3, 4, seed=1))
    opt = torch.optim.Adam(learn.parameters(), lr=0.01)
    for p in learn.parameters():
        p.grad = torch.ones_like(p)
    norm = torch.nn.utils.clip_grad_norm_(learn.parameters(), 1e-3)
    assert np.isfinite(float(norm))
    before = learn.quantizer_C.detach().clone()
    opt.step()
    assert learn.quantizer_C.dtype == torch.float64 and not torch.equal(before, learn.quantizer_C)
    from training_framework import _grad_norm
    assert np.isfinite(_grad_norm(learn))
