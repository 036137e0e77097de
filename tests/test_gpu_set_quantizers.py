"""
GPU tests (-m gpu) of ldpc_decoder_set_quantizers / ``DecodeEngine.set_quantizers``: an engine whose threshold table was
replaced decodes, in every engine mode the table admits, bit for bit as an engine freshly created with that table, and
reports the same ``info()``.  The tables flip, one after the other, everything the native decoder derives from the threshold
values: sorted -> unsorted (the code-pair form, the layered kernels' lean instantiation), tau_0 = 0 -> tau_0 != 0 (the
resident kernels' per-check quantisation and the compact plan's check words, the layered plans' zero flag), a threshold
outside [2^-50, 2^50] (the float form of the 4-level key), and back.
"""
import numpy as np
import pytest
import torch

import pjt_rcq_cases as cases

pytestmark = pytest.mark.gpu

T = 6
B = 70
MODES = ("auto", "stream", "sweeps", "gather", "pair")
KINDS = ("small-wrcq2", "small-wrcq1", "wide-wrcq2", "small-rcq-layered-ref", "small-wrcq-paper")


def tables(bc):
    """[(name, float32 [3, L])]: the walk through the derived flags, ending where it started"""
    from rcq_decoder import NonUniformQuantizer, _threshold_table
    base = _threshold_table([NonUniformQuantizer(bc, C, g) for C, g in cases.QP3])
    unsorted = base.copy()
    unsorted[:, [1, 2]] = unsorted[:, [2, 1]]                      # tau_1 > tau_2
    gamma0 = _threshold_table([NonUniformQuantizer(bc, C, 0.0) for C in (2.0, 3.0, 4.0)])     # every tau = C: tau_0 != 0
    far = base.copy()
    far[:, -1] = np.float32(2.0 ** 55)                             # sorted and positive, outside the float key's range
    assert np.all(np.diff(base[:, 1:], axis=1) > 0) and np.all(base[:, 0] == 0) and np.all(gamma0[:, 0] != 0)
    return [("QP3", base), ("unsorted", unsorted), ("gamma0", gamma0), ("far", far), ("QP3 again", base)]


def engine_kwargs(kind, bc):
    """-> (code, keyword arguments of DecodeEngine without the thresholds)"""
    import _native as nat
    from rcq_decoder import _quantizer_schedule
    name, what = kind.split("-", 1)
    code = cases.load(name, T)
    g = code.tanner_graph()
    kw = dict(dtype=torch.float32, c2v_form=nat.C2V_RCQ, iters=T, q_of_iter=_quantizer_schedule(3, T))
    if what == "rcq-layered-ref":
        kw.update(schedule=nat.SCHED_LAYERED_REF, beta=np.ones((T, 1), np.float32), beta_slot=np.zeros(g.E, np.int32),
                  alpha=np.ones((T, 1), np.float32), alpha_slot=np.zeros(g.n, np.int32))
        return code, kw
    paper = what.endswith("paper")
    dec = cases.make_decoder(code, 2 if paper else int(what[4]), bc, cases.QP3, T, seed=5, layered="paper" if paper else False)
    lay = dec._sharing_layout()
    beta, alpha = dec.weight_tables()
    kw.update(schedule=dec._schedule(), beta=beta, beta_slot=lay.beta_slot, alpha=alpha, alpha_slot=lay.alpha_slot)
    return code, kw


def decodes(eng, x):
    out = []
    for es in (True, False):
        r = eng.decode(x, early_stop=es)
        out.append((r.bits.clone(), r.posterior.clone(), r.iterations.clone(), r.success.clone()))
    return out


def same(a, b):
    return all(torch.equal(u, v) for ra, rb in zip(a, b) for u, v in zip(ra, rb))


def admitted(eng, mode):
    try:
        eng.set_mode(mode)
        return True
    except NotImplementedError:
        return False


@pytest.mark.parametrize("bc", [3, 8], ids=["4-levels", "128-levels"])
@pytest.mark.parametrize("kind", KINDS)
def test_set_quantizers_equals_a_fresh_decoder(gpu_device, kind, bc):
    from engine import DecodeEngine
    code, kw = engine_kwargs(kind, bc)
    g = code.tanner_graph()
    x = torch.from_numpy(cases.channel(np.random.default_rng(31), B, code.n, (1.0, 6.0))).to(gpu_device)
    walk = tables(bc)
    eng = DecodeEngine(g, device=gpu_device, thresholds=walk[0][1], **kw)
    handle = eng.handle.value
    seen = set()
    for name, thr in walk:
        eng.set_mode("auto")
        eng.set_quantizers(thr)
        assert eng.handle.value == handle and np.array_equal(eng.current_thresholds(), thr)
        fresh = DecodeEngine(g, device=gpu_device, thresholds=thr, **kw)
        for mode in MODES:
            ok = admitted(fresh, mode)
            assert admitted(eng, mode) == ok, (name, mode)
            if not ok:
                continue
            assert eng.info() == fresh.info(), (name, mode, eng.info(), fresh.info())
            seen.add((name, fresh.info()["kernel"], fresh.info()["stream_form"]))
            assert same(decodes(eng, x), decodes(fresh, x)), (name, mode)
    print(sorted(seen, key=str))
    # the walk did change what runs (on the decoders that have more than one form)
    if kind == "small-wrcq2" and bc == 3:
        assert ("QP3", "code_pair", "rcq-code-pair") in seen and not any(n == "unsorted" and f == "rcq-code-pair" for n, _, f in seen)

    # a forced form the new table does not admit: refused, and the decoder is what it was
    eng.set_mode("auto")
    eng.set_quantizers(walk[0][1])
    if admitted(eng, "pair"):
        before = decodes(eng, x)
        info = eng.info()
        with pytest.raises(NotImplementedError):
            eng.set_quantizers(walk[1][1])
        assert np.array_equal(eng.current_thresholds(), walk[0][1]) and eng.info() == info
        assert same(decodes(eng, x), before)
        eng.set_quantizers(walk[2][1])             # sorted: admitted under the forced form
        fresh = DecodeEngine(g, device=gpu_device, thresholds=walk[2][1], **kw).set_mode("pair")
        assert same(decodes(eng, x), decodes(fresh, x))
    else:
        assert not (kind == "small-wrcq2" and bc == 3)


def test_set_quantizers_refusals(gpu_device):
    from neural_2d_decoder import Neural2DMinSumDecoder
    code = cases.load("small", T)
    eng = Neural2DMinSumDecoder(code, 2, T)._get_engine(gpu_device)
    with pytest.raises(NotImplementedError):
        eng.set_quantizers(np.zeros((3, 4), np.float32))
    import ctypes
    import _native as nat
    assert eng._lib.ldpc_decoder_set_quantizers(eng.handle, nat.ptr(np.zeros((3, 4), np.float32)), ctypes.c_void_p(0)) == -3
    code, kw = engine_kwargs("small-wrcq2", 3)
    from engine import DecodeEngine
    rcq = DecodeEngine(code.tanner_graph(), device=gpu_device, thresholds=tables(3)[0][1], **kw)
    with pytest.raises(ValueError):
        rcq.set_quantizers(np.zeros((3, 8), np.float32))          # same shapes only


def test_a_learnable_decoder_keeps_its_engine_across_threshold_changes(gpu_device):
    import pjt_rcq_levels_reference as lv
    code = cases.load("small", T)
    plain = cases.make_decoder(code, 2, 3, cases.QP3, T, seed=5)
    dec = lv.learnable(plain)
    x = torch.from_numpy(cases.channel(np.random.default_rng(32), B, code.n, (1.0, 6.0))).to(gpu_device)
    with torch.no_grad():
        a, b = dec(x), plain(x)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        eng = dec._get_engine(gpu_device)
        handle = eng.handle.value
        dec.quantizer_C.data.mul_(1.25)
        dec.quantizer_gamma.data[0] = 0.0
        from rcq_decoder import WeightedRCQDecoder
        qp = list(zip(dec.quantizer_C.tolist(), dec.quantizer_gamma.tolist()))
        other = WeightedRCQDecoder(code, 3, 8, qp, 2, T)
        other.load_state_dict(plain.state_dict())
        a, b = dec(x), other(x)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        assert dec._get_engine(gpu_device) is eng and eng.handle.value == handle
        assert other._get_engine(gpu_device) is not eng
