"""
``schedule="layered"`` of the min-sum decoders (-m gpu): BasicMinSumDecoder, Neural2DMinSumDecoder (types 1-4),
Neural2DOffsetMinSumDecoder, NeuralMinSumDecoder and NeuralOffsetMinSumDecoder on the LDS-resident kernel
(layered_minsum_lds, ldpc_layered.hip: check records in LDS) and the HBM-streaming one (layered_minsum,
ldpc_kernels.hip: fp32 messages; LDPC_ENGINE_MODE=stream, checks wider than a wavefront, the (16200,7200) code).

Nothing in the reference executes this schedule: the yardstick is the numpy restatement of
tests/layered_minsum_reference.py (pinned by tests/test_layered_minsum_host.py), and every comparison is
``np.array_equal`` on decisions, fp32 posteriors, iterations and success.  The per-edge messages are compared where the
engine keeps them -- the streaming kernel's workspace (``DecodeEngine.debug_c2v``); the LDS kernel keeps check records in
their place, which nothing copies out, so there its messages are pinned through the posteriors of the iterations that
subtract them.  One anchor does not pass through the restatement: on a graph whose variables all have degree <= 1 the
first layered iteration IS the first flooding iteration.

Inputs and decoders come from tests/layered_minsum_cases.py; the host test shows that the restatement decodes between
20 % and 80 % of every input set, so stopped rows sit beside live ones in one wave.
"""
import numpy as np
import pytest
import torch

import layered_minsum_cases as cs
import layered_minsum_reference as ref
# the refusals and the keyword's own checks need no device; they run here too (on the GPU box only this file may run)
from test_layered_minsum_host import (recorded, test_forward_with_autograd_on_is_refused,  # noqa: F401
                                      test_joint_posterior_loss_is_refused, test_schedule_reaches_the_engine_descriptor,
                                      test_unknown_schedule_raises_value_error)

pytestmark = pytest.mark.gpu

MODES = ("auto", "stream")
LDS, STREAM = "layered_minsum_lds", "layered_minsum"


@pytest.fixture(autouse=True)
def inference_mode():
    with torch.no_grad():
        yield


def fresh_engine(dec, device, mode, monkeypatch):
    """the decoder's engine, rebuilt so that it reads the mode"""
    from simulation_framework import _engine_of
    monkeypatch.setenv("LDPC_ENGINE_MODE", mode)
    if hasattr(dec, "_engines"):
        dec._engines = {}
    else:
        dec._engine = None
    return _engine_of(dec, device)


def check(name, device, monkeypatch, *, family=None, T=None, rows=None, max_iters=None, modes=MODES, stops=(True, False),
          want_kernel=None):
    """decode input set `name` under every mode and stop rule; everything equals the restatement (and so each other)"""
    code_name, fam0, T0, seed, _ = cs.INPUT_SETS[name]
    family, T = family or fam0, T0 if T is None else T
    dec = cs.make(family, cs.load(code_name), T, seed)
    llr = cs.input_llr(name) if rows is None else cs.input_llr(name)[:rows]
    x = torch.from_numpy(np.ascontiguousarray(llr)).to(device)
    B = x.shape[0]
    for mode in modes:
        eng = fresh_engine(dec, device, mode, monkeypatch)
        kernel = eng.info()["kernel"]
        if want_kernel is not None:
            assert kernel == (want_kernel if mode == "auto" else STREAM), (name, mode, eng.info())
        for es in stops:
            want = cs.reference(name, family=family, T=T, early_stop=es, max_iters=max_iters, rows=rows)
            res = eng.decode(x, early_stop=es, want_packed=True, max_iters=max_iters)
            tag = f"{name} {family} T={T} B={B} es={es} cap={max_iters} {mode}"
            np.testing.assert_array_equal(res.iterations.cpu().numpy(), want[2], err_msg=tag)
            np.testing.assert_array_equal(res.success.cpu().numpy(), want[3], err_msg=tag)
            np.testing.assert_array_equal(res.bits.cpu().numpy(), want[0], err_msg=tag)
            np.testing.assert_array_equal(res.posterior.cpu().numpy(), want[1], err_msg=tag)
            np.testing.assert_array_equal(np.unpackbits(res.packed_bits.cpu().numpy(), axis=1, bitorder="little")[:, :llr.shape[1]],
                                          want[0], err_msg=tag)
            if kernel == STREAM:
                np.testing.assert_array_equal(eng.debug_c2v(B, max_iters).cpu().numpy(), want[4], err_msg=tag)


# ---- families ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", cs.FAMILIES)
def test_every_family_on_toy_and_small(family, gpu_device, monkeypatch):
    """Basic with beta 0.7; the degree-shared types with random betas (one zero, one negative slot) and variable-side
    alphas the schedule must ignore; the offset form with a non-zero check-side alpha; both per-edge decoders"""
    check("toy", gpu_device, monkeypatch, family=family, want_kernel=LDS)
    check("small", gpu_device, monkeypatch, family=family, want_kernel=LDS)


def test_variable_side_alpha_has_no_effect(gpu_device, monkeypatch):
    dec = cs.make("n2d2", cs.load("small_96_48"), 10, seed=8)
    x = torch.from_numpy(np.array(cs.input_llr("small"))).to(gpu_device)
    for mode in MODES:
        eng = fresh_engine(dec, gpu_device, mode, monkeypatch)
        before = eng.decode(x)
        with torch.no_grad():
            for p in dec.alpha_weights.values():
                p.mul_(1.7)
        from simulation_framework import _engine_of
        after = _engine_of(dec, gpu_device).decode(x)
        assert torch.equal(before.posterior, after.posterior) and torch.equal(before.iterations, after.iterations)


# ---- codes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lw", cs.LANE_WIDTHS)
def test_every_lane_width(lw, gpu_device, monkeypatch):
    """a random graph per lane width of the LDS kernel: a check that fills the row exactly, a degree-1 and a degree-0 check"""
    check(f"lw{lw}", gpu_device, monkeypatch, want_kernel=LDS)
    check(f"lw{lw}", gpu_device, monkeypatch, family="basic", T=2, want_kernel=LDS)


@pytest.mark.parametrize("family", ["basic", "n2d_oms"])
def test_checks_wider_than_a_wavefront_stream(family, gpu_device, monkeypatch):
    check("wide", gpu_device, monkeypatch, family=family, want_kernel=STREAM)


def test_ira_1998_1512(gpu_device, monkeypatch):
    """128 codewords, T = 10 on the LDS kernel and the streaming one; the size condition of the check record: at least four
    one-wave workgroups per CU, and no more LDS per codeword than layered_paper_lds keeps on the same code"""
    check("ira", gpu_device, monkeypatch, want_kernel=LDS)
    from rcq_decoder import WeightedRCQDecoder
    monkeypatch.setenv("LDPC_ENGINE_MODE", "auto")
    code = cs.load("ira_1998_1512")
    paper = WeightedRCQDecoder(code, 3, 8, [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)], weight_sharing_type=2, max_iterations=10,
                               layered="paper")._get_engine(gpu_device).info()
    assert paper["kernel"] == "layered_paper_lds"
    for family in ("basic", "n2d_oms"):
        info = fresh_engine(cs.make(family, code, 10, 1), gpu_device, "auto", monkeypatch).info()
        assert info["kernel"] == LDS and info["workgroups_per_cu"] >= 4, info
        assert info["lds_bytes"] / info["codewords_per_workgroup"] <= paper["lds_bytes"] / paper["codewords_per_workgroup"], (info, paper)


def test_dvbs2_like_16200_7200_streams(gpu_device, monkeypatch):
    """64.8 KB of posteriors and 9000 check records do not leave a wave per SIMD: the streaming kernel under both modes"""
    check("dvbs2", gpu_device, monkeypatch, want_kernel=STREAM, stops=(True,))


# ---- shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [0, 1, 2, 10])
@pytest.mark.parametrize("family", ["n2d1", "n2d_oms"])
def test_iteration_counts_and_ragged_batches(T, family, gpu_device, monkeypatch):
    """T = 0 returns the LLRs; batches of 1, 3, 5 and 67 leave a partly filled wave and a partly filled tile"""
    for rows in (1, 3, 5, None):
        check("small", gpu_device, monkeypatch, family=family, T=T, rows=rows, want_kernel=LDS)


@pytest.mark.parametrize("cap", [1, 3])
def test_max_iters_below_T(cap, gpu_device, monkeypatch):
    """ldpc_decode_capped: iteration t keeps the tables of iteration t, an open codeword reports the cap and no success"""
    check("small", gpu_device, monkeypatch, family="n2d_oms", max_iters=cap, want_kernel=LDS)
    check("wide", gpu_device, monkeypatch, family="n2d1", max_iters=cap, want_kernel=STREAM)
    assert (cs.reference("small", family="n2d_oms", max_iters=cap)[2] == cap).any()


# ---- an anchor that does not pass through the restatement -----------------------------------------------------------------
@pytest.mark.parametrize("family", ["basic", "n2d2", "n2d_oms"])
def test_first_iteration_equals_flooding_where_no_variable_is_shared(family, gpu_device, monkeypatch):
    """variables of degree <= 1: u = llr on every edge and each posterior receives one message, so layered T = 1 and the
    existing flooding engine's T = 1 are both llr + message (the alpha of these decoders' flooding form is exactly 1)"""
    from ldpc_decoder import LDPCCode
    rng = np.random.default_rng(41)
    degs = [1, 7, 0, 2, 16, 3, 33, 5]
    n = sum(degs) + 4                                        # four variables in no check
    H = np.zeros((len(degs), n), dtype=np.int64)
    perm, at = rng.permutation(n), 0
    for i, dc in enumerate(degs):
        H[i, perm[at:at + dc]] = 1
        at += dc
    code = LDPCCode(n=n, k=n - len(degs), H=H, max_iterations=1)
    llr = cs.awgn(rng, 37, n, 1.0)
    llr[0, :3] = 0.0
    llr[1] = np.round(llr[1])
    x = torch.from_numpy(llr).to(gpu_device)
    lay, flo = cs.make(family, code, 1, seed=3), cs.make(family, code, 1, seed=3, schedule=None)
    if family == "n2d2":
        with torch.no_grad():
            for d in (lay, flo):
                for p in d.alpha_weights.values():
                    p.fill_(1.0)
    for mode in MODES:
        a = fresh_engine(lay, gpu_device, mode, monkeypatch).decode(x, early_stop=False)
        b = fresh_engine(flo, gpu_device, mode, monkeypatch).decode(x, early_stop=False)
        np.testing.assert_array_equal(a.posterior.cpu().numpy(), b.posterior.cpu().numpy(), err_msg=mode)
        np.testing.assert_array_equal(a.success.cpu().numpy(), b.success.cpu().numpy(), err_msg=mode)
        assert (a.posterior != x).any()


# ---- weight updates on a live engine ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family", ["n2d1", "n2d_oms", "edge_nms"])
def test_set_weights_reaches_the_live_engine(family, mode, gpu_device, monkeypatch):
    from simulation_framework import _engine_of
    code = cs.load("small_96_48")
    dec = cs.make(family, code, 10, seed=2)
    llr = cs.input_llr("small")
    x = torch.from_numpy(np.array(llr)).to(gpu_device)
    eng = fresh_engine(dec, gpu_device, mode, monkeypatch)
    first = eng.decode(x)
    cs.randomise(dec, np.random.default_rng(99), cs.form_of(family) == ref.OMS)      # beta, and the offset form's check-side alpha
    assert _engine_of(dec, gpu_device) is eng                                         # same engine, new tables
    beta_e, a_e = cs.edge_tables(dec, family, 10)
    want = ref.restate(code.tanner_graph(), llr, 10, cs.form_of(family), beta_e, a_e)
    res = eng.decode(x)
    np.testing.assert_array_equal(res.iterations.cpu().numpy(), want[2])
    np.testing.assert_array_equal(res.posterior.cpu().numpy(), want[1])
    np.testing.assert_array_equal(res.success.cpu().numpy(), want[3])
    assert not torch.equal(first.posterior, res.posterior)


# ---- host interface ------------------------------------------------------------------------------------------------------
def test_host_classes_return_the_layered_decode(gpu_device, monkeypatch):
    """forward / decode of the host classes (GPU tensors and the small-host-batch path) give the engine's result"""
    monkeypatch.setenv("LDPC_ENGINE_MODE", "auto")
    llr = cs.input_llr("small")
    x = torch.from_numpy(np.array(llr)).to(gpu_device)
    for family in ("n2d3", "edge_oms"):
        want = cs.reference("small", family=family)
        dec = cs.make(family, cs.load("small_96_48"), 10, cs.INPUT_SETS["small"][3])
        bits, post, iters = dec(x)
        assert post.grad_fn is None
        np.testing.assert_array_equal(post.cpu().numpy(), want[1])
        np.testing.assert_array_equal(iters.cpu().numpy(), want[2])
        hb, hp, hi = dec(torch.from_numpy(np.array(llr[:9])))          # host tensor, <= 64 rows: decode_host
        np.testing.assert_array_equal(hp.numpy(), want[1][:9])
        np.testing.assert_array_equal(hb.numpy(), want[0][:9])
    basic = cs.make("basic", cs.load("small_96_48"), 10, 0)
    want = cs.reference("small")
    bits, succ, iters = basic.decode(x)
    np.testing.assert_array_equal(bits.cpu().numpy(), want[0])
    np.testing.assert_array_equal(succ.cpu().numpy(), want[3])
    b1, s1, i1 = basic.decode(llr[4])                                   # the reference's call shape, fp32 vector
    assert np.array_equal(b1, want[0][4]) and s1 == bool(want[3][4]) and i1 == int(want[2][4])
    assert basic._engines and all(e.info()["kernel"] == LDS for e in basic._engines.values())


def test_what_the_c_abi_refuses(gpu_device, monkeypatch):
    import _native as nat
    from engine import DecodeEngine
    monkeypatch.setenv("LDPC_ENGINE_MODE", "auto")
    code = cs.load("small_96_48")
    g = code.tanner_graph()
    x = torch.from_numpy(np.array(cs.input_llr("small"))).to(gpu_device)
    basic = cs.make("basic", code, 10, 0)
    with pytest.raises(NotImplementedError, match="fp32 only"):            # float64 in -> fp64 engine -> refused
        basic.decode(x.double())
    tables = dict(beta=np.full((10, 1), 0.7, np.float32), beta_slot=np.zeros(g.E, np.int32),
                  alpha=np.ones((10, 1), np.float32), alpha_slot=np.zeros(g.n, np.int32))
    with pytest.raises(NotImplementedError):                                # the reference's schedule has no min-sum form
        DecodeEngine(g, dtype=torch.float32, c2v_form=nat.C2V_NMS, iters=10, schedule=nat.SCHED_LAYERED_REF,
                     device=gpu_device, **tables)
    eng = DecodeEngine(g, dtype=torch.float32, c2v_form=nat.C2V_NMS, iters=10, schedule=nat.SCHED_LAYERED,
                       device=gpu_device, **tables)
    for call in (lambda: eng.decode_saving(x), lambda: eng.train_joint(x)):
        with pytest.raises(NotImplementedError, match="layered schedule"):
            call()
    saved = torch.empty(256, dtype=torch.uint8, device=gpu_device)
    with pytest.raises(NotImplementedError, match="layered schedule"):
        eng.backward(saved, x, torch.ones(x.shape[0], dtype=torch.int32, device=gpu_device), torch.zeros_like(x))


# ---- simulator -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("staged", [False, True])
def test_simulator_counts_equal_restated_blocks(staged, gpu_device, monkeypatch, tmp_path):
    """LDPSimulator drives a layered decoder like any other; staged: the streaming kernel, blocks capped and the stragglers
    restarted from their LLRs -- the same decode.  The blocks the simulator draws are decoded by the restatement and counted by
    the reference's per-frame loop (the pattern of tests/test_simulation_framework.py)."""
    from simulation_framework import LDPSimulator, SimulationConfig, _engine_of
    monkeypatch.setenv("LDPC_ENGINE_MODE", "stream" if staged else "auto")
    code = cs.load("small_96_48")
    g = code.tanner_graph()
    dec = cs.make("basic", code, 10, 0)
    assert _engine_of(dec, gpu_device).info()["kernel"] == (STREAM if staged else LDS)
    beta_e = np.full((10, g.E), 0.7, dtype=np.float32)
    snr_db, max_frames, max_errors, block = 2.0, 700, 60, 256
    cfg = SimulationConfig(max_frames=max_frames, max_errors=max_errors, batch_frames=block, seed=9,
                           results_dir=str(tmp_path), save_results=False, staged_early_stop=staged, stage_min_block=64)
    sim = LDPSimulator(cfg)
    fer, ber, avg_it, _t, frames, errs = sim.simulate_single_snr(dec, dec.code, snr_db, max_frames, max_errors)
    gen = torch.Generator(device=gpu_device)
    gen.manual_seed(9 * 1_000_003 + int(round(snr_db * 1000)))
    total = frame_errors = bit_errors = total_iterations = 0
    while total < max_frames and frame_errors < max_errors:
        x = sim._draw_llr(gen, min(block, max_frames - total), code.n, snr_db, gpu_device).cpu().numpy()
        ob, _, oi, _, _ = ref.restate(g, x, 10, ref.NMS, beta_e)
        for r in range(len(x)):
            if not (total < max_frames and frame_errors < max_errors):
                break
            if ob[r].any():
                frame_errors += 1
                bit_errors += int(ob[r].sum())
            total_iterations += int(oi[r])
            total += 1
    assert frame_errors > 0 and (frames, errs) == (total, frame_errors)
    assert fer == frame_errors / total and ber == bit_errors / (total * code.n) and avg_it == total_iterations / total
