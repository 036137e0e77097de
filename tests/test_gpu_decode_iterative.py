"""
GPU tests (-m gpu) of iterative demapping with decoder feedback: ``DecodeEngine.decode_iterative`` against the loop restated
from the public pieces, its independence of the batch's composition, the three classes of frames the shared case was chosen
for (tests/decode_iterative_cases.py), and the ``SimulationConfig(iterative_demapping=3)`` sweep with ``replay_errors``.
One case: small_96_48, set-partitioned 8-PSK, BasicMinSumDecoder, 67 frames of random codewords.
"""
import numpy as np
import pytest
import torch

import decode_iterative_cases as dc

pytestmark = pytest.mark.gpu

FIELDS = ("bits", "posterior", "iterations", "success", "packed_bits", "rounds")


@pytest.fixture(scope="module")
def case(gpu_device):
    """the engine, the constellation, the frames' samples and the loop restated once from engine.demap and eng.decode over the
    full batch every round, merged per frame with torch.where"""
    import codes
    import engine
    from ldpc_decoder import BasicMinSumDecoder
    code = codes.load_code(dc.CODE, max_iterations=dc.T)
    dec = BasicMinSumDecoder(code, factor=dc.FACTOR)
    eng = dec._engine(torch.float32, gpu_device)
    con = dc.constellation()
    n = code.n
    cw = engine.encode_random(eng.encoder(), dc.BATCH, seed=dc.SEED, stream_id=dc.STREAM, first_frame=dc.FIRST, device=gpu_device)
    assert np.array_equal(np.unpackbits(cw.cpu().numpy(), axis=1, bitorder="little")[:, :n], dc.codewords())
    llr1, rec = engine.sym_llr(dc.BATCH, n, seed=dc.SEED, stream_id=dc.STREAM, first_frame=dc.FIRST, modulation=con,
                               snr_db=dc.SNR_DB, codeword=cw, device=gpu_device, want_received=True)
    kw = dict(early_stop=True, want_packed=True)
    llr = engine.demap(rec, n, modulation=con)
    assert torch.equal(llr, llr1)
    res = eng.decode(llr, **kw)
    want = {f: getattr(res, f).clone() for f in FIELDS[:-1]}
    want["rounds"] = torch.ones(dc.BATCH, dtype=torch.int32, device=gpu_device)
    closed = res.success.clone()
    per_round = [res]
    for _ in range(1, dc.ROUNDS):
        llr = engine.demap(rec, n, modulation=con, prior=res.posterior, prior_sub=llr)
        res = eng.decode(llr, **kw)
        per_round.append(res)
        live = ~closed
        for f in ("bits", "posterior", "packed_bits"):
            want[f] = torch.where(live[:, None], getattr(res, f), want[f])
        want["success"] = torch.where(live, res.success, want["success"])
        want["iterations"] = torch.where(live, want["iterations"] + res.iterations, want["iterations"])
        want["rounds"] = torch.where(live, want["rounds"] + 1, want["rounds"])
        closed = closed | res.success
    return dict(code=code, dec=dec, eng=eng, con=con, n=n, cw=cw, rec=rec, llr1=llr1, want=want, per_round=per_round)


def assert_same(res, want, rows=slice(None), what=""):
    for f in FIELDS:
        got, exp = getattr(res, f), want[f][rows]
        assert got.dtype == exp.dtype and got.shape == exp.shape, (what, f)
        if got.dtype == torch.float32:
            assert torch.equal(got.view(torch.int32), exp.view(torch.int32)), (what, f)      # bit for bit
        else:
            assert torch.equal(got, exp), (what, f)


def test_one_round_is_demap_then_decode(case):
    import engine
    eng, con, rec, n = case["eng"], case["con"], case["rec"], case["n"]
    for early in (True, False):
        one = eng.decode_iterative(rec, modulation=con, rounds=1, early_stop=early, want_packed=True)
        ref = eng.decode(engine.demap(rec, n, modulation=con), early_stop=early, want_packed=True)
        want = {f: getattr(ref, f) for f in FIELDS[:-1]}
        want["rounds"] = torch.ones(dc.BATCH, dtype=torch.int32, device=rec.device)
        assert_same(one, want, what=f"rounds=1 early_stop={early}")
    assert ref.rounds is None                                                                # every other producer leaves it None
    lean = eng.decode_iterative(rec, modulation=con, rounds=1, want_bits=False, want_posterior=False)
    assert lean.bits is None and lean.posterior is None and lean.packed_bits is None and lean.rounds is not None


def test_three_rounds_are_the_restated_loop_and_feed_back(case):
    eng, con, rec, want = case["eng"], case["con"], case["rec"], case["want"]
    res = eng.decode_iterative(rec, modulation=con, rounds=dc.ROUNDS, want_packed=True)
    assert res.rounds.dtype == torch.int32 and res.iterations.dtype == torch.int32 and res.success.dtype == torch.bool
    assert_same(res, want, what="rounds=3")
    rounds, success = res.rounds.cpu().numpy(), res.success.cpu().numpy()
    first = int((success & (rounds == 1)).sum())
    later = int((success & (rounds > 1)).sum())
    never = int((~success).sum())
    print(f"closed in round 1: {first}, in a later round: {later}, never: {never}; iterations {int(res.iterations.sum())}")
    assert min(first, later, never) >= dc.MIN_PER_CLASS                                      # chosen so on the CPU (decode_iterative_cases)
    assert (rounds[~success] == dc.ROUNDS).all() and (rounds >= 1).all() and (rounds <= dc.ROUNDS).all()
    # a frame that closed keeps the outputs of the round it closed in, and every closed frame is a codeword
    for r, per in enumerate(case["per_round"], start=1):
        rows = torch.nonzero(res.success & (res.rounds == r)).reshape(-1)
        assert torch.equal(res.bits[rows], per.bits[rows]) and bool(per.success[rows].all())
    # the fed-back rounds are not the first one again: some frame's LLRs moved, and a later round closed frames round 1 left open
    assert not bool(case["per_round"][0].success[res.success & (res.rounds > 1)].any())
    # round 1's LLRs handed in (what sym_llr returned beside the samples): the same result, and they are left as they were
    mine = case["llr1"].clone()
    given = eng.decode_iterative(rec, modulation=con, rounds=dc.ROUNDS, want_packed=True, llr=mine)
    assert_same(given, want, what="llr given")
    assert torch.equal(mine.view(torch.int32), case["llr1"].view(torch.int32))
    with pytest.raises(ValueError, match="llr must be"):
        eng.decode_iterative(rec, modulation=con, rounds=2, llr=mine[:, :-1])
    # lean outputs: the same packed decisions, iterations and rounds
    lean = eng.decode_iterative(rec, modulation=con, rounds=dc.ROUNDS, want_bits=False, want_posterior=False, want_packed=True)
    assert lean.bits is None and lean.posterior is None
    assert torch.equal(lean.packed_bits, res.packed_bits) and torch.equal(lean.iterations, res.iterations)
    assert torch.equal(lean.rounds, res.rounds) and torch.equal(lean.success, res.success)


def test_frames_do_not_depend_on_the_batch_they_are_in(case):
    eng, con, rec, want = case["eng"], case["con"], case["rec"], case["want"]
    for rows in ([0], [66], [5, 6, 7], list(range(40, 67)), [3, 1, 2]):
        idx = torch.tensor(rows, device=rec.device)
        res = eng.decode_iterative(rec[idx].contiguous(), modulation=con, rounds=dc.ROUNDS, want_packed=True)
        assert_same(res, want, idx, what=f"rows {rows}")


def test_without_early_stop_every_frame_runs_every_round(case):
    import engine
    eng, con, rec, n = case["eng"], case["con"], case["rec"], case["n"]
    res = eng.decode_iterative(rec, modulation=con, rounds=dc.ROUNDS, early_stop=False, want_packed=True)
    assert (res.rounds == dc.ROUNDS).all()
    llr = engine.demap(rec, n, modulation=con)
    ref = eng.decode(llr, early_stop=False, want_packed=True)
    for _ in range(1, dc.ROUNDS):
        llr = engine.demap(rec, n, modulation=con, prior=ref.posterior, prior_sub=llr)
        ref = eng.decode(llr, early_stop=False, want_packed=True)
    want = {f: getattr(ref, f) for f in FIELDS[:-1]}
    want["rounds"] = torch.full((dc.BATCH,), dc.ROUNDS, dtype=torch.int32, device=rec.device)
    assert_same(res, want, what="early_stop=False")
    # a scale of the feedback is the demapper's prior_scale
    half = eng.decode_iterative(rec, modulation=con, rounds=2, prior_scale=0.5, early_stop=False)
    l1 = engine.demap(rec, n, modulation=con)
    r1 = eng.decode(l1, early_stop=False)
    r2 = eng.decode(engine.demap(rec, n, modulation=con, prior=r1.posterior, prior_sub=l1, prior_scale=0.5), early_stop=False)
    assert torch.equal(half.posterior.view(torch.int32), r2.posterior.view(torch.int32))


def test_what_decode_iterative_refuses(case):
    from ldpc_decoder import BasicMinSumDecoder
    from modulation import Modulation
    eng, con, rec = case["eng"], case["con"], case["rec"]
    for bad in (0, -1, 1.5, True, None, "3"):
        with pytest.raises(ValueError, match="rounds"):
            eng.decode_iterative(rec, modulation=con, rounds=bad)
    with pytest.raises(ValueError, match="Constellation"):
        eng.decode_iterative(rec, modulation=Modulation("qpsk"), rounds=2)
    with pytest.raises(ValueError, match="received"):
        eng.decode_iterative(rec.cpu(), modulation=con, rounds=2)
    e64 = BasicMinSumDecoder(case["code"], factor=dc.FACTOR)._engine(torch.float64, rec.device)
    with pytest.raises(TypeError, match="fp32"):
        e64.decode_iterative(rec, modulation=con, rounds=2)


def test_sweep_counts_the_same_frames_whatever_the_block_and_replays_them(case, tmp_path):
    from simulation_framework import LDPSimulator, SimulationConfig
    want = case["want"]
    counters = []
    for block in (16, 67):
        cfg = SimulationConfig(snr_range=(dc.SNR_DB, dc.SNR_DB), snr_step=1.0, max_frames=dc.BATCH, max_errors=10 ** 6,
                               batch_frames=block, seed=dc.SEED, channel="device", codeword="random", save_results=False,
                               results_dir=str(tmp_path), modulation=case["con"], iterative_demapping=dc.ROUNDS)
        sim = LDPSimulator(cfg)
        counters.append(sim._simulate_device(case["eng"], case["n"], dc.SNR_DB, dc.BATCH, 10 ** 6))
    assert [c.pop("blocks_seen") for c in counters] == [5, 1]                                # the block size changes this word alone
    assert counters[0] == counters[1]
    c = counters[0]
    assert c["frames"] == dc.BATCH and c["iterations"] == int(want["iterations"].sum())
    sent = torch.from_numpy(dc.codewords().astype(np.int32)).to(want["bits"].device)
    wrong = (want["bits"] != sent).sum(dim=1)
    assert c["frame_errors"] == int((wrong > 0).sum()) and c["bit_errors"] == int(wrong.sum())
    # the public sweep gives the same point
    fer, ber, avg, _, frames, errors = sim.simulate_single_snr(case["dec"], case["code"], dc.SNR_DB, dc.BATCH, 10 ** 6)
    assert (frames, errors) == (dc.BATCH, c["frame_errors"]) and avg == c["iterations"] / dc.BATCH
    # three frames again: one of each class where the run has them
    rounds, success = want["rounds"].cpu().numpy(), want["success"].cpu().numpy()
    pick = [int(np.flatnonzero(success & (rounds == 1))[0]), int(np.flatnonzero(success & (rounds > 1))[0]),
            int(np.flatnonzero(~success)[-1])]
    rep = sim.replay_errors(case["dec"], case["code"], dc.SNR_DB, pick)
    idx = torch.tensor(pick, device=want["bits"].device)
    assert rep["frames"] == pick
    for f in ("bits", "posterior", "iterations", "success", "rounds"):
        assert torch.equal(rep[f], want[f][idx]), f
    assert torch.equal(rep["llr"], case["llr1"][idx]) and torch.equal(rep["received"], case["rec"][idx])
    assert torch.equal(rep["codewords"], case["cw"][idx])
    # K = 1 takes the path it took before: no `rounds` in the replay
    cfg1 = SimulationConfig(snr_range=(dc.SNR_DB, dc.SNR_DB), max_frames=dc.BATCH, seed=dc.SEED, channel="device",
                            codeword="random", save_results=False, modulation=case["con"])
    assert "rounds" not in LDPSimulator(cfg1).replay_errors(case["dec"], case["code"], dc.SNR_DB, pick[:1])
