"""
The one case the iterative-demapping GPU tests share (tests/test_gpu_decode_iterative.py), and the numpy restatement that chose
it: code small_96_48, set-partitioned 8-PSK, BasicMinSumDecoder(0.7) with T iterations, 67 frames of random codewords drawn
on the device channel at (SEED, STREAM, FIRST) and Es/N0 = SNR_DB.  Not a test module.

``restate`` runs the rounds on the CPU -- the channel from the Philox words (tests/modulation_reference.py; normals in
float64, so the samples are the device's to about 1e-5, not bit for bit), the rule (tests/demap_prior_reference.py) and the
oracle decoder in fp32 -- and returns per frame the round it closed in (0: never).  SEED and SNR_DB were chosen with it so
that every class -- closing in round 1, closing in a later round, never closing -- holds clearly more than three of the 67
frames (``python tests/decode_iterative_cases.py`` prints the counts); the GPU test asserts at least three of each on the
device's own result, so a loop that never feeds back cannot pass.
"""
import numpy as np

import constellation_reference as cref
import demap_prior_reference as pref
import modulation_reference as mref

CODE, BATCH, T, ROUNDS, FACTOR = "small_96_48", 67, 10, 3, 0.7
SNR_DB = 6.5
# the frames a SimulationConfig(seed=SEED, codeword="random") sweep draws first at SNR_DB: stream round(1000 SNR_DB), frame 0 on
SEED, STREAM, FIRST = 0x2545f4914f6cdd1d, 6500, 0
MIN_PER_CLASS = 3


def constellation():
    from modulation import Constellation
    return Constellation(pref.sp_psk8(), name="psk8sp")


def codewords(batch=BATCH, seed=SEED, stream=STREAM, first=FIRST):
    """0/1 uint8 [batch, n]: the codewords engine.encode_random draws for these frames, from the host encoder and the restated
    information-bit stream"""
    import codes
    import encode_reference as eref
    enc = codes.Encoder.from_graph(codes.load_graph(CODE))
    return enc.encode(eref.info_bits(batch, enc.k, seed, stream, first))


def received(con, cw_bits, snr_db=SNR_DB, seed=SEED, stream=None, first=FIRST):
    """float32 [batch, S, 4]: the restated samples of the frames (no fading)"""
    batch, n = cw_bits.shape
    m = con.bits_per_symbol
    S = (n + m - 1) // m
    stream = int(round(snr_db * 1000)) if stream is None else stream
    words = mref.symbol_words(batch, S, seed, stream, first)
    z = mref.symbol_normals(words).astype(np.float32)
    e = np.full((batch, S), con.amp(snr_db), dtype=np.float32)
    v = cref.received32(con.points, mref.symbol_bits(cw_bits, m), e, z)
    rec = np.zeros((batch, S, 4), dtype=np.float32)
    rec[..., :2], rec[..., 2] = v, e
    return rec


def restate(snr_db=SNR_DB, seed=SEED, rounds=ROUNDS, prior_scale=1.0):
    """-> (closed_in int [batch]: the round a frame's decode first succeeded in, 0 for never; iterations int [batch] summed
    over the rounds a frame ran)"""
    import codes
    import oracle
    oracle.build()
    g = codes.load_graph(CODE)
    og = oracle.OracleGraph(n=g.n, check_ptr=np.asarray(g.check_ptr), var_idx=np.asarray(g.var_idx, dtype=np.int64))
    con = constellation()
    cw = codewords(seed=seed, stream=int(round(snr_db * 1000)))
    n, m = cw.shape[1], con.bits_per_symbol
    rec = received(con, cw, snr_db, seed)
    llr = cref.to_variables(cref.demap(rec, con.points), n)
    closed = np.zeros(cw.shape[0], dtype=np.int64)
    iters = np.zeros(cw.shape[0], dtype=np.int64)
    for r in range(1, rounds + 1):
        _, post, it, ok = oracle.basic_minsum(og, llr, FACTOR, T, dtype=np.float32)
        open_ = closed == 0
        iters[open_] += it[open_]
        closed[open_ & ok] = r
        la = pref.symbol_priors(pref.apriori(post, llr, prior_scale), m)
        llr = pref.to_variables(pref.demap(rec, con.points, la), n)
    return closed, iters


if __name__ == "__main__":
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(os.path.dirname(here), "oracle"),
                    os.path.join(os.path.dirname(here), [d for d in os.listdir(os.path.dirname(here)) if d.endswith("_amd")][0])]
    closed, iters = restate()
    print("closed in round:", {r: int((closed == r).sum()) for r in range(ROUNDS + 1)}, "iterations", int(iters.sum()))
