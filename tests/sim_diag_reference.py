"""
numpy restatement of the diagnostic Monte-Carlo counters (ldpc_sim_count_diag of include/ldpc_hip.h): the diag buffer
{ undetected, captured, 0, 0, hist[T + 1], records[capture][4] } over the frames that the in-order stop rule of
philox_reference.sim_fold consumes.  Not a test module; tests/test_sim_diag_host.py and the GPU tests import it.
"""
import numpy as np

import philox_reference as ref


def diag_words(T, capture):
    return 4 + T + 1 + 4 * capture


def signed64(v):
    """a frame index (mod 2^64, as the device adds it) as the int64 word that holds it"""
    v = int(v) & (2 ** 64 - 1)
    return v - 2 ** 64 if v >= 2 ** 63 else v


def sim_fold_diag(state, diag, wrong, iterations, success, first_frame, T, capture, max_frames, max_errors):
    """ldpc_sim_count_diag on a state of 8 and a diag buffer of diag_words(T, capture) python ints -> (state, diag), both new
    lists.  wrong[b] wrong bits, iterations[b], success[b] of frame first_frame + b."""
    assert len(diag) == diag_words(T, capture)
    out = ref.sim_fold(state, wrong, iterations, max_frames, max_errors)          # the state, stop rule included
    d = [int(v) for v in diag]
    take = out[0] - state[0]                                                      # the block's first `take` frames are consumed
    rec = 4 + T + 1
    for b in range(take):
        w, it, und = int(wrong[b]), int(iterations[b]), int(wrong[b] > 0 and success[b] != 0)
        d[4 + min(max(it, 0), T)] += 1
        if w > 0:
            d[0] += und
            k = d[1]
            if k < capture:
                d[rec + 4 * k:rec + 4 * k + 4] = [signed64(first_frame + b), w, it, und]
                d[1] = k + 1
    return out, d
