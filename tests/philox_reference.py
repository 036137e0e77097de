"""
numpy restatement of the on-device Monte-Carlo definitions (include/ldpc_hip.h, INTEGRATION.md "Noise stream"): the
Philox4x32-10 counter stream, its fp32 uniforms, Box-Muller normals and BI-AWGN LLRs, and the in-order counter fold of
ldpc_sim_count.  Not a test module; tests/test_sim_host.py and the GPU tests import it.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
TWO_PI_F32 = np.float32(6.2831853071795865)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """ten rounds on arrays (or scalars) of 32-bit words held in uint64 -> four uint32 arrays"""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return tuple(v.astype(np.uint32) for v in (c0, c1, c2, c3))


def stream_words(batch, quads, seed, stream_id=0, first_frame=0):
    """uint32 [batch, quads, 4]: the words of quad q of frame first_frame + b"""
    f = (np.uint64(first_frame) + np.arange(batch, dtype=np.uint64))[:, None]      # wraps mod 2^64 like the device
    q = np.arange(quads, dtype=np.uint64)[None, :]
    seed = int(seed) & (2 ** 64 - 1)
    x = philox4x32_10(f & MASK, f >> np.uint64(32), q, np.uint64(int(stream_id) & 0xFFFFFFFF),
                      np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))
    return np.stack(x, axis=-1)


def uniform(x):
    """u(x) = fmaf((float)x, 2^-32, 2^-33) exactly: (float)x rounds to nearest, the product by a power of two and the sum
    are exact in float64 (34 significant bits at most), one rounding to fp32"""
    xf = x.astype(np.float32).astype(np.float64)
    return (xf * 2.0 ** -32 + 2.0 ** -33).astype(np.float32)


def normals(words, n):
    """float64 [batch, n]: z with u and theta in fp32 as defined (exact) and log / sqrt / sin / cos in float64"""
    u = uniform(words)
    zs = []
    for a, b in ((0, 1), (2, 3)):
        r = np.sqrt(-2.0 * np.log(u[..., a].astype(np.float64)))
        theta = (TWO_PI_F32 * u[..., b]).astype(np.float64)          # fp32 product, rounded once
        assert (TWO_PI_F32 * u[..., b]).dtype == np.float32
        zs += [r * np.cos(theta), r * np.sin(theta)]
    z = np.stack(zs, axis=-1).reshape(words.shape[0], -1)
    return z[:, :n]


def awgn_normals(batch, n, seed, stream_id=0, first_frame=0):
    return normals(stream_words(batch, (n + 3) // 4, seed, stream_id, first_frame), n)


def sim_fold(state, frame_wrong, iterations, max_frames, max_errors):
    """ldpc_sim_count on a state of 8 python ints: frame_wrong[b] wrong bits, iterations[b], frames consumed in order"""
    frames, ferrs, berrs, its, done, seen = state[:6]
    out = list(state)
    out[5] = seen + 1
    if done:
        return out
    wrong = np.asarray(frame_wrong, dtype=np.int64)
    itr = np.asarray(iterations, dtype=np.int64)
    take = 0
    for b in range(len(wrong)):                                       # the reference's loop, frame by frame
        if not (frames + take < max_frames and ferrs < max_errors):
            break
        ferrs += int(wrong[b] > 0)
        berrs += int(wrong[b])
        its += int(itr[b])
        take += 1
    frames += take
    out[:5] = [frames, ferrs, berrs, its, int(frames >= max_frames or ferrs >= max_errors)]
    return out


def wrong_bits(packed, n, codeword_packed=None):
    """popcount(packed XOR codeword) over bits < n per row of uint8 [B, ceil(n/8)]"""
    p = np.asarray(packed, dtype=np.uint8)
    if codeword_packed is not None:
        p = p ^ np.asarray(codeword_packed, dtype=np.uint8)[None, :]
    bits = np.unpackbits(p, axis=1, bitorder="little")[:, :n]
    return bits.sum(axis=1, dtype=np.int64)
