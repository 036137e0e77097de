"""
numpy restatement of the information-bit stream of ldpc_encode_random (include/ldpc_hip.h, INTEGRATION.md "Information-bit
stream") and the small parity-check matrices the encoder tests share.  Not a test module; tests/test_encode_host.py and
tests/test_gpu_encode.py import it.
"""
import numpy as np

import philox_reference as ref

TOY_PERMUTATION = [3, 4, 5, 6, 0, 1, 2]      # the toy's last four columns become dependent: scattered positions


def toy_H(kind="toy"):
    """the reference's 4 x 7 toy matrix; "reversed": its columns reversed; "permuted": columns TOY_PERMUTATION (information
    and parity positions interleave); "deficient": the sum of rows 0 and 2 appended (rank stays 4)"""
    from ldpc_decoder import create_test_ldpc_code
    H = np.asarray(create_test_ldpc_code().H, dtype=np.int64)
    if kind == "reversed":
        return H[:, ::-1].copy()
    if kind == "permuted":
        return H[:, TOY_PERMUTATION].copy()
    if kind == "deficient":
        return np.vstack([H, H[0] ^ H[2]])
    assert kind == "toy"
    return H


def toy_graph(kind="toy"):
    from tanner_graph import TannerGraph
    return TannerGraph.from_dense(toy_H(kind))


def info_bits(batch, k, seed, stream_id=0, first_frame=0):
    """uint8 [batch, k]: information bit i of frame first_frame + b is bit i % 32 of word x[(i / 32) % 4] of
    Philox4x32-10(counter = (f lo, f hi, 0x80000000 | (i / 128), stream_id), key = (seed lo, seed hi))"""
    f = (np.uint64(first_frame) + np.arange(batch, dtype=np.uint64))[:, None]      # wraps mod 2^64 like the device
    calls = np.arange((k + 127) // 128, dtype=np.uint64)[None, :]
    seed = int(seed) & (2 ** 64 - 1)
    x = ref.philox4x32_10(f & ref.MASK, f >> np.uint64(32), np.uint64(0x80000000) | calls,
                          np.uint64(int(stream_id) & 0xFFFFFFFF), np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))
    words = np.stack(x, axis=-1).reshape(batch, -1)                                # uint32 [batch, 4 * calls]
    bits = (words[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & np.uint32(1)
    return bits.reshape(batch, -1)[:, :k].astype(np.uint8)


def pack_rows(bits):
    """0/1 [B, n] -> uint8 [B, ceil(n/8)], bit j at byte j/8, bit j%8, pad bits 0"""
    return np.packbits(np.asarray(bits, dtype=np.uint8), axis=1, bitorder="little")


def unpack_rows(packed, n):
    return np.unpackbits(np.asarray(packed, dtype=np.uint8), axis=1, bitorder="little")[:, :n]
