"""
On-device Monte-Carlo, host side (no GPU): the numpy restatement of the noise stream against published Philox4x32-10
answers, the restated counter fold against frames_to_count, the moments of the restated normals, SimulationConfig's new
fields and the exports.
"""
import dataclasses

import numpy as np
import pytest

import philox_reference as ref


@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, out):
    got = ref.philox4x32_10(*ctr, *key)
    assert tuple(int(v) for v in got) == out


def test_stream_words_use_the_frame_as_a_64_bit_counter():
    """counter = (f & 0xffffffff, f >> 32, quad, stream_id), key = (seed & 0xffffffff, seed >> 32)"""
    seed, sid, first = 0x0123456789abcdef, 77, 2 ** 32 - 2
    w = ref.stream_words(4, 3, seed, sid, first)
    assert w.shape == (4, 3, 4) and w.dtype == np.uint32
    for b in range(4):
        f = first + b
        for q in range(3):
            one = ref.philox4x32_10(f & 0xffffffff, f >> 32, q, sid, seed & 0xffffffff, seed >> 32)
            assert [int(v) for v in one] == [int(v) for v in w[b, q]]
    assert not np.array_equal(w[1], w[2])                        # 2^32 - 1 -> 2^32: the high word changes
    np.testing.assert_array_equal(ref.stream_words(2, 3, seed, sid, first + 1), w[1:3])


def test_uniforms_lie_in_the_half_open_unit_interval():
    x = np.array([0, 1, 2 ** 24 - 1, 2 ** 31, 2 ** 32 - 129, 2 ** 32 - 1], dtype=np.uint32)
    u = ref.uniform(x)
    assert u.dtype == np.float32 and u[0] == np.float32(2.0 ** -33) and u[-1] == np.float32(1.0)
    assert (u > 0).all() and (u <= 1).all()
    assert np.sqrt(-2.0 * np.log(2.0 ** -33)) < 6.77             # the tails end at 6.76 sigma


def test_moments_of_the_restated_normals():
    N = 10 ** 6
    z = ref.awgn_normals(500, 2000, seed=2024, stream_id=3000)
    assert z.shape == (500, 2000) and z.size == N
    tol = 5.0 / np.sqrt(N)
    assert abs(z.mean()) <= tol
    assert abs(z.var() - 1.0) <= tol                             # 3.5 standard deviations of a sample variance (sqrt(2 / N))
    assert abs((z ** 2).mean() - 1.0) <= tol
    assert np.abs(z).max() <= 6.76


def _frames_to_count_fold(state, wrong, iters, max_frames, max_errors):
    """the driver's host path: frames_to_count and the three sums"""
    from simulation_framework import frames_to_count
    frames, ferrs, berrs, its, done, seen = state[:6]
    out = list(state)
    out[5] = seen + 1
    if done:
        return out
    ferr = np.asarray(wrong) > 0
    take = frames_to_count(ferr, frames, ferrs, max_frames, max_errors)
    frames += take
    ferrs += int(ferr[:take].sum())
    berrs += int(np.asarray(wrong)[:take].sum())
    its += int(np.asarray(iters)[:take].sum())
    out[:5] = [frames, ferrs, berrs, its, int(frames >= max_frames or ferrs >= max_errors)]
    return out


def test_restated_fold_equals_frames_to_count():
    rng = np.random.default_rng(11)
    for trial in range(300):
        p = rng.choice([0.0, 0.02, 0.3, 1.0])
        max_frames, max_errors = int(rng.integers(1, 3000)), int(rng.integers(0, 40))
        a = b = [0] * 8
        while not a[4]:
            B = int(rng.integers(1, 600))
            wrong = (rng.random(B) < p) * rng.integers(1, 50, B)
            iters = rng.integers(1, 11, B)
            a = ref.sim_fold(a, wrong, iters, max_frames, max_errors)
            b = _frames_to_count_fold(b, wrong, iters, max_frames, max_errors)
            assert a == b
        assert a[0] <= max_frames and (a[0] == max_frames or a[1] >= max_errors)
        again = ref.sim_fold(a, np.ones(5), np.ones(5), max_frames, max_errors)
        assert again == a[:5] + [a[5] + 1, 0, 0]


# (state before, wrong bits per frame, max_frames, max_errors) -> (frames, frame_errors, bit_errors, iterations, done)
ADVERSARIAL = {
    "frames_limit_mid_block": ([95, 2, 9, 400, 0, 3, 0, 0], [0, 3, 0, 0, 0, 1, 0, 1, 0, 0], 100, 50, [100, 3, 12, 415, 1]),
    "error_limit_on_last_frame": ([10, 4, 20, 60, 0, 1, 0, 0], [0, 0, 0, 7], 1000, 5, [14, 5, 27, 70, 1]),
    "error_limit_mid_block": ([10, 3, 20, 60, 0, 1, 0, 0], [1, 0, 2, 0, 5, 5], 1000, 5, [13, 5, 23, 66, 1]),
    "already_done": ([14, 5, 27, 70, 1, 2, 0, 0], [1, 1, 1], 1000, 5, [14, 5, 27, 70, 1]),
    "limits_met_without_the_flag": ([100, 0, 0, 300, 0, 1, 0, 0], [1, 1, 1], 100, 5, [100, 0, 0, 300, 1]),
    "max_errors_zero": ([0] * 8, [0, 4, 0], 100, 0, [0, 0, 0, 0, 1]),
}


@pytest.mark.parametrize("name", sorted(ADVERSARIAL))
def test_restated_fold_on_adversarial_blocks(name):
    state, wrong, max_frames, max_errors, want = ADVERSARIAL[name]
    iters = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10][:len(wrong)]
    got = ref.sim_fold(state, wrong, iters, max_frames, max_errors)
    assert got[:5] == want and got[5] == state[5] + 1 and got[6:] == [0, 0]
    assert got == _frames_to_count_fold(state, wrong, iters, max_frames, max_errors)


def test_wrong_bits_ignore_the_pad_bits():
    rng = np.random.default_rng(5)
    for n in (7, 96, 1998):
        bits = (rng.random((9, n)) < 0.4).astype(np.uint8)
        cw = (rng.random(n) < 0.5).astype(np.uint8)
        pad = np.ones((9, (-n) % 8), np.uint8)
        packed = np.packbits(np.concatenate([bits, pad], axis=1), axis=1, bitorder="little")
        np.testing.assert_array_equal(ref.wrong_bits(packed, n), bits.sum(axis=1))
        cwp = np.packbits(cw, bitorder="little")
        np.testing.assert_array_equal(ref.wrong_bits(packed, n, cwp), (bits ^ cw[None, :]).sum(axis=1))


def test_simulation_config_channel_and_codeword():
    from simulation_framework import SimulationConfig
    cfg = SimulationConfig()
    assert cfg.channel == "torch" and cfg.codeword is None       # the default path is the torch.randn one, unchanged
    names = [f.name for f in dataclasses.fields(SimulationConfig)]
    assert names[:14] == ["snr_range", "snr_step", "max_frames", "max_errors", "min_frames", "parallel_workers", "device",
                          "save_results", "results_dir", "batch_frames", "seed", "llr_convention", "staged_early_stop",
                          "stage_min_block"]
    assert SimulationConfig(channel="device").channel == "device"
    for bad in ("cuda", "Device", "", "philox"):
        with pytest.raises(ValueError):
            SimulationConfig(channel=bad)
    cw = np.zeros(96, dtype=np.uint8)
    assert SimulationConfig(channel="device", codeword=cw).codeword is cw
    with pytest.raises(ValueError):
        SimulationConfig(codeword=cw)
    with pytest.raises(ValueError):
        SimulationConfig(channel="torch", codeword=cw)


def test_scale_and_shift_of_the_two_conventions():
    import engine
    scale, shift = engine.awgn_scale_shift(3.0)
    s2 = 10.0 ** (-0.3)
    assert scale == pytest.approx(2.0 / s2 ** 0.5, rel=1e-14) and shift == pytest.approx(2.0 / s2, rel=1e-14)
    assert engine.awgn_scale_shift(3.0, "reference") == (scale, -shift)
    with pytest.raises(ValueError):
        engine.awgn_scale_shift(3.0, "other")


def test_exports_and_descriptor_layout():
    import ctypes

    import _native
    for name in ("ldpc_channel_awgn", "ldpc_sim_count", "ldpc_simulate_workspace_bytes", "ldpc_simulate"):
        assert name in _native.PRODUCT_EXPORTS
    assert "ldpc_debug_philox" in _native.DEBUG_EXPORTS
    assert "ldpc_sim.hip" in _native.SOURCES
    d = _native.SimDesc
    assert [f[0] for f in d._fields_] == ["seed", "stream_id", "first_frame", "scale", "shift", "codeword_packed",
                                          "max_frames", "max_errors", "block", "poll_blocks"]
    assert (d.seed.offset, d.stream_id.offset, d.first_frame.offset, d.scale.offset, d.shift.offset) == (0, 8, 16, 24, 28)
    assert (d.codeword_packed.offset, d.max_frames.offset, d.max_errors.offset, d.block.offset, d.poll_blocks.offset) == \
        (32, 40, 48, 56, 64) and ctypes.sizeof(d) == 72
    lib = _native.load()
    assert len(lib.ldpc_channel_awgn.argtypes) == 10 and len(lib.ldpc_sim_count.argtypes) == 9
    assert len(lib.ldpc_simulate.argtypes) == 6 and len(lib.ldpc_debug_philox.argtypes) == 7


def test_torch_operator_is_registered():
    import torch

    import torch_ops  # noqa: F401
    assert hasattr(torch.ops.ldpc, "awgn_llr")
