"""
Host side of stream training (no GPU): the SNR grid, the frame ranges of the steps, the point of a frame, the operator
``ldpc::awgn_llr_mix`` and the surface of ``PosteriorJointTrainer.train_stream``.
"""
import dataclasses
import inspect

import numpy as np
import pytest
import torch


def test_snr_grid():
    import engine
    g = engine.snr_grid((0.0, 6.0), 0.5)
    assert g.dtype == np.float64 and len(g) == 13
    np.testing.assert_array_equal(g, 0.5 * np.arange(13))
    g = engine.snr_grid((1.0, 4.0), 0.5)
    np.testing.assert_array_equal(g, [1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0])
    for step in (0.5, 0.1, 7.0):
        np.testing.assert_array_equal(engine.snr_grid((3.0, 3.0), step), [3.0])
    # a step the range is no whole multiple of stops below hi; one that float division lands just under a whole number keeps its
    # last point
    np.testing.assert_array_equal(engine.snr_grid((0.0, 1.0), 0.4), [0.0, 0.4, 0.8])
    assert len(engine.snr_grid((0.0, 0.3), 0.1)) == 4
    for step in (0.0, -0.5):
        with pytest.raises(ValueError):
            engine.snr_grid((0.0, 6.0), step)
    with pytest.raises(ValueError):
        engine.snr_grid((4.0, 1.0), 0.5)


@pytest.mark.parametrize("world", [1, 3])
def test_stream_first_frame_tiles_the_stream(world):
    from training_framework import stream_first_frame
    B, steps = 64, 5
    firsts = sorted(stream_first_frame(g, B, r, world) for g in range(steps) for r in range(world))
    assert firsts == [k * B for k in range(steps * world)]           # disjoint [first, first + B) that tile [0, 5 w B)
    for g in range(steps):                                           # a step's ranks draw consecutive blocks
        assert [stream_first_frame(g, B, r, world) for r in range(world)] == [(g * world + r) * B for r in range(world)]
    assert stream_first_frame(2 ** 40, 4096, 7, 8) == (2 ** 40 * 8 + 7) * 4096      # Python integers: no 64-bit wrap
    with pytest.raises(ValueError):
        stream_first_frame(0, B, world, world)
    with pytest.raises(ValueError):
        stream_first_frame(-1, B, 0, world)


def test_mix_points_above_two_to_the_63():
    import engine
    first, K = 2 ** 63 + 5, 13
    p = engine.mix_points(first, 40, K)
    assert p.dtype == torch.int64 and p.shape == (40,) and p.device.type == "cpu"
    assert p.tolist() == [(first + b) % K for b in range(40)]
    assert engine.mix_points(0, 100, 7).bincount(minlength=7).tolist() == [15, 15, 14, 14, 14, 14, 14]
    assert engine.mix_points(2 ** 64 - 3, 3, 4096).tolist() == [(2 ** 64 - 3 + b) % 4096 for b in range(3)]
    assert engine.mix_points(9, 0, 3).shape == (0,)
    with pytest.raises(ValueError):
        engine.mix_points(0, 4, 0)


def test_operator_is_registered_with_its_schema():
    import torch_ops  # noqa: F401
    schema = str(torch.ops.ldpc.awgn_llr_mix.default._schema).replace("SymInt", "int")     # custom_op registers int as SymInt
    assert schema == ("ldpc::awgn_llr_mix(int batch, int n, int seed, int stream_id, int first_frame, "
                      "Tensor scale_tab, Tensor shift_tab, Tensor? codeword_packed, Device device) -> Tensor"), schema


def test_native_binding_declares_the_entry_point():
    import _native
    assert "ldpc_channel_awgn_mix" in _native.PRODUCT_EXPORTS
    assert "int ldpc_channel_awgn_mix(" in open(_native.HEADER).read()
    lib = _native.load()
    assert len(lib.ldpc_channel_awgn_mix.argtypes) == 11
    # an empty block touches no pointer, and the argument checks come before it: no device is needed for either
    assert lib.ldpc_channel_awgn_mix(None, 0, 8, 0, 0, 0, None, None, 1, None, None) == 0
    assert lib.ldpc_channel_awgn_mix(None, 0, 8, 0, 0, 0, None, None, 0, None, None) == -1 and b"n_points" in lib.ldpc_last_error()


def test_training_config_is_unchanged():
    from training_framework import TrainingConfig
    assert [f.name for f in dataclasses.fields(TrainingConfig)] == [
        "batch_size", "num_epochs", "learning_rate", "snr_range", "snr_step", "max_grad_norm", "use_posterior_training",
        "use_gradient_clipping", "clip_threshold", "device", "llr_convention", "data_parallel", "seed", "joint_posterior_loss"]


def test_train_stream_signature():
    from training_framework import PosteriorJointTrainer
    sig = inspect.signature(PosteriorJointTrainer.train_stream)
    kinds = [(p.name, p.kind, p.default) for p in sig.parameters.values()]
    P = inspect.Parameter
    assert kinds == [("self", P.POSITIONAL_OR_KEYWORD, P.empty), ("code", P.POSITIONAL_OR_KEYWORD, P.empty),
                     ("steps_per_epoch", P.POSITIONAL_OR_KEYWORD, P.empty), ("val_frames", P.POSITIONAL_OR_KEYWORD, 0),
                     ("train_stream_id", P.KEYWORD_ONLY, 0), ("val_stream_id", P.KEYWORD_ONLY, 1)]


def test_no_targets_is_the_all_zero_codeword():
    from training_framework import _frames_ok
    decoded = torch.tensor([[0, 0, 0], [0, 1, 0], [0, 0, 0]], dtype=torch.int32)
    assert _frames_ok(decoded, None).tolist() == [True, False, True] == _frames_ok(decoded, torch.zeros(3, 3)).tolist()
