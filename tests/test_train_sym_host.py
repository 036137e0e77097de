"""
Host side of training on the symbol channel (no GPU): ``Modulation.amp_table``, what ``PosteriorJointTrainer`` refuses with a
modulation, the argument errors of ``engine.sym_llr_mix`` that need no device, what ``_StreamBlocks`` yields, and the surface
of the native entry point ``ldpc_channel_sym_mix``.
"""
import inspect

import numpy as np
import pytest
import torch

SCHEMES = ("bpsk", "qpsk", "qam16", "qam64", "qam256")


def test_amp_table_is_amp_per_point_cast_to_fp32():
    from modulation import Modulation
    grid = [-3.0, 0.0, 0.5, 4.25, 7.0, 12.5, 30.0]
    for scheme in SCHEMES:
        for fading in (None, "rayleigh"):
            mod = Modulation(scheme, fading)
            tab = mod.amp_table(grid)
            assert isinstance(tab, np.ndarray) and tab.dtype == np.float32 and tab.shape == (len(grid),)
            for p, s in enumerate(grid):
                assert tab[p] == np.float32(mod.amp(s)), (scheme, s)
            assert (np.diff(tab) > 0).all()
    mod = Modulation("qam16")
    assert mod.amp_table(np.array([2.0])).shape == (1,) and mod.amp_table([]).shape == (0,)
    import engine
    assert np.array_equal(mod.amp_table(engine.snr_grid((0.0, 6.0), 0.5)),
                          np.array([np.float32(mod.amp(0.5 * k)) for k in range(13)], dtype=np.float32))
    for bad in (3.0, [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            mod.amp_table(bad)


def small_model():
    import codes
    from neural_2d_decoder import Neural2DMinSumDecoder
    code = codes.load_code("small_96_48", max_iterations=3)
    return code, Neural2DMinSumDecoder(code, 2, 3)


def test_what_the_trainer_refuses():
    from modulation import Modulation
    from rate_matching import RateMatching
    from training_framework import PosteriorJointTrainer, TrainingConfig
    code, model = small_model()
    cfg = TrainingConfig(device="cpu", batch_size=8, num_epochs=1)
    qam, qpsk = Modulation("qam16", "rayleigh"), Modulation("qpsk")
    rm = RateMatching(code.n, punctured=[0, 1])
    word = np.zeros(code.n, dtype=np.uint8)
    with pytest.raises(ValueError, match="rate_matching"):
        PosteriorJointTrainer(model, cfg, rate_matching=rm, modulation=qam, codeword="random")
    with pytest.raises(ValueError, match="llr_convention"):
        PosteriorJointTrainer(model, TrainingConfig(device="cpu", llr_convention="reference"), modulation=qam, codeword="random")
    for scheme in ("qam16", "qam64", "qam256"):
        with pytest.raises(ValueError, match="all-zero"):
            PosteriorJointTrainer(model, cfg, modulation=Modulation(scheme))
    with pytest.raises(ValueError, match="needs a modulation"):
        PosteriorJointTrainer(model, cfg, codeword="random")
    with pytest.raises(ValueError, match="needs a modulation"):
        PosteriorJointTrainer(model, cfg, codeword=word)
    with pytest.raises(ValueError, match="modulation.Modulation"):
        PosteriorJointTrainer(model, cfg, modulation="qam16", codeword="random")
    with pytest.raises(ValueError, match="codeword"):
        PosteriorJointTrainer(model, cfg, modulation=qam, codeword="zero")
    with pytest.raises(ValueError, match="codeword"):
        PosteriorJointTrainer(model, cfg, modulation=qam, codeword=np.full(code.n, 2))
    # what it accepts: the all-zero word under BPSK / QPSK, a word or random words under every scheme
    for mod, cw in ((qpsk, None), (Modulation("bpsk", "rayleigh"), None), (qam, "random"), (qam, word), (qpsk, "random")):
        trainer = PosteriorJointTrainer(model, cfg, modulation=mod, codeword=cw)
        assert trainer.modulation is mod and trainer.rate_matching is None
        with pytest.raises(ValueError, match="train_stream"):
            trainer.train(code, 8, 8)
    plain = PosteriorJointTrainer(model, cfg)
    assert plain.modulation is None and plain.codeword is None


def test_the_constructor_keeps_its_positional_surface():
    from training_framework import PosteriorJointTrainer
    P = inspect.Parameter
    # the call takes the two new keywords, keyword only, and hands everything else to __init__, which keeps the list it had
    call = inspect.signature(PosteriorJointTrainer).parameters
    for name in ("modulation", "codeword"):
        assert call[name].kind is P.KEYWORD_ONLY and call[name].default is None
    with pytest.raises(TypeError):
        PosteriorJointTrainer(None, None, None)                        # rate_matching stays keyword only
    assert list(inspect.signature(PosteriorJointTrainer.__init__).parameters) == ["self", "model", "config", "rate_matching"]


def test_sym_llr_mix_argument_errors_need_no_device():
    """every refusal below is raised before a device is asked for, so it is a ValueError with or without a GPU"""
    import engine
    from modulation import Modulation
    mod = Modulation("qam16")
    kw = dict(seed=1, modulation=mod)
    with pytest.raises(ValueError, match="either snr_db or amp"):
        engine.sym_llr_mix(4, 96, **kw)
    with pytest.raises(ValueError, match="either snr_db or amp"):
        engine.sym_llr_mix(4, 96, snr_db=[1.0, 2.0], amp=[1.0, 2.0], **kw)
    with pytest.raises(ValueError, match="modulation"):
        engine.sym_llr_mix(4, 96, seed=1, modulation="qam16", snr_db=[1.0])
    for k in (0, engine.MIX_MAX_POINTS + 1):
        with pytest.raises(ValueError, match="number of SNR points"):
            engine.sym_llr_mix(4, 96, snr_db=np.zeros(k), **kw)
        with pytest.raises(ValueError, match="number of SNR points"):
            engine.sym_llr_mix(4, 96, amp=np.ones(k), **kw)
        with pytest.raises(ValueError, match="number of SNR points"):
            engine.sym_llr_mix(4, 96, amp=torch.ones(k), **kw)
    with pytest.raises(ValueError, match="1-D"):
        engine.sym_llr_mix(4, 96, snr_db=[[1.0, 2.0]], **kw)
    with pytest.raises(ValueError, match="1-D"):
        engine.sym_llr_mix(4, 96, amp=[[1.0, 2.0]], **kw)
    for bad in ([1.0, -0.5], [1.0, float("nan")], [float("inf")]):
        with pytest.raises(ValueError, match="finite"):
            engine.sym_llr_mix(4, 96, amp=bad, **kw)
    with pytest.raises(ValueError, match="batch"):
        engine.sym_llr_mix(-1, 96, snr_db=[1.0], **kw)
    with pytest.raises(ValueError, match="batch"):
        engine.sym_llr_mix(2 ** 31, 96, snr_db=[1.0], **kw)
    with pytest.raises(ValueError, match="n >= 1"):
        engine.sym_llr_mix(4, 0, snr_db=[1.0], **kw)


def test_stream_blocks_yield_what_the_draw_returns():
    from training_framework import _StreamBlocks
    calls, steps = [], []
    llr, targets = torch.zeros(2, 3), torch.ones(2, 3)

    def bare(first, frames):
        calls.append((first, frames))
        return llr

    blocks = _StreamBlocks([(0, 2), (64, 2)], bare, lambda: steps.append(len(calls)))
    assert len(blocks) == 2
    got = list(blocks)
    assert calls == [(0, 2), (64, 2)] and steps == [1, 2]
    assert all(isinstance(g, tuple) and len(g) == 2 and g[0] is llr and g[1] is None for g in got)

    got = list(_StreamBlocks([(5, 2)], lambda first, frames: (llr, targets)))
    assert len(got) == 1 and got[0][0] is llr and got[0][1] is targets


def test_native_binding_declares_the_entry_point():
    import _native
    header = open(_native.HEADER).read()
    assert "ldpc_channel_sym_mix" in _native.PRODUCT_EXPORTS and "int ldpc_channel_sym_mix(" in header
    assert "training on this channel" not in header
    lib = _native.load()
    assert lib.ldpc_abi_version() == 1
    assert len(lib.ldpc_channel_sym_mix.argtypes) == 13
    import ctypes as C
    mod = C.byref(_native.ModulationDesc(bits_per_symbol=4, fading=1, amp=float("nan")))       # mod->amp is ignored
    call = lambda batch, md, k, stride=0: lib.ldpc_channel_sym_mix(None, batch, 8, 0, 0, 0, md, None, k, None, stride, None, None)
    # an empty block touches no pointer, and the scalar checks come before it: no device is needed for either
    assert call(0, mod, 1) == 0 and call(0, mod, 4096) == 0 and call(0, mod, 13, 1) == 0
    for k in (0, 4097, -1):
        assert call(0, mod, k) == -1 and b"n_points" in lib.ldpc_last_error()
    assert call(0, mod, 13, 2) == -1 and b"codeword_stride" in lib.ldpc_last_error()
    assert call(0, None, 13) == -1 and b"mod" in lib.ldpc_last_error()
    assert call(0, C.byref(_native.ModulationDesc(bits_per_symbol=3)), 13) == -1 and b"bits_per_symbol" in lib.ldpc_last_error()
    assert call(-1, mod, 13) == -1
    assert call(2 ** 31, mod, 13) == -1 and b"2^31" in lib.ldpc_last_error()
    assert call(1, mod, 13) == -1 and b"amp_tab" in lib.ldpc_last_error()                      # NULL table, batch > 0
