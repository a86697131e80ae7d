"""CPU: the exponential moving average of the parameters (efficient_tts_amd/ema.py) -- everything that needs no device: the host half of
the C ABI (efts_ema_hyper against the Python-float formula of tests/ema_reference.py, the argument errors of both exports), the ABI
checks over the new exports, and every refusal that is decided before a launch: `ParamEMA`, `bin/train`'s `ema_decay` and the
`--use_ema` of bin/inference and bin/score."""
import ctypes as C
import importlib.util
import os

import pytest
import torch

import ema_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from efficient_tts_amd import build as B, lib as L
    B.build(verbose=False)
    return L.load()


# around where (1 + n) / (10 + n) crosses 0.999 (n = 8990: 8991 / 9000 = 0.999 exactly in the rationals), and far behind it
UPDATES = [0, 1, 8, 89, 8990, 8991, 10 ** 9]


@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("updates", UPDATES)
def test_ema_hyper_equals_a_python_computation(lib, updates, warmup):
    """the one word, bit for bit the Python-float computation rounded to fp32 once"""
    arr = (C.c_float * 1)()
    for decay in (0.999, 0.9, 0.0, 0.9999):
        assert lib.efts_ema_hyper(decay, int(warmup), updates, arr) == 0
        assert arr[0] == R.word(decay, warmup, updates), (decay, updates)
        assert 0.0 <= arr[0] <= 1.0
    # what the numbers are: the first warmed-up update takes 9/10 of p, the ramp is over from update 8991 on
    assert lib.efts_ema_hyper(0.999, 1, 0, arr) == 0 and arr[0] == R.f32(1.0 - 0.1)
    assert R.decay_at(0.999, True, 8989) < 0.999 and R.decay_at(0.999, True, 8991) == 0.999
    assert R.decay_at(0.999, False, 0) == 0.999


def test_new_symbols_pass_the_abi_checks(lib):
    """tests/test_abi_cpu.py's own checks, unchanged, see the new exports; the revision stays"""
    from efficient_tts_amd import lib as L
    spec = importlib.util.spec_from_file_location("abi_checks", os.path.join(ROOT, "tests", "test_abi_cpu.py"))
    abi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(abi)
    abi.test_header_symbols_are_exported(lib)
    abi.test_version_and_argument_errors(lib)
    abi.test_args_layouts_match_header()
    assert {"efts_ema_update", "efts_ema_hyper"} <= set(L.exported_symbols()) and L.ABI_VERSION == 602 == lib.efts_version()
    assert C.sizeof(L.OptimArgs) == 128            # the optimizer's argument block did not grow for it (test_args_layouts_match_header
                                                   # above holds the mirror against the header)


def test_argument_errors_come_before_any_launch(lib):
    arr = (C.c_float * 1)()
    for bad in ((0.999, 1, 0, None), (1.0, 1, 0, arr), (-0.1, 0, 0, arr), (float("nan"), 0, 0, arr), (0.999, 1, -1, arr)):
        assert lib.efts_ema_hyper(*bad) == -1, bad
    assert b"efts_ema_hyper" in lib.efts_last_error()
    e, p = 4096, 8192
    for bad in ((None, p, 8, 0.5), (e, None, 8, 0.5), (e, p, 0, 0.5), (e, p, -3, 0.5), (e, p, 8, -0.25), (e, p, 8, 1.5), (e, p, 8, float("nan"))):
        assert lib.efts_ema_update(*bad, None) == -1, bad
    assert b"efts_ema_update" in lib.efts_last_error()
    for bad in ((e + 4, p, 8, 0.5), (e, p + 8, 8, 0.5)):
        assert lib.efts_ema_update(*bad, None) == -3, bad


def _small_model():
    from efficient_tts_amd import EfficientTTSCNN
    return EfficientTTSCNN(num_symbols=76, symbol_embedding_dim=256, n_channels=256, n_text_encoder_layer=1, n_mel_encoder_layer=1,
                           n_decoder_layer=1, dropout_rate=0.0, use_masking=True)


def test_param_ema_refusals():
    """a stock optimizer is a TypeError, a decay outside (0, 1) a ValueError, and without a device the constructor fails loudly: there is
    no host form of the update"""
    from efficient_tts_amd import lib as L, optimizers
    from efficient_tts_amd.ema import ParamEMA
    model = _small_model()
    with pytest.raises(TypeError, match="FlatOptimizer"):
        ParamEMA(torch.optim.Adam(model.parameters()))
    opt = optimizers.Adam(model)
    assert opt.ema is None
    for decay in (0.0, 1.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="decay"):
            ParamEMA(opt, decay=decay)
    if not torch.cuda.is_available():
        with pytest.raises(L.EftsError, match="device"):
            ParamEMA(opt)
        assert opt.ema is None


def test_train_refuses_a_bad_ema_decay_and_a_stock_optimizer():
    from efficient_tts_amd.bin.train import build_ema
    assert build_ema({}) is None and build_ema(dict(ema_decay=0.999)) is None and build_ema(dict(ema_decay=0.9, ema_warmup=False)) is None
    for decay in (0.0, 1.0, 1.5, -0.1, True, "0.999"):
        with pytest.raises(ValueError, match="ema_decay"):
            build_ema(dict(ema_decay=decay))
    with pytest.raises(ValueError, match="ema_warmup"):
        build_ema(dict(ema_decay=0.999, ema_warmup=3))
    with pytest.raises(ValueError, match="ema_warmup"):
        build_ema(dict(ema_warmup=True))
    model = _small_model()
    with pytest.raises(ValueError) as err:
        build_ema(dict(ema_decay=0.999, optimizer_type="SGD"), torch.optim.SGD(model.parameters(), lr=0.1))
    assert "ema_decay" in str(err.value) and "SGD" in str(err.value)          # the message names both


@pytest.mark.parametrize("tool", ["inference", "score"])
def test_use_ema_is_a_flag_and_fails_loudly(tmp_path, tool):
    import importlib
    from efficient_tts_amd.bin.inference import averaged_weights
    mod = importlib.import_module(f"efficient_tts_amd.bin.{tool}")
    common = ["--checkpoint", str(tmp_path / "checkpoint-3steps.pkl"), "--test_fid_scp", "t.txt", "--outdir", str(tmp_path / "o")]
    assert mod.get_parser().parse_args(common).use_ema is False
    assert mod.get_parser().parse_args(common + ["--use_ema"]).use_ema is True
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            mod.main(common + ["--use_ema"])
    # a checkpoint as a run without `ema_decay` writes it
    plain = dict(model={"w": torch.zeros(2)}, optimizer={}, scheduler={}, steps=3, epochs=0)
    with pytest.raises(ValueError, match="ema_decay"):
        averaged_weights(plain, "checkpoint-3steps.pkl")
    with pytest.raises(ValueError, match="ema_decay"):
        averaged_weights(dict(plain, ema=dict(decay=0.9)), "checkpoint-3steps.pkl")
    avg = {"w": torch.ones(2)}
    assert averaged_weights(dict(plain, ema=dict(decay=0.9, warmup=True, updates=3, model=avg))) is avg
