"""CPU: the IIR filter's reference against scipy where it is installed, the block-carry scheme against the sequential definition on the inputs
of tests/test_iir_gpu.py, the closed-form designs, and every refusal of the class, the recipe keys and the command lines.  No device."""
import math
import os
import re

import numpy as np
import pytest
import torch

import iir_reference as R

from efficient_tts_amd import iir as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _filters():
    return {
        "highpass60_order2": S.highpass_sos(R.RATE, 60.0, 2),
        "highpass20_order4": S.highpass_sos(R.RATE, 20.0, 4),
        "deemphasis097": S.deemphasis_sos(0.97),
        "pre_then_deemphasis097": np.concatenate([S.preemphasis_sos(0.97), S.deemphasis_sos(0.97)]),
    }


def _response(sos, f, rate=R.RATE):
    z = np.exp(-2j * np.pi * np.asarray(f, dtype=np.float64) / rate)
    h = np.ones_like(z)
    for b0, b1, b2, a1, a2 in sos:
        h = h * (b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z)
    return h


def test_sequential_reference_agrees_with_scipy_sosfilt():
    signal = pytest.importorskip("scipy.signal")
    x = np.random.default_rng(0).standard_normal(5000)
    for name, sos in _filters().items():
        sos6 = np.insert(sos, 3, 1.0, axis=1)
        assert np.abs(R.sequential(x, sos) - signal.sosfilt(sos6, x)).max() <= 1e-12, name


@pytest.mark.parametrize("name", list(_filters()))
def test_block_carry_agrees_with_the_sequential_reference_on_the_gpu_tests_inputs(name):
    """to 1e-10 of the peak in float64; and rounded to fp32 it stays inside the bound that the device is held to"""
    sos = S.check_sos(_filters()[name])
    m = S.cached_powers(sos)
    assert m.shape == (6, 2 * len(sos), 2 * len(sos)) and np.array_equal(m, R.powers(sos))     # the product's matrices are the restatement's
    audio, lengths = R.batch(False)
    ref = R.reference(sos)
    worst, unequal = 0.0, 0
    for b, n in enumerate(lengths):
        y = R.block_carry(audio[b, :n], sos, m)
        assert y.shape == ref[b].shape
        if n:
            worst = max(worst, float(np.abs(y - ref[b]).max()))
            y32 = y.astype(np.float32)
            assert np.all(np.abs(y32.astype(np.float64) - ref[b]) <= R.bound(ref[b])), (name, b)
            unequal += int(np.count_nonzero(y32 != ref[b].astype(np.float32)))
    print(f"{name}: max |block carry - sequential| = {worst:.3e} in float64; {unequal} elements round to another fp32 value")
    assert worst <= 1e-10 * R.PEAK


def test_the_batch_is_what_the_issue_describes():
    audio, lengths = R.batch(False)
    assert tuple(lengths) == (0, 1, 255, 256, 257, 16383, 16384, 16385, 12345, 40000) and audio.shape == (10, R.N) and R.N % 4
    x = R.signal().astype(np.float64)
    for i in R.IMPULSES:
        x[i] -= 1.0
    assert 0.45 < np.abs(x).max() <= R.PEAK and abs(x.mean() - 0.1) < 0.01
    pcm, _ = R.batch(True)
    assert pcm.dtype == np.int16 and np.array_equal(R.twin(pcm).astype(np.float64) * 32768.0, pcm.astype(np.float64))


def test_highpass_design():
    for order in (2, 4):
        for rate, fc in ((22050, 60.0), (22050, 20.0), (48000, 1000.0), (16000, 3999.0)):
            sos = S.highpass_sos(rate, fc, order)
            assert sos.shape == (order // 2, 5) and sos.dtype == np.float64
            S.check_sos(sos)
            assert abs(20.0 * math.log10(abs(_response(sos, [fc], rate)[0])) + 10.0 * math.log10(2.0)) <= 1e-9, (order, rate, fc)
            for b0, b1, b2, a1, a2 in sos:
                assert b0 + b1 + b2 == 0.0                                   # the magnitude at DC is exactly 0
            grid = np.linspace(0.0, rate / 2.0, 256)
            mag = np.abs(_response(sos, grid, rate))
            # monotone up to the rounding of the evaluation itself: some ten float64 operations per section on values of magnitude <= 1
            assert mag[0] == 0.0 and np.all(np.diff(mag) >= -16 * 2.0 ** -52) and abs(mag[-1] - 1.0) < 1e-12
    # order 4: the product of two sections with the Butterworth Q values 1 / (2 cos(pi / 8)) and 1 / (2 cos(3 pi / 8))
    k = math.tan(math.pi * 20.0 / 22050)
    sos = S.highpass_sos(22050, 20.0, 4)
    for (b0, b1, b2, a1, a2), q in zip(sos, (0.5411961001461969, 1.3065629648763766)):
        n = 1.0 + k / q + k * k
        assert np.allclose([b0, b1, b2, a1, a2], [1 / n, -2 / n, 1 / n, 2 * (k * k - 1) / n, (1 - k / q + k * k) / n], rtol=1e-14, atol=0)
    f = np.array([5.0, 20.0, 100.0, 3000.0])
    assert np.allclose(np.abs(_response(sos, f)), 1.0 / np.sqrt(1.0 + (np.tan(np.pi * 20.0 / 22050) / np.tan(np.pi * f / 22050)) ** 8), rtol=1e-9)
    assert np.array_equal(S.highpass_sos(22050, 60), S.highpass_sos(22050, 60.0, 2))
    for args in ((22050, 0.0), (22050, -5.0), (22050, 11025.0), (22050, 20000.0), (22050, float("nan")), (22050, 60.0, 3), (22050, 60.0, 6),
                 (22050, "60"), (0, 60.0), (22050, True)):
        with pytest.raises(ValueError):
            S.highpass_sos(*args)


def test_stability_check_and_sos_layouts():
    good = [[1.0, 0.0, 0.0, -1.8, 0.81]]
    assert S.check_sos(good).shape == (1, 5)
    assert np.array_equal(S.check_sos([[1.0, 0.0, 0.0, 1.0, -1.8, 0.81]]), S.check_sos(good))        # scipy's layout
    for bad in ([[1.0, 0.0, 0.0, -2.0, 1.0]],            # a double pole on the unit circle
                [[1.0, 0.0, 0.0, 0.0, 1.0]],             # poles at +-i
                [[1.0, 0.0, 0.0, -2.1, 1.08]],           # a pole at 1.2
                [[1.0, 0.0, 0.0, -1.0, 0.0]],            # the integrator: a pole at 1
                [[1.0, 0.0, 0.0, 0.0, -1.5]],
                [[1.0, 0.0, 0.0, 2.0, -1.8, 0.81]],      # a0 != 1
                [[1.0, 0.0, 0.0, float("nan"), 0.0]],
                [[1.0, 0.0, 0.0, 0.0]], [1.0, 0.0, 0.0, 0.0, 0.0], np.zeros((0, 5)), np.tile(good, (5, 1))):
        with pytest.raises(ValueError):
            S.check_sos(bad)
        with pytest.raises(ValueError):
            S.IIRFilter(None, bad)
    assert S.check_sos(np.tile(good, (4, 1))).shape == (4, 5)


def test_deemphasis_after_preemphasis_returns_the_input():
    x = np.random.default_rng(1).standard_normal(20000)
    for c in (0.0, 0.5, 0.97):
        y = R.sequential(R.sequential(x, S.preemphasis_sos(c)), S.deemphasis_sos(c))
        assert np.abs(y - x).max() <= 1e-12, c
        assert np.abs(R.sequential(x, np.concatenate([S.preemphasis_sos(c), S.deemphasis_sos(c)])) - x).max() <= 1e-12, c
    assert np.array_equal(S.preemphasis_sos(0.97), [[1.0, -0.97, 0.0, 0.0, 0.0]]) and np.array_equal(S.deemphasis_sos(0.97), [[1.0, 0.0, 0.0, -0.97, 0.0]])
    x = np.array([1.0, 0.0, 0.0, 2.0])
    assert np.array_equal(R.sequential(x, S.preemphasis_sos(0.5)), [1.0, -0.5, 0.0, 2.0])
    assert np.array_equal(R.sequential(x, S.deemphasis_sos(0.5)), [1.0, 0.5, 0.25, 2.125])
    for design in (S.preemphasis_sos, S.deemphasis_sos):
        for c in (1.0, -0.1, 1.5, float("nan"), "0.97", True, None):
            with pytest.raises(ValueError):
                design(c)


def test_host_class_checks_its_arguments():
    f = S.IIRFilter(None, S.highpass_sos(22050, 60.0))
    assert (f.sections, f.max_wav_value) == (1, 32768.0) and f.powers.shape == (6, 2, 2) and f.powers is S.IIRFilter(None, f.sos).powers
    with pytest.raises(ValueError):
        S.IIRFilter(None)
    with pytest.raises(ValueError):
        S.IIRFilter(None, f.sos, max_wav_value=0.0)
    with pytest.raises(ValueError):
        f(torch.zeros(4, dtype=torch.float32))
    with pytest.raises(ValueError):
        f(torch.zeros(1, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError):                                # no CPU path
        f(torch.zeros(1, 4, dtype=torch.float32))
    chain = S.build_chain(None, 22050, 60.0, 4, 0.97)
    assert chain.sections == 3 and np.array_equal(chain.sos[:2], S.highpass_sos(22050, 60.0, 4)) and np.array_equal(chain.sos[2:], S.deemphasis_sos(0.97))
    assert S.build_chain(None, 22050) is None and S.build_chain(None, 22050, deemphasis=0.5).sections == 1
    with pytest.raises(ValueError):
        S.build_chain(None, 22050, None, 4)


def test_recipe_keys_parse_and_are_refused():
    from efficient_tts_amd.bin import train as T
    assert T.build_highpass({}) is None and T.build_preemphasis({}) is None
    hp = T.build_highpass({"highpass_hz": 60})
    assert np.array_equal(hp.sos, S.highpass_sos(22050, 60.0, 2))
    hp = T.build_highpass({"highpass_hz": 30.0, "highpass_order": 4, "frontend_params": {"sampling_rate": 16000, "max_wav_value": 1.0}})
    assert np.array_equal(hp.sos, S.highpass_sos(16000, 30.0, 4)) and hp.max_wav_value == 1.0
    assert np.array_equal(T.build_preemphasis({"preemphasis": 0.97}).sos, S.preemphasis_sos(0.97))
    for cfg in ({"highpass_hz": 0}, {"highpass_hz": -1.0}, {"highpass_hz": 11025}, {"highpass_hz": "60"}, {"highpass_hz": True},
                {"highpass_hz": 60, "highpass_order": 3}, {"highpass_hz": 60, "highpass_order": "4"}, {"highpass_order": 2},
                {"highpass_hz": 9000, "frontend_params": {"sampling_rate": 16000}}):
        with pytest.raises(ValueError):
            T.build_highpass(cfg)
    for cfg in ({"preemphasis": 1.0}, {"preemphasis": -0.5}, {"preemphasis": "0.97"}, {"preemphasis": True}):
        with pytest.raises(ValueError):
            T.build_preemphasis(cfg)
    import inspect
    src = inspect.getsource(T.main)                                    # refused at start-up, before any data is read
    assert src.index("build_highpass(config)") < src.index("_build_data") and src.index("build_preemphasis(config)") < src.index("_build_data")
    from efficient_tts_amd.trainer import EfficientTTSTrainer
    stage = inspect.getsource(EfficientTTSTrainer._stage)             # behind the resampler, in front of the gate; pre-emphasis last
    order = [stage.index(s) for s in ("self.resampler(", "self.highpass(", "self.gate(", "self.trimmer(", "self.loudness(", "self.preemphasis(",
                                      "self.frontend(")]
    assert order == sorted(order)


def test_command_lines_parse_and_are_refused():
    from efficient_tts_amd.bin import inference as I
    from efficient_tts_amd.bin import score as C
    from efficient_tts_amd.bin import vocoder_score as V
    base = ["--checkpoint", "exp/checkpoint-7steps.pkl", "--test_fid_scp", "t.txt", "--outdir", "o"]
    a = I.get_parser().parse_args(base)
    assert (a.highpass_hz, a.highpass_order, a.deemphasis) == (None, None, None) and I.build_filter(a) is None
    f = I.build_filter(I.get_parser().parse_args(base + ["--highpass_hz", "60"]))
    assert np.array_equal(f.sos, S.highpass_sos(22050, 60.0, 2))
    f = I.build_filter(I.get_parser().parse_args(base + ["--highpass_hz", "20", "--highpass_order", "4", "--deemphasis", "0.97"]))
    assert np.array_equal(f.sos, np.concatenate([S.highpass_sos(22050, 20.0, 4), S.deemphasis_sos(0.97)]))      # the high-pass first
    assert np.array_equal(I.build_filter(I.get_parser().parse_args(base + ["--deemphasis", "0.97"])).sos, S.deemphasis_sos(0.97))
    for extra in (["--highpass_hz", "60", "--no_vocoder"], ["--deemphasis", "0.97", "--no_vocoder"], ["--highpass_hz", "0"],
                  ["--highpass_hz", "11025"], ["--highpass_hz", "60", "--highpass_order", "3"], ["--highpass_order", "2"], ["--deemphasis", "1.0"],
                  ["--deemphasis", "-0.1"], ["--highpass_hz", "nan"]):
        a = I.get_parser().parse_args(base + extra)
        with pytest.raises(ValueError):
            I.build_filter(a)
        with pytest.raises(ValueError):                               # and at start-up, before anything is loaded or any device is asked for
            I.run_tts(a)
    # the recordings of the two scoring commands
    sbase = ["--checkpoint", "exp/checkpoint-7steps.pkl", "--test_fid_scp", "t.txt", "--outdir", "o"]
    a = C.get_parser().parse_args(sbase)
    assert a.highpass_hz is None and C.build_highpass(a) is None
    assert np.array_equal(C.build_highpass(C.get_parser().parse_args(sbase + ["--highpass_hz", "60", "--highpass_order", "4"])).sos,
                          S.highpass_sos(22050, 60.0, 4))
    vbase = ["--test_fid_scp", "t.txt", "--outdir", "o", "--vocoder", "griffinlim"]
    a = V.get_parser().parse_args(vbase)
    assert a.highpass_hz is None and V.build_highpass(a) is None
    V.check_args(a)
    assert np.array_equal(V.build_highpass(V.get_parser().parse_args(vbase + ["--highpass_hz", "60"])).sos, S.highpass_sos(22050, 60.0, 2))
    for extra in (["--highpass_hz", "0"], ["--highpass_hz", "20000"], ["--highpass_hz", "60", "--highpass_order", "5"], ["--highpass_order", "4"]):
        with pytest.raises(ValueError):
            C.build_highpass(C.get_parser().parse_args(sbase + extra))
        with pytest.raises(ValueError):
            C.run_score(C.get_parser().parse_args(sbase + extra))
        with pytest.raises(ValueError):
            V.check_args(V.get_parser().parse_args(vbase + extra))
        with pytest.raises(ValueError):
            V.run_score(V.get_parser().parse_args(vbase + extra))


def test_header_has_the_section_and_stays_at_revision_602():
    hdr = open(os.path.join(ROOT, "include", "efts_abi.h")).read()
    assert int(re.search(r"#define EFTS_ABI_VERSION (\d+)", hdr).group(1)) == 602
    assert "IIR filtering of a padded batch" in hdr
    assert int(re.search(r"#define EFTS_IIR_SEGMENT (\d+)", hdr).group(1)) == R.L == S.SEGMENT
    assert int(re.search(r"#define EFTS_IIR_MAX_SECTIONS (\d+)", hdr).group(1)) == S.MAX_SECTIONS
    assert re.search(r"\+ efts_iir, efts_iir_pcm16, efts_iir_workspace_bytes", hdr)
    for name in ("efts_iir", "efts_iir_pcm16", "efts_iir_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, hdr)


def test_library_exports_and_refuses_on_the_host():
    """the three entry points are bound, and arguments are refused before anything is launched (no device needed)"""
    import ctypes
    from efficient_tts_amd import build as B
    from efficient_tts_amd import lib as L
    B.build(verbose=False)
    lib = L.load()
    for name in ("efts_iir", "efts_iir_pcm16", "efts_iir_workspace_bytes"):
        assert name in L.exported_symbols() and hasattr(lib, name)
    assert lib.efts_iir_workspace_bytes(0, 100) == 0 and lib.efts_iir_workspace_bytes(2, 0) == 0 and lib.efts_iir_workspace_bytes(2, 2 ** 31) == 0
    assert lib.efts_iir_workspace_bytes(3, 256) == 3 * 64 and lib.efts_iir_workspace_bytes(3, 257) == 3 * 2 * 64
    sos = (ctypes.c_double * 5)(1.0, 0.0, 0.0, -0.97, 0.0)
    assert lib.efts_iir(None, 100, None, sos, 1, None, None, 100, None, 1, None) == -1 and b"null" in lib.efts_last_error()          # EFTS_EINVAL
    assert lib.efts_iir(None, 0, None, sos, 1, None, None, 100, None, 1, None) == -2                                                 # EFTS_ESHAPE
    assert lib.efts_iir(None, 100, None, sos, 1, None, None, 99, None, 1, None) == -2
    assert lib.efts_iir(None, 100, None, sos, 5, None, None, 100, None, 1, None) == -2 and lib.efts_iir(None, 100, None, sos, 0, None, None, 100, None, 1, None) == -2
    assert lib.efts_iir_pcm16(None, 100, None, sos, 1, None, 1.0 / 32768, None, 100, None, 65536, None) == -2
    # with pointers that pass the null and alignment checks (nothing is launched: the refusals below come first)
    buf = (ctypes.c_double * 72)()
    p = (ctypes.addressof(buf) + 63) & ~63                            # 64-byte aligned, 512 bytes behind it
    bad = (ctypes.c_double * 5)(1.0, 0.0, 0.0, -1.0, 0.0)
    assert lib.efts_iir(p, 8, p, bad, 1, p, p + 256, 8, p, 1, None) == -1 and b"unit circle" in lib.efts_last_error()
    assert lib.efts_iir(p, 8, p, sos, 1, p, p + 16, 8, p, 1, None) == -1 and b"overlaps" in lib.efts_last_error()
    assert lib.efts_iir_pcm16(p, 8, p, sos, 1, p, 0.0, p + 256, 8, p, 1, None) == -1 and b"pcm_scale" in lib.efts_last_error()
