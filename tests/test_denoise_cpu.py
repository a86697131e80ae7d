"""No GPU: the bias denoiser's definition as tests/denoise_reference.py restates it against torch's float64 stft / istft; what strength 0 and
short items do; the condition on the inputs of tests/test_denoise_gpu.py; what the library refuses before any launch; what the host class
and the command lines refuse; the header.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import denoise_reference as R

from efficient_tts_amd import denoise as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("length", R.TORCH_LENGTHS)
def test_reference_equals_torch_float64(length):
    x, bias = R.signal(length, length), R.bias_spectrum()
    for s in R.STRENGTHS:
        err = np.abs(R.denoise(x, bias, s) - R.denoise_torch(x, bias, s, torch.float64)).max()
        print(f"len {length} strength {s}: max |reference - torch float64| = {err:.3g}")
        assert err <= 1e-12


def test_strength_zero_returns_the_input():
    for length in (513, 700, 2049, 12345):
        x = R.signal(length, 5)
        assert np.abs(R.denoise(x, R.bias_spectrum(), 0.0) - x.astype(np.float64)).max() <= 1e-12


def test_short_items_pass_through():
    for length in (0, 1, 300, 512):
        x = R.signal(length, 6)
        assert R.frame_count(length) == 0 and np.array_equal(R.denoise(x, R.bias_spectrum(), 5.0), x.astype(np.float64))
    assert R.frame_count(513) == 3 and R.frame_count(2049) == 9 and R.frame_count(2304) == 10


def test_gpu_inputs_exercise_both_branches_of_the_gain():
    """at strength 0.5 between 5 % and 95 % of the (frame, bin) cells are clamped, and the output level says the same"""
    ref, share = R.reference_batch()
    audio, lengths = R.batch()
    print(f"share of clamped cells at strength 0.5: {share:.3f}")
    assert 0.05 <= share <= 0.95
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))
    b = len(R.LENGTHS) - 1
    r05, r5 = rms(ref[0.5][b]) / rms(audio[b, :lengths[b]]), rms(ref[5.0][b]) / rms(audio[b, :lengths[b]])
    print(f"output RMS over input RMS, 12 345 samples: {r05:.3f} at 0.5, {r5:.3f} at 5")
    assert 0.9 < r05 < 1.0 and 0.5 < r5 < r05
    hum = R.hum(12345)
    before, after = R.level_db(hum), R.level_db(R.denoise(hum, R.frame0_magnitude(hum), 1.0))
    print(f"hum alone, bias = its frame 0, strength 1: {before:.2f} dB -> {after:.2f} dB")
    assert after < before - 20.0 and after > -100.0                   # gone by more than 20 dB, and what is left is far above fp32 rounding


def test_host_class_refusals():
    bias = R.bias_spectrum()
    for bad in (dict(bias=None), dict(bias=bias[:512]), dict(bias=-bias), dict(bias=bias, strength=-1.0), dict(bias=bias, strength=float("nan")),
                dict(bias=np.full(513, np.inf, np.float32))):
        with pytest.raises(ValueError):
            D.BiasDenoiser(None, **bad)
    d = D.BiasDenoiser(None, torch.from_numpy(bias))
    assert d.strength == 0.01 and d.bias.shape == (513,) and d.bias.dtype == torch.float32
    with pytest.raises(RuntimeError, match="no CPU path"):
        d(torch.zeros(1, 2048, dtype=torch.float32))
    with pytest.raises(ValueError, match="int16"):
        d(torch.zeros(1, 2048, dtype=torch.int16))
    with pytest.raises(ValueError, match=r"\[B, n\]"):
        d(torch.zeros(2048, dtype=torch.float32))
    with pytest.raises(ValueError, match="strength"):
        d(torch.zeros(1, 2048, dtype=torch.float32), strength=-0.5)


def test_command_line_refusals():
    from efficient_tts_amd.bin import inference as I
    from efficient_tts_amd.bin import vocoder_score as V
    base = ["--checkpoint", "exp/checkpoint-7steps.pkl", "--test_fid_scp", "t.txt", "--outdir", "o"]
    a = I.get_parser().parse_args(base)
    assert a.denoise is None and I.build_denoiser(a) is None
    assert I.build_denoiser(I.get_parser().parse_args(base + ["--denoise", "0.01"])) is None      # host-only call: the checks, nothing built
    for extra in (["--denoise", "0"], ["--denoise", "-0.1"], ["--denoise", "nan"], ["--denoise", "inf"], ["--denoise", "0.01", "--no_vocoder"]):
        with pytest.raises(ValueError, match="--denoise"):
            I.build_denoiser(I.get_parser().parse_args(base + extra))
    with pytest.raises(ValueError, match="--denoise"):                 # run_tts refuses before anything is loaded (the checkpoint does not exist)
        I.run_tts(I.get_parser().parse_args(base + ["--denoise", "0"]))
    vbase = ["--test_fid_scp", "t.txt", "--outdir", "o", "--vocoder", "griffinlim"]
    assert V.get_parser().parse_args(vbase).denoise is None
    V.check_args(V.get_parser().parse_args(vbase + ["--denoise", "0.01"]))
    for s in ("0", "-1", "nan"):
        with pytest.raises(ValueError, match="--denoise"):
            V.check_args(V.get_parser().parse_args(vbase + ["--denoise", s]))


def test_header_has_the_section_and_stays_at_revision_602():
    hdr = open(os.path.join(ROOT, "include", "efts_abi.h")).read()
    assert int(re.search(r"#define EFTS_ABI_VERSION (\d+)", hdr).group(1)) == 602
    assert "Spectral denoiser for a vocoder's bias noise" in hdr and re.search(r"\+ efts_denoise, efts_denoise_workspace_bytes", hdr)
    for name in ("efts_denoise", "efts_denoise_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, hdr)


def test_library_exports_and_refuses_on_the_host():
    """both entry points are bound, and every refusal of the header comes back before anything is launched (no device needed)"""
    from efficient_tts_amd import build as B
    from efficient_tts_amd import lib as L
    B.build(verbose=False)
    lib = L.load()
    for name in ("efts_denoise", "efts_denoise_workspace_bytes"):
        assert name in L.exported_symbols() and hasattr(lib, name)
    assert lib.efts_denoise_workspace_bytes(0, 100) == 0 and lib.efts_denoise_workspace_bytes(2, 0) == 0 and lib.efts_denoise_workspace_bytes(70000, 100) == 0
    need = lib.efts_denoise_workspace_bytes(4, 16384)
    assert need == 0                                                   # the overlap-add runs in registers
    # host arrays stand in for device memory: a call that passes every check would launch, so every call below fails one check
    n = 2048
    f = (ctypes.c_float * (4 * n + 4))()
    g = (ctypes.c_float * (4 * n + 4))()
    ints = (ctypes.c_int32 * 16)()
    A, G, I = ctypes.addressof(f), ctypes.addressof(g), ctypes.addressof(ints)
    good = dict(audio=A, ld=n, lengths=I, max_len=n, window=A, bias=A, strength=0.5, out=G, ld_out=n, frames=I + 32, ws=None, wsb=0, B=2)

    def call(**kw):
        a = dict(good, **kw)
        return lib.efts_denoise(a["audio"], a["ld"], a["lengths"], a["max_len"], a["window"], a["bias"], a["strength"], a["out"], a["ld_out"],
                                a["frames"], a["ws"], a["wsb"], a["B"], None)
    EINVAL = -1
    cases = [dict(audio=None), dict(lengths=None), dict(window=None), dict(bias=None), dict(out=None), dict(frames=None),        # null
             dict(audio=A + 2), dict(out=G + 1), dict(lengths=I + 2), dict(window=A + 2), dict(bias=A + 1), dict(frames=I + 33), dict(ws=A + 8),   # misaligned
             dict(B=0), dict(B=65536), dict(B=-1),
             dict(max_len=0), dict(max_len=-5), dict(max_len=2 ** 31 - 8192, ld=2 ** 31, ld_out=2 ** 31 - 1),
             dict(ld=n - 1), dict(ld_out=n - 1), dict(ld_out=2 ** 31),
             dict(strength=-0.5), dict(strength=float("nan")), dict(strength=float("inf")),
             dict(wsb=-1),
             dict(out=A), dict(out=A + 4 * n), dict(out=A + 4 * (2 * n - 1)), dict(audio=G + 4 * (2 * n - 4))]                   # out overlaps audio
    for kw in cases:
        rc = call(**kw)
        msg = lib.efts_last_error()
        assert rc == EINVAL and msg.startswith(b"efts_denoise:"), (kw, rc, msg)
    assert b"overlaps" in lib.efts_last_error()
    assert call(strength=-0.0, B=0) == EINVAL                          # (-0 is a legal strength: refused for B only)
