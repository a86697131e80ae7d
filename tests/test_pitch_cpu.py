"""No GPU: the float64 restatements of tests/pitch_reference.py against known pitch, known unvoiced input, the oracle's framing and the
scorer's reference; the margin rule on the inputs of the GPU decision tests; and the new library entries as far as they go without a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pitch_reference as P
import score_reference as R
from efficient_tts_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(sr=P.SR, n_fft=1024, hop=256, fmin=60.0, fmax=600.0, threshold=0.15)
STAGE_CONFIGS = [(1024, 256, 60.0), (512, 128, 100.0)]         # (n_fft, hop, fmin) of the GPU d' and decision tests; fmax 600, threshold 0.15


def test_reference_accuracy_on_known_pitch():
    worst = 0.0
    for name, fa, fb in P.TONES:
        x, f = P.tone(fa, fb, P.TONE_SAMPLES)
        r = P.yin_reference(x.astype(np.float32), x.shape[0], **CFG)
        inside = P.inside_frames(x.shape[0], 1024, 256)
        assert len(inside) >= 15
        errs = [abs(r["f0"][t] - P.true_f0(f, t, 1024, 256)) / P.true_f0(f, t, 1024, 256) for t in inside]
        print(f"{name}: {len(inside)} frames, worst relative f0 error {max(errs):.3e}")
        assert all(r["f0"][t] > 0 for t in inside), name
        worst = max(worst, max(errs))
    print(f"reference tone error {worst:.4e} (module constant {P.REFERENCE_TONE_ERROR:.4e})")
    assert 0.9 * P.REFERENCE_TONE_ERROR <= worst <= P.REFERENCE_TONE_ERROR


def test_reference_unvoiced_cases():
    rng = np.random.default_rng(3)
    noise = (0.3 * rng.standard_normal(4000)).astype(np.float32)
    r = P.yin_reference(noise, 4000, **CFG)
    assert r["f0"].shape[0] == 15 and not (r["f0"] > 0).any() and (r["aperiodicity"] >= 0.15).all()
    z = P.yin_reference(np.zeros(2000, np.float32), 2000, **CFG)
    assert not (z["f0"] > 0).any() and (z["dp"] == 1.0).all() and (z["aperiodicity"] == 1.0).all()


def test_reference_framing_equals_the_oracle():
    from oracle import logmel_oracle as O
    lengths = [5999, 1901, 677, O.PAD + 2, 4096]
    audio = torch.zeros(len(lengths), max(lengths))
    _, frames = O.batch_logmel(audio, torch.tensor(lengths))
    for n, want in zip(lengths, frames.tolist()):
        idx = P.frame_indices(n, O.N_FFT, O.HOP)
        padded = torch.nn.functional.pad(torch.arange(n, dtype=torch.float64)[None, None], (O.PAD, O.PAD), mode="reflect")[0, 0].numpy()
        assert idx.shape == (want, O.N_FFT)
        for t in range(want):
            assert (idx[t] == padded[t * O.HOP:t * O.HOP + O.N_FFT]).all()            # first and last sample index, and every one between


def test_reference_paths():
    rng = np.random.default_rng(11)
    for tx, ty, d, exact in ((1, 1, 1, True), (1, 6, 2, False), (7, 1, 2, True), (9, 13, 3, False), (40, 33, 13, False), (25, 31, 1, True)):
        x = rng.integers(-3, 4, size=(tx, d)).astype(np.float64) if exact else rng.normal(size=(tx, d))
        y = rng.integers(-3, 4, size=(ty, d)).astype(np.float64) if exact else rng.normal(size=(ty, d))
        cost, n, path = P.dtw_path_reference(x, y)
        ref_cost, ref_n, _ = R.dtw(x, y)
        assert P.path_is_valid(path, tx, ty) and path.shape == (n, 2)
        assert cost == ref_cost and n == ref_n
        along = sum(float(np.sqrt(((x[i] - y[j]) ** 2).sum())) for i, j in path)
        assert along == pytest.approx(cost, rel=1e-12, abs=1e-12)
    assert not P.path_is_valid(np.array([[0, 0], [2, 1]]), 3, 2) and not P.path_is_valid(np.array([[0, 0], [1, 1]]), 3, 2)


def test_reference_f0_error():
    path = np.array([[0, 0], [1, 1], [2, 1], [3, 2]])
    a, b = np.array([100.0, 200.0, 0.0, 220.0]), np.array([200.0, 100.0, 110.0])
    rmse, vuv, n = P.f0_error_reference(a, b, path)
    assert n == 3 and rmse == pytest.approx(1200.0) and vuv == 0.25
    rmse, vuv, n = P.f0_error_reference(np.zeros(4), b, path)
    assert n == 0 and np.isnan(rmse) and vuv == 1.0
    assert np.isnan(P.f0_error_reference(a, b, np.zeros((0, 2)))[1])


@pytest.mark.parametrize("n_fft,hop,fmin", STAGE_CONFIGS)
def test_margin_rule_holds_on_the_inputs_of_the_gpu_decision_tests(n_fft, hop, fmin):
    """at most 5 % of the frames may lack margin (no comparison that determines the decision closer than 1e-3 in d')"""
    items, kinds = P.stage_batch(n_fft, hop, seed=7)
    for pcm in (False, True):
        total = without = 0
        for x, kind in zip(items, kinds):
            a = P.as_pcm16(x).astype(np.float32) * np.float32(1.0 / 32768.0) if pcm else x.astype(np.float32)
            r = P.yin_reference(a, a.shape[0], P.SR, n_fft, hop, fmin, 600.0, 0.15)
            total += r["margin"].shape[0]
            without += int((r["margin"] < P.MARGIN).sum())
            if kind in ("noise", "zero"):
                assert not (r["f0"] > 0).any()
        print(f"n_fft {n_fft} pcm16 {pcm}: {without} of {total} frames without margin")
        assert without <= 0.05 * total


def test_symbols_and_revision():
    with open(os.path.join(ROOT, "include", "efts_abi.h")) as f:
        header = f.read()
    lib = L.load()
    for name in ("efts_yin", "efts_yin_pcm16", "efts_dtw_path", "efts_dtw_path_workspace_bytes", "efts_f0_path_error"):
        m = re.search(r"^int(?:64_t)? %s\(([^;]*)\);" % name, header, re.M)
        assert m, name
        assert len(L._SIGS[name][1]) == len(m.group(1).split(",")) and name in L.exported_symbols() and hasattr(lib, name)
    assert "#define EFTS_ABI_VERSION 602\n" in header and L.ABI_VERSION == 602 and lib.efts_version() == 602


def test_library_refuses_before_any_launch():
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    one = ctypes.addressof(buf)                                 # non-null and 16-byte checks aside, nothing is read: every check precedes the launch
    yin = lambda n_fft=1024, hop=256, sr=22050, fmin=60.0, fmax=600.0, audio=one: lib.efts_yin(audio, 4096, one, one, one, None, 1, 4, n_fft, hop, sr, fmin,
                                                                                             fmax, 0.15, None)
    assert yin(audio=None) == -1 and lib.efts_yin_pcm16(None, 4096, 1.0 / 32768, one, one, one, None, 1, 4, 1024, 256, 22050, 60.0, 600.0, 0.15, None) == -1
    for bad in (dict(n_fft=768), dict(n_fft=4096), dict(hop=255), dict(hop=0), dict(fmax=12000.0), dict(fmin=40.0), dict(n_fft=512, fmin=60.0),
                dict(fmin=590.0)):
        assert yin(**bad) == -2, bad
        assert b"efts_yin" in lib.efts_last_error()
    assert lib.efts_yin_pcm16(one, 4096, 1.0 / 32768, one, one, one, None, 1, 4, 1000, 250, 22050, 60.0, 600.0, 0.15, None) == -2
    assert b"efts_yin_pcm16" in lib.efts_last_error()
    ws = lambda tx, ty: lib.efts_dtw_path_workspace_bytes(tx, ty)
    path = lambda tx=4, ty=4, x=one, nbytes=1 << 30: lib.efts_dtw_path(x, 13, 0, one, tx, one, 13, 0, one, ty, 13, one, one, one, one, nbytes, 1, None)
    assert path(x=None) == -1
    for tx, ty in ((8193, 4), (4, 8193), (0, 4), (4, 0)):
        assert path(tx, ty) == -2 and b"efts_dtw_path" in lib.efts_last_error()
        assert ws(tx, ty) == 0
    assert path(nbytes=ws(4, 4) - 1) == -2
    assert lib.efts_f0_path_error(None, 4, 4, one, 4, 4, one, 7, one, one, one, one, 1, None) == -1
    assert lib.efts_f0_path_error(one, 3, 4, one, 4, 4, one, 7, one, one, one, one, 1, None) == -2 and b"efts_f0_path_error" in lib.efts_last_error()
    sizes = [1, 2, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 8192]
    for a in sizes:
        for i, b in enumerate(sizes[:-1]):
            assert 0 < ws(a, b) <= ws(a, sizes[i + 1]) and ws(b, a) <= ws(sizes[i + 1], a)
    assert ws(1024, 800) == (800 + 255) * 256 and ws(1025, 800) == 2 * (800 + 255) * 256


def test_python_owners_refuse_on_the_host():
    from efficient_tts_amd import pitch as T
    from efficient_tts_amd import score as S
    assert T.lag_range(22050, 1024, 60.0, 600.0) == (36, 367) == P.lag_range(22050, 1024, 60.0, 600.0)
    for bad in ((22050, 512, 60.0, 600.0), (22050, 1024, 60.0, 12000.0), (22050, 1024, 590.0, 600.0), (22050, 1024, 0.0, 600.0)):
        with pytest.raises(ValueError):
            T.lag_range(*bad)
    with pytest.raises(ValueError):
        T.PitchTracker("cpu", n_fft=768)
    with pytest.raises(ValueError):
        T.PitchTracker("cpu", hop_size=255)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.dtw_path(torch.zeros(1, 4, 13), torch.tensor([4]), torch.zeros(1, 5, 13), torch.tensor([5]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.F0Error("cpu")(torch.zeros(1, 4), torch.zeros(1, 5), torch.zeros(1, 8, 2, dtype=torch.int32), torch.tensor([0]))
    with pytest.raises(ValueError):
        S.F0Error("cpu")(torch.zeros(1, 4), torch.zeros(1, 5), torch.zeros(1, 8, 2), torch.tensor([0]))
