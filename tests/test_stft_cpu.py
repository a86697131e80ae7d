"""No GPU: the definition of the STFT distance as tests/stft_reference.py restates it against the reference's formula through torch.stft in
float64; the frame count and the short-item rule; the conditions on the inputs of tests/test_stft_gpu.py; the new exports and what they
refuse before any launch; the host classes; the command line of efficient_tts_amd.bin.vocoder_score."""
import os
import re

import numpy as np
import pytest
import torch

import stft_reference as R
from efficient_tts_amd import lib as L
from efficient_tts_amd import stft as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_mag(x, N, H, W, dtype=torch.float64):
    """magnitudes [B, T, N / 2 + 1] the way the reference computes them (stft_loss.py:12-32), in `dtype`; the window is the definition's:
    built in float64 and rounded once to fp32 (torch.hann_window in fp32 differs from it by an ulp at some taps)"""
    spec = torch.stft(x.to(dtype), N, H, W, torch.hann_window(W, dtype=torch.float64).to(torch.float32).to(dtype), return_complex=True)
    return torch.sqrt(torch.clamp(spec.real ** 2 + spec.imag ** 2, min=1e-7)).transpose(2, 1)


def torch_losses(x, y, resolutions, dtype=torch.float64):
    """(sc, log_mag) per resolution of the reference's formula over a whole batch of equal lengths (stft_loss.py:53, :74)"""
    res = []
    for N, H, W in resolutions:
        mx, my = torch_mag(x, N, H, W, dtype), torch_mag(y, N, H, W, dtype)
        res.append((float(torch.norm(my - mx, p="fro") / torch.norm(my, p="fro")), float(torch.nn.functional.l1_loss(torch.log(my), torch.log(mx)))))
    return res


def test_restatement_agrees_with_the_reference_formula():
    lengths = (4099, 4099)
    x, y = R.batch(lengths, seed=5)
    yf = y.astype(np.float64) / R.MAX_WAV
    out = R.distance(x, y, lengths)
    want = torch_losses(torch.from_numpy(x), torch.from_numpy(yf), R.DEFAULT)
    sc_b, mag_b = R.batch_loss(out)
    assert sc_b == pytest.approx(np.mean([w[0] for w in want]), rel=1e-12) and mag_b == pytest.approx(np.mean([w[1] for w in want]), rel=1e-12)
    # per item: the same formula on a batch of one
    for b in range(2):
        one = torch_losses(torch.from_numpy(x[b:b + 1]), torch.from_numpy(yf[b:b + 1]), R.DEFAULT)
        for r in range(3):
            assert out["sc"][b, r] == pytest.approx(one[r][0], rel=1e-12) and out["log_mag"][b, r] == pytest.approx(one[r][1], rel=1e-12)
    # the magnitudes themselves, every cell, and the window
    for N, H, W in R.DEFAULT + ((256, 64, 256), (512, 77, 301)):
        got = R.magnitudes(x[0], N, H, W)
        ref = torch_mag(torch.from_numpy(x[:1]), N, H, W)[0].numpy()
        assert got.shape == ref.shape == (1 + 4099 // H, N // 2 + 1)
        np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-12)
        assert np.array_equal(R.window(W), torch.hann_window(W, dtype=torch.float64).to(torch.float32).numpy())
        assert np.array_equal(S.hann_window(W), R.window(W))


def test_frame_count_and_short_items():
    assert S.DEFAULT_RESOLUTIONS == R.DEFAULT == ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
    for N, H in ((1024, 120), (2048, 240), (512, 50), (256, 64)):
        for Ln in (0, 1, N // 2 - 1, N // 2):
            assert S.frame_count(Ln, N, H) == R.frame_count(Ln, N, H) == 0
        for Ln in (N // 2 + 1, N, 4 * N + 3):
            assert S.frame_count(Ln, N, H) == R.frame_count(Ln, N, H) == 1 + Ln // H
            assert R.magnitudes(np.ones(Ln, dtype=np.float32), N, H, N).shape == (1 + Ln // H, N // 2 + 1)
        with pytest.raises(Exception):                       # torch refuses the reflect padding of such an item as well
            torch.stft(torch.zeros(1, N // 2), N, H, N, torch.hann_window(N), return_complex=True)
    out = R.distance(*R.batch(), R.LENGTHS)
    assert out["cells"].tolist() == [[9 * 513, 5 * 1025, 21 * 257], [9 * 513, 0, 21 * 257], [35 * 513, 18 * 1025, 82 * 257]]
    nan = np.isnan(out["sc"])
    assert nan.sum() == 1 and nan[1, 1] and np.array_equal(nan, np.isnan(out["log_mag"]))


def test_gpu_inputs_reach_both_branches_of_the_clamp():
    """The long item holds whole frames of exact zeros at every default resolution (20 %, 11 % and 30 % of its cells at 1024, 2048 and 512 sit
    at the clamp), the short items have no zero stretch; the handful of their cells that reach the clamp all the same are bins of the
    symmetric first and last frames that happen to vanish."""
    x, y = R.batch()
    assert x.dtype == np.float32 and y.dtype == np.int16
    assert np.array_equal(x, np.round(x * 32768.0).astype(np.float32) / np.float32(32768.0))             # on the int16 grid
    out = R.distance(x, y, R.LENGTHS)
    print(out["clamped"])
    assert (out["clamped"][2] > 0.05).all() and (out["clamped"][2] < 0.35).all()
    assert (out["clamped"][:2] < 1e-3).all()
    lo = (4099 - 1500) // 2
    assert not x[2, lo:lo + 1500].any() and not y[2, lo:lo + 1500].any() and x[2, lo - 1] != 0 and y[2, lo + 1500] != 0


def test_symbols_refusals_and_revision():
    with open(os.path.join(ROOT, "include", "efts_abi.h")) as f:
        header = f.read()
    assert "#define EFTS_ABI_VERSION 602" in header and L.ABI_VERSION == 602
    lib = L.load()
    assert lib.efts_version() == 602
    for name in ("efts_stft_mag", "efts_stft_dist", "efts_stft_dist_workspace_bytes"):
        assert re.search(r"^(int|int64_t) %s\(" % name, header, re.M), name
        assert name in L.exported_symbols()
        assert hasattr(lib, name)
    assert lib.efts_stft_dist_workspace_bytes(3, 4099, 1024, 120) >= 3 * 35 * 12
    assert lib.efts_stft_dist_workspace_bytes(3, 4099, 1000, 120) == 0 and lib.efts_stft_dist_workspace_bytes(0, 4099, 1024, 120) == 0
    assert lib.efts_stft_dist_workspace_bytes(3, 4099, 1024, 0) == 0 and lib.efts_stft_dist_workspace_bytes(3, 0, 1024, 120) == 0

    def mag(B=1, n=4099, ld=4099, N=1024, H=120, W=600):
        return lib.efts_stft_mag(None, 0, 1.0, ld, None, n, None, None, None, B, N, H, W, None)

    def dist(B=1, n=4099, ldx=4099, ldy=4099, N=1024, H=120, W=600, ws=1 << 20):
        return lib.efts_stft_dist(None, 0, ldx, None, 1, ldy, 1.0 / 32768, None, n, None, None, None, None, ws, B, N, H, W, None)

    # refusals that need no device: they come before any launch, and the entry's name is in the message
    for call, who in ((mag, "efts_stft_mag"), (dist, "efts_stft_dist")):
        for kw, word in ((dict(N=128), "FFT size"), (dict(N=4096), "FFT size"), (dict(N=1000), "FFT size"), (dict(H=0), "hop"), (dict(H=1025), "hop"),
                         (dict(W=1), "window"), (dict(W=1025), "window"), (dict(B=0), "items"), (dict(B=-1), "items"), (dict(n=0), "max_len"),
                         (dict(), "null pointer")):
            assert call(**kw) == -1, kw
            msg = lib.efts_last_error().decode()
            assert msg.startswith(who + ":") and word in msg, msg
    assert mag(ld=4098) == -1 and "leading dimension" in lib.efts_last_error().decode()
    assert dist(ldx=4098) == -1 and "leading dimension" in lib.efts_last_error().decode()
    assert dist(ldy=4098) == -1 and "leading dimension" in lib.efts_last_error().decode()
    assert dist(ws=16) == -1 and "workspace" in lib.efts_last_error().decode()


def test_host_classes_refuse():
    for kw in (dict(n_fft=128), dict(n_fft=1000), dict(n_fft=1024.0), dict(hop_size=0), dict(hop_size=1025), dict(win_length=1), dict(win_length=1025),
               dict(max_wav_value=0.0)):
        with pytest.raises(ValueError):
            S.STFTMagnitude(None, **kw)
    for res in ((), ((1000, 120, 600),), ((1024, 0, 600),), ((1024, 120, 2000),), ((1024, 120),)):
        with pytest.raises((ValueError, TypeError)):
            S.MultiResolutionSTFTDistance(None, res)
    d = S.MultiResolutionSTFTDistance()
    assert d.resolutions == R.DEFAULT and d.max_wav_value == 32768.0
    m = S.STFTMagnitude()
    assert (m.n_fft, m.hop, m.win_length) == (1024, 120, 600)
    with pytest.raises(RuntimeError, match="no CPU path"):
        d(torch.zeros(1, 3000), torch.zeros(1, 3000, dtype=torch.int16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 3000))
    with pytest.raises(ValueError):
        m(torch.zeros(3000))
    with pytest.raises(ValueError):
        d(torch.zeros(1, 3000, dtype=torch.float64), torch.zeros(1, 3000))
    # batch_loss is plain tensor arithmetic on the sums: the reference's reduction
    out = R.distance(*R.batch((4099, 4099), seed=5), (4099, 4099))
    sc, mag = S.MultiResolutionSTFTDistance.batch_loss({"sums": torch.from_numpy(out["sums"]), "cells": torch.from_numpy(out["cells"])})
    want = R.batch_loss(out)
    assert float(sc) == pytest.approx(want[0], rel=1e-14) and float(mag) == pytest.approx(want[1], rel=1e-14)


def test_command_line():
    from efficient_tts_amd.bin import vocoder_score as V
    a = V.get_parser().parse_args(["--test_fid_scp", "t.txt", "--outdir", "o"])
    assert (a.vocoder, a.vocoder_config, a.vocoder_checkpoint, a.gl_iters, a.precision, a.batch_size, a.wav_path) == ("hifigan", None, None, 32, "bf16x3", 16, None)
    with pytest.raises(ValueError, match="vocoder_checkpoint"):
        V.run_score(a)                                                  # refused before a device or a file is looked for
    with pytest.raises(ValueError, match="vocoder_checkpoint"):
        V.check_args(V.get_parser().parse_args(["--test_fid_scp", "t.txt", "--outdir", "o", "--vocoder_checkpoint", "g.pt"]))
    V.check_args(V.get_parser().parse_args(["--test_fid_scp", "t.txt", "--outdir", "o", "--vocoder_checkpoint", "g.pt", "--vocoder_config", "c.json"]))
    a = V.get_parser().parse_args(["--test_fid_scp", "t.txt", "--outdir", "o", "--vocoder", "griffinlim", "--gl_iters", "4", "--wav_path", "d"])
    V.check_args(a)
    assert (a.vocoder, a.gl_iters, a.wav_path) == ("griffinlim", 4, "d")
    assert V.columns() == ["utt", "samples", "sc_1024_120_600", "log_mag_1024_120_600", "sc_2048_240_1200", "log_mag_2048_240_1200", "sc_512_50_240",
                           "log_mag_512_50_240", "sc_mean", "log_mag_mean"]
    nan = float("nan")
    lines, sc_mean, lm_mean = V.format_rows([("a", 5000, [0.1, 0.2, 0.3], [1.0, 2.0, 3.0]), ("b", 900, [0.3, nan, 0.5], [2.0, nan, 4.0])])
    assert len(lines) == 3 and all(len(line.split("\t")) == len(V.columns()) for line in lines)
    assert lines[0].split("\t") == ["a", "5000", "0.100000", "1.000000", "0.200000", "2.000000", "0.300000", "3.000000", "0.200000", "2.000000"]
    assert lines[1].split("\t")[4:6] == ["nan", "nan"] and lines[1].split("\t")[-2:] == ["nan", "nan"]
    # the means leave out what has no value: column by column
    assert lines[2].split("\t") == ["mean", "-", "0.200000", "1.500000", "0.200000", "2.000000", "0.400000", "3.500000", "0.200000", "2.000000"]
    assert sc_mean == pytest.approx(0.2) and lm_mean == pytest.approx(2.0)
