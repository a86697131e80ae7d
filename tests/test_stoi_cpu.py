"""No GPU: the STOI / ESTOI definition as tests/stoi_reference.py restates it -- the band table, what a perfect copy, noise, too few kept frames
and silence give --; the condition on the inputs of tests/test_stoi_gpu.py; the columns of `vocoder_score --stoi`; what the library and the
host class refuse before any launch."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import stoi_reference as R

from efficient_tts_amd import stoi as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_band_table_equals_the_formula_and_the_window_is_hanning_258():
    assert R.bands_from_formula() == R.BAND_TABLE and len(R.BAND_TABLE) == R.BANDS
    assert np.array_equal(R.window(), np.hanning(258)[1:-1].astype(np.float32).astype(np.float64))
    assert np.array_equal(S.stoi_window().astype(np.float64), R.window()) and S.stoi_window().dtype == np.float32
    assert (S.FS, S.FRAME, S.HOP, S.N_FFT, S.BANDS, S.SEGMENT) == (R.FS, R.FRAME, R.HOP, R.N_FFT, R.BANDS, R.SEGMENT)
    src = open(os.path.join(ROOT, "efficient_tts_amd", "csrc", "efts_stoi.hip")).read()
    for name, col in (("si_lo", 0), ("si_hi", 1)):                     # the kernel's own table
        got = [int(v) for v in re.search(r"%s\[16\] = \{([^}]*)\}" % name, src).group(1).split(",")]
        assert got == [b[col] for b in R.BAND_TABLE] + [0]


def test_a_perfect_copy_scores_one_and_noise_lowers_both_scores_strictly():
    ref = R.reference_batch()
    scored = [b for b, r in enumerate(ref[None]) if r["segments"]]
    assert len(scored) == 3
    for b in scored:
        assert abs(ref[None][b]["stoi"] - 1.0) <= 1e-12 and abs(ref[None][b]["estoi"] - 1.0) <= 1e-12
        for key in ("stoi", "estoi"):
            v = [ref[snr][b][key] for snr in (None, 20.0, 5.0, -5.0)]
            assert v[0] > v[1] > v[2] > v[3] > 0.0, (b, key, v)


def test_counts_and_nan_for_items_without_a_segment():
    x, lengths, names = R.batch()
    ref = R.reference_batch()[5.0]
    by = dict(zip(names, ref))
    assert (by["n255"]["frames"], by["n255"]["kept"], by["n255"]["segments"]) == (0, 0, 0) and math.isnan(by["n255"]["stoi"])
    assert R.frame_count(255) == 0 and R.frame_count(256) == 1 and R.frame_count(383) == 1 and R.frame_count(384) == 2
    assert (by["K30"]["kept"], by["K30"]["segments"]) == (30, 0) and math.isnan(by["K30"]["stoi"]) and math.isnan(by["K30"]["estoi"])
    assert (by["K31"]["kept"], by["K31"]["segments"]) == (31, 1) and 0.0 < by["K31"]["estoi"] < by["K31"]["stoi"] < 1.0
    assert by["zero_x"]["frames"] == 92 and by["zero_x"]["kept"] == 0 and math.isnan(by["zero_x"]["stoi"]) and math.isnan(by["zero_x"]["estoi"])
    for name in ("15001", "23456"):                                    # silent frames are removed, and not all of them
        assert 0.3 * by[name]["frames"] < by[name]["kept"] < 0.7 * by[name]["frames"]
        assert by[name]["segments"] == by[name]["kept"] - 30


def test_the_inputs_of_the_gpu_test_keep_every_frame_away_from_the_threshold():
    """an fp32 frame energy lies within about 1e-5 dB of its exact value; every frame of every input of tests/test_stoi_gpu.py lies at least
    0.01 dB from the 40 dB threshold, so no frame can be kept on the device and dropped by the reference or the other way round"""
    for pcm16 in (False, True):
        for snr, items in R.reference_batch(pcm16).items():
            for r in items:
                assert r["margin_db"] >= 0.01, (pcm16, snr, r)
    x = R.speech_like(23456, 9)
    for n in (9000, 15001, 23456):
        r = R.stoi(x[:n], x[:n])
        assert 0.01 <= r["margin_db"] < 40.0 and r["kept"] < r["frames"]
    assert 0.0 < R.yardstick() < 1e-5 and 0.0 < R.yardstick(True) < 1e-5       # an fp32 rounding error on scores of at most 1


def test_columns_and_rows_with_and_without_the_addition():
    from efficient_tts_amd.bin import vocoder_score as V
    base = ["utt", "samples", "sc_1024_120_600", "log_mag_1024_120_600", "sc_2048_240_1200", "log_mag_2048_240_1200", "sc_512_50_240", "log_mag_512_50_240",
            "sc_mean", "log_mag_mean"]
    assert V.columns() == base and V.columns(stoi=False) == base and V.columns(stoi=True) == base + ["stoi", "estoi", "stoi_kept_frames"]
    nan = float("nan")
    rows = [("a", 5000, [0.1, 0.2, 0.3], [1.0, 2.0, 3.0]), ("b", 900, [0.3, nan, 0.5], [2.0, nan, 4.0]), ("c", 700, [0.5, 0.5, 0.5], [1.0, 1.0, 1.0])]
    plain = V.format_rows(rows)
    assert len(plain) == 3 and plain[0] == V.format_rows(rows, stoi=None)[0]
    assert plain[0][0].split("\t") == ["a", "5000", "0.100000", "1.000000", "0.200000", "2.000000", "0.300000", "3.000000", "0.200000", "2.000000"]
    assert plain[0][3].split("\t")[:2] == ["mean", "-"] and all(len(line.split("\t")) == len(base) for line in plain[0])
    lines, sc_mean, lm_mean, s_mean, e_mean = V.format_rows(rows, stoi=[(0.9, 0.8, 77), (nan, nan, 12), (0.7, 0.5, 40)])
    assert (sc_mean, lm_mean) == plain[1:] and s_mean == pytest.approx(0.8) and e_mean == pytest.approx(0.65)
    assert all(len(line.split("\t")) == len(V.columns(stoi=True)) for line in lines)
    assert ["\t".join(line.split("\t")[:len(base)]) for line in lines] == plain[0]          # the columns in front are untouched
    assert [line.split("\t")[len(base):] for line in lines] == [["0.900000", "0.800000", "77"], ["nan", "nan", "12"], ["0.700000", "0.500000", "40"],
                                                                 ["0.800000", "0.650000", "-"]]
    with pytest.raises(ValueError, match="one"):
        V.format_rows(rows, stoi=[(0.9, 0.8, 77)])
    vbase = ["--test_fid_scp", "t.txt", "--outdir", "o", "--vocoder", "griffinlim"]
    assert V.get_parser().parse_args(vbase).stoi is False and V.get_parser().parse_args(vbase + ["--stoi"]).stoi is True
    V.check_args(V.get_parser().parse_args(vbase + ["--stoi", "--denoise", "0.01"]))
    with pytest.raises(ValueError, match="vocoder_checkpoint"):        # the flag changes no refusal
        V.run_score(V.get_parser().parse_args(["--test_fid_scp", "t.txt", "--outdir", "o", "--stoi"]))
    assert "--stoi" in V.__doc__


def test_what_the_host_class_refuses():
    for bad, match in ((dict(sampling_rate=0), "positive"), (dict(sampling_rate=22050.0), "integer"), (dict(quality="better"), "quality"),
                       (dict(max_wav_value=0.0), "max_wav_value")):
        with pytest.raises(ValueError, match=match):
            S.ShortTimeIntelligibility(None, **bad)
    m = S.ShortTimeIntelligibility(None)
    assert (m.sampling_rate, m.resampler.dst_rate, m.resampler.L, m.resampler.M) == (22050, 10000, 200, 441)
    assert S.ShortTimeIntelligibility(None, 10000).resampler.identity
    x = torch.zeros(2, 4000)
    with pytest.raises(RuntimeError, match="no CPU path"):             # a host tensor is refused like everywhere else
        m(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.ShortTimeIntelligibility(None, 10000)(x, x)
    for a, b in ((torch.zeros(4000), x), (x, torch.zeros(2, 4000, dtype=torch.float64)), (x, torch.zeros(2, 0))):
        with pytest.raises(ValueError):
            m(a, b)


def test_header_has_the_section_and_stays_at_revision_602():
    hdr = open(os.path.join(ROOT, "include", "efts_abi.h")).read()
    assert int(re.search(r"#define EFTS_ABI_VERSION (\d+)", hdr).group(1)) == 602
    assert "Short-time objective intelligibility" in hdr and re.search(r"\+ efts_stoi, efts_stoi_workspace_bytes", hdr)
    assert "returns 1e-5" in hdr                                       # where the reference code differs
    for name in ("efts_stoi", "efts_stoi_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, hdr)


def test_library_exports_and_refuses_on_the_host():
    """both entry points are bound, and every refusal of the header comes back before anything is launched (no device needed)"""
    from efficient_tts_amd import build as B
    from efficient_tts_amd import lib as L
    B.build(verbose=False)
    lib = L.load()
    for name in ("efts_stoi", "efts_stoi_workspace_bytes"):
        assert name in L.exported_symbols() and hasattr(lib, name)
    assert lib.efts_stoi_workspace_bytes(0, 100) == 0 and lib.efts_stoi_workspace_bytes(2, 0) == 0 and lib.efts_stoi_workspace_bytes(70000, 100) == 0
    assert lib.efts_stoi_workspace_bytes(3, 255) == 16                 # no frames: nothing but the alignment unit
    F, T, M = 182, 181, 152                                            # 23 456 samples
    need = lib.efts_stoi_workspace_bytes(3, 23456)
    assert need % 16 == 0 and need >= 3 * (F * 8 + T * 128 + M * 16) and need <= 3 * (F * 8 + T * 128 + M * 16) + 5 * 16
    # host arrays stand in for device memory: a call that passes every check would launch, so every call below fails one check
    n = 2048
    f = (ctypes.c_float * (4 * n + 4))()
    d = (ctypes.c_double * 16)()
    ints = (ctypes.c_int32 * 32)()
    ws = (ctypes.c_char * (1 << 16))()
    A, D, I = ctypes.addressof(f), ctypes.addressof(d), ctypes.addressof(ints)
    W = (ctypes.addressof(ws) + 15) & ~15
    good = dict(x=A, ldx=n, y=A, ldy=n, lengths=I, max_len=n, window=A, stoi=D, estoi=D + 32, frames=I + 32, kept=I + 64, segments=I + 96, ws=W,
                wsb=lib.efts_stoi_workspace_bytes(2, n), B=2)

    def call(**kw):
        a = dict(good, **kw)
        return lib.efts_stoi(a["x"], a["ldx"], a["y"], a["ldy"], a["lengths"], a["max_len"], a["window"], a["stoi"], a["estoi"], a["frames"], a["kept"],
                             a["segments"], a["ws"], a["wsb"], a["B"], None)
    EINVAL = -1
    cases = [dict(x=None), dict(y=None), dict(lengths=None), dict(window=None), dict(stoi=None), dict(estoi=None), dict(frames=None), dict(kept=None),
             dict(segments=None), dict(ws=None),                                                                                    # null
             dict(x=A + 2), dict(y=A + 1), dict(lengths=I + 2), dict(window=A + 2), dict(stoi=D + 4), dict(estoi=D + 36), dict(frames=I + 33),
             dict(kept=I + 66), dict(segments=I + 97), dict(ws=W + 8),                                                               # misaligned
             dict(B=0), dict(B=65536), dict(B=-1), dict(max_len=0), dict(max_len=-5), dict(max_len=2 ** 31 - 8192, ldx=2 ** 31, ldy=2 ** 31),
             dict(ldx=n - 1), dict(ldy=n - 1), dict(wsb=good["wsb"] - 1), dict(wsb=0), dict(wsb=-1)]
    assert good["wsb"] > 16
    for kw in cases:
        rc = call(**kw)
        msg = lib.efts_last_error()
        assert rc == EINVAL and msg.startswith(b"efts_stoi:"), (kw, rc, msg)
