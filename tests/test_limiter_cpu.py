"""No GPU: the true-peak and limiter definition as tests/limiter_reference.py restates it -- the table, the fs / 4 sine, the properties that
hold by construction --, the condition on the inputs of tests/test_limiter_gpu.py under which the counts of limited samples must match
exactly, what the host classes refuse, the header's section and the command lines' plumbing."""
import math
import os
import re

import numpy as np
import pytest
import torch

import limiter_reference as R

from efficient_tts_amd import limiter as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_phase_zero_is_the_identity_and_every_entry_is_the_formula():
    h = S.true_peak_table()
    assert h.shape == (4, 25) and h.dtype == np.float32
    want0 = np.zeros(25, np.float32)
    want0[12] = 1.0
    assert np.array_equal(h[0], want0) and not np.signbit(h[0]).any()                    # exact: +0.0 and 1
    ref = R.table64()                                                                    # its own Bessel series, entry by entry
    assert np.all(np.abs(h.astype(np.float64) - ref) <= np.abs(ref) * 2.0 ** -24 * (1 + 1e-6))       # one rounding of the float64 value
    assert np.array_equal(h, R.table32())
    assert np.all(h[1:, 0] == 0.0) and np.all(h[1:, 24] != 0.0)                          # |q / 4 + 12| >= 12 lies outside the window
    assert np.allclose(h[3][1:], h[1][1:][::-1], rtol=0, atol=1e-7)                      # phase 3 mirrors phase 1: t = 3 / 4 - k = -(1 / 4 - (1 - k))
    assert np.all(np.abs(h[1:].astype(np.float64).sum(axis=1) - 0.99997) < 2e-5)         # the DC gains of the other phases


def test_fs4_sine_reads_a_sample_peak_of_0_7071_and_a_true_peak_of_one():
    """in the steady state: the first and last 24 samples carry the transient of a tone switched on at full level, whose true peak really is
    higher (1.089 on the whole item)"""
    x = R.fs4_sine(4099)
    p = R.oversampled_peak(x, np.float64)
    assert abs(np.abs(x).max() - math.sqrt(0.5)) < 1e-12
    steady = p[24:-24].max()
    print(f"true peak of the fs / 4 sine in the steady state: {steady:.7f}; over the whole item {p.max():.4f}")
    assert abs(steady - 1.0) < 1e-3
    assert abs(p[24:-24].astype(np.float32).max() - R.oversampled_peak(x.astype(np.float32), np.float32)[24:-24].max()) < 1e-6
    tp, sp = R.peaks(x.astype(np.float32), np.float64)
    assert tp >= sp and abs(tp - p.max()) < 1e-6 and abs(sp - math.sqrt(0.5)) < 1e-7


def test_properties_that_hold_by_construction_on_every_case():
    """g <= r, |out| <= c up to the two roundings, m[j] <= r[i] inside the mean, true peak >= sample peak, an item under the ceiling unchanged"""
    for pcm16, c, h, s in R.cases():
        for dtype in ("float64", "float32"):
            for b, (x, r) in enumerate(zip(R.items(pcm16), R.limit_batch(pcm16, c, h, s, dtype))):
                n = x.shape[0]
                assert r["out"].shape == (n,) and np.all(r["g"] <= r["r"]) and np.all(r["g"] > 0) and np.all(r["g"] <= 1)
                assert np.all(np.abs(r["out"]) <= c * (1 + 2e-7))
                assert np.all(r["p"] >= np.abs(R.samples(x, r["p"].dtype)))
                for i in range(0, n, max(1, n // 7)):
                    assert np.all(r["m"][i:i + 2 * s + 1] <= r["r"][i])
                if n and r["true_peak_in"] <= c:
                    assert np.array_equal(r["out"], R.samples(x, r["out"].dtype)) and r["limited"] == 0 and r["gain_min"] == 1.0
        res = R.limit_batch(pcm16, c, h, s, "float64")
        assert res[R.UNDER]["limited"] == 0 and res[R.ZERO]["limited"] == 0 and res[R.SINE]["limited"] > 4000
        assert all(res[b]["limited"] > 0 for b in range(1, 8)) and res[0]["limited"] == 0 and res[0]["gain_min"] == 1.0
    for pcm16 in (False, True):
        for tp, sp in R.peaks_batch(pcm16, "float64"):
            assert tp >= sp >= 0.0
        assert R.peaks_batch(pcm16, "float64")[0] == (0.0, 0.0) and R.peaks_batch(pcm16, "float64")[R.ZERO] == (0.0, 0.0)


def test_margins_that_the_gpu_tests_rely_on():
    """`limited` can only be asked to be equal when no decision is close: every p is at least 1e-5 (relative) from the ceiling and every gain
    below 1 is below 1 - 1e-6, in the reference and in the fp32 yardstick, on every case of tests/test_limiter_gpu.py"""
    worst_p, worst_g = np.inf, np.inf
    for pcm16, c, h, s in R.cases():
        ref, yard = R.limit_batch(pcm16, c, h, s, "float64"), R.limit_batch(pcm16, c, h, s, "float32")
        for a, y in zip(ref, yard):
            if a["p"].size:
                worst_p = min(worst_p, float(np.abs(a["p"] / c - 1.0).min()))
            below = a["g"][a["g"] < 1.0]
            if below.size:
                worst_g = min(worst_g, float(1.0 - below.max()))
            assert a["limited"] == y["limited"]
    print(f"closest p to a ceiling: {worst_p:.3e} relative; closest gain below 1: 1 - {worst_g:.3e}")
    assert worst_p >= 1e-5 and worst_g > 1e-6


def test_excess_of_the_true_peak_over_the_ceiling_is_what_the_smoothness_of_g_leaves():
    """nothing asserted beyond its sign and size: the sample peak is bounded exactly, the true peak as far as g is smooth"""
    for c, h, s in ((R.CEILINGS[0], 32, 32), (R.CEILINGS[0], 16, 8), (R.CEILINGS[1], 32, 32)):
        res = R.limit_batch(False, c, h, s, "float64")
        worst = max(R.excess_db(float(r["true_peak_out"]), c) for r in res[1:8])
        print(f"ceiling {c:.4f}, hold {h}, smooth {s}: true peak of the output {worst:+.4f} dB over the ceiling")
        assert -0.5 < worst < 0.5


def test_host_classes_check_their_arguments():
    lim = S.PeakLimiter(None)
    assert (lim.sampling_rate, lim.hold, lim.smooth, lim.max_wav_value) == (22050, 33, 33, 32768.0)
    assert lim.ceiling == R.CEILINGS[1] and lim.ceiling_dbtp == -1.0
    assert (S.PeakLimiter(None, 48000).hold, S.PeakLimiter(None, 16000).smooth) == (72, 24)
    assert (S.PeakLimiter(None, hold=64).smooth, S.PeakLimiter(None, hold=16).smooth, S.PeakLimiter(None, hold=128, smooth=1).smooth) == (33, 16, 1)
    assert S.PeakLimiter(None, ceiling_dbtp=20.0 * math.log10(0.5)).ceiling == 0.5
    for kw in (dict(hold=129), dict(hold=8, smooth=9), dict(smooth=0), dict(hold=0), dict(sampling_rate=96000), dict(ceiling_dbtp=0.5),
               dict(ceiling_dbtp=float("nan")), dict(lookahead_ms=0.0), dict(hold=2.5), dict(sampling_rate=0), dict(max_wav_value=0.0)):
        with pytest.raises(ValueError):
            S.PeakLimiter(None, **kw)
    with pytest.raises(ValueError):
        S.TruePeakMeter(None, max_wav_value=-1.0)
    for mod in (lim, S.TruePeakMeter(None)):
        with pytest.raises(ValueError):
            mod(torch.zeros(4, dtype=torch.float32))
        with pytest.raises(ValueError):
            mod(torch.zeros(1, 4, dtype=torch.float64))
        with pytest.raises(RuntimeError):                            # no CPU path
            mod(torch.zeros(1, 4, dtype=torch.float32))


def test_command_line_plumbing_and_refusals():
    from efficient_tts_amd.bin import inference as I
    from efficient_tts_amd.bin import loudness as C
    base = ["--checkpoint", "exp/checkpoint-7steps.pkl", "--test_fid_scp", "t.txt", "--outdir", "o"]
    a = I.get_parser().parse_args(base)
    assert a.limit_true_peak is None and I.build_limiter(a) is None and a.loudness_peak_ceiling == 0.99
    a = I.get_parser().parse_args(base + ["--limit_true_peak", "-1"])
    lim = I.build_limiter(a, 22050)
    assert (lim.ceiling_dbtp, lim.sampling_rate, lim.hold, lim.smooth) == (-1.0, 22050, 33, 33) and I.build_loudness(a) is None
    assert I.build_limiter(I.get_parser().parse_args(base + ["--limit_true_peak", "-2", "--sampling_rate", "48000"]), 48000).hold == 72
    # with --loudness the normaliser has no ceiling of its own; without the new flag it keeps 0.99
    a = I.get_parser().parse_args(base + ["--loudness", "-16", "--limit_true_peak", "-1"])
    assert I.build_loudness(a).peak_ceiling is None and I.build_limiter(a).ceiling == R.CEILINGS[1]
    assert I.build_loudness(I.get_parser().parse_args(base + ["--loudness", "-16"])).peak_ceiling == 0.99
    for extra in (["--limit_true_peak", "0.5"], ["--limit_true_peak", "nan"], ["--limit_true_peak", "-1", "--no_vocoder"],
                  ["--limit_true_peak", "-1", "--loudness", "-16", "--loudness_peak_ceiling", "0.99"],
                  ["--limit_true_peak", "-1", "--loudness_peak_ceiling", "0.9"], ["--limit_true_peak", "-1", "--sampling_rate", "96000"]):
        a = I.get_parser().parse_args(base + extra)
        with pytest.raises(ValueError):
            I.build_limiter(a, 22050 if a.sampling_rate is None else a.sampling_rate)
        with pytest.raises(ValueError):                               # and at start-up, before anything is loaded or any device is asked for
            I.run_tts(a)
    assert I.build_limiter(I.get_parser().parse_args(base + ["--limit_true_peak", "0"])).ceiling == 1.0
    # looking at a corpus
    a = C.get_parser().parse_args(["--filelist", "f", "--wav_path", "d", "--outdir", "o"])
    assert a.true_peak is False and C.COLUMNS == ("id", "seconds", "lufs", "gain_db", "limited")
    assert C.get_parser().parse_args(["--filelist", "f", "--wav_path", "d", "--outdir", "o", "--true_peak"]).true_peak is True
    assert C.PEAK_COLUMNS == ("sample_peak_db", "true_peak_dbtp") and C._db(0.0) == float("-inf") and C._db(0.1) == pytest.approx(-20.0)


def test_header_has_the_section_and_stays_at_revision_602():
    hdr = open(os.path.join(ROOT, "include", "efts_abi.h")).read()
    assert int(re.search(r"#define EFTS_ABI_VERSION (\d+)", hdr).group(1)) == 602
    assert "True-peak metering after ITU-R BS.1770 Annex 2" in hdr
    assert int(re.search(r"#define EFTS_LIMITER_CHUNK (\d+)", hdr).group(1)) == R.CHUNK
    assert int(re.search(r"#define EFTS_LIMITER_MAX_HOLD (\d+)", hdr).group(1)) == R.MAX_HOLD == S.MAX_HOLD
    assert re.search(r"\+ efts_true_peak, efts_true_peak_pcm16, efts_peak_limit, efts_peak_limit_pcm16, efts_limiter_workspace_bytes", hdr)
    for name in ("efts_true_peak", "efts_true_peak_pcm16", "efts_peak_limit", "efts_peak_limit_pcm16", "efts_limiter_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, hdr)


def test_library_exports_and_refuses_on_the_host():
    """the five entry points are bound, and arguments are refused before anything is launched (no device needed)"""
    import ctypes
    from efficient_tts_amd import build as B
    from efficient_tts_amd import lib as L
    B.build(verbose=False)
    lib = L.load()
    for name in ("efts_true_peak", "efts_true_peak_pcm16", "efts_peak_limit", "efts_peak_limit_pcm16", "efts_limiter_workspace_bytes"):
        assert name in L.exported_symbols() and hasattr(lib, name)
    assert lib.efts_limiter_workspace_bytes(0, 100) == 0 and lib.efts_limiter_workspace_bytes(2, 0) == 0 and lib.efts_limiter_workspace_bytes(2, 2 ** 31) == 0
    assert lib.efts_limiter_workspace_bytes(3, 2048) == 3 * 16 and lib.efts_limiter_workspace_bytes(3, 2049) == 3 * 2 * 16
    table = (ctypes.c_float * 100)(*S.true_peak_table().reshape(-1).tolist())
    assert lib.efts_true_peak(None, 100, None, table, None, None, None, 1, None) == -1 and b"null" in lib.efts_last_error()          # EFTS_EINVAL
    assert lib.efts_true_peak(None, 0, None, table, None, None, None, 1, None) == -2                                                 # EFTS_ESHAPE
    assert lib.efts_true_peak_pcm16(None, 100, None, table, 1.0 / 32768, None, None, None, 65536, None) == -2
    tail = (None, 100, None, None, None, None)
    assert lib.efts_peak_limit(None, 100, None, table, 0.5, 32, 32, *tail, 1, None) == -1 and b"efts_peak_limit" in lib.efts_last_error()
    for hold, smooth in ((129, 1), (8, 9), (8, 0), (0, 0)):
        assert lib.efts_peak_limit(None, 100, None, table, 0.5, hold, smooth, *tail, 1, None) == -2
    assert lib.efts_peak_limit(None, 100, None, table, 0.5, 32, 32, None, 99, None, None, None, None, 1, None) == -2                 # ld_out < ld_in
    assert lib.efts_peak_limit_pcm16(None, 100, None, table, 1.0 / 32768, 0.5, 32, 32, *tail, 0, None) == -2
    # what needs valid pointers to get that far: a ceiling that is no positive number, a table whose phase 0 is not the identity
    buf = (ctypes.c_float * 128)()
    ws = (ctypes.c_char * 64)()
    ws_p = ctypes.c_void_p((ctypes.addressof(ws) + 15) & ~15)
    p = lambda off: ctypes.c_void_p(ctypes.addressof(buf) + 4 * off)
    for c in (0.0, -0.5, float("nan"), float("inf")):
        assert lib.efts_peak_limit(p(0), 16, p(16), table, c, 4, 4, p(32), 16, p(48), p(52), p(56), ws_p, 1, None) == -1 and b"ceiling" in lib.efts_last_error()
    assert lib.efts_peak_limit(p(0), 16, p(64), table, 0.5, 4, 4, p(8), 16, p(48), p(52), p(56), ws_p, 1, None) == -1 and b"overlaps" in lib.efts_last_error()
    bad = (ctypes.c_float * 100)(*S.true_peak_table().reshape(-1).tolist())
    bad[11] = 1e-9
    assert lib.efts_true_peak(p(0), 16, p(16), bad, p(48), p(52), ws_p, 1, None) == -1 and b"identity" in lib.efts_last_error()
    assert lib.efts_true_peak_pcm16(p(0), 16, p(16), table, 0.0, p(48), p(52), ws_p, 1, None) == -1 and b"pcm_scale" in lib.efts_last_error()
