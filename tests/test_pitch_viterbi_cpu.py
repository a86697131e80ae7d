"""No GPU: the pitch smoother (efficient_tts_amd/pitch.py `ViterbiSmoother`, csrc/efts_pitch_viterbi.hip) as far as it goes without a device --
the two library entries and their refusals, the int64 restatement of tests/viterbi_reference.py on signals with a known answer (d' from
tests/pitch_reference.py), and the command-line switches."""
import ctypes
import os
import re

import numpy as np
import pytest

import pitch_reference as P
import viterbi_reference as V
from efficient_tts_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(sr=P.SR, n_fft=1024, hop=256, fmin=60.0, fmax=600.0, threshold=0.15)
TAU_MIN, TAU_MAX = 36, 367


def smoothed(x):
    r = P.yin_reference(np.asarray(x, dtype=np.float32), len(x), **CFG)
    lag, _ = V.viterbi_reference(r["dp"].astype(np.float32), TAU_MIN, TAU_MAX)
    return r, lag


def test_symbols_and_revision():
    with open(os.path.join(ROOT, "include", "efts_abi.h")) as f:
        header = f.read()
    lib = L.load()
    for name in ("efts_f0_viterbi", "efts_f0_viterbi_workspace_bytes"):
        m = re.search(r"^int(?:64_t)? %s\(([^;]*)\);" % name, header, re.M)
        assert m, name
        assert len(L._SIGS[name][1]) == len(m.group(1).split(",")) and name in L.exported_symbols() and hasattr(lib, name)
    assert "#define EFTS_ABI_VERSION 602\n" in header and L.ABI_VERSION == 602 and lib.efts_version() == 602
    assert "efts_f0_viterbi, efts_f0_viterbi_workspace_bytes" in header.split("#define EFTS_ABI_VERSION")[0]


def test_library_refuses_before_any_launch():
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    one = ctypes.addressof(buf)                                 # non-null; nothing is read: every check precedes the launch
    Q = 65536
    ws = lib.efts_f0_viterbi_workspace_bytes

    def call(cmnd=one, frames=one, lg=one, f0=one, ap=one, lag=one, work=one, nbytes=1 << 40, item_stride=4 * 368, frame_stride=368, B=1, T=4, tau_min=36,
             tau_max=367, sr=22050, costs=(9830, 1311, 22938, 9175)):
        return lib.efts_f0_viterbi(cmnd, item_stride, frame_stride, frames, lg, f0, ap, lag, work, nbytes, B, T, tau_min, tau_max, sr, *costs, None)

    for name in ("cmnd", "frames", "lg", "f0", "ap", "lag", "work"):
        assert call(**{name: None}) == -1, name
        assert b"efts_f0_viterbi" in lib.efts_last_error()
    bad = [dict(tau_min=1), dict(tau_min=366), dict(tau_min=367), dict(tau_max=1025, frame_stride=1026), dict(T=0), dict(T=(1 << 20) + 1), dict(B=0),
           dict(B=65536), dict(sr=0), dict(frame_stride=367), dict(item_stride=-1), dict(nbytes=ws(4, 36, 367) - 1), dict(B=3, nbytes=3 * ws(4, 36, 367) - 1),
           dict(costs=(-1, 0, 0, 0)), dict(costs=(0, 16 * Q + 1, 0, 0)), dict(costs=(0, 0, 1 << 30, 0)), dict(costs=(0, 0, 0, 16 * Q + 1))]
    for kw in bad:
        assert call(**kw) == -2, kw
        assert b"efts_f0_viterbi" in lib.efts_last_error()
    for args in ((0, 36, 367), (4, 1, 367), (4, 366, 367), (4, 36, 1025), ((1 << 20) + 1, 36, 367)):
        assert ws(*args) == 0, args


def test_workspace_size_is_positive_and_monotone():
    ws = L.load().efts_f0_viterbi_workspace_bytes
    frames = [1, 2, 5, 37, 800, 801, 9000, 1 << 20]
    ranges = [(2, 4), (2, 8), (36, 220), (36, 367), (2, 1023), (2, 1024)]      # S ascending: 2, 6, 184, 331, 1021, 1022
    for i, T in enumerate(frames):
        for j, (lo, hi) in enumerate(ranges):
            assert ws(T, lo, hi) >= T * (hi - lo + 1) * 2 > 0 and ws(T, lo, hi) % 16 == 0
            if i:
                assert ws(frames[i - 1], lo, hi) <= ws(T, lo, hi)
            if j:
                assert ws(T, *ranges[j - 1]) <= ws(T, lo, hi)
    assert ws(800, 36, 367) == 800 * 332 * 2


def test_python_owner_refuses_on_the_host():
    from efficient_tts_amd import pitch as T
    for bad in (dict(unvoiced_cost=-0.1), dict(octave_cost=16.5), dict(jump_cost=float("nan")), dict(vuv_cost=17.0)):
        with pytest.raises(ValueError):
            T.ViterbiSmoother("cpu", 22050, 36, 367, **bad)
    for lo, hi in ((1, 367), (36, 37), (36, 1025)):
        with pytest.raises(ValueError):
            T.ViterbiSmoother("cpu", 22050, lo, hi)
    assert T.cost_q16("x", 0.15) == 9830 and T.cost_q16("x", 16.0) == 16 * 65536 and T.cost_q16("x", 0.0) == 0
    lg = T.log2_table(1024).numpy()
    assert lg.dtype == np.int32 and (lg == V.log2_table(1024)).all() and lg[1] == 0 and lg[2] == 65536 and lg[1024] == 10 * 65536 and lg[3] == 103872


def test_reference_quantisation_and_ties():
    x = np.array([0.0, 0.5, 1.0 - 2.0 ** -17, 3.9999998, 4.0, 7.0, np.inf, np.nan, -np.inf, -5.0, 2.0 ** -17, 3.0 * 2.0 ** -17], dtype=np.float32)
    want = [0, 32768, 65536, 262144, 262144, 262144, 262144, 262144, -262144, -262144, 0, 2]        # rint: halves go to the even neighbour
    assert V.quantise(x).tolist() == want
    # constant d': every voiced state costs the same but for the octave term; with that at 0 only the tie rule is left, and the lowest state wins
    flat = np.full((6, 9), 0.1, dtype=np.float32)
    lag, states = V.viterbi_reference(flat, 2, 8, octave_cost=0.0)
    assert lag.tolist() == [2] * 6 and states.tolist() == [0] * 6
    lag, _ = V.viterbi_reference(np.full((6, 9), 0.5, dtype=np.float32), 2, 8, octave_cost=0.0)
    assert lag.tolist() == [0] * 6
    assert V.viterbi_reference(np.zeros((0, 9), np.float32), 2, 8)[0].shape == (0,)


def test_reference_removes_the_octave_glitch():
    x = V.glitch_signal()
    assert x.shape == (8000,) and abs(np.abs(x).max() - 0.9) < 1e-12
    r, lag = smoothed(x)
    assert lag.shape == (31,)
    print("yin   ", r["tau"].tolist())
    print("smooth", lag.tolist())
    assert all(72 <= r["tau"][t] <= 74 for t in (13, 14, 15))
    assert all(146 <= lag[t] <= 148 for t in range(2, 31))


def test_reference_leaves_clean_tones_alone():
    for name, fa, fb in P.TONES:
        x, _ = P.tone(fa, fb, P.TONE_SAMPLES)
        r, lag = smoothed(x)
        voiced = r["tau"] > 0
        assert voiced.sum() >= 15, name
        assert (np.abs(lag[voiced] - r["tau"][voiced]) <= 1).all(), (name, r["tau"].tolist(), lag.tolist())


def test_reference_keeps_noise_unvoiced_between_tones():
    t = np.arange(3000) / P.SR
    rng = np.random.default_rng(3)
    x = np.concatenate([0.9 * np.sin(2 * np.pi * 200.0 * t), 0.3 * rng.standard_normal(3000), 0.9 * np.sin(2 * np.pi * 220.0 * t)])
    _, lag = smoothed(x)
    print("smooth", lag.tolist())
    assert lag.shape == (35,) and (lag[12:25] == 0).all()
    assert (lag[2:11] == 110).all() and (lag[26:] == 100).all()                     # the tones, away from the seams and the reflected start
    assert set(lag[:2].tolist()) <= {0, 110} and lag[11] in (0, 110) and lag[25] in (0, 100)
    _, lag = smoothed(np.zeros(4000))
    assert (lag == 0).all()


def test_cli_switches():
    from efficient_tts_amd.bin import inference as I
    from efficient_tts_amd.bin import score as C
    base = ["--checkpoint", "c.pkl", "--test_fid_scp", "t.txt", "--outdir", "o"]
    assert C.get_parser().parse_args(base).f0_smooth is False and I.get_parser().parse_args(base).f0_smooth is False
    a = C.get_parser().parse_args(base + ["--f0", "--f0_smooth", "--vocoder", "griffinlim"])
    assert a.f0 and a.f0_smooth
    C.check_f0_args(a)
    with pytest.raises(ValueError, match="--f0_smooth"):
        C.run_score(C.get_parser().parse_args(base + ["--f0_smooth"]))             # before the device, the checkpoint or the list is touched
    a = I.get_parser().parse_args(base + ["--write_f0", "--f0_smooth"])
    assert a.write_f0 and a.f0_smooth
    I.check_f0_smooth(a)
    with pytest.raises(ValueError, match="--f0_smooth"):
        I.run_tts(I.get_parser().parse_args(base + ["--f0_smooth"]))
