"""No GPU: the table of the waveform mel-cepstra against tests/mcep_reference.py (which restates the analysis without a table), the condition on
the inputs of tests/test_mcep_gpu.py, what the two entries and the host classes refuse before any launch, and the header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mcep_reference as R

from efficient_tts_amd import mcep as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_known_mel_cepstrum_comes_back_through_the_table():
    """ln|X| = sum_m c~[m] cos(m w~), w~ = w + 2 atan2(alpha sin w, 1 - alpha cos w): the table applied to ln P = 2 ln|X| returns c~[1 .. M] --
    the warp direction and every scale factor at once"""
    rng = np.random.default_rng(1)
    for alpha in (0.455, 0.42, 0.554):
        c = 0.3 * rng.standard_normal(R.ORDER + 1)
        L = 2.0 * R.warped_log_magnitude(c, alpha)
        table = M.mcep_table(R.N, R.ORDER, alpha)
        assert table.dtype == np.float64 and table.shape == (R.ORDER, R.K + 1)
        assert np.abs(table @ L - c[1:]).max() <= 1e-13
        assert np.abs(R.mel_cepstrum_of_log_power(L, R.ORDER, alpha) - c[1:]).max() <= 1e-13       # and through the reference's own route
    table = M.mcep_table()
    assert np.abs(table).max() < 5.3e-3 and np.abs(table).sum(axis=1).max() < 0.64


def test_the_table_equals_the_reference_analysis_of_every_unit_spectrum():
    table = M.mcep_table(R.N, R.ORDER, R.ALPHA)
    ref = R.mel_cepstrum_of_log_power(np.eye(R.K + 1)).T                # column f: the analysis of the log power spectrum e_f
    assert np.abs(table - ref).max() <= 1e-15
    small = M.mcep_table(64, 5, 0.3)
    assert np.abs(small - R.mel_cepstrum_of_log_power(np.eye(33), 5, 0.3).T).max() <= 1e-15


def test_alpha_zero_gives_the_plain_truncated_cepstrum():
    A = M.freqt_matrix(R.K + 1, R.ORDER, 0.0)
    assert np.array_equal(A, np.eye(R.ORDER + 1, R.K + 1))             # the identity followed by zeros
    rng = np.random.default_rng(2)
    L = rng.standard_normal((3, R.K + 1))
    plain = R.one_sided_cepstrum(0.5 * L)[:, 1:R.ORDER + 1]
    assert np.abs(L @ M.mcep_table(R.N, R.ORDER, 0.0).T - plain).max() <= 1e-15


def test_rows_annihilate_a_constant_log_spectrum():
    for alpha in (0.0, 0.455, 0.554):
        assert np.abs(M.mcep_table(R.N, R.ORDER, alpha) @ np.full(R.K + 1, np.log(1e-7))).max() <= 1e-13
    assert np.abs(R.mel_cepstrum(np.zeros(2049))).max() <= 1e-13      # the clamp case: every cell at exactly 1e-7


def test_defaults_and_what_the_host_side_refuses():
    assert M.ALPHAS == {16000: 0.42, 22050: 0.455, 24000: 0.466, 44100: 0.544, 48000: 0.554}
    m = M.MelCepstrum(None)
    assert (m.sampling_rate, m.n_fft, m.hop, m.win_length, m.order, m.alpha, m.max_wav_value) == (22050, 1024, 256, 1024, 24, 0.455, 32768.0)
    assert m.table.dtype == np.float32 and np.array_equal(m.table, M.mcep_table().astype(np.float32))
    assert M.MelCepstrum(None, 48000).alpha == 0.554 and M.MelCepstrum(None, 8000, alpha=0.31).alpha == 0.31
    for bad, match in ((dict(sampling_rate=8000), "alpha"), (dict(sampling_rate=22050.0), "integer"), (dict(n_fft=512), "n_fft"), (dict(hop_size=0), "hop_size"),
                       (dict(hop_size=1025), "hop_size"), (dict(win_length=1), "win_length"), (dict(order=0), "order"), (dict(order=33), "order"),
                       (dict(alpha=1.0), "alpha"), (dict(max_wav_value=0.0), "max_wav_value")):
        with pytest.raises(ValueError, match=match):
            M.MelCepstrum(None, **bad)
    x = torch.zeros(2, 4000)
    with pytest.raises(RuntimeError, match="no CPU path"):             # a host tensor is refused like everywhere else
        m(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.WaveformMCD(None)(x, None, x, None)
    with pytest.raises(ValueError, match="no path"):
        M.WaveformMCD(None)(x, None, x, None, aligned=True, return_path=True)
    for bad in (torch.zeros(4000), torch.zeros(2, 4000, dtype=torch.float64), torch.zeros(2, 0)):
        with pytest.raises(ValueError):
            m(bad)


def test_the_inputs_of_the_gpu_test_keep_every_power_cell_a_hundred_times_above_the_clamp():
    """ln of a near-null bin is ill-conditioned, and that is not what the GPU test is about"""
    assert R.LENGTHS == (0, 512, 513, 1024, 2049, 12345)
    for _, pcm16, H, W in R.CONFIGS:
        for variant in (0, 1):
            ref = R.reference_batch(pcm16, H, W, variant)
            assert [len(mc) for mc, _ in ref] == [0, 0] + [1 + L // H for L in R.LENGTHS[2:]]
            assert all(low >= 1e-5 for _, low in ref), (pcm16, H, W, variant, [low for _, low in ref])
    x16, _ = R.batch(True)
    x32, _ = R.batch(False)
    assert np.array_equal(x32, x16.astype(np.float32) / np.float32(32768.0)) and np.abs(x16).max() < 32000
    assert len(R.reference_batch()[2][0]) == 3                          # 513 samples: an odd count, the last transform has no partner
    n = 2049                                                            # the noise lies 40 dB under the harmonics
    assert abs(10 * np.log10(np.var(R.signal(n, 4, 7) - R.signal(n, 4, 7, noise_db=-400.0)) / np.var(R.signal(n, 4, 7, noise_db=-400.0))) + 40.0) < 1.0
    for _, pcm16, H, W in R.CONFIGS:
        assert 0.0 < R.yardstick(pcm16, H, W) < 1e-4                    # an fp32 rounding error on values of at most a few tenths


def test_header_has_the_section_and_stays_at_revision_602():
    hdr = open(os.path.join(ROOT, "include", "efts_abi.h")).read()
    assert int(re.search(r"#define EFTS_ABI_VERSION (\d+)", hdr).group(1)) == 602
    assert re.search(r"\+ efts_logspec_project, efts_frame_dist", hdr) and "Oppenheim's recursion" in hdr
    for name in ("efts_logspec_project", "efts_frame_dist"):
        assert re.search(r"\bint %s\s*\(" % name, hdr)


def test_library_exports_and_refuses_on_the_host():
    """both entry points are bound, and every refusal of the header comes back before anything is launched (no device needed)"""
    from efficient_tts_amd import build as B
    from efficient_tts_amd import lib as L
    B.build(verbose=False)
    lib = L.load()
    assert lib.efts_version() == 602
    for name in ("efts_logspec_project", "efts_frame_dist"):
        assert name in L.exported_symbols() and hasattr(lib, name)
    # host arrays stand in for device memory: a call that passes every check would launch, so every call below fails one check
    n = 2048
    f = (ctypes.c_float * (40 * 513 + n))()
    d = (ctypes.c_double * 8)()
    ints = (ctypes.c_int32 * 32)()
    A, D, I = ctypes.addressof(f), ctypes.addressof(d), ctypes.addressof(ints)
    EINVAL, ESHAPE = -1, -2
    good = dict(audio=A, pcm16=0, ld=n, lengths=I, max_len=n, window=A, table=A, n_coef=24, out=A, frames=I + 32, B=2, N=1024, H=256, W=1024)

    def project(**kw):
        a = dict(good, **kw)
        return lib.efts_logspec_project(a["audio"], a["pcm16"], 1.0 / 32768.0, a["ld"], a["lengths"], a["max_len"], a["window"], a["table"], a["n_coef"],
                                        a["out"], a["frames"], a["B"], a["N"], a["H"], a["W"], None)
    shape = [dict(N=512), dict(N=2048), dict(N=256), dict(N=0), dict(n_coef=0), dict(n_coef=33), dict(n_coef=-1), dict(B=0), dict(B=65536), dict(B=-1),
             dict(ld=n - 1), dict(H=0), dict(H=1025), dict(W=1), dict(W=1025), dict(max_len=0), dict(max_len=2 ** 31 - 8192, ld=2 ** 31)]
    inval = [dict(audio=None), dict(lengths=None), dict(window=None), dict(table=None), dict(out=None), dict(frames=None),
             dict(audio=A + 2), dict(audio=A + 1, pcm16=1), dict(lengths=I + 2), dict(window=A + 1), dict(table=A + 2), dict(out=A + 3), dict(frames=I + 33)]
    for code, cases in ((ESHAPE, shape), (EINVAL, inval)):
        for kw in cases:
            rc = project(**kw)
            msg = lib.efts_last_error()
            assert rc == code and msg.startswith(b"efts_logspec_project:"), (kw, rc, msg)
    good = dict(x=A, ldx=24, sx=24 * 50, xf=I, Tx=50, y=A, ldy=24, sy=24 * 50, yf=I + 16, Ty=50, D=24, cost=D, count=I + 32, B=2)

    def dist(**kw):
        a = dict(good, **kw)
        return lib.efts_frame_dist(a["x"], a["ldx"], a["sx"], a["xf"], a["Tx"], a["y"], a["ldy"], a["sy"], a["yf"], a["Ty"], a["D"], a["cost"], a["count"],
                                   a["B"], None)
    shape = [dict(D=0), dict(D=33), dict(B=0), dict(B=65536), dict(Tx=0), dict(Ty=0), dict(ldx=23), dict(ldy=23), dict(sx=-1), dict(sy=-1)]
    inval = [dict(x=None), dict(xf=None), dict(y=None), dict(yf=None), dict(cost=None), dict(count=None), dict(x=A + 2), dict(y=A + 1), dict(xf=I + 2),
             dict(yf=I + 17), dict(cost=D + 4), dict(count=I + 33)]
    for code, cases in ((ESHAPE, shape), (EINVAL, inval)):
        for kw in cases:
            rc = dist(**kw)
            msg = lib.efts_last_error()
            assert rc == code and msg.startswith(b"efts_frame_dist:"), (kw, rc, msg)
