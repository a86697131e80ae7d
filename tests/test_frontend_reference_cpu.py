"""No device: tests/frontend_reference.py against the committed fixture and against itself, and the conditions on its inputs that
tests/test_frontend_kernels_gpu.py relies on (no compared cell near the clamp, every `_check` case well conditioned, the filterbanks on the
side of every table limit the GPU tests say they are on)."""
import os

import numpy as np
import pytest
import torch

import frontend_reference as R
from kernel_check import conditioned

GOLD = os.path.join(os.path.dirname(__file__), "golden", "logmel_small.npz")
RADIX_CASES = ((1024, 2), (1024, 4), (1024, 8), (1024, 16), (512, 2), (512, 4))


def test_reference_matches_the_committed_fixture():
    """the float64 restatement against the fp32 torch.stft oracle's recorded output: 2e-4 in the log domain, the margin test_frontend.py uses for
    fp32 torch.stft against a float64 DFT"""
    g = np.load(GOLD)
    basis, _ = R.slaney_bank(80, 8000.0)
    T = g["mel"].shape[1]
    for b, L in enumerate(g["lengths"]):
        pcm = g["audio"][b, :int(L)]
        assert R.frame_count(len(pcm)) == int(g["frames"][b])
        ref = R.pad_rows(R.logmel(pcm, basis), T)
        err = np.abs(ref - g["mel"][b]).max()
        print(f"item {b}: float64 reference against the fixture {err:.2e}")
        assert err < 2e-4
        assert not ref[int(g["frames"][b]):].any()


def test_frames_are_the_definition_written_out():
    """reflect padding without edge repeat, T = L // hop, the periodic window: against plain loops on a short item"""
    pcm, _ = R.signal(700, 1)
    x = pcm.astype(np.float64) / 32768.0
    fr = R.frames(pcm, 512, 128)
    assert fr.shape == (5, 512)
    w = R.window(512).astype(np.float64)
    assert w[0] == 0.0 and w[256] == 1.0 and w[1] == w[511]
    for t in (0, 4):
        for k in (0, 1, 191, 192, 400, 511):
            s = t * 128 + k - 192
            s = -s if s < 0 else s
            s = 2 * (700 - 1) - s if s >= 700 else s
            assert fr[t, k] == x[s] * w[k]


@pytest.mark.parametrize("n_fft,radix", RADIX_CASES)
def test_deinterleave_and_recombine(n_fft, radix):
    pcm, _ = R.signal(4 * n_fft + 3, 2)
    fr = R.frames(pcm, n_fft, n_fft // 4)
    de = R.deinterleave(fr, radix)
    M = n_fft // radix
    for p in range(radix):
        assert np.array_equal(de[:, p * M:(p + 1) * M], fr[:, p::radix])
    X = R.recombine(R.radix_rows(fr, radix), radix)
    ref = np.fft.rfft(fr, axis=1)
    assert np.abs(X - ref).max() <= 1e-12 * np.abs(ref).max()
    rows = R.radix_rows(fr, radix)
    for p in range(radix):                                    # block p of a row: the real M-point DFT of columns p M .. of the de-interleaved frame
        Y = np.fft.rfft(de[:, p * M:(p + 1) * M], axis=1)
        assert np.array_equal(rows[:, p * M:p * M + M // 2 + 1], Y.real) and np.array_equal(rows[:, p * M + M // 2 + 1:(p + 1) * M], Y.imag[:, 1:M // 2])


def test_clamp_conditions():
    """every mel energy of the `signal` items at least 100 x the clamp, silence below clamp / 2 in every filter: for the four Slaney banks and the
    two ragged ones"""
    banks = [R.slaney_bank(n, f)[0] for n, f in R.SLANEY] + [R.ragged_bank(0)[0], R.ragged_bank(1)[0]]
    lowest, loudest = np.inf, 0.0
    for i, basis in enumerate(banks):
        # (the persistent-loop case runs on the (80, 8000) bank alone)
        for name, pcm, _ in R.items() + (R.persistent_items(R.PERSISTENT_MAX_B) if i == 0 else ()):
            if name in ("silence", "square"):
                continue
            e = R.mel_energy(R.magnitude(R.spectrum(pcm)), basis)
            live = basis.any(axis=1)
            lowest = min(lowest, float(e[:, live].min()))
        quiet = R.mel_energy(R.magnitude(R.spectrum(R.items()[R.SILENT][1])), basis)
        loudest = max(loudest, float(quiet.max()))
    print(f"lowest mel energy of a signal item {lowest:.3e}, largest of the silent item {loudest:.3e}")
    assert lowest >= 100 * R.CLAMP
    assert loudest < R.CLAMP / 2


def test_every_fused_case_is_conditioned():
    """kernel_check.conditioned for every item x bank that test_fused_whole_banks and test_fused_persistent_loop pass to `_check`"""
    worst = 0.0
    for i, (bank, (basis, _)) in enumerate(R.whole_banks()):
        its = R.items() + (R.persistent_items(R.PERSISTENT_MAX_B) if i == 0 else ())
        for name, pcm, f32 in its:
            ref64 = torch.from_numpy(R.logmel(pcm, basis))
            ok, e32 = conditioned(ref64, R.logmel32(f32, basis))
            if (name, bank) in R.ILL_CONDITIONED:
                print(f"{name} x {bank}: e32 {e32:.3e}, left to the per-cell bound")
                assert not ok
                continue
            worst = max(worst, e32)
            assert ok, (bank, name, e32)
    print(f"largest e32 of a fused case {worst:.3e}")


def test_every_stage_case_is_conditioned():
    """the same for the cases of efts_logmel and efts_logmel_dit alone (Slaney, ragged and fat banks on the reference spectrum / radix rows cast to fp32)"""
    worst = 0.0
    for n_fft, hop in ((1024, 256), (512, 128)):
        nb = n_fft // 2 + 1
        fr = R.stage_frames(n_fft)
        spec = np.fft.rfft(fr, axis=1)
        re, im = spec.real.astype(np.float32), spec.imag.astype(np.float32)
        banks = [R.slaney(80, 8000.0, n_fft=n_fft), R.slaney(130, 8000.0, n_fft=n_fft), R.slaney(1, 8000.0, n_fft=n_fft), R.slaney(128, 8000.0, n_fft=n_fft),
                 R.slaney(129, 8000.0, n_fft=n_fft), R.ragged_bank(0, nb)[0], R.ragged_bank(1, nb)[0]] + ([R.fat_bank()[0]] if n_fft == 1024 else [])
        for basis in banks:
            ref64 = R.log_clamp(R.mel_energy(np.sqrt(re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2 + R.MAG_EPS), basis))
            ok, e32 = conditioned(torch.from_numpy(ref64), R.logmel_of_spectrum32(torch.from_numpy(re), torch.from_numpy(im), basis))
            worst = max(worst, e32)
            assert ok, (n_fft, basis.shape, e32)
            for radix in [r for n, r in RADIX_CASES if n == n_fft]:
                rows = R.radix_rows(fr, radix).astype(np.float32)
                tw = R.twiddles(radix, n_fft).astype(np.float32)
                X = R.recombine(rows, radix, tw)
                ref64 = R.log_clamp(R.mel_energy(R.magnitude(X), basis))
                xr, xi = R.recombine32(rows, radix, tw)
                ok, e32 = conditioned(torch.from_numpy(ref64), R.logmel_of_spectrum32(xr, xi, basis))
                worst = max(worst, e32)
                assert ok, (n_fft, radix, basis.shape, e32)
    print(f"largest e32 of a stage case {worst:.3e}")


def test_bank_properties():
    for n_mels, n_bins in ((80, 513), (80, 257)):
        banks = R.onehot_banks(n_mels, n_bins)
        narrow = np.zeros(n_bins, dtype=int)
        wide = np.zeros(n_bins, dtype=int)
        for basis, rng in banks:
            assert basis.shape == (n_mels, n_bins) and rng.shape == (n_mels, 2)
            for m in range(n_mels):
                lo, hi = rng[m]
                if hi == lo:
                    assert (lo, hi) == (0, 0) and not basis[m].any()
                    continue
                assert hi == lo + 1 and basis[m, lo] == 1.0 and basis[m].sum() == 1.0
                (narrow if m < R.FF_WIDE else wide)[lo] += 1
            assert R.fused_table_floats(rng) <= R.FF_CB
        assert (narrow == 1).all() and (wide == 1).all()
    for which in (0, 1):
        basis, rng = R.ragged_bank(which)
        assert basis.shape == (80, 513) and (basis >= 0).all() and np.array_equal(rng, R.ranges_of(basis))
        n = rng[:, 1] - rng[:, 0]
        assert set(R.RAGGED_NARROW[which]) <= set(n[:64].tolist()) and set(R.RAGGED_WIDE[which]) <= set(n[64:].tolist())
        assert n[:64].max() == max(R.RAGGED_NARROW[which]) and n[64:].max() == max(R.RAGGED_WIDE[which])
        for part in (slice(0, 64), slice(64, 80)):
            assert (n[part] == 0).sum() == 1 and (rng[part, 0][n[part] > 0] == 0).any() and (rng[part, 1] == 513).any()
        # S0 * 64 + 4 * SQ * 16 with the kernel's w0, w1, from the span lengths
        w0, w1 = (n[:64].max() + 3) // 4, (n[64:].max() + 15) // 16
        need = 4 * (w0 | 1) * 64 + 4 * 4 * (w1 | 1) * 16
        assert need == R.fused_table_floats(rng) and need <= R.FF_CB
        assert 513 + 4 * w0 <= 16 * 68 and 513 + 16 * w1 <= 16 * 68                 # the padded steps stay inside a wave's buffer
    assert set(R.RAGGED_NARROW[0]) | set(R.RAGGED_NARROW[1]) == {1, 3, 4, 5, 27}
    assert set(R.RAGGED_WIDE[0]) | set(R.RAGGED_WIDE[1]) == {1, 15, 16, 17, 63, 64, 65, 144}
    # all of those spans in ONE bank would need 28 * 64 + 144 * 16 = 4096 floats
    assert 4 * (7 | 1) * 64 + 16 * (9 | 1) * 16 > R.FF_CB
    basis, rng = R.fat_bank()
    assert basis.shape == (128, 513) and ((rng[:, 1] - rng[:, 0]) == 20).all() and np.array_equal(rng, R.ranges_of(basis))
    assert (rng[:, 1] - rng[:, 0]).sum() == 2560 > R.LM_CB
    # the Slaney banks: three fit the fused kernel's table, (64, 11025) does not and is the one that runs span_global
    need = {cfg: R.fused_table_floats(R.slaney_bank(*cfg)[1]) for cfg in R.SLANEY}
    print(need)
    assert need[(64, 11025.0)] == 3328 > R.FF_CB
    assert all(v <= R.FF_CB for cfg, v in need.items() if cfg != (64, 11025.0))
    assert (R.slaney_bank(80, 8000.0)[1][:, 1] - R.slaney_bank(80, 8000.0)[1][:, 0]).sum() <= R.LM_CB
    # DC and Nyquist: weight exactly 0 in every Slaney bank (why the one-hot banks exist)
    for cfg in R.SLANEY:
        b = R.slaney_bank(*cfg)[0]
        assert not b[:, 0].any() and not b[:, 512].any()


def test_constants_match_the_kernel_source():
    """FF_CB, FF_WIDE, LM_CB here against csrc/efts_frontend.hip"""
    import re
    src = open(os.path.join(os.path.dirname(__file__), "..", "efficient_tts_amd", "csrc", "efts_frontend.hip")).read()
    ff = re.search(r"FF_CB = (\d+), FF_WIDE = (\d+)", src)
    lm = re.search(r"LM_CB = (\d+)", src)
    assert (int(ff.group(1)), int(ff.group(2)), int(lm.group(1))) == (R.FF_CB, R.FF_WIDE, R.LM_CB)


def test_items_reach_the_branches():
    its = R.items()
    assert [n for n, _, _ in its] == list(R.ITEM_NAMES)
    lens = [len(p) for _, p, _ in its]
    assert lens[:4] == [385, 1408, 1407, 4099] and R.frame_count(385) == 1
    s0 = 2 * R.HOP - (R.N_FFT - R.HOP) // 2
    assert s0 + 20 * 64 == 1408 and R.frame_count(1408) == R.frame_count(1407) == 5
    sq = its[R.SQUARE][1]
    assert set(np.unique(sq).tolist()) == {-32768, 32767}
    for _, p, f in its:
        assert np.array_equal(f.astype(np.float64) * 32768.0, p.astype(np.float64))
    assert R.persistent_batch_size(256) * ((R.PERSISTENT_T + 1) // 2) > 12 * 256 and R.persistent_batch_size(256) <= R.PERSISTENT_MAX_B
