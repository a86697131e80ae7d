"""Every launch of the on-device audio kernels writes, bit for bit, what the commit named in tests/golden/audio_digests.json wrote
(tests/record_audio_digests.py, run against a library built from that commit, records the file): a change of csrc/ that is meant to keep
their results -- moving the paired-frame STFT analysis into shared helpers, say -- keeps these.

One batch serves every launch: seeded noise plus a tone with a quiet stretch, B = 4, row stride 20480, lengths 512 (no frame at N = 1024),
700 (three frames, all reflected, the last one unpaired), 9000 (shorter than one denoiser run) and 20000 (two denoiser workgroups); fp32 and
int16 PCM where the entry point takes both.  Every output buffer and workspace starts from a canary, and the digest is the sha256 of all of
them, padding included.
"""
import hashlib
import json
import math
import os

import pytest
import torch

from kernel_check import _call, _dev, _st, load_lib

pytestmark = pytest.mark.gpu

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio_digests.json")
B, LD, LENGTHS, MAX_LEN = 4, 20480, (512, 700, 9000, 20000), 20000
PCM_SCALE = 1.0 / 32768.0


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _sha(*buffers):
    h = hashlib.sha256()
    for t in buffers:
        h.update(t.cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:32]


def _signals():
    """(x fp32, x int16, y fp32, y int16) [B][LD] on the host: whole rows are filled, the samples behind an item's length too"""
    g = torch.Generator().manual_seed(20251)
    n = torch.arange(LD, dtype=torch.float64)
    env = torch.ones(LD, dtype=torch.float64)
    env[2000:6000] = 0.02                                        # the quiet stretch that the noise profile and the trimmer find
    out = []
    for k in range(2):
        noise = torch.randn(B, LD, generator=g, dtype=torch.float64)
        tone = torch.sin(2 * math.pi * (220.0 + 40.0 * k) / 22050.0 * n)
        x = (env * (0.08 * noise + 0.4 * tone)).clamp(-1, 1)
        q = (x * 32767.0).round().to(torch.int16)
        out += [x.float(), q]
    return out


def audio_digests(lib):
    """{"<launch>": sha256 of its raw output buffers}"""
    dev = _dev()
    xf, xq, yf, yq = (t.to(dev) for t in _signals())
    lengths = torch.tensor(LENGTHS, dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(7)
    st = _st()
    out = {}

    def canary(*shape, dtype=torch.float32):
        return torch.full(shape, -7, dtype=dtype, device=dev)

    def rand(*shape):
        return torch.rand(*shape, generator=g).to(dev)

    def hann(n):
        return torch.hann_window(n, periodic=True, dtype=torch.float64).float().to(dev)

    def both(name, run):
        """run(audio, pcm16 flag, scale) -> buffers, once per sample format"""
        out[name + "/fp32"] = _sha(*run(xf, 0, 1.0))
        out[name + "/int16"] = _sha(*run(xq, 1, PCM_SCALE))

    # ---- the log-mel front-end: 80 filters, 64 narrow ones and 16 wide ones, spans in ascending order
    T = LD // 256
    basis = torch.zeros(80, 513)
    ranges = torch.zeros(80, 2, dtype=torch.int32)
    for m in range(80):
        lo = 2 + 6 * m if m < 64 else 380 + 6 * (m - 64)
        hi = lo + 12 if m < 64 else min(lo + 40, 513)
        basis[m, lo:hi] = torch.rand(hi - lo, generator=g) * 0.1
        ranges[m, 0], ranges[m, 1] = lo, hi
    basis, ranges, w1024 = basis.to(dev), ranges.to(dev), hann(1024)

    def logmel(a, pcm, scale):
        o = canary(B, T, 80)
        if pcm:
            _call("efts_logmel_fft_pcm16", lib.efts_logmel_fft_pcm16(a.data_ptr(), LD, scale, lengths.data_ptr(), w1024.data_ptr(), basis.data_ptr(),
                                                                      ranges.data_ptr(), o.data_ptr(), B, T, 1024, 256, 80, st))
        else:
            _call("efts_logmel_fft", lib.efts_logmel_fft(a.data_ptr(), LD, lengths.data_ptr(), w1024.data_ptr(), basis.data_ptr(), ranges.data_ptr(), o.data_ptr(),
                                                          B, T, 1024, 256, 80, st))
        return [o]
    both("logmel_fft", logmel)

    # ---- STFT magnitudes and distance: hop N / 4; the window shorter than the frame at two of the sizes
    for N in (256, 512, 1024, 2048):
        H, W = N // 4, N if N in (256, 2048) else 3 * N // 4
        win, T_max = hann(W), 1 + MAX_LEN // H

        def mag(a, pcm, scale):
            o, fr = canary(B, T_max, N // 2 + 1), canary(B, dtype=torch.int32)
            _call("efts_stft_mag", lib.efts_stft_mag(a.data_ptr(), pcm, scale, LD, lengths.data_ptr(), MAX_LEN, win.data_ptr(), o.data_ptr(), fr.data_ptr(), B, N, H, W, st))
            return [o, fr]
        both(f"stft_mag/{N}", mag)
        if N in (512, 2048):
            nbytes = lib.efts_stft_dist_workspace_bytes(B, MAX_LEN, N, H)
            for name, x, y, pcm in (("fp32", xf, yf, 0), ("int16", xq, yq, 1)):
                sums, cells, ws = canary(B, 3, dtype=torch.float64), canary(B, dtype=torch.int64), canary(nbytes, dtype=torch.uint8)
                _call("efts_stft_dist", lib.efts_stft_dist(x.data_ptr(), pcm, LD, y.data_ptr(), pcm, LD, PCM_SCALE, lengths.data_ptr(), MAX_LEN, win.data_ptr(),
                                                            sums.data_ptr(), cells.data_ptr(), ws.data_ptr(), nbytes, B, N, H, W, st))
                out[f"stft_dist/{N}/{name}"] = _sha(sums, cells, ws)

    # ---- the projection of the log spectrum: 24 coefficients
    table, T_max = (rand(24, 513) - 0.5), 1 + MAX_LEN // 256

    def project(a, pcm, scale):
        o, fr = canary(B, T_max, 24), canary(B, dtype=torch.int32)
        _call("efts_logspec_project", lib.efts_logspec_project(a.data_ptr(), pcm, scale, LD, lengths.data_ptr(), MAX_LEN, w1024.data_ptr(), table.data_ptr(), 24,
                                                                o.data_ptr(), fr.data_ptr(), B, 1024, 256, 1024, st))
        return [o, fr]
    both("logspec_project/24", project)

    # ---- denoiser, gate (item 2 bypassed), noise profile
    bias, profile = rand(513) * 2.0, rand(B, 513) * 2.0
    bypass = torch.tensor([0, 0, 1, 0], dtype=torch.int32, device=dev)
    o, fr, ws = canary(B, LD), canary(B, dtype=torch.int32), canary(16, dtype=torch.uint8)
    _call("efts_denoise", lib.efts_denoise(xf.data_ptr(), LD, lengths.data_ptr(), MAX_LEN, w1024.data_ptr(), bias.data_ptr(), 1.0, o.data_ptr(), LD, fr.data_ptr(),
                                            ws.data_ptr(), 16, B, st))
    out["denoise/fp32"] = _sha(o, fr)

    def gate(a, pcm, scale):
        o, fr = canary(B, LD), canary(B, dtype=torch.int32)
        _call("efts_spectral_gate", lib.efts_spectral_gate(a.data_ptr(), pcm, scale, LD, lengths.data_ptr(), MAX_LEN, w1024.data_ptr(), profile.data_ptr(), 513, 1.5, 0.1,
                                                            bypass.data_ptr(), o.data_ptr(), LD, fr.data_ptr(), B, st))
        return [o, fr]
    both("spectral_gate", gate)

    nbytes = lib.efts_noise_profile_workspace_bytes(B, MAX_LEN)

    def noise(a, pcm, scale):
        prof, nf, fr, db = canary(B, 513), canary(B, dtype=torch.int32), canary(B, dtype=torch.int32), canary(B, dtype=torch.float64)
        ws = canary(nbytes, dtype=torch.uint8)
        _call("efts_noise_profile", lib.efts_noise_profile(a.data_ptr(), pcm, scale, LD, lengths.data_ptr(), MAX_LEN, w1024.data_ptr(), 100.0, 1, prof.data_ptr(), 513,
                                                            nf.data_ptr(), fr.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes, B, st))
        return [prof, nf, fr, db]
    both("noise_profile", noise)

    # ---- Griffin-Lim: three iterations per phase mode, then the signal; and the plain analysis of a padded signal
    GT = 40
    gmag, gframes = rand(B, GT, 513), torch.tensor([0, 3, 35, 40], dtype=torch.int32, device=dev)
    for mode in (0, 1):
        spec, prev, wf = canary(B, GT, 513, 2), canary(B, GT, 513, 2), canary(B, GT, 1024)
        _call("efts_gl_init", lib.efts_gl_init(gmag.data_ptr(), spec.data_ptr(), prev.data_ptr(), B, GT, mode, 1234, st))
        for _ in range(3):
            _call("efts_gl_synthesis", lib.efts_gl_synthesis(spec.data_ptr(), gframes.data_ptr(), w1024.data_ptr(), wf.data_ptr(), B, GT, 1024, 256, st))
            _call("efts_gl_analysis", lib.efts_gl_analysis(wf.data_ptr(), 0, 0, gframes.data_ptr(), w1024.data_ptr(), gmag.data_ptr(), prev.data_ptr(), spec.data_ptr(),
                                                            0.99, B, GT, 1024, 256, st))
        _call("efts_gl_synthesis", lib.efts_gl_synthesis(spec.data_ptr(), gframes.data_ptr(), w1024.data_ptr(), wf.data_ptr(), B, GT, 1024, 256, st))
        wave = canary(B, 256 * GT)
        _call("efts_gl_overlap_add", lib.efts_gl_overlap_add(wf.data_ptr(), gframes.data_ptr(), w1024.data_ptr(), wave.data_ptr(), 256 * GT, 384, 256 * GT, B, GT, 1024,
                                                              256, st))
        out[f"griffin_lim/mode{mode}"] = _sha(spec, prev, wf, wave)
    spec = canary(B, GT, 513, 2)
    _call("efts_gl_analysis", lib.efts_gl_analysis(0, xf.data_ptr(), LD, gframes.data_ptr(), w1024.data_ptr(), 0, 0, spec.data_ptr(), 0.0, B, GT, 1024, 256, st))
    out["griffin_lim/analysis_of_signal"] = _sha(spec)

    # ---- trimmer
    def trim(a, pcm, scale):
        nbytes = lib.efts_trim_workspace_bytes(B, LD, 256, pcm)
        o, ws = canary(B, LD), canary(nbytes, dtype=torch.uint8)
        nl, start, gain = canary(B, dtype=torch.int32), canary(B, dtype=torch.int32), canary(B)
        if pcm:
            _call("efts_trim_pcm16", lib.efts_trim_pcm16(a.data_ptr(), LD, lengths.data_ptr(), 1024, 256, 100.0, 1, 0.9, scale, o.data_ptr(), LD, nl.data_ptr(),
                                                          start.data_ptr(), gain.data_ptr(), ws.data_ptr(), B, st))
        else:
            _call("efts_trim", lib.efts_trim(a.data_ptr(), LD, lengths.data_ptr(), 1024, 256, 100.0, 1, 0.9, o.data_ptr(), LD, nl.data_ptr(), start.data_ptr(),
                                              gain.data_ptr(), ws.data_ptr(), B, st))
        return [o, nl, start, gain]
    both("trim", trim)

    # ---- YIN pitch with the d' rows (tau_max = 22050 / 60 = 367)
    def yin(a, pcm, scale):
        f0, ap, cm = canary(B, T), canary(B, T), canary(B, T, 368)
        if pcm:
            _call("efts_yin_pcm16", lib.efts_yin_pcm16(a.data_ptr(), LD, scale, lengths.data_ptr(), f0.data_ptr(), ap.data_ptr(), cm.data_ptr(), B, T, 1024, 256, 22050,
                                                        60.0, 400.0, 0.1, st))
        else:
            _call("efts_yin", lib.efts_yin(a.data_ptr(), LD, lengths.data_ptr(), f0.data_ptr(), ap.data_ptr(), cm.data_ptr(), B, T, 1024, 256, 22050, 60.0, 400.0, 0.1, st))
        return [f0, ap, cm]
    both("yin", yin)

    # ---- resampler, ratio 2 / 3; any table will do for the bits
    rtab, ld_out = (rand(2, 17) - 0.5), (LD * 2 + 2) // 3

    def resample(a, pcm, scale):
        o, ol = canary(B, ld_out), canary(B, dtype=torch.int32)
        if pcm:
            _call("efts_resample_pcm16", lib.efts_resample_pcm16(a.data_ptr(), LD, scale, lengths.data_ptr(), rtab.data_ptr(), 2, 3, 8, o.data_ptr(), ld_out, ol.data_ptr(),
                                                                  B, st))
        else:
            _call("efts_resample", lib.efts_resample(a.data_ptr(), LD, lengths.data_ptr(), rtab.data_ptr(), 2, 3, 8, o.data_ptr(), ld_out, ol.data_ptr(), B, st))
        return [o, ol]
    both("resample/2:3", resample)
    torch.cuda.synchronize()
    return out


def test_audio_bits_equal_the_recorded_launches(lib):
    """Every launch writes, bit for bit, what the commit named in tests/golden/audio_digests.json wrote."""
    with open(DIGESTS) as f:
        want = json.load(f)["digests"]
    got = audio_digests(lib)
    assert sorted(got) == sorted(want), "the launches differ from the recorded set"
    bad = sorted(k for k in got if got[k] != want[k])
    assert not bad, f"{len(bad)} of {len(got)} launches differ from the recorded bits: {bad}"
