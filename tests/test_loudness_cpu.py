"""No GPU: the loudness definition as tests/loudness_reference.py restates it, on the standard's own conformance point and on cases worked out
by hand; the condition on the inputs of tests/test_loudness_gpu.py under which gate decisions must match exactly; what the host classes
refuse; the recipe and command-line plumbing; the header.
"""
import os
import re

import numpy as np
import pytest

import loudness_reference as R

from efficient_tts_amd import loudness as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ITU-R BS.1770-4, table 1 and table 2 (48 kHz)
TABLE = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
         1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]


def test_coefficients_at_48_khz_are_the_standards_table():
    got = S.k_weighting(48000)
    assert got.dtype == np.float64 and got.shape == (10,)
    assert np.abs(got - np.array(TABLE)).max() <= 1e-12
    bs, as_, bh, ah = R.coefficients(48000)
    assert np.abs(np.concatenate([bs, as_[1:], bh, ah[1:]]) - np.array(TABLE)).max() <= 1e-12
    for fs in (8000, 16000, 22050, 24000, 44100, 48000):            # product and reference state the same formulas
        bs, as_, bh, ah = R.coefficients(fs)
        assert as_[0] == ah[0] == 1.0
        assert np.array_equal(S.k_weighting(fs), np.concatenate([bs, as_[1:], bh, ah[1:]]))


def test_full_scale_997_hz_sine_measures_minus_3_01():
    fs = 48000
    x = np.sin(2.0 * np.pi * 997.0 * np.arange(3 * fs) / fs).astype(np.float32)
    res = R.measure(x, fs)
    print(f"997 Hz, 0 dBFS: {res['lufs']:.4f} LKFS, blocks {res['blocks']}")
    assert abs(res["lufs"] - -3.01) <= 0.01
    assert res["flags"] == 0 and res["blocks"] == (27, 27)            # 30 sub-blocks: 27 blocks, all of one level


def test_relative_gate_drops_the_quiet_blocks():
    rng = np.random.default_rng(5)
    fs = 22050
    x = R._bursts(rng, 3 * fs, fs).astype(np.float32)                # 0.5 s at 0.3, 0.5 s 50 dB under it, ...
    res = R.measure(x, fs)
    nA, nG = res["blocks"]
    print(f"bursts: {res['lufs']:.3f} LUFS, |A| {nA}, |G| {nG}")
    assert nA == 27 and 0 < nG < nA                                  # the quiet blocks are over the absolute gate (-66 LUFS) and under the relative one
    loud = R.measure(x[:fs // 2], fs)["lufs"]
    ungated = -0.691 + 10.0 * np.log10(res["z"].mean())
    assert ungated < res["lufs"] < loud                              # ... so the result lies over the plain average and under the bursts' own level
    # the gain brings the item to the target: measured again, it is there
    g = res["gain"]
    again = R.measure((x * g).astype(np.float32), fs, target=-23.0)
    assert res["flags"] == 0 and abs(again["lufs"] - -23.0) < 1e-4


def test_silence_and_short_items_have_no_loudness():
    fs = 22050
    for dtype in (np.int16, np.float32):
        for x in (np.zeros(3 * fs, dtype), np.zeros(0, dtype), np.full(4 * (fs // 10) - 1, 1000, dtype).astype(dtype)):
            res = R.measure(x, fs, ceiling=0.99)
            assert res["lufs"] == -np.inf and res["flags"] == 1 and res["blocks"][1] == 0
            assert res["gain"] == (np.float32(1.0 / 32768.0) if dtype == np.int16 else np.float32(1.0))
    assert R.measure(np.full(4 * (fs // 10), 1000, np.int16), fs)["blocks"][0] == 1     # exactly four sub-blocks: one block


def test_ceiling_limits_the_gain():
    rng = np.random.default_rng(6)
    fs = 16000
    x = rng.uniform(-0.02, 0.02, size=fs).astype(np.float32)
    x[::1000] = 0.9
    free = R.measure(x, fs, target=-14.0)
    res = R.measure(x, fs, target=-14.0, ceiling=0.5)
    assert free["flags"] == 0 and res["flags"] == 2 and res["gain"] < free["gain"]
    out = x * res["gain"]
    assert np.abs(out).max() <= 0.5 and np.abs(out).max() > 0.5 * (1 - 1e-6)
    assert R.measure(x, fs, target=-60.0, ceiling=0.5)["flags"] == 0  # a gain that stays under the ceiling is left alone


def test_gpu_inputs_keep_clear_of_both_gates():
    """every z_j of every input of tests/test_loudness_gpu.py, int16 and fp32, is at least 0.01 LU from both gates, and the ceiling decision
    is 0.1 % from its threshold: 1e4 times the device's tolerance of 1e-6 LU, so the counts and flags are compared with =="""
    for name, case in R.cases().items():
        for dtype in (np.int16, np.float32):
            for b, res in enumerate(R.reference(case, dtype)):
                print(f"{name} {np.dtype(dtype).name} item {b}: {res['lufs']:.4f} LUFS, blocks {res['blocks']}, flags {res['flags']}, "
                      f"margin {res['margin_lu']:.4f} LU, ceiling margin {res['ceiling_margin']:.4g}")
                assert res["margin_lu"] >= 0.01 and res["ceiling_margin"] >= 1e-3
    ref = R.reference(R.cases()["main"])
    assert ref[0]["blocks"][1] < ref[0]["blocks"][0] and ref[1]["flags"] == 0 and ref[2]["flags"] == 1 and ref[3]["flags"] == 1
    assert all(r["flags"] == 2 for r in R.reference(R.cases()["ceiling"]))
    assert all(r["flags"] == 0 and r["blocks"][0] > 0 for r in R.reference(R.cases()["edges"]) + R.reference(R.cases()["dc"]) + R.reference(R.cases()["48k"]))


def test_host_side_refusals():
    for bad in (dict(sampling_rate=11025), dict(sampling_rate=96000), dict(sampling_rate=7990), dict(sampling_rate=22050.0),
                dict(target_lufs=float("nan")), dict(target_lufs=float("inf")), dict(peak_ceiling=0.0), dict(peak_ceiling=float("nan")),
                dict(max_wav_value=0.0)):
        with pytest.raises(ValueError):
            S.LoudnessNormalizer(None, **bad)
    with pytest.raises(ValueError):
        S.LoudnessMeter(None, 11025)
    n = S.LoudnessNormalizer()
    assert (n.sampling_rate, n.target_lufs, n.peak_ceiling, n.max_wav_value) == (22050, -23.0, 0.99, 32768.0)
    assert S.LoudnessNormalizer(None, 48000, -27.0, None).peak_ceiling is None and S.LoudnessMeter(None, 8000).sampling_rate == 8000
    import torch
    with pytest.raises(ValueError):
        n(torch.zeros(4, dtype=torch.float32))
    with pytest.raises(RuntimeError):                                # no CPU path
        n(torch.zeros(1, 4, dtype=torch.float32))


def test_recipe_and_command_line_plumbing():
    from efficient_tts_amd.bin import inference as I
    from efficient_tts_amd.bin import loudness as C
    from efficient_tts_amd.bin.train import build_loudness, build_trimmer
    cfg = dict(frontend_params=dict(sampling_rate=16000, max_wav_value=32767.0))
    assert build_loudness({}) is None and build_loudness(dict(cfg, loudness_peak_ceiling=0.5)) is None and build_loudness(dict(normalize_loudness=None)) is None
    n = build_loudness(dict(cfg, normalize_loudness=-27))
    assert (n.sampling_rate, n.target_lufs, n.peak_ceiling, n.max_wav_value) == (16000, -27.0, 0.99, 32767.0)
    n = build_loudness(dict(normalize_loudness=-23.0, loudness_peak_ceiling=None, dataset_params=dict(sampling_rate=24000)))
    assert (n.sampling_rate, n.target_lufs, n.peak_ceiling) == (24000, -23.0, None)
    with pytest.raises(ValueError, match="normalize_peak"):          # level is set once
        build_loudness(dict(normalize_loudness=-23.0, normalize_peak=0.95))
    with pytest.raises(ValueError):
        build_loudness(dict(normalize_loudness=-23.0, frontend_params=dict(sampling_rate=11025)))
    assert build_trimmer(dict(normalize_loudness=-23.0)) is None     # the new key switches nothing else on
    assert build_loudness(dict(normalize_loudness=-23.0, trim_silence=True)).target_lufs == -23.0
    # synthesis
    base = ["--checkpoint", "exp/checkpoint-7steps.pkl", "--test_fid_scp", "t.txt", "--outdir", "o"]
    a = I.get_parser().parse_args(base)
    assert a.loudness is None and a.loudness_peak_ceiling == 0.99 and I.build_loudness(a) is None
    n = I.build_loudness(I.get_parser().parse_args(base + ["--loudness", "-23", "--loudness_peak_ceiling", "0.9"]))
    assert (n.sampling_rate, n.target_lufs, n.peak_ceiling) == (22050, -23.0, 0.9)
    assert I.build_loudness(I.get_parser().parse_args(base + ["--loudness", "-16", "--loudness_peak_ceiling", "0"])).peak_ceiling is None
    with pytest.raises(ValueError):
        I.build_loudness(I.get_parser().parse_args(base + ["--loudness", "-23", "--no_vocoder"]))
    with pytest.raises(ValueError):
        I.build_loudness(I.get_parser().parse_args(base + ["--loudness", "nan"]))
    # looking before training
    a = C.get_parser().parse_args(["--filelist", "f", "--wav_path", "d", "--outdir", "o"])
    assert (a.target, a.peak_ceiling, a.batch_size) == (-23.0, 0.99, 16) and C.COLUMNS == ("id", "seconds", "lufs", "gain_db", "limited")
    # the trainer has the attribute next to the trimmer, unset
    import torch
    from efficient_tts_amd.trainer import EfficientTTSTrainer
    t = EfficientTTSTrainer(steps=0, epochs=0, data_loader={}, sampler={}, model=torch.nn.Linear(2, 2), optimizer=None, scheduler=None,
                            config=dict(outdir="/tmp"))
    assert t.loudness is None and t.trimmer is None


def test_header_has_the_section_and_stays_at_revision_602():
    hdr = open(os.path.join(ROOT, "include", "efts_abi.h")).read()
    assert int(re.search(r"#define EFTS_ABI_VERSION (\d+)", hdr).group(1)) == 602
    assert "Integrated loudness after ITU-R BS.1770" in hdr
    assert int(re.search(r"#define EFTS_LOUDNESS_SEGMENT (\d+)", hdr).group(1)) == R.SEGMENT
    assert re.search(r"\+ efts_loudness, efts_loudness_pcm16, efts_loudness_workspace_bytes", hdr)
    for name in ("efts_loudness", "efts_loudness_pcm16", "efts_loudness_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, hdr)


def test_library_exports_and_refuses_on_the_host():
    """the three entry points are bound, and arguments are refused before anything is launched (no device needed)"""
    import ctypes
    from efficient_tts_amd import build as B
    from efficient_tts_amd import lib as L
    B.build(verbose=False)
    lib = L.load()
    for name in ("efts_loudness", "efts_loudness_pcm16", "efts_loudness_workspace_bytes"):
        assert name in L.exported_symbols() and hasattr(lib, name)
    assert lib.efts_loudness_workspace_bytes(0, 100, 22050) == 0 and lib.efts_loudness_workspace_bytes(2, 100, 11025) == 0
    # [B][ceil(n / 512)][2] fp64 + [B][ceil(n / 512)] fp32 + [B][n / h + 1] fp64
    assert lib.efts_loudness_workspace_bytes(3, 66150, 22050) >= 3 * (130 * 16 + 130 * 4 + 31 * 8)
    kw = (ctypes.c_double * 10)(*S.k_weighting(22050).tolist())
    tail = (None, 100, None, None, None, None, None)
    assert lib.efts_loudness(None, 100, None, 22050, kw, -23.0, 0.99, *tail, 1, None) == -1 and b"null" in lib.efts_last_error()     # EFTS_EINVAL
    assert lib.efts_loudness(None, 100, None, 11025, kw, -23.0, 0.99, *tail, 1, None) == -2                                          # EFTS_ESHAPE
    assert lib.efts_loudness(None, 100, None, 96000, kw, -23.0, 0.99, *tail, 1, None) == -2
    assert lib.efts_loudness(None, 100, None, 22050, kw, -23.0, 0.99, *tail, 0, None) == -2
    assert lib.efts_loudness(None, 0, None, 22050, kw, -23.0, 0.99, *tail, 1, None) == -2
    assert lib.efts_loudness_pcm16(None, 100, None, 22050, kw, -23.0, 0.99, 1.0 / 32768, *tail, 65536, None) == -2
