"""No GPU: the noise profile's and the spectral gate's definitions as tests/gate_reference.py restates them -- against the bias denoiser's
reference, against torch's float64 stft / istft, and the condition on the inputs of tests/test_gate_gpu.py; what the host classes, the
training recipe and the library refuse; the header.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import yaml

import denoise_reference as D
import gate_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gate_at_floor_zero_with_a_shared_profile_is_the_bias_denoiser_exactly():
    bias = D.bias_spectrum()
    for length in (300, 513, 2049, 12345):
        x = D.signal(length, length)
        for s in D.STRENGTHS:
            assert np.array_equal(R.gate(x, bias, s, 0.0), D.denoise(x, bias, s))
    assert np.array_equal(R.window(), D.window()) and all(R.frame_count(n) == D.frame_count(n) for n in (0, 512, 513, 4096))


@pytest.mark.parametrize("length", (513, 1024, 4097, 12345))
def test_reference_stft_and_istft_equal_torch_float64(length):
    x = R.batch()[1][7, :length]
    X = R.spectra(x)
    Xt, _ = R.stft_torch(x, torch.float64)
    scale = float(np.abs(X).max())
    err = float(np.abs(X - Xt.numpy().T).max()) / scale
    print(f"len {length}: max |reference STFT - torch float64| / max |X| = {err:.3g}")
    assert err <= 4e-15
    prof = R.noise_profile(R.batch()[1][7, :12345])["profile"]
    for s, f in ((1.0, 0.1), (2.5, 0.0), (0.0, 1.0)):
        err = float(np.abs(R.gate(x, prof, s, f) - R.gate_torch(x, prof, s, f, torch.float64)).max())
        print(f"len {length} strength {s} floor {f}: max |reference - torch float64| = {err:.3g}")
        assert err <= 2e-15
    flags = np.arange(X.shape[0]) % 2 == 0
    assert np.abs(np.abs(X)[flags].mean(axis=0) - R.profile_torch(x, flags, torch.float64)).max() <= 4e-15 * scale


def test_gpu_inputs_meet_their_condition_and_cover_the_cases():
    pcm, audio, lengths = R.batch()
    ref = R.reference_profiles()                                       # asserts the 0.01 dB margin of every frame of every item
    by = dict(zip(list(R.LENGTHS) + list(R.EXTRA), ref))
    print({k: (p["frames"], p["noise_frames"], round(p["noise_db"], 2), round(p["margin_db"], 3)) for k, p in by.items()})
    assert lengths.tolist() == list(R.LENGTHS) + [R.EXTRA_LEN[k] for k in R.EXTRA]
    assert np.array_equal(audio, (pcm.astype(np.float64) / 32768.0).astype(np.float32)) and float(np.abs(audio).max()) <= 0.51   # the 0.5 peak plus the noise
    assert [p["frames"] for p in ref[:8]] == [0, 0, 3, 5, 16, 17, 17, 49]
    assert by["zeros"]["noise_frames"] == 0 and by["tone"]["noise_frames"] == 0 and by["zeros"]["margin_db"] == float("inf")
    assert by["exact"]["noise_frames"] == R.MIN_FRAMES and by["short"]["noise_frames"] == R.MIN_FRAMES - 1
    assert not by["short"]["profile"].any() and by["exact"]["profile"].min() > 0
    gated = [k for k, p in by.items() if p["noise_frames"] >= R.MIN_FRAMES]
    assert 12345 in gated and 4097 in gated and "exact" in gated and len(gated) >= 4
    for k in gated:                                                    # the floor lies where it was put: 50 dB under a 0.5 peak, about
        assert -52.0 < by[k]["noise_db"] < -40.0                       # 44 dB under the loudest frame
    # the gate does something on them: at strength 1 and floor 0.1 the noise-only head of the longest item drops by 10 to 20 dB
    x, p = audio[7, :12345], by[12345]
    out = R.gate(x, p["profile"], 1.0, 0.1)
    drop = D.level_db(out[:2048]) - D.level_db(x[:2048])
    print(f"noise-only head of the 12 345-sample item: {drop:.2f} dB")
    assert -20.5 <= drop <= -6.0
    assert abs(D.level_db(out[4115:8230]) - D.level_db(x[4115:8230])) <= 0.1   # and the burst keeps its level


def test_host_class_refusals():
    from efficient_tts_amd import denoise as M
    for bad in (dict(top_db=0.0), dict(top_db=float("nan")), dict(top_db=-3.0), dict(min_frames=0), dict(min_frames=2.5), dict(min_frames=True),
                dict(max_wav_value=0.0)):
        with pytest.raises(ValueError):
            M.NoiseProfile(None, **bad)
        with pytest.raises(ValueError):
            M.SpectralGate(None, **bad)
    for bad in (dict(strength=-1.0), dict(strength=float("inf")), dict(floor=-0.1), dict(floor=1.5), dict(floor=float("nan"))):
        with pytest.raises(ValueError):
            M.SpectralGate(None, **bad)
    p, g = M.NoiseProfile(None), M.SpectralGate(None)
    assert (p.top_db, p.min_frames, p.max_wav_value, p.ratio) == (40.0, 8, 32768.0, 1e4)
    assert (g.strength, g.floor, g.top_db, g.min_frames) == (1.0, 0.1, 40.0, 8)
    for m in (p, g):
        with pytest.raises(RuntimeError, match="no CPU path"):
            m(torch.zeros(1, 2048, dtype=torch.float32))
        with pytest.raises(ValueError, match=r"\[B, n\]"):
            m(torch.zeros(2048, dtype=torch.float32))
        with pytest.raises(ValueError, match=r"\[B, n\]"):
            m(torch.zeros(1, 2048, dtype=torch.float64))
    x = torch.zeros(2, 2048, dtype=torch.int16)
    with pytest.raises(ValueError, match="strength"):
        g(x, strength=-0.5)
    with pytest.raises(ValueError, match="floor"):
        g(x, floor=2.0)
    for shape in ((512,), (3, 513), (2, 512), (1, 2, 513)):
        with pytest.raises(ValueError, match="profile"):
            g(x, profile=torch.zeros(shape))


def test_recipe_keys_are_parsed_and_refused():
    from efficient_tts_amd.bin.train import build_gate
    from efficient_tts_amd.denoise import SpectralGate
    for text in ("{}", "denoise_corpus: false", "trim_silence: true"):
        assert build_gate(yaml.safe_load(text)) is None
    g = build_gate(yaml.safe_load("denoise_corpus: true"))
    assert isinstance(g, SpectralGate) and (g.strength, g.floor, g.top_db, g.min_frames, g.max_wav_value) == (1.0, 0.1, 40.0, 8, 32768.0)
    g = build_gate(yaml.safe_load("denoise_corpus: true\ndenoise_strength: 1.5\ndenoise_floor: 0.05\ndenoise_top_db: 35\ndenoise_min_frames: 12\n"
                                  "frontend_params: {max_wav_value: 32767.0}"))
    assert (g.strength, g.floor, g.top_db, g.min_frames, g.max_wav_value) == (1.5, 0.05, 35.0, 12, 32767.0)
    for text in ("denoise_corpus: 1", "denoise_corpus: 'yes'", "denoise_strength: 1.0", "denoise_corpus: false\ndenoise_floor: 0.1",
                 "denoise_corpus: true\ndenoise_strength: -1", "denoise_corpus: true\ndenoise_floor: 1.5", "denoise_corpus: true\ndenoise_top_db: 0",
                 "denoise_corpus: true\ndenoise_min_frames: 0", "denoise_corpus: true\ndenoise_min_frames: 2.5"):
        with pytest.raises(ValueError, match="denoise_|strength|floor|top_db|min_frames"):
            build_gate(yaml.safe_load(text))


def test_no_key_means_no_gate_on_the_trainer():
    from efficient_tts_amd.trainer import EfficientTTSTrainer
    cfg = dict(outdir="/tmp", log_interval_steps=5, eval_interval_steps=0, save_interval_steps=10, train_max_steps=20, grad_norm=1.0)
    t = EfficientTTSTrainer(steps=0, epochs=0, data_loader={}, sampler={}, model=torch.nn.Linear(2, 2), optimizer=None, scheduler=None, config=cfg)
    assert t.gate is None and t.trimmer is None


def test_command_line_arguments():
    from efficient_tts_amd.bin import gate as G
    a = G.get_parser().parse_args(["--filelist", "f", "--wav_path", "d", "--outdir", "o"])
    assert (a.strength, a.floor, a.top_db, a.min_frames, a.write_wavs) == (1.0, 0.1, 40.0, 8, False)
    assert G.COLUMNS == ("id", "seconds", "frames", "noise_frames", "noise_db", "bypassed")
    for extra in (["--floor", "2"], ["--strength", "-1"], ["--top_db", "0"], ["--min_frames", "0"]):
        with pytest.raises(ValueError):                                # refused before a device or a file is looked for
            G.run_gate(G.get_parser().parse_args(["--filelist", "f", "--wav_path", "d", "--outdir", "o"] + extra))


def test_header_has_the_section_and_stays_at_revision_602():
    hdr = open(os.path.join(ROOT, "include", "efts_abi.h")).read()
    assert int(re.search(r"#define EFTS_ABI_VERSION (\d+)", hdr).group(1)) == 602
    assert "Spectral gating of a corpus with a noise profile per recording" in hdr
    assert re.search(r"\+ efts_noise_profile, efts_noise_profile_workspace_bytes, efts_spectral_gate", hdr)
    from efficient_tts_amd import lib as L
    for name in ("efts_noise_profile", "efts_noise_profile_workspace_bytes", "efts_spectral_gate"):
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m and len(L._SIGS[name][1]) == len(m.group(1).split(","))


def test_library_exports_and_refuses_on_the_host():
    """the three entry points are bound with their ctypes signatures, and every refusal of the header comes back before anything is launched"""
    from efficient_tts_amd import build as B
    from efficient_tts_amd import lib as L
    B.build(verbose=False)
    lib = L.load()
    i32, i64, f32, vp, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_double
    want = {"efts_noise_profile_workspace_bytes": (i64, [i32, i32]),
            "efts_noise_profile": (i32, [vp, i32, f32, i64, vp, i32, vp, f64, i32, vp, i64, vp, vp, vp, vp, i64, i32, vp]),
            "efts_spectral_gate": (i32, [vp, i32, f32, i64, vp, i32, vp, vp, i64, f32, f32, vp, vp, i64, vp, i32, vp])}
    for name, (res, args) in want.items():
        assert name in L.exported_symbols() and getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == args
    size = lib.efts_noise_profile_workspace_bytes
    assert size(0, 100) == 0 and size(2, 0) == 0 and size(70000, 100) == 0
    T, Rn = 1 + 16384 // 256, -(-(1 + 16384 // 256) // 16)
    r16 = lambda v: (v + 15) & ~15
    assert size(4, 16384) == r16(4 * T * 8) + r16(4 * T * 4) + r16(4 * Rn * 4) + r16(4 * Rn * 513 * 8)
    # host arrays stand in for device memory: a call that passes every check would launch, so every call below fails one check
    n = 2048
    f = (ctypes.c_float * (4 * n + 4))()
    g = (ctypes.c_float * (4 * n + 4))()
    ints = (ctypes.c_int32 * 32)()
    dbl = (ctypes.c_double * 8)()
    ws = (ctypes.c_double * 8)()
    A, G, I, Dd, W = (ctypes.addressof(v) for v in (f, g, ints, dbl, ws))
    W += (-W) % 16
    EINVAL = -1
    good = dict(audio=A, pcm=0, scale=1.0, ld=n, lengths=I, max_len=n, window=A, profile=G, ldp=513, strength=1.0, floor=0.1, bypass=None, out=G,
                ld_out=n, frames=I + 32, B=2)

    def gate(**kw):
        a = dict(good, **kw)
        return lib.efts_spectral_gate(a["audio"], a["pcm"], a["scale"], a["ld"], a["lengths"], a["max_len"], a["window"], a["profile"], a["ldp"],
                                      a["strength"], a["floor"], a["bypass"], a["out"], a["ld_out"], a["frames"], a["B"], None)
    cases = [dict(audio=None), dict(lengths=None), dict(window=None), dict(profile=None), dict(out=None), dict(frames=None),
             dict(audio=A + 2), dict(audio=A + 1, pcm=1), dict(out=G + 1), dict(lengths=I + 2), dict(window=A + 2), dict(profile=G + 1), dict(frames=I + 33),
             dict(bypass=I + 1), dict(B=0), dict(B=65536), dict(max_len=0), dict(max_len=2 ** 31 - 8192, ld=2 ** 31, ld_out=2 ** 31 - 1),
             dict(ld=n - 1), dict(ld_out=n - 1), dict(ld_out=2 ** 31), dict(ldp=512), dict(ldp=-1), dict(ldp=1),
             dict(strength=-0.5), dict(strength=float("nan")), dict(strength=float("inf")), dict(floor=-0.1), dict(floor=1.01), dict(floor=float("nan")),
             dict(pcm=1, scale=0.0), dict(pcm=1, scale=float("nan")),
             dict(out=A), dict(out=A + 4 * n), dict(audio=G + 4 * (2 * n - 4)), dict(pcm=1, audio=G + 4 * n)]
    for kw in cases:
        rc = gate(**kw)
        assert rc == EINVAL and lib.efts_last_error().startswith(b"efts_spectral_gate:"), (kw, rc, lib.efts_last_error())
    assert b"overlaps" in lib.efts_last_error()
    good = dict(audio=A, pcm=0, scale=1.0, ld=n, lengths=I, max_len=n, window=A, r=1e4, min_frames=8, profile=G, ldp=513, noise=I + 32, frames=I + 64,
                db=Dd, ws=W, wsb=1 << 30, B=2)

    def prof(**kw):
        a = dict(good, **kw)
        return lib.efts_noise_profile(a["audio"], a["pcm"], a["scale"], a["ld"], a["lengths"], a["max_len"], a["window"], a["r"], a["min_frames"],
                                      a["profile"], a["ldp"], a["noise"], a["frames"], a["db"], a["ws"], a["wsb"], a["B"], None)
    cases = [dict(audio=None), dict(lengths=None), dict(window=None), dict(profile=None), dict(noise=None), dict(frames=None), dict(db=None), dict(ws=None),
             dict(audio=A + 2), dict(audio=A + 1, pcm=1), dict(lengths=I + 2), dict(window=A + 2), dict(profile=G + 1), dict(noise=I + 33), dict(frames=I + 65),
             dict(db=Dd + 4), dict(ws=W + 8), dict(B=0), dict(B=65536), dict(max_len=0), dict(max_len=2 ** 31 - 8192, ld=2 ** 31), dict(ld=n - 1),
             dict(ldp=512), dict(ldp=0), dict(r=1.0), dict(r=0.5), dict(r=float("nan")), dict(r=float("inf")), dict(min_frames=0), dict(min_frames=-1),
             dict(pcm=1, scale=0.0), dict(wsb=size(2, n) - 1), dict(wsb=0)]
    for kw in cases:
        rc = prof(**kw)
        assert rc == EINVAL and lib.efts_last_error().startswith(b"efts_noise_profile:"), (kw, rc, lib.efts_last_error())
    assert b"workspace" in lib.efts_last_error()
