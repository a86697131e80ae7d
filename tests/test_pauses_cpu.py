"""No GPU: the pause shortener's reference (tests/pauses_reference.py) on hand-made cases with the answer written out, the host side of
efficient_tts_amd/pauses.py (fade table, the rounding of max_pause_ms to chunks, the constructor's refusals) and the wiring: the YAML keys of
bin/train.py and the flags of bin/score.py and bin/trim.py.
"""
import numpy as np
import pytest
import torch

import pauses_reference as R
from efficient_tts_amd import pauses as P


def _flags(text):
    return [ch == "S" for ch in text]


def _kept(text, M):
    keep, joints, runs = R.plan(_flags(text), M)
    return "".join(ch for ch, k in zip(text, keep) if k), joints, runs


def test_runs_of_exactly_m_and_m_plus_one():
    assert _kept("SqqqS", 3) == ("SqqqS", {}, [(1, 4)])                       # n == M: whole
    assert _kept("SqqqqS", 3) == ("SqqqS", {2: 4}, [(1, 5)])                  # n == M + 1: head 2, tail 1; chunk 3 goes, chunk 2 fades into chunk 4
    keep, joints, _ = R.plan(_flags("SqqqqS"), 3)
    assert keep == [True, True, True, False, True, True]


def test_m_of_1_2_and_7():
    text = "S" + "q" * 10 + "S"
    keep, joints, _ = R.plan(_flags(text), 1)                                  # head 1, tail 0: the first quiet chunk alone, fading into the sound
    assert [i for i, k in enumerate(keep) if not k] == list(range(2, 11)) and joints == {1: 11}
    keep, joints, _ = R.plan(_flags(text), 2)                                  # head 1, tail 1
    assert [i for i, k in enumerate(keep) if not k] == list(range(2, 10)) and joints == {1: 10}
    keep, joints, _ = R.plan(_flags(text), 7)                                  # head 4, tail 3
    assert [i for i, k in enumerate(keep) if not k] == [5, 6, 7] and joints == {4: 8}


def test_quiet_ends_are_left_alone_and_two_pauses_around_one_sound_chunk():
    assert _kept("qqqqqSSqqqqq", 1) == ("qqqqqSSqqqqq", {}, [])
    kept, joints, runs = _kept("qqqSqqqSqqqqSqqq", 2)
    assert kept == "qqqSqqSqqSqqq" and joints == {4: 6, 8: 11} and runs == [(4, 7), (8, 12)]
    assert _kept("qqqq", 1) == ("qqqq", {}, []) and _kept("", 1) == ("", {}, [])


def _signal(text, H, dtype=np.int16, tail=0):
    """chunks of a full-scale square wave (S) or of zeros with one count (q), `tail` more quiet samples"""
    x = np.concatenate([np.where(np.arange(H) % 2 == 0, 12000, -12000) if ch == "S" else np.ones(H) for ch in text] + [np.ones(tail)]).astype(np.int16)
    return x if dtype == np.int16 else (x.astype(np.float32) / np.float32(32768.0)).astype(np.float32)


def test_shorten_writes_out_the_answer():
    # W = 512, H = 512: a frame is its chunk, so the flags are the letters
    H, F = 512, 4
    x = _signal("qSqqqqqSq", H, tail=7)
    ref = R.shorten(x, W=512, H=H, M=2, F=F)
    assert ref["flags"] == _flags("qSqqqqqSq") + [False] and ref["runs"] == [(2, 7)]
    assert (ref["new_len"], ref["removed"], ref["pauses"], ref["chunk_src"]) == (len(x) - 3 * H, 3 * H, 1, [0, 1, 2, 6, 7, 8, 9])
    scaled = x.astype(np.float32) * np.float32(1.0 / 32768.0)
    assert np.array_equal(ref["out"][:3 * H - F], scaled[:3 * H - F].astype(np.float64))
    assert np.array_equal(ref["out"][3 * H:], scaled[6 * H:].astype(np.float64))
    assert ref["is_fade"].nonzero()[0].tolist() == list(range(3 * H - F, 3 * H))
    # the fade: both sides are the constant 1 / 32768, so every weight gives that value back
    assert np.array_equal(ref["out"][3 * H - F:3 * H], np.full(F, 1.0 / 32768.0))
    # a step across the joint: x_a = 0.25, x_b = 0.75, weights 1/8, 3/8, 5/8, 7/8
    y = np.full(9 * H, 0.25, np.float32)
    y[H:2 * H] = np.where(np.arange(H) % 2 == 0, 0.9, -0.9)
    y[7 * H:8 * H] = y[H:2 * H]
    y[5 * H:7 * H] = 0.75
    out = R.shorten(y, W=512, H=H, top_db=1.5, M=2, F=F)
    assert out["runs"] == [(2, 7)] and out["chunk_src"] == [0, 1, 2, 6, 7, 8]
    assert out["out"][3 * H - F:3 * H].tolist() == [0.25 + 0.5 * w for w in (0.125, 0.375, 0.625, 0.875)] and out["out"][3 * H] == 0.75
    # F = 0 is a plain cut
    cut = R.shorten(y, W=512, H=H, top_db=1.5, M=2, F=0)
    assert not cut["is_fade"].any() and np.array_equal(cut["out"], np.concatenate([y[:3 * H], y[6 * H:]]).astype(np.float64))


@pytest.mark.parametrize("n", [0, 1, 255, 256])
def test_lengths_of_0_1_h_minus_1_and_h(n):
    for dtype in (np.int16, np.float32):
        x = _signal("S", 256, dtype)[:n]
        ref = R.shorten(x, W=1024, H=256, M=1, F=64)
        assert (ref["new_len"], ref["removed"], ref["pauses"], ref["chunk_src"]) == (n, 0, 0, [0] if n else [])
        want = x.astype(np.float32) * np.float32(1.0 / 32768.0) if dtype == np.int16 else x
        assert np.array_equal(ref["out"], want.astype(np.float64))


def test_an_all_quiet_item_comes_back_unchanged():
    x = np.zeros(5 * 256 + 3, np.int16)
    ref = R.shorten(x, M=1)
    assert ref["flags"] == [False] * 6 and (ref["new_len"], ref["removed"], ref["pauses"]) == (len(x), 0, 0) and ref["chunk_src"] == list(range(6))


def test_fade_table():
    assert P.fade_table(0).shape == (0,) and P.fade_table(0).dtype == np.float32
    assert P.fade_table(4).tolist() == [0.125, 0.375, 0.625, 0.875]
    t = P.fade_table(64)
    assert t.dtype == np.float32 and np.array_equal(t, R.fade_table(64)) and t[0] == np.float32(0.5 / 64) and t[63] == np.float32(63.5 / 64)
    t = P.fade_table(3)                                                        # not exact in binary: float64 first, one rounding
    assert [v.item() for v in t] == [float(np.float32(0.5 / 3.0)), 0.5, float(np.float32(2.5 / 3.0))]
    with pytest.raises(ValueError):
        P.fade_table(-1)
    with pytest.raises(ValueError):
        P.fade_table(2.0)


def test_max_pause_ms_is_rounded_to_chunks():
    assert P.pause_chunks(300.0, 22050, 256) == 26                             # 25.84
    assert P.pause_chunks(290.0, 22050, 256) == 25                             # 24.98
    assert P.pause_chunks(1.0, 22050, 256) == 1                                # 0.09: never under one chunk
    assert P.pause_chunks(16.0, 16000, 256) == 1 and P.pause_chunks(40.0, 16000, 256) == 2      # 1.0, and 2.5 to the even neighbour
    assert P.pause_chunks(56.0, 16000, 256) == 4                               # 3.5
    for ms, rate, hop in ((300.0, 22050, 256), (120.0, 16000, 64), (77.7, 44100, 200)):
        assert P.pause_chunks(ms, rate, hop) == R.pause_chunks(ms, rate, hop)
    s = P.PauseShortener(None, 22050, max_pause_ms=300)
    assert s.chunks == 26 and (s.frame_length, s.hop, s.fade, s.top_db) == (1024, 256, 64, 40.0) and s.ratio == R.ratio(40.0)


def test_constructor_refusals():
    ok = dict(sampling_rate=22050, max_pause_ms=300.0, frame_length=1024, hop_size=256, top_db=40.0, fade=64)
    P.PauseShortener(None, **ok)
    P.PauseShortener(None, **dict(ok, frame_length=512, hop_size=64, fade=64))
    P.PauseShortener(None, **dict(ok, fade=0))
    P.PauseShortener(None, **dict(ok, fade=256))
    bad = [dict(frame_length=1000), dict(frame_length=256), dict(frame_length=4096), dict(hop_size=0), dict(hop_size=2048), dict(hop_size=255),
           dict(hop_size=256.0), dict(top_db=0.0), dict(top_db=-3.0), dict(top_db=float("nan")), dict(max_pause_ms=0.0), dict(max_pause_ms=-1.0),
           dict(max_pause_ms=float("inf")), dict(fade=-1), dict(fade=257), dict(fade=1.5), dict(sampling_rate=0), dict(max_wav_value=0.0)]
    for change in bad:
        with pytest.raises(ValueError):
            P.PauseShortener(None, **dict(ok, **change))
    s = P.PauseShortener(None, **ok)
    with pytest.raises(ValueError):
        s(torch.zeros(4, dtype=torch.float32))                                 # not [B, n]
    with pytest.raises(ValueError):
        s(torch.zeros(2, 8, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        s(torch.zeros(2, 8, dtype=torch.int16))


def test_yaml_keys():
    from efficient_tts_amd.bin.train import build_pauses
    from efficient_tts_amd.trainer import EfficientTTSTrainer
    cfg = dict(outdir="/tmp", frontend_params=dict(hop_size=256, sampling_rate=22050))
    t = EfficientTTSTrainer(steps=0, epochs=0, data_loader={}, sampler={}, model=torch.nn.Linear(2, 2), optimizer=None, scheduler=None, config=cfg,
                            device=torch.device("cpu"))
    assert t.pauses is None
    assert build_pauses(cfg) is None
    s = build_pauses(dict(cfg, max_pause_ms=300))
    assert isinstance(s, P.PauseShortener) and (s.chunks, s.hop, s.frame_length, s.fade, s.top_db, s.sampling_rate) == (26, 256, 1024, 64, 40.0, 22050)
    s = build_pauses(dict(cfg, max_pause_ms=120.5, pause_top_db=35, pause_frame_length=2048, pause_fade=0,
                          frontend_params=dict(hop_size=200, sampling_rate=16000, max_wav_value=30000.0)))
    assert (s.chunks, s.hop, s.frame_length, s.fade, s.top_db, s.sampling_rate, s.max_wav_value) == (10, 200, 2048, 0, 35.0, 16000, 30000.0)
    for value in (0, -5, 0.0, True, "300"):
        with pytest.raises(ValueError, match="max_pause_ms"):
            build_pauses(dict(cfg, max_pause_ms=value))
    for key, value in (("pause_top_db", 40.0), ("pause_frame_length", 1024), ("pause_fade", 64)):
        with pytest.raises(ValueError, match="without max_pause_ms"):
            build_pauses(dict(cfg, **{key: value}))
    with pytest.raises(ValueError):
        build_pauses(dict(cfg, max_pause_ms=300, pause_fade=300))              # longer than the hop
    with pytest.raises(ValueError):
        build_pauses(dict(cfg, max_pause_ms=300, pause_frame_length=1000))


def test_flags_of_score_and_trim():
    from efficient_tts_amd.bin import score as C
    from efficient_tts_amd.bin import trim as T
    base = ["--checkpoint", "c.pkl", "--test_fid_scp", "t.txt", "--outdir", "o"]
    a = C.get_parser().parse_args(base)
    assert a.max_pause_ms is None and a.pause_top_db == 40.0 and C.build_pauses(a, 22050, 256, 32768.0) is None
    a = C.get_parser().parse_args(base + ["--max_pause_ms", "250", "--pause_top_db", "35"])
    s = C.build_pauses(a, 22050, 256, 32768.0)
    assert (s.max_pause_ms, s.chunks, s.top_db, s.hop) == (250.0, 22, 35.0, 256)
    with pytest.raises(ValueError):
        C.build_pauses(C.get_parser().parse_args(base + ["--max_pause_ms", "0"]), 22050, 256, 32768.0)
    base = ["--filelist", "f.txt", "--wav_path", "d", "--outdir", "o"]
    a = T.get_parser().parse_args(base)
    assert a.max_pause_ms is None and a.pause_top_db == 40.0 and T.build_pauses(a) is None
    a = T.get_parser().parse_args(base + ["--max_pause_ms", "300", "--pause_top_db", "45", "--frame_length", "512", "--hop_size", "128"])
    s = T.build_pauses(a, 16000)
    assert (s.chunks, s.top_db, s.frame_length, s.hop, s.sampling_rate) == (38, 45.0, 512, 128, 16000)          # 37.5 to the even neighbour
    with pytest.raises(ValueError):
        T.build_pauses(T.get_parser().parse_args(base + ["--max_pause_ms", "-1"]))


def test_gpu_inputs_hold_their_condition():
    """what tests/test_pauses_gpu.py relies on, for both settings: every fp32 frame at least 0.01 dB from the threshold, runs shorter than,
    equal to and longer than every M, a lead-in gap of one chunk, quiet ends, and pauses across the plan's tile boundaries"""
    tile = R.plan_tile()
    for (W, H), count in (((1024, 256), 7), ((512, 64), 8)):
        x, lengths = R.batch(W, H, np.float32, tile, count)
        pcm, _ = R.batch(W, H, np.int16, tile, count)
        assert np.array_equal(x, pcm.astype(np.float32) * np.float32(2.0 ** -15))
        lens = set()
        for b, n in enumerate(lengths):
            flags, margin = R.sound_flags(x[b, :n], W, H)
            assert margin >= 0.01 and flags == R.sound_flags(pcm[b, :n], W, H)[0]
            keep, joints, runs = R.plan(flags, 1)
            lens |= {c1 - c0 for c0, c1 in runs}
            if n == 12345:
                assert not any(flags[:8]) and not any(flags[-8:])              # quiet ends longer than every M
            if n == 40000:
                assert flags[0] and not any(flags[-8:])                         # the one-chunk lead-in is under the first burst's frames
            if n == 70000:
                assert [r for r in runs if r[0] < tile < r[1]] and [r for r in runs if r[0] < 2 * tile < r[1]] and [r for r in runs if r[0] < 3 * tile < r[1]]
                assert len(flags) == 1094
        assert {1, 2, 3, 7, 8, 12} <= lens
