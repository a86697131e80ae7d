"""No GPU: the definition of the silence trimmer as tests/trim_reference.py restates it, on cases worked out by hand; the condition on the
fp32 inputs of tests/test_trim_gpu.py; what the host class refuses; the recipe and command-line plumbing.

The hand-worked cases use W = 1024, H = 256 (pad = 384): frame t covers samples 256 t - 384 .. 256 t + 639, and with top_db = 40 a frame
that holds one full-level sample of the only sound is sound (r = 10^4), a frame of zeros never is.
"""
import os
import re

import numpy as np
import pytest
import torch

import trim_reference as R
from efficient_tts_amd import lib as L
from efficient_tts_amd import trim as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bounds(x, **kw):
    res = R.trim(x, **kw)
    return res["start"], res["new_len"]


def test_single_click():
    x = np.zeros(4000, dtype=np.int16)
    x[2000] = 32767
    # frames 6 .. 9 hold sample 2000 (256 * 6 - 384 = 1152 <= 2000 <= 256 * 9 + 639 = 2943; frame 5 ends at 1919, frame 10 begins at 2176)
    assert _bounds(x, keep_frames=0) == (1536, 1024)
    assert _bounds(x, keep_frames=2) == (1024, 2048)
    res = R.trim(x, keep_frames=0, peak=0.95)
    assert res["gain"] == np.float32(0.95) / np.float32(32767) and res["out"][2000 - 1536] == np.float32(32767) * res["gain"]
    assert np.count_nonzero(res["out"]) == 1 and res["gain"].dtype == np.float32
    assert R.trim(x, keep_frames=0)["gain"] == np.float32(1.0 / 32768.0)
    f = np.zeros(4000, dtype=np.float32)
    f[2000] = 0.5
    res = R.trim(f, keep_frames=0, peak=0.95)
    assert (res["start"], res["new_len"]) == (1536, 1024) and res["gain"] == np.float32(0.95) / np.float32(0.5)
    assert R.trim(f, keep_frames=0)["gain"] == np.float32(1.0)


def test_keep_frames_clamps_at_both_ends():
    x = np.zeros(4000, dtype=np.int16)
    x[2000] = 32767
    assert _bounds(x, keep_frames=10) == (0, 4000)                 # (6 - 10) * 256 < 0 and (9 + 1 + 10) * 256 = 5120 > 4000
    assert _bounds(x, keep_frames=6) == (0, 4000)                  # 0 and min(4000, 4096)
    assert _bounds(x, keep_frames=5) == (256, 3840 - 256)


def test_sound_from_the_first_sample():
    x = np.zeros(4000, dtype=np.int16)
    x[:1000] = 1000
    # frames 0 .. 5 hold some of samples 0 .. 999 (frame 5 begins at 896, frame 6 at 1152)
    assert _bounds(x, keep_frames=0) == (0, 1536)
    assert _bounds(x, keep_frames=2) == (0, 2048)


def test_sound_to_the_last_sample():
    x = np.zeros(4000, dtype=np.int16)
    x[3000:] = 1000
    # T = 16; frame 9 ends at 2943, frame 10 at 3199: first sound frame 10, last 15; end = min(4000, 4096)
    assert _bounds(x, keep_frames=0) == (2560, 1440)
    assert _bounds(x, keep_frames=2) == (2048, 1952)


def test_all_zero_empty_and_short_items():
    for dtype in (np.int16, np.float32):
        res = R.trim(np.zeros(1000, dtype=dtype), peak=0.95)
        assert (res["start"], res["new_len"], res["gain"]) == (0, 1000, np.float32(1.0)) and not res["out"].any()
        res = R.trim(np.zeros(0, dtype=dtype), peak=0.95)
        assert (res["start"], res["new_len"], res["gain"]) == (0, 0, np.float32(1.0)) and res["out"].shape == (0,)
    x = np.zeros(37, dtype=np.int16)
    x[20] = -5
    res = R.trim(x, keep_frames=0, peak=0.5)                       # one frame, it holds everything
    assert (res["start"], res["new_len"]) == (0, 37) and res["gain"] == np.float32(0.5) / np.float32(5) and len(res["energies"]) == 1
    assert res["energies"][0] == 25 and res["out"][20] == np.float32(-5) * res["gain"]


def test_threshold_is_strict_and_exact():
    # two frames' worth of level 100 in front of level 10000: 40 dB apart sample by sample.  W = H = 512 (pad 0): the frames do not overlap
    x = np.concatenate([np.full(1024, 100), np.full(1024, 10000)]).astype(np.int16)
    assert R.trim(x, W=512, H=512, top_db=40.0, keep_frames=0)["energies"] == [512 * 10 ** 4] * 2 + [512 * 10 ** 8] * 2
    assert _bounds(x, W=512, H=512, top_db=40.0, keep_frames=0) == (1024, 1024)        # E r == E_max is not sound
    assert _bounds(x, W=512, H=512, top_db=40.1, keep_frames=0) == (0, 2048)
    assert R.trim(x, W=512, H=512, top_db=40.0, keep_frames=0)["margin_db"] == 0.0
    # trimming switched off: the bounds stay, the level is still set from the whole item
    res = R.trim(x, W=512, H=512, peak=1.0, trimming=False)
    assert (res["start"], res["new_len"], res["gain"]) == (0, 2048, np.float32(1.0) / np.float32(10000))


@pytest.mark.parametrize("W,H", R.PAIRS)
def test_fp32_gpu_cases_keep_their_distance_from_the_threshold(W, H):
    """An fp32 sum of at most 2048 squares is off by at most 2048 * 2^-23 relative = 0.0011 dB whatever its order: with every frame at least
    0.01 dB from the threshold, the device's decisions are the reference's.  A condition on the inputs, not a tolerance on the kernel."""
    x = R.items(np.float32)
    pcm = R.items(np.int16)
    trimmed = []
    for b, n in enumerate(R.LENGTHS):
        res = R.trim(x[b, :n], W=W, H=H)
        print(f"W {W} H {H} item {b} len {n}: start {res['start']} new_len {res['new_len']} margin {res['margin_db']:.4f} dB")
        assert res["margin_db"] >= 0.01
        ref = R.trim(pcm[b, :n], W=W, H=H)
        assert (res["start"], res["new_len"]) == (ref["start"], ref["new_len"])
        trimmed.append(res["new_len"] < n)
    # 5 dB under the threshold is cut, 5 dB over it is kept (frames of 2048 with 2 kept around the sound cover all 4001 samples)
    assert trimmed[0] == (W < 2048) and not trimmed[2] and not trimmed[1]
    if (W, H) == (1024, 256):
        for top_db, keep in R.OTHER:
            res = [R.trim(x[b, :n], top_db=top_db, keep_frames=keep, peak=1.0) for b, n in enumerate(R.LENGTHS)]
            assert min(v["margin_db"] for v in res) >= 0.01
            assert (res[2]["new_len"] < R.LENGTHS[2]) == (top_db == 30.0)


def test_constructor_refusals():
    for kw in (dict(frame_length=1000), dict(frame_length=4096), dict(frame_length=1024.0), dict(hop_size=255), dict(hop_size=0),
               dict(frame_length=512, hop_size=1024), dict(top_db=0.0), dict(top_db=-3.0), dict(top_db=float("nan")), dict(peak=0.0), dict(peak=1.5),
               dict(peak=-0.95), dict(keep_frames=-1), dict(keep_frames=1.5), dict(max_wav_value=0.0)):
        with pytest.raises(ValueError):
            S.SilenceTrimmer(None, **kw)
    t = S.SilenceTrimmer()
    assert (t.frame_length, t.hop, t.top_db, t.keep_frames, t.peak, t.max_wav_value, t.trim) == (1024, 256, 40.0, 2, None, 32768.0, True)
    assert t.ratio == R.ratio(40.0) == 10000.0
    assert S.SilenceTrimmer(None, 1024, 200, peak=1.0, keep_frames=0).peak == 1.0
    with pytest.raises(RuntimeError, match="no CPU path"):
        t(torch.zeros(1, 100))
    with pytest.raises(ValueError):
        t(torch.zeros(100))
    with pytest.raises(ValueError):
        t(torch.zeros(1, 100, dtype=torch.float64))


def test_recipe_wiring():
    from efficient_tts_amd.bin.train import build_trimmer
    from efficient_tts_amd.trainer import EfficientTTSTrainer
    cfg = dict(outdir="/tmp", log_interval_steps=5, eval_interval_steps=0, save_interval_steps=10, train_max_steps=20, grad_norm=1.0)
    t = EfficientTTSTrainer(steps=0, epochs=0, data_loader={}, sampler={}, model=torch.nn.Linear(2, 2), optimizer=None, scheduler=None, config=cfg)
    assert t.trimmer is None
    assert build_trimmer(cfg) is None and build_trimmer(dict(cfg, trim_silence=False)) is None
    assert build_trimmer(dict(cfg, trim_top_db=30.0, trim_keep_frames=1)) is None       # companions alone switch nothing on
    tr = build_trimmer(dict(cfg, trim_silence=True))
    assert (tr.trim, tr.peak, tr.top_db, tr.keep_frames, tr.frame_length, tr.hop) == (True, None, 40.0, 2, 1024, 256)
    tr = build_trimmer(dict(cfg, trim_silence=True, trim_top_db=30, trim_keep_frames=0, trim_frame_length=2048, normalize_peak=0.9,
                            frontend_params=dict(hop_size=512, max_wav_value=32767.0)))
    assert (tr.trim, tr.peak, tr.top_db, tr.keep_frames, tr.frame_length, tr.hop, tr.max_wav_value) == (True, 0.9, 30.0, 0, 2048, 512, 32767.0)
    tr = build_trimmer(dict(cfg, normalize_peak=0.95))
    assert (tr.trim, tr.peak) == (False, 0.95)
    assert build_trimmer(dict(cfg, normalize_peak=True)).peak == 0.95
    with pytest.raises(ValueError):
        build_trimmer(dict(cfg, normalize_peak=1.5))


def test_command_lines():
    from efficient_tts_amd.bin import score as C
    from efficient_tts_amd.bin import trim as T
    base = ["--checkpoint", "c.pkl", "--test_fid_scp", "t.txt", "--outdir", "o"]
    a = C.get_parser().parse_args(base)
    assert a.trim_silence is False and a.trim_top_db == 40.0 and a.normalize_peak is None and C.build_trimmer(a, 256, 32768.0) is None
    a = C.get_parser().parse_args(base + ["--trim_silence", "--trim_top_db", "35", "--normalize_peak", "0.95"])
    tr = C.build_trimmer(a, 256, 32768.0)
    assert (tr.trim, tr.top_db, tr.peak, tr.hop) == (True, 35.0, 0.95, 256)
    tr = C.build_trimmer(C.get_parser().parse_args(base + ["--normalize_peak", "0.5"]), 256, 32768.0)
    assert (tr.trim, tr.peak) == (False, 0.5)
    a = T.get_parser().parse_args(["--filelist", "f.txt", "--wav_path", "d", "--outdir", "o"])
    assert (a.top_db, a.keep_frames, a.normalize_peak, a.write_wavs, a.batch_size) == (40.0, 2, None, False, 16)
    a = T.get_parser().parse_args(["--filelist", "f.txt", "--wav_path", "d", "--outdir", "o", "--top_db", "30", "--keep_frames", "0",
                                   "--normalize_peak", "0.95", "--write_wavs"])
    assert (a.top_db, a.keep_frames, a.normalize_peak, a.write_wavs) == (30.0, 0, 0.95, True)


def test_symbols_in_header_and_binding():
    with open(os.path.join(ROOT, "include", "efts_abi.h")) as f:
        header = f.read()
    for name in ("efts_trim", "efts_trim_pcm16", "efts_trim_workspace_bytes"):
        assert re.search(r"^(int|int64_t) %s\(" % name, header, re.M), name
        assert name in L.exported_symbols()
        assert hasattr(L.load(), name)
    lib = L.load()
    assert lib.efts_trim_workspace_bytes(0, 100, 256, 1) == 0 and lib.efts_trim_workspace_bytes(3, 4003, 256, 1) >= 3 * 16 * 12
    assert lib.efts_trim_workspace_bytes(3, 4003, 256, 0) >= 3 * 16 * 8
    # refusals that need no device: they come before any launch
    null = lib.efts_trim_pcm16(None, 100, None, 1024, 256, 1e4, 2, 0.0, 1.0 / 32768, None, 100, None, None, None, None, 1, None)
    assert null == -1
    assert lib.efts_trim_pcm16(None, 100, None, 1024, 256, 1e4, 2, 0.0, 1.0 / 32768, None, 99, None, None, None, None, 1, None) == -2
    assert lib.efts_trim(None, 100, None, 1000, 256, 1e4, 2, 0.0, None, 100, None, None, None, None, 1, None) == -2
    assert lib.efts_trim(None, 100, None, 1024, 255, 1e4, 2, 0.0, None, 100, None, None, None, None, 1, None) == -2
    assert lib.efts_trim(None, 100, None, 1024, 256, 1e4, 2, 0.0, None, 100, None, None, None, None, 0, None) == -2
