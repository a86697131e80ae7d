"""GPU (-m gpu): the pitch tracker (efficient_tts_amd/pitch.py, csrc/efts_pitch.hip) against the float64 restatement of tests/pitch_reference.py.

Two stages, checked apart.  Stage 1: every d'(tau) the kernel writes to `cmnd` against float64 on the same fp32 samples, within a relative
(2 W + 16) 2^-24 -- W non-negative fused terms of one rounding each plus the rounding of the difference, in numerator and running sum alike:
derived, not measured; absolute, against the same figure, where the reference d' is below 1e-6.  Stage 2: the decision and the
interpolation, float64 `decide` on the kernel's OWN d', on the frames whose comparisons all keep a margin of 1e-3 in d' (at most 5 % of the
frames may lack it; tests/test_pitch_cpu.py holds the reference to that cap on these inputs): the same voicing, f0 within a relative 1e-5.
End to end on tones of known pitch the bound comes from the reference's own error, P.REFERENCE_TONE_ERROR.
"""
import numpy as np
import pytest
import torch

import pitch_reference as P
from efficient_tts_amd import lib as L
from efficient_tts_amd.pitch import PitchTracker

pytestmark = pytest.mark.gpu

CONFIGS = [(1024, 256, 60.0), (512, 128, 100.0)]           # (n_fft, hop, fmin); fmax 600 Hz, threshold 0.15
FMAX, THRESHOLD = 600.0, 0.15
_cache = {}


@pytest.fixture(scope="module")
def dev():
    L.load()
    L.require_device()
    return torch.device("cuda:0")


def _pad(items, dtype, fill):
    buf = np.full((len(items), max(x.shape[0] for x in items) + 37), fill, dtype=dtype)
    for b, x in enumerate(items):
        buf[b, :x.shape[0]] = x
    return buf


def _stage(dev, n_fft, hop, fmin, pcm16):
    """one call on the ragged batch (NaN behind every fp32 item's end, -32768 behind every int16 one's; two frames more than the longest item
    has), and the reference of every item: computed once, shared by the tests, never modified"""
    key = (n_fft, hop, pcm16)
    if key not in _cache:
        items, kinds = P.stage_batch(n_fft, hop, seed=7)
        if pcm16:
            raw = [P.as_pcm16(x) for x in items]
            seen = [r.astype(np.float32) * np.float32(1.0 / 32768.0) for r in raw]
            audio = torch.from_numpy(_pad(raw, np.int16, -32768))
        else:
            seen = [x.astype(np.float32) for x in items]
            audio = torch.from_numpy(_pad(seen, np.float32, np.nan))
        lengths = torch.tensor([x.shape[0] for x in items])
        tracker = PitchTracker(dev, sampling_rate=P.SR, n_fft=n_fft, hop_size=hop, fmin=fmin, fmax=FMAX, threshold=THRESHOLD)
        T = max(x.shape[0] // hop for x in items) + 2
        f0, ap, frames, cmnd = tracker(audio.to(dev), lengths, max_frames=T, return_cmnd=True)
        torch.cuda.synchronize()
        refs = [P.yin_reference(s, s.shape[0], P.SR, n_fft, hop, fmin, FMAX, THRESHOLD) for s in seen]
        _cache[key] = dict(kinds=kinds, f0=f0.cpu().numpy(), ap=ap.cpu().numpy(), frames=frames.cpu().numpy(), cmnd=cmnd.cpu().numpy(), refs=refs,
                           tracker=tracker, audio=audio, lengths=lengths, T=T)
    return _cache[key]


@pytest.mark.parametrize("pcm16", [False, True])
@pytest.mark.parametrize("n_fft,hop,fmin", CONFIGS)
def test_stage1_cmnd_against_float64(dev, n_fft, hop, fmin, pcm16):
    s = _stage(dev, n_fft, hop, fmin, pcm16)
    bound = (2 * (n_fft // 2) + 16) * 2.0 ** -24
    tiny = 0
    for b, (ref, kind) in enumerate(zip(s["refs"], s["kinds"])):
        n = ref["dp"].shape[0]
        assert int(s["frames"][b]) == n
        got, want = s["cmnd"][b, :n].astype(np.float64), ref["dp"]
        assert got.shape == want.shape
        small = want < 1e-6
        tiny += int(small.sum())
        err = np.where(small, np.abs(got - want), np.abs(got - want) / np.where(small, 1.0, want))
        print(f"n_fft {n_fft} pcm16 {pcm16} {kind}: {n} frames, worst error {err.max():.3e} = {err.max() / bound:.3f} of the bound {bound:.3e}")
        assert err.max() <= bound
        if kind == "zero":
            assert (got == 1.0).all()
    assert tiny > 0                                         # the exactly periodic item reached the absolute comparison


@pytest.mark.parametrize("pcm16", [False, True])
@pytest.mark.parametrize("n_fft,hop,fmin", CONFIGS)
def test_padding_and_raggedness(dev, n_fft, hop, fmin, pcm16):
    s = _stage(dev, n_fft, hop, fmin, pcm16)
    for b, ref in enumerate(s["refs"]):
        n = ref["dp"].shape[0]
        assert n < s["T"]
        assert (s["f0"][b, n:] == 0).all() and (s["ap"][b, n:] == 0).all() and (s["cmnd"][b, n:] == 0).all()      # rows beyond an item's frames
    for name in ("f0", "ap", "cmnd"):
        assert np.isfinite(s[name]).all(), name             # the NaN (or -32768) behind an item's end reached nothing
    # the int16 padding value would show as a jump: the last frame of every item equals the reference, which never saw the padding (stage 1 above)


@pytest.mark.parametrize("pcm16", [False, True])
@pytest.mark.parametrize("n_fft,hop,fmin", CONFIGS)
def test_stage2_decision_on_the_kernels_own_cmnd(dev, n_fft, hop, fmin, pcm16):
    s = _stage(dev, n_fft, hop, fmin, pcm16)
    tau_min, tau_max = P.lag_range(P.SR, n_fft, fmin, FMAX)
    thr = float(np.float32(THRESHOLD))
    total = without = 0
    worst = 0.0
    for b, ref in enumerate(s["refs"]):
        for t in range(ref["dp"].shape[0]):
            tau, f0, ap, margin = P.decide(s["cmnd"][b, t], P.SR, tau_min, tau_max, thr)
            total += 1
            if margin < P.MARGIN:
                without += 1
                continue
            got = float(s["f0"][b, t])
            assert (got > 0) == (tau > 0), (b, t)
            if tau > 0:
                worst = max(worst, abs(got - f0) / f0)
                assert abs(got - f0) <= 1e-5 * f0, (b, t, got, f0)
            assert float(s["ap"][b, t]) == pytest.approx(ap, rel=1e-6)
    print(f"n_fft {n_fft} pcm16 {pcm16}: {without} of {total} frames without margin; worst relative f0 difference {worst:.3e}")
    assert without <= 0.05 * total
    voiced = sum(int((s["f0"][b] > 0).sum()) for b in range(len(s["refs"])))
    assert voiced >= 20                                     # the comparison above did run on voiced frames


def test_end_to_end_on_known_pitch(dev):
    tones = [P.tone(fa, fb, P.TONE_SAMPLES) for _, fa, fb in P.TONES]
    rng = np.random.default_rng(3)
    items = [x for x, _ in tones] + [0.3 * rng.standard_normal(4000), np.zeros(2000)]
    audio = torch.from_numpy(_pad([x.astype(np.float32) for x in items], np.float32, np.nan))
    tracker = PitchTracker(dev, sampling_rate=P.SR)
    f0, ap, frames = tracker(audio.to(dev), torch.tensor([x.shape[0] for x in items]))
    f0, frames = f0.cpu().numpy(), frames.cpu().numpy()
    bound = 2.0 * P.REFERENCE_TONE_ERROR + 1e-4
    for b, ((name, _, _), (x, f)) in enumerate(zip(P.TONES, tones)):
        inside = P.inside_frames(x.shape[0], 1024, 256)
        errs = [abs(f0[b, t] - P.true_f0(f, t, 1024, 256)) / P.true_f0(f, t, 1024, 256) for t in inside]
        print(f"{name}: worst relative f0 error {max(errs):.3e} (bound {bound:.3e})")
        assert all(f0[b, t] > 0 for t in inside) and max(errs) <= bound
    for b in (len(tones), len(tones) + 1):
        assert frames[b] == items[b].shape[0] // 256 and not (f0[b] > 0).any()


def test_an_item_gives_the_same_bits_anywhere(dev):
    s = _stage(dev, 1024, 256, 60.0, False)
    tracker, audio, lengths = s["tracker"], s["audio"], s["lengths"]
    again = tracker(audio.to(dev), lengths, max_frames=s["T"], return_cmnd=True)
    for got, name in zip(again, ("f0", "ap", "frames", "cmnd")):
        assert np.array_equal(got.cpu().numpy(), s[name]), name                                   # a second call
    for b in range(audio.shape[0]):
        n = int(lengths[b])
        alone = tracker(audio[b:b + 1, :n].contiguous().to(dev), lengths[b:b + 1], max_frames=s["T"], return_cmnd=True)
        order = [(b + 1) % 4, b, (b + 2) % 4]                                                       # another position, other neighbours
        moved = tracker(audio[order].to(dev), lengths[order], max_frames=s["T"], return_cmnd=True)
        for k, name in ((0, "f0"), (1, "ap"), (3, "cmnd")):
            assert np.array_equal(alone[k][0].cpu().numpy(), s[name][b]), (b, name)
            assert np.array_equal(moved[k][1].cpu().numpy(), s[name][b]), (b, name)
