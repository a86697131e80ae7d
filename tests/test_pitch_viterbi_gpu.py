"""GPU (-m gpu): the pitch smoother (efficient_tts_amd/pitch.py `ViterbiSmoother`, csrc/efts_pitch_viterbi.hip) against the int64 restatement of
tests/viterbi_reference.py.  The recurrence is integer-only, so wherever lags are compared the kernel's `lag` must EQUAL the reference's,
everywhere: no tolerance and no margin rule."""
import numpy as np
import pytest
import torch

import pitch_reference as P
import viterbi_reference as V
from efficient_tts_amd import lib as L
from efficient_tts_amd.pitch import PitchTracker, ViterbiSmoother, cost_q16, log2_table

pytestmark = pytest.mark.gpu

SR = 22050
DEFAULT = (0.15, 0.02, 0.35, 0.14)                           # unvoiced, octave, jump, vuv
FRAMES = [37, 1, 0, 20]
SENTINEL = -7.0
_cache = {}


@pytest.fixture(scope="module")
def dev():
    L.load()
    L.require_device()
    return torch.device("cuda:0")


def synthetic(lo, hi, T, seed):
    """d' [4, T, hi + 1]: uniform in [0, 1.2), with values >= 4, +inf and NaN sprinkled in and blocks of exactly equal values (whole frames, runs
    of neighbouring lags, and one item on a grid of sixteenths) so that ties and the clip decide"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.2, size=(4, T, hi + 1)).astype(np.float32)
    x[rng.random((4, T)) < 0.6] *= np.float32(0.2)                                  # frames with lags under the unvoiced cost: voiced stretches
    x[3] = np.round(x[3] * 16.0) / 16.0
    x[rng.random(x.shape) < 0.01] = 4.0
    x[rng.random(x.shape) < 0.01] = 6.5
    x[rng.random(x.shape) < 0.01] = np.inf
    x[rng.random(x.shape) < 0.01] = np.nan
    x[0, T // 2:T // 2 + 2, :] = 0.25
    x[:, :, lo + 1:lo + 4] = x[:, :, lo + 1:lo + 2]
    return x.astype(np.float32)


def run_raw(dev, cmnd, frames, lo, hi, costs=DEFAULT):
    """the library entry itself on a device tensor cmnd [B, T, hi + 1] of any item and frame stride, into outputs that lie between guard rows of a
    sentinel: returns (f0, aperiodicity, lag) as numpy [B, T] after checking that the guards still hold the sentinel"""
    lib = L.load()
    B, T = cmnd.shape[0], cmnd.shape[1]
    assert cmnd.stride(2) == 1
    f0 = torch.full((B + 2, T), SENTINEL, dtype=torch.float32, device=dev)
    ap = torch.full((B + 2, T), SENTINEL, dtype=torch.float32, device=dev)
    lag = torch.full((B + 2, T), int(SENTINEL), dtype=torch.int32, device=dev)
    fr = torch.tensor(frames, dtype=torch.int32, device=dev)
    lg = log2_table(hi).to(dev)
    ws = torch.empty(B * lib.efts_f0_viterbi_workspace_bytes(T, lo, hi), dtype=torch.uint8, device=dev)
    q = [cost_q16("cost", c) for c in costs]
    torch.cuda.synchronize()
    L.check(lib.efts_f0_viterbi(cmnd.data_ptr(), cmnd.stride(0), cmnd.stride(1), fr.data_ptr(), lg.data_ptr(), f0[1].data_ptr(), ap[1].data_ptr(),
                                lag[1].data_ptr(), ws.data_ptr(), ws.numel(), B, T, lo, hi, SR, *q, None), "efts_f0_viterbi")
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in (f0, ap, lag)]
    for o in out:
        assert (o[0] == SENTINEL).all() and (o[-1] == SENTINEL).all()          # nothing outside [B, T] is touched
    return [o[1:-1] for o in out]


def reference(x, frames, lo, hi, costs=DEFAULT):
    """(lag, f0, aperiodicity, den) [B, T] of a batch, zeros at and beyond an item's count"""
    B, T = x.shape[0], x.shape[1]
    lag, f0, ap, den = np.zeros((B, T), np.int64), np.zeros((B, T)), np.zeros((B, T)), np.full((B, T), np.nan)
    for b in range(B):
        n = max(0, min(int(frames[b]), T))
        lag[b, :n] = V.viterbi_reference(x[b, :n], lo, hi, *costs)[0]
        f0[b, :n], ap[b, :n], den[b, :n] = V.outputs_reference(x[b, :n], lag[b, :n], SR, lo, hi)
    return lag, f0, ap, den


def ragged(dev, lo, hi, T, costs=DEFAULT):
    """one call on the ragged synthetic batch and its reference: computed once, shared by the tests, never modified"""
    key = (lo, hi, T, costs)
    if key not in _cache:
        x = synthetic(lo, hi, T, seed=hi)
        _cache[key] = dict(x=x, got=run_raw(dev, torch.from_numpy(x).to(dev), FRAMES, lo, hi, costs), ref=reference(x, FRAMES, lo, hi, costs))
    return _cache[key]


def rows_beyond_are_zero(got, T):
    for o in got:
        for b, n in enumerate(FRAMES):
            assert (o[b, min(n, T):] == 0).all()


@pytest.mark.parametrize("lo,hi,T", [(2, 8, 37), (36, 220, 37), (2, 1024, 5)])
def test_lag_equals_the_reference_on_synthetic_rows(dev, lo, hi, T):
    s = ragged(dev, lo, hi, T)
    lag = s["got"][2]
    print(f"lags {lo} .. {hi}: {int((lag > 0).sum())} voiced of {sum(min(n, T) for n in FRAMES)} frames")
    assert np.array_equal(lag, s["ref"][0])
    rows_beyond_are_zero(s["got"], T)
    n_voiced = int((lag > 0).sum())
    assert 0 < n_voiced < sum(min(n, T) for n in FRAMES)                          # both kinds of state are on the paths


@pytest.mark.parametrize("costs", [(0.3, 0.0, 16.0, 0.05), (0.1, 0.5, 0.0, 0.0), (16.0, 16.0, 0.0, 0.0)])
def test_lag_equals_the_reference_with_other_costs(dev, costs):
    s = ragged(dev, 36, 220, 37, costs)
    assert np.array_equal(s["got"][2], s["ref"][0])
    rows_beyond_are_zero(s["got"], 37)


def test_strided_rows(dev):
    lo, hi, T = 36, 220, 37
    s = ragged(dev, lo, hi, T)
    wide = torch.full((4, T + 3, hi + 1 + 5), float("nan"), device=dev)             # item stride > T (hi + 1), frame stride > hi + 1
    view = wide[:, :T, :hi + 1]
    view.copy_(torch.from_numpy(s["x"]))
    assert view.stride(0) > T * (hi + 1) and view.stride(1) > hi + 1
    got = run_raw(dev, view, FRAMES, lo, hi)
    for a, b in zip(got, s["got"]):
        assert np.array_equal(a, b, equal_nan=True)
    f0, ap, lag = ViterbiSmoother(dev, SR, lo, hi)(view, torch.tensor(FRAMES))      # the owner passes the strides on, and gives the same bits
    for a, b in zip((f0, ap, lag), s["got"]):
        assert np.array_equal(a.cpu().numpy(), b, equal_nan=True)


@pytest.mark.parametrize("lo,hi", [(2, 8), (36, 220)])
def test_constant_rows_leave_only_the_tie_rule(dev, lo, hi):
    T = 12
    x = np.zeros((4, T, hi + 1), np.float32)
    x[0], x[1] = 0.5, 0.0
    x[2] = 0.125                                                                   # under the unvoiced cost: voiced, every lag tied but for the octave term
    x[3] = 0.15                                                                    # q(0.15f) against rint(0.15 Q): decided by one unit of Q16
    frames = [T, T, T, T]
    for costs in (DEFAULT, (0.15, 0.0, 0.35, 0.14), (0.15, 0.0, 0.0, 0.0)):
        got = run_raw(dev, torch.from_numpy(x).to(dev), frames, lo, hi, costs)
        want = reference(x, frames, lo, hi, costs)
        assert np.array_equal(got[2], want[0]), costs
    assert (want[0][0] == 0).all() and (want[0][1] == lo).all() and (want[0][2] == lo).all()


def test_nine_thousand_frames_do_not_overflow(dev):
    """every d' >= 4 and unvoiced_cost 16: each frame adds at least 4 Q to every state, so a plain int32 sum wraps near frame 8192"""
    lo, hi, T = 2, 8, 9000
    rng = np.random.default_rng(5)
    x = (4.0 + rng.uniform(0.0, 2.0, size=(1, T, hi + 1))).astype(np.float32)
    x[0, 100:200] = np.inf
    costs = (16.0, 0.02, 0.35, 0.14)
    got = run_raw(dev, torch.from_numpy(x).to(dev), [T], lo, hi, costs)
    want = reference(x, [T], lo, hi, costs)
    assert (x >= 4.0).all() and (want[0] > 0).all()                                # 4 Q a frame on the cheapest path: 2^31 after 8192 frames
    assert np.array_equal(got[2], want[0])
    assert np.array_equal(got[1], want[2].astype(np.float32))


def test_an_item_alone_and_a_second_run_give_the_same_bits(dev):
    lo, hi, T = 36, 220, 37
    s = ragged(dev, lo, hi, T)
    x = torch.from_numpy(s["x"]).to(dev)
    again = run_raw(dev, x, FRAMES, lo, hi)
    for a, b in zip(again, s["got"]):
        assert a.tobytes() == b.tobytes()
    for b in range(4):
        alone = run_raw(dev, x[b:b + 1], FRAMES[b:b + 1], lo, hi)
        for a, whole in zip(alone, s["got"]):
            assert a[0].tobytes() == whole[b].tobytes(), b


def test_f0_and_aperiodicity(dev):
    lo, hi, T = 36, 220, 37
    s = ragged(dev, lo, hi, T)
    (f0, ap, lag), (_, f0_ref, ap_ref, den) = s["got"], s["ref"]
    voiced = lag > 0
    k = lag[voiced].astype(np.float64)
    assert (f0[voiced] >= np.float32(SR / (k + 1.0)) * (1 - 1e-6)).all() and (f0[voiced] <= np.float32(SR / (k - 1.0)) * (1 + 1e-6)).all()
    assert (f0[~voiced] == 0).all()
    sure = voiced & (np.abs(den) >= 1e-4) & np.isfinite(den)
    rel = np.abs(f0[sure] - f0_ref[sure]) / f0_ref[sure]
    print(f"{int(sure.sum())} of {int(voiced.sum())} voiced frames with |den| >= 1e-4: worst relative f0 error {rel.max():.3e}")
    assert sure.sum() >= 10 and rel.max() <= 1e-5
    assert np.array_equal(ap, ap_ref.astype(np.float32), equal_nan=True)           # d' at the lag, or the row's minimum: copies, so exact


def test_end_to_end_on_the_octave_glitch(dev):
    x = V.glitch_signal()
    short, _ = P.tone(200.0, 200.0, 2000)
    lengths = torch.tensor([x.shape[0], short.shape[0]])
    for pcm16 in (False, True):
        if pcm16:
            audio = np.full((2, x.shape[0] + 11), -32768, np.int16)
            audio[0, :x.shape[0]], audio[1, :short.shape[0]] = P.as_pcm16(x), P.as_pcm16(short)
        else:
            audio = np.full((2, x.shape[0] + 11), np.nan, np.float32)
            audio[0, :x.shape[0]], audio[1, :short.shape[0]] = x, short
        audio = torch.from_numpy(audio).to(dev)
        smooth = PitchTracker(dev, smooth=True)
        f0, ap, frames, cmnd = smooth(audio, lengths, return_cmnd=True)
        assert frames.tolist() == [31, 7] and cmnd.shape == (2, 31, smooth.tau_max + 1) and (smooth.tau_min, smooth.tau_max) == (36, 367)
        assert len(smooth(audio, lengths)) == 3
        f0_s, ap_s, lag = ViterbiSmoother(dev, SR, smooth.tau_min, smooth.tau_max)(cmnd, frames)
        assert torch.equal(f0, f0_s) and torch.equal(ap, ap_s)
        lag, own = lag.cpu().numpy(), cmnd.cpu().numpy()
        want = reference(own, frames.tolist(), smooth.tau_min, smooth.tau_max)[0]   # the reference on the kernel's own d'
        print("pcm16" if pcm16 else "fp32", "smoothed", lag[0].tolist())
        assert np.array_equal(lag, want)
        assert ((lag[0, 2:31] >= 146) & (lag[0, 2:31] <= 148)).all()
        plain = PitchTracker(dev, smooth=False)
        p0, pa, pf = plain(audio, lengths)
        period = SR / p0[0, 13:16].cpu().numpy().clip(min=1.0)
        print("plain lags on frames 13 .. 15:", period.tolist())
        assert ((period >= 71.0) & (period <= 75.0)).any()                          # a lag of 72 .. 74, moved by the parabola by at most 1
        d0, da, df = PitchTracker(dev)(audio, lengths)
        assert d0.cpu().numpy().tobytes() == p0.cpu().numpy().tobytes() and da.cpu().numpy().tobytes() == pa.cpu().numpy().tobytes() and torch.equal(df, pf)
        assert plain.smoother is None
