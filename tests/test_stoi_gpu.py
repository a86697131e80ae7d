"""GPU (-m gpu): `efts_stoi` through `ShortTimeIntelligibility` against the float64 definition of tests/stoi_reference.py on one ragged batch at
10 000 Hz -- a perfect copy and three noise levels, as fp32 and as int16 --: the counts and the places of NaN exactly, the two scores within
four times what the same definition in fp32 numpy loses against that reference on the same inputs.  Then invariance, the 22 050 Hz path and
capture.

Measured on an MI355X (profiles/stoi_error.json): the device's largest error over both scores is 5.94e-7 on the fp32 batch and 9.80e-7 on the
int16 one; the fp32 numpy yardstick's is 9.44e-7 and 1.10e-6, so the bounds are 3.77e-6 and 4.41e-6."""
import json
import os

import numpy as np
import pytest
import torch

import stoi_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
KEYS = ("stoi", "estoi", "frames", "kept", "segments")


def _scorer(rate=10000):
    from efficient_tts_amd.stoi import ShortTimeIntelligibility
    return ShortTimeIntelligibility(DEV, rate)


def _inputs(snr, pcm16=False):
    x, lengths, _ = R.batch()
    y = R.processed(snr)
    if pcm16:
        x, y = R.to_pcm16(x), R.to_pcm16(y)
    return torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), torch.from_numpy(lengths).to(DEV)


def _same(a, b):
    return all(torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)) for k in KEYS)      # (bits: NaN equals NaN)


def test_counts_nan_and_scores_against_the_float64_reference_within_four_times_the_fp32_yardstick():
    s = _scorer()
    report = {}
    for pcm16 in (False, True):
        ref, yard = R.reference_batch(pcm16), R.yardstick(pcm16)
        worst = 0.0
        for snr in R.SNRS:
            out = s(*_inputs(snr, pcm16))
            assert out["stoi"].dtype == out["estoi"].dtype == torch.float64 and out["frames"].dtype == out["kept"].dtype == out["segments"].dtype == torch.int64
            got = {k: out[k].cpu().numpy() for k in KEYS}
            for b, r in enumerate(ref[snr]):
                assert (int(got["frames"][b]), int(got["kept"][b]), int(got["segments"][b])) == (r["frames"], r["kept"], r["segments"]), (pcm16, snr, b)
                for k in ("stoi", "estoi"):
                    assert np.isnan(got[k][b]) == np.isnan(r[k]), (pcm16, snr, b, k)
                    if not np.isnan(r[k]):
                        worst = max(worst, abs(float(got[k][b]) - r[k]))
                        assert 0.0 < got[k][b] <= 1.0 + 1e-6
        print(f"int16 {pcm16}: max |device - reference| = {worst:.3e}; the definition in fp32 numpy on the CPU: {yard:.3e}; bound 4 x = {4 * yard:.3e}")
        report["int16" if pcm16 else "fp32"] = {"device_max_abs_error": worst, "yardstick_fp32_numpy_cpu_max_abs_error": yard, "bound": 4 * yard}
    if os.environ.get("EFTS_WRITE_PROFILES"):                          # how profiles/stoi_error.json is produced
        with open(os.path.join(ROOT, "profiles", "stoi_error.json"), "w") as f:
            json.dump(dict(report, lengths=[int(n) for n in R.batch()[1]], snr_db=[None if v is None else float(v) for v in R.SNRS]), f)
            f.write("\n")
    for v in report.values():
        assert 0.0 < v["yardstick_fp32_numpy_cpu_max_abs_error"] < 1e-5
        assert v["device_max_abs_error"] <= v["bound"]


def test_every_item_alone_twice_permuted_and_with_nan_behind_it_gives_the_same_bits():
    s = _scorer()
    x, y, lengths = _inputs(5.0)
    out = s(x, y, lengths)
    assert _same(s(x, y, lengths), out)
    for b in range(x.shape[0]):
        alone = s(x[b:b + 1], y[b:b + 1], lengths[b:b + 1])
        assert all(torch.equal(alone[k].view(torch.int64), out[k][b:b + 1].view(torch.int64)) for k in KEYS), b
        n = int(lengths[b])                                            # and in buffers of its own size, with no lengths given
        tight = s(x[b:b + 1, :n].contiguous(), y[b:b + 1, :n + 3].contiguous())
        assert all(torch.equal(tight[k].view(torch.int64), out[k][b:b + 1].view(torch.int64)) for k in KEYS), b
    px, py = x.clone(), y.clone()
    for b, n in enumerate(lengths.tolist()):
        px[b, n:] = float("nan")
        py[b, n:] = float("nan")
    assert _same(s(px, py, lengths), out)
    perm = torch.tensor([4, 0, 5, 2, 1, 3], device=DEV)
    permuted = s(x[perm].contiguous(), y[perm].contiguous(), lengths[perm])
    assert all(torch.equal(permuted[k].view(torch.int64), out[k][perm].view(torch.int64)) for k in KEYS)


def test_at_22050_hz_the_scores_are_the_core_call_on_the_resamplers_own_outputs():
    from efficient_tts_amd.resample import Resampler
    rng = np.random.default_rng(5)
    n = 44100
    x = np.stack([R.speech_like(n, 21), R.speech_like(n, 22)])         # (played at 22 050 Hz: every frequency 2.2 times as high)
    y = (x + 0.02 * rng.standard_normal(x.shape)).astype(np.float32)
    lengths = torch.tensor([n, 30000], device=DEV)
    x, y = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    s = _scorer(22050)
    out = s(x, y, lengths)
    r = Resampler(DEV, 22050, 10000)
    x10, n10 = r(x, lengths)
    y10, _ = r(y, lengths)
    assert n10.tolist() == [20000, (30000 * 200 + 440) // 441]
    core = s.score_10k(x10, y10, n10)
    assert _same(out, core) and _same(_scorer(10000)(x10, y10, n10), core)
    assert out["frames"].tolist() == [R.frame_count(int(v)) for v in n10.tolist()]
    assert int(out["segments"][0]) > 0 and 0.0 < float(out["estoi"][0]) < float(out["stoi"][0]) < 1.0


def test_a_captured_call_replays_the_eager_bits():
    s = _scorer()
    x, y, lengths = _inputs(20.0)
    eager = s(x, y, lengths)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        s(x, y, lengths)                                               # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = s(x, y, lengths)
    for k in ("stoi", "estoi"):
        captured[k].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same(captured, eager)
