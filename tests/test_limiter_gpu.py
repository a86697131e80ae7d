"""GPU (-m gpu): true-peak metering and the look-ahead limiter (efficient_tts_amd/limiter.py, csrc/efts_limiter.hip) through the Python
classes, and therefore the C ABI, against the float64 restatement in tests/limiter_reference.py, which never sees the product's code.

Tolerances.  Nothing fixed in advance: every figure (the peaks, the output samples, the smallest gain, the true peak of the output) may
differ from the float64 reference by four times what the same definition in fp32 numpy loses against that reference on the same inputs,
the largest error over the batch on either side.  The sample peak and the count of limited samples must be equal: tests/test_limiter_cpu.py
asserts that no decision on these inputs is close.  |out| <= c (1 + 2e-7): the division and the product round once each.  Bits: an item under
the ceiling, an all-zero item, +0.0 behind every length, an item alone against the same item in the batch, two runs, a captured call.

Measured on an MI355X (profiles/limiter_error.json): the device's largest errors over all cases are 6.7e-7 on the output, 7.1e-7 on the
smallest gain and 1.7e-7 on the true peak, at most 1.3 times the fp32 numpy yardstick's on the same case; the true peak of the output stands
+0.033 dB over a ceiling of 0.5 with (H, S) = (32, 32), +0.0002 dB with (16, 8) and +0.034 dB over -1 dBTP with (32, 32), reference and device
alike.

Then the two command lines with their new flags on tiny files that the tests write."""
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml

import limiter_reference as R
import loudness_reference as LR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
REPORT = {}


def _meter():
    from efficient_tts_amd.limiter import TruePeakMeter
    return TruePeakMeter(DEV)


def _limiter(c, h, s):
    from efficient_tts_amd.limiter import PeakLimiter
    lim = PeakLimiter(DEV, ceiling_dbtp=20.0 * math.log10(c), hold=h, smooth=s)
    assert lim.ceiling == c
    return lim


def _inputs(pcm16):
    audio, lengths = R.batch(pcm16)
    return torch.from_numpy(audio.copy()).to(DEV), torch.from_numpy(lengths.copy()).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _record(name, entry):
    REPORT[name] = entry
    if os.environ.get("EFTS_WRITE_PROFILES"):                          # how profiles/limiter_error.json is produced
        with open(os.path.join(ROOT, "profiles", "limiter_error.json"), "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)
            f.write("\n")


@pytest.mark.parametrize("pcm16", [False, True], ids=["fp32", "int16"])
def test_peaks_against_the_float64_reference(pcm16):
    audio, lengths = _inputs(pcm16)
    tp, sp = _meter()(audio, lengths)
    assert tp.dtype == sp.dtype == torch.float32 and tp.shape == sp.shape == (audio.shape[0],)
    tp, sp = tp.cpu().numpy(), sp.cpu().numpy()
    ref, yard = R.peaks_batch(pcm16, "float64"), R.peaks_batch(pcm16, "float32")
    worst = max(abs(float(tp[b]) - float(r[0])) for b, r in enumerate(ref))
    bound = 4.0 * max(abs(float(y[0]) - float(r[0])) for y, r in zip(yard, ref))
    print(f"true peak: max |device - reference| = {worst:.3e}; the definition in fp32 numpy: {bound / 4:.3e}; bound 4 x = {bound:.3e}")
    _record(f"meter_{'int16' if pcm16 else 'fp32'}", {"device_max_abs_error": worst, "yardstick_fp32_numpy_cpu_max_abs_error": bound / 4, "bound": bound})
    for b, r in enumerate(ref):
        assert float(sp[b]) == float(r[1]), b                          # a maximum of fp32 values: exact
        assert tp[b] >= sp[b]
    assert tp[0] == 0.0 and sp[0] == 0.0 and tp[R.ZERO] == 0.0
    assert abs(float(sp[R.SINE]) - math.sqrt(0.5)) < 1e-4 and float(tp[R.SINE]) > 0.99
    assert 0.0 < bound < 4e-6 and worst <= bound


@pytest.mark.parametrize("pcm16,c,h,s", R.cases(), ids=[f"{'int16' if p else 'fp32'}-c{c:.3f}-h{h}-s{s}" for p, c, h, s in R.cases()])
def test_limiter_against_the_float64_reference(pcm16, c, h, s):
    audio, lengths = _inputs(pcm16)
    out, gain_min, limited, tp_in = _limiter(c, h, s)(audio, lengths, return_stats=True)
    assert out.dtype == gain_min.dtype == tp_in.dtype == torch.float32 and limited.dtype == torch.int32 and out.shape == audio.shape
    tp_out = _meter()(out, lengths)[0].cpu().numpy()
    o, gm, lm, ti = out.cpu().numpy(), gain_min.cpu().numpy(), limited.cpu().numpy(), tp_in.cpu().numpy()
    ref, yard = R.limit_batch(pcm16, c, h, s, "float64"), R.limit_batch(pcm16, c, h, s, "float32")
    err = dict(out=0.0, gain_min=0.0, true_peak_in=0.0, true_peak_out=0.0)
    yerr = dict(err)
    for b, (r, y) in enumerate(zip(ref, yard)):
        n = int(lengths[b])
        if n:
            err["out"] = max(err["out"], float(np.abs(o[b, :n] - r["out"]).max()))
            yerr["out"] = max(yerr["out"], float(np.abs(y["out"] - r["out"]).max()))
            assert np.all(np.abs(o[b, :n].astype(np.float64)) <= c * (1 + 2e-7)), b
        for k, got in (("gain_min", gm[b]), ("true_peak_in", ti[b]), ("true_peak_out", tp_out[b])):
            err[k] = max(err[k], abs(float(got) - float(r[k])))
            yerr[k] = max(yerr[k], abs(float(y[k]) - float(r[k])))
        assert int(lm[b]) == r["limited"], (b, int(lm[b]), r["limited"])
        assert not _bits(out[b, n:]).any(), b                          # +0.0 behind the length, whatever lay there
    src = audio.float() * (1.0 / 32768.0) if pcm16 else audio
    for b in (R.UNDER, R.ZERO):                                        # under the ceiling: every gain is exactly 1
        n = int(lengths[b])
        assert torch.equal(_bits(out[b, :n]), _bits(src[b, :n])) and int(lm[b]) == 0 and float(gm[b]) == 1.0
    assert int(lm[0]) == 0 and float(gm[0]) == 1.0 and float(ti[0]) == 0.0
    clicks = range(1, 8)
    excess_ref = max(R.excess_db(float(ref[b]["true_peak_out"]), c) for b in clicks)
    excess_dev = max(R.excess_db(float(tp_out[b]), c) for b in clicks)
    print(f"max |device - reference|: {err}; the definition in fp32 numpy: {yerr}; true peak of the output over the ceiling: "
          f"reference {excess_ref:+.5f} dB, device {excess_dev:+.5f} dB")
    _record(f"limit_{'int16' if pcm16 else 'fp32'}_c{c:.4f}_h{h}_s{s}",
            {"device_max_abs_error": err, "yardstick_fp32_numpy_cpu_max_abs_error": yerr, "bound_factor": 4,
             "excess_over_ceiling_db_reference": excess_ref, "excess_over_ceiling_db_device": excess_dev})
    for k in err:                                                      # the true peak of the output included: no absolute bound on the excess
        assert 0.0 < yerr[k] < 1e-5 and err[k] <= 4.0 * yerr[k], (k, err[k], yerr[k])


@pytest.mark.parametrize("pcm16", [False, True], ids=["fp32", "int16"])
def test_an_item_gives_the_same_bits_alone_twice_and_whatever_lies_behind_it(pcm16):
    audio, lengths = _inputs(pcm16)
    lim, meter = _limiter(0.5, 32, 32), _meter()
    got = lim(audio, lengths, return_stats=True) + meter(audio, lengths)
    again = lim(audio, lengths, return_stats=True) + meter(audio, lengths)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, again))
    other = audio.clone()
    for b, n in enumerate(lengths.tolist()):
        other[b, n:] = 0 if pcm16 else float("nan")
    behind = lim(other, lengths, return_stats=True) + meter(other, lengths)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, behind))
    for b, n in enumerate(lengths.tolist()):
        x = audio[b:b + 1, :max(n, 1)].contiguous()                    # in a buffer of its own size (the empty item: one sample, length 0)
        alone = lim(x, lengths[b:b + 1], return_stats=True) + meter(x, lengths[b:b + 1])
        assert torch.equal(_bits(alone[0][0, :n]), _bits(got[0][b, :n])), b
        assert all(torch.equal(_bits(a), _bits(g[b:b + 1])) for a, g in zip(alone[1:], got[1:])), b
    perm = torch.arange(audio.shape[0] - 1, -1, -1, device=DEV)
    permuted = lim(audio[perm].contiguous(), lengths[perm], return_stats=True)
    assert all(torch.equal(_bits(a), _bits(g[perm])) for a, g in zip(permuted, got[:4]))


def test_a_captured_call_replays_the_eager_bits():
    audio, lengths = _inputs(False)
    lim, meter = _limiter(R.CEILINGS[1], 64, 32), _meter()
    eager = lim(audio, lengths, return_stats=True) + meter(audio, lengths)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        lim(audio, lengths, return_stats=True)                         # warm-up on the capture stream
        meter(audio, lengths)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = lim(audio, lengths, return_stats=True) + meter(audio, lengths)
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(captured, eager))


def test_a_row_that_is_not_16_byte_aligned_takes_the_element_stores():
    """ld_out = 1001: rows 1 .. 3 begin off a 16-byte boundary, and the last group of four is cut"""
    x = torch.from_numpy(np.stack([R.click_signal(1001, 50 + b) for b in range(3)]).astype(np.float32)).to(DEV)
    lengths = torch.tensor([1001, 1000, 3], device=DEV)
    out = _limiter(0.5, 16, 8)(x, lengths)
    worst = yard = 0.0
    for b, n in enumerate(lengths.tolist()):
        item = x[b, :n].cpu().numpy()
        r = R.limit(item, 0.5, 16, 8, np.float64)
        worst = max(worst, float(np.abs(out[b, :n].cpu().numpy() - r["out"]).max()))
        yard = max(yard, float(np.abs(R.limit(item, 0.5, 16, 8, np.float32)["out"] - r["out"]).max()))
        assert not _bits(out[b, n:]).any()
    print(f"max |device - reference| = {worst:.3e}; the definition in fp32 numpy: {yard:.3e}")
    assert 0.0 < yard < 1e-6 and worst <= 4.0 * yard


def test_loudness_tsv_with_true_peak(tmp_path):
    from scipy.io.wavfile import write
    from efficient_tts_amd.bin.loudness import COLUMNS, PEAK_COLUMNS, main
    fs = 16000
    rng = np.random.default_rng(3)
    wavs = {"a": LR._quantise(rng.uniform(-0.3, 0.3, size=fs)), "s": np.round(R.fs4_sine(fs) * 20000.0).astype(np.int16), "z": np.zeros(fs // 2, np.int16)}
    (tmp_path / "wavs").mkdir()
    for k, v in wavs.items():
        write(str(tmp_path / "wavs" / f"{k}.wav"), fs, v)
    (tmp_path / "list.txt").write_text("".join(f"DUMMY/{k}.wav|some text\n" for k in wavs))
    common = ["--filelist", str(tmp_path / "list.txt"), "--wav_path", str(tmp_path / "wavs"), "--batch_size", "2"]
    assert main(common + ["--outdir", str(tmp_path / "plain")]) == 0 and main(common + ["--outdir", str(tmp_path / "peaks"), "--true_peak"]) == 0
    plain = [line.split("\t") for line in (tmp_path / "plain" / "loudness.tsv").read_text().splitlines()]
    rows = [line.split("\t") for line in (tmp_path / "peaks" / "loudness.tsv").read_text().splitlines()]
    assert tuple(plain[0]) == COLUMNS and tuple(rows[0]) == COLUMNS + PEAK_COLUMNS == COLUMNS + ("sample_peak_db", "true_peak_dbtp")
    assert [r[:5] for r in rows] == plain                             # the flag appends, nothing else moves
    for row, (k, v) in zip(rows[1:], wavs.items()):
        tp, sp = R.peaks(v, np.float64)
        if k == "z":
            assert row[5] == row[6] == "-inf"
        else:
            assert float(row[5]) == pytest.approx(20 * math.log10(sp), abs=2e-3) and float(row[6]) == pytest.approx(20 * math.log10(tp), abs=2e-3)
    assert float(rows[2][6]) - float(rows[2][5]) > 2.9                 # the fs / 4 sine: 3 dB that the sample peak does not see


def test_inference_cli_without_and_with_the_flag(tmp_path, monkeypatch):
    from scipy.io.wavfile import read
    from efficient_tts_amd import EfficientTTSCNN
    from efficient_tts_amd.bin import inference as I
    exp = tmp_path / "exp"
    exp.mkdir()
    phones = ["_"] + [f"P{i}" for i in range(1, 76)]
    (tmp_path / "phn.txt").write_text("\n".join(phones) + "\n")
    rng = np.random.default_rng(1)
    lines = [f"DUMMY/utt{n}.wav|" + " ".join(phones[int(i)] for i in rng.integers(1, 76, size=k)) for n, k in enumerate((30, 24))]
    (tmp_path / "test.txt").write_text("\n".join(lines) + "\n")
    params = dict(num_symbols=76, dropout_rate=0.0, use_masking=True, use_weighted_masking=False, sigma=0.01)
    with open(exp / "config.yml", "w") as f:
        yaml.dump(dict(model_name="EfficientTTSCNN", model_params=params, dataset_params=dict(use_phnseq=True, phnset_path=str(tmp_path / "phn.txt"))), f)
    torch.manual_seed(0)
    m = EfficientTTSCNN(**params)
    with torch.no_grad():
        m.duration_predictor.linear.bias.fill_(1.5)                  # a few frames per phoneme with random weights
    torch.save({"model": m.state_dict(), "steps": 7}, exp / "checkpoint-7steps.pkl")
    base = ["--checkpoint", str(exp / "checkpoint-7steps.pkl"), "--test_fid_scp", str(tmp_path / "test.txt"), "--verbose", "0"]

    def build_vocoder(args, device):
        """stands in for the generator: seeded uniform noise of amplitude 0.1 (about -25.5 LUFS) with +0.97 on every 4001st sample"""
        def vocoder(mel, lens=None):
            g = torch.Generator().manual_seed(int(mel.shape[2]))
            x = torch.rand(mel.shape[0], 1, mel.shape[2] * 256, generator=g) * 0.2 - 0.1
            x[:, :, 1000::4001] = 0.97
            return x.to(mel.device)
        return vocoder
    monkeypatch.setattr(I, "build_vocoder", build_vocoder)

    class Refuse:
        def __init__(self, *a, **k):
            raise AssertionError("no limiter may be built without --limit_true_peak")
    real = I.PeakLimiter
    monkeypatch.setattr(I, "PeakLimiter", Refuse)
    assert I.main(base + ["--outdir", str(tmp_path / "plain")]) == 0   # without the flag nothing of the feature is even constructed
    assert I.main(base + ["--outdir", str(tmp_path / "loud"), "--loudness", "-16"]) == 0
    monkeypatch.setattr(I, "PeakLimiter", real)
    assert I.main(base + ["--outdir", str(tmp_path / "lim"), "--limit_true_peak", "-1"]) == 0
    assert I.main(base + ["--outdir", str(tmp_path / "lim2"), "--limit_true_peak", "-1", "--batch_size", "2"]) == 0
    assert I.main(base + ["--outdir", str(tmp_path / "both"), "--limit_true_peak", "-1", "--loudness", "-16", "--batch_size", "2"]) == 0
    assert I.main(base + ["--outdir", str(tmp_path / "rate"), "--limit_true_peak", "-1", "--sampling_rate", "16000"]) == 0
    c = R.CEILINGS[1]
    top = int(math.floor(c * 32767.0 + 0.5))
    for n in range(2):
        sr, a = read(str(tmp_path / "plain" / f"utt{n}_7steps.wav"))
        noise = build_vocoder(None, None)(torch.zeros(1, 80, a.shape[0] // 256))[0, 0]
        assert np.array_equal(a, (noise.clamp(-1.0, 1.0) * 32767.0).round().to(torch.int16).numpy())       # the file of before, byte for byte
        assert sr == 22050 and a.shape[0] >= 8820 and np.abs(a).max() == round(0.97 * 32767)
        # (a batch of two is one call of the stand-in, seeded by the longer item: its rows are other noise than the single calls')
        frames = [read(str(tmp_path / "plain" / f"utt{k}_7steps.wav"))[1].shape[0] // 256 for k in range(2)]
        noise2 = build_vocoder(None, None)(torch.zeros(2, 80, max(frames)))[n, 0, :a.shape[0]]
        for name, x in (("lim", noise), ("lim2", noise2)):
            want = np.round(R.limit(x.numpy(), c, 33, 33, np.float64)["out"] * 32767.0)
            _, b = read(str(tmp_path / name / f"utt{n}_7steps.wav"))
            assert b.shape == a.shape and np.abs(b.astype(np.int64) - want).max() <= 1 and np.abs(b).max() <= top
            assert np.array_equal(b[:900], (x[:900] * 32767.0).round().to(torch.int16).numpy())      # far from a peak nothing changes
        _, loud = read(str(tmp_path / "loud" / f"utt{n}_7steps.wav"))
        _, both = read(str(tmp_path / "both" / f"utt{n}_7steps.wav"))
        l_loud, l_both = LR.measure(loud, 22050)["lufs"], LR.measure(both, 22050)["lufs"]
        print(f"utt{n}: --loudness -16 alone reaches {l_loud:.2f} LUFS (its ceiling cut the gain back); with the limiter {l_both:.2f} LUFS, peak {np.abs(both).max()}")
        assert l_loud < -20.0                                          # the one loud sample costs the normaliser alone several LU
        assert abs(l_both - -16.0) <= 0.5 and np.abs(both).max() <= top
        sr16, r16 = read(str(tmp_path / "rate" / f"utt{n}_7steps.wav"))
        assert sr16 == 16000 and np.abs(r16).max() <= top              # built for the output rate, behind the conversion
