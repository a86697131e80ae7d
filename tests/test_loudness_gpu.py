"""GPU (-m gpu): loudness metering and normalisation (efficient_tts_amd/loudness.py, csrc/efts_loudness.hip) through the Python classes, and
therefore the C ABI, against the strictly sequential float64 restatement in tests/loudness_reference.py, which never sees the product's code.

Tolerances.  lufs: 1e-6 LU -- the device filters segments of 512 samples from zero state with 0.2 s of warm-up, which costs at most 2e-8 dB
against the sequential filter, and fp64 rounding over 1e5 operations costs about 1e-10 dB; 1e-6 leaves 50x and is far below anything
audible.  gains: 4e-7 relative -- 1.2e-7 from the loudness tolerance, one fp32 rounding, the ulp of `pow`.  Block counts and flags: ==,
tests/test_loudness_cpu.py asserts that every block of these inputs is at least 0.01 LU from both gates.  Samples: bit for bit
float32(x) * the device's own gain; exact zeros behind every length.  The padding behind every item is full scale.
"""
import numpy as np
import pytest
import torch

import loudness_reference as R
from efficient_tts_amd import lib as L
from efficient_tts_amd.loudness import LoudnessMeter, LoudnessNormalizer

pytestmark = pytest.mark.gpu

LUFS_TOL, GAIN_RTOL = 1e-6, 4e-7
DTYPES = [np.int16, np.float32]


@pytest.fixture(scope="module")
def dev():
    L.load()
    L.require_device()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases():
    """every case with its reference results, computed once: name -> (case, {dtype: x}, {dtype: [per item]})"""
    out = {}
    for name, c in R.cases().items():
        xs = {np.int16: c["x"], np.float32: R.as_float(c["x"])}
        xs[np.float32].setflags(write=False)
        out[name] = (c, xs, {d: R.reference(c, d) for d in DTYPES})
    return out


def _run(dev, case, x, **kw):
    n = LoudnessNormalizer(dev, case["fs"], target_lufs=case["target"], peak_ceiling=case["ceiling"])
    res = n(torch.from_numpy(np.array(x)).to(dev), torch.tensor(case["lengths"]), return_stats=True, **kw)
    torch.cuda.synchronize()
    return n, res


def _check(name, case, x, ref, res):
    out, lufs, gains, flags, blocks = (t.cpu().numpy() for t in res)
    assert out.dtype == np.float32 and out.shape == x.shape and lufs.dtype == np.float64 and gains.dtype == np.float32
    assert flags.dtype == np.int32 and blocks.dtype == np.int32 and blocks.shape == (x.shape[0], 2)
    for b, v in enumerate(case["lengths"]):
        r = ref[b]
        d_lufs = 0.0 if lufs[b] == r["lufs"] else abs(lufs[b] - r["lufs"])
        d_gain = abs(float(gains[b]) / float(r["gain"]) - 1.0)
        print(f"{name} {x.dtype.name} item {b} len {v}: {lufs[b]:.9f} LUFS (ref {r['lufs']:.9f}, off {d_lufs:.3g} LU) gain {gains[b]!r} "
              f"(ref {r['gain']!r}, off {d_gain:.3g}) flags {flags[b]} ({r['flags']}) blocks {tuple(blocks[b])} ({r['blocks']})")
        assert d_lufs <= LUFS_TOL
        assert tuple(int(k) for k in blocks[b]) == r["blocks"]
        assert int(flags[b]) == r["flags"]
        assert d_gain <= GAIN_RTOL
        want = x[b, :v].astype(np.float32) * gains[b]
        assert np.array_equal(out[b, :v].view(np.uint32), want.view(np.uint32))
        assert np.array_equal(out[b, v:].view(np.uint32), np.zeros(x.shape[1] - v, np.uint32))       # +0.0 behind the length


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["main", "48k", "dc", "edges"])
def test_equals_the_reference(dev, cases, name, dtype):
    """main: B = 4, 22 050 Hz, 3 s, lengths 66150, 40000, 8819 (one sample short of a block), 0; 48k: the slowest decay in samples; dc: an
    offset plus 30 Hz, the worst case for the high-pass state; edges: lengths around a multiple of the segment and of h"""
    case, xs, refs = cases[name]
    _, res = _run(dev, case, xs[dtype])
    _check(name, case, xs[dtype], refs[dtype], res)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ceiling_limits_the_gain(dev, cases, dtype):
    case, xs, refs = cases["ceiling"]
    _, res = _run(dev, case, xs[dtype])
    _check("ceiling", case, xs[dtype], refs[dtype], res)
    out, flags = res[0].cpu().numpy(), res[3].cpu().numpy()
    assert (flags & 2).all()
    for b in range(out.shape[0]):
        peak = float(np.abs(out[b]).max())
        print(f"ceiling item {b}: max |out| {peak!r}")
        assert peak <= case["ceiling"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_items_alone_elsewhere_and_again(dev, cases, dtype):
    case, xs, _ = cases["main"]
    x = torch.from_numpy(np.array(xs[dtype])).to(dev)
    lengths = torch.tensor(case["lengths"])
    n = LoudnessNormalizer(dev, case["fs"], target_lufs=case["target"], peak_ceiling=case["ceiling"])
    batch = n(x, lengths, return_stats=True)
    again = n(x, lengths, return_stats=True)
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(batch, again))
    assert torch.equal(batch[1].view(torch.int64), again[1].view(torch.int64))                      # the loudness to the bit, -inf included
    order = [2, 3, 1, 0]                                             # every item at another position, behind another neighbour
    moved = n(x[order], lengths[order], return_stats=True)
    for pos, b in enumerate(order):
        assert torch.equal(moved[0][pos], batch[0][b]) and torch.equal(moved[1][pos].view(torch.int64), batch[1][b].view(torch.int64))
        assert all(torch.equal(m[pos], a[b]) for m, a in zip(moved[2:], batch[2:]))
    for b, v in enumerate(case["lengths"]):
        alone = n(x[b:b + 1, :max(v, 1)].contiguous(), lengths[b:b + 1], return_stats=True)         # its own row length: another workspace layout
        assert torch.equal(alone[0][0], batch[0][b, :max(v, 1)]) and torch.equal(alone[1][0].view(torch.int64), batch[1][b].view(torch.int64))
        assert all(torch.equal(a[0], c[b]) for a, c in zip(alone[2:], batch[2:]))


def test_meter_equals_the_normalisers_loudness(dev, cases):
    case, xs, refs = cases["main"]
    lengths = torch.tensor(case["lengths"])
    for dtype in DTYPES:
        x = torch.from_numpy(np.array(xs[dtype])).to(dev)
        lufs = LoudnessMeter(dev, case["fs"])(x, lengths)
        ref = LoudnessNormalizer(dev, case["fs"])(x, lengths, return_stats=True)[1]
        assert lufs.dtype == torch.float64 and torch.equal(lufs.view(torch.int64), ref.view(torch.int64))
        assert lufs.cpu().tolist()[2:] == [-np.inf, -np.inf]
    # no lengths: whole rows, the padding included (row 0 has none; the step up to full scale behind row 1's item adds to it)
    whole = LoudnessMeter(dev, case["fs"])(x)
    assert whole[0].item() == lufs[0].item() and whole[1].item() != lufs[1].item()
    # without a ceiling and at another target the gain moves by exactly the difference, in dB
    g23 = LoudnessNormalizer(dev, case["fs"], -23.0, None)(x, lengths, return_stats=True)[2]
    g29 = LoudnessNormalizer(dev, case["fs"], -29.0, None)(x, lengths, return_stats=True)[2]
    assert torch.allclose(g23[:2] / g29[:2], torch.full((2,), 10.0 ** (6.0 / 20.0), device=dev), rtol=1e-6) and torch.equal(g23[2:], g29[2:])


def test_refusal_before_any_launch(dev, cases):
    case, xs, _ = cases["edges"]
    n = LoudnessNormalizer(dev, case["fs"])
    x = torch.from_numpy(np.array(xs[np.int16])).to(dev)
    with pytest.raises(ValueError):
        n(x, torch.tensor([1, 2]))                                   # lengths of another batch
    n.target_lufs = float("nan")                                     # past the constructor: the library refuses it, EFTS_EINVAL
    with pytest.raises(ValueError, match="efts_loudness_pcm16"):
        n(x)
    n.target_lufs, n.sampling_rate = -23.0, 11025                    # EFTS_ESHAPE (the workspace size is 0 for it)
    n._ws.clear()
    with pytest.raises(ValueError, match="sampling rate"):
        n(x)


def test_trainer_stage_runs_the_normaliser(dev):
    from efficient_tts_amd.bin.train import build_loudness
    from efficient_tts_amd.datasets import SyntheticTextAudio, TextMelCollate
    from efficient_tts_amd.frontend import LogMelFrontend
    from efficient_tts_amd.trainer import EfficientTTSTrainer
    cfg = dict(outdir="/tmp", log_interval_steps=5, eval_interval_steps=0, save_interval_steps=10, train_max_steps=20, grad_norm=1.0,
               bucket_frames=0, bucket_phones=0)
    t = EfficientTTSTrainer(steps=0, epochs=0, data_loader={}, sampler={}, model=torch.nn.Linear(2, 2), optimizer=None, scheduler=None, config=cfg,
                            device=dev)
    t.frontend = LogMelFrontend(dev)
    batch = TextMelCollate()([(text, audio) for text, audio in SyntheticTextAudio(n_items=3, min_phones=6, max_phones=12)])
    text, text_lengths, audio, lengths = batch
    assert t.loudness is None                                        # the key absent: the path of before, bit for bit
    mel0, ml0 = t._stage(batch)[2:]
    ref0, rl0 = t.frontend(audio, lengths)
    assert torch.equal(mel0, ref0) and torch.equal(ml0, rl0)
    t.loudness = build_loudness(dict(cfg, normalize_loudness=-23.0), dev)
    out = t._stage(batch)
    level = np.zeros(tuple(audio.shape), dtype=np.float32)
    for b in range(audio.shape[0]):
        v = int(lengths[b])
        ref = R.measure(audio[b, :v].numpy(), 22050, -23.0, 0.99)
        level[b, :v] = audio[b, :v].numpy().astype(np.float32) * ref["gain"]
    ref_mel, ref_frames = t.frontend(torch.from_numpy(level).to(dev), lengths)
    assert torch.equal(out[3], ref_frames) and torch.equal(out[3], ml0)                              # lengths stay
    # the reference's gain may differ from the device's in its last bits (4e-7): log-mels then agree to that, far inside 1e-4
    assert float((out[2] - ref_mel).abs().max()) <= 1e-4 and not torch.equal(out[2], mel0)
    assert torch.equal(out[0].cpu(), text) and torch.equal(out[1].cpu(), text_lengths)
