"""GPU (-m gpu): `efts_noise_profile` and `efts_spectral_gate` through `NoiseProfile` and `SpectralGate` against the float64 definitions of
tests/gate_reference.py on one ragged batch.  The counts and flags must be equal (the inputs keep every frame 0.01 dB from the threshold);
the error bounds of the profile and of the gated signal are not fixed by hand but computed: four times what the same definitions through
torch.stft / torch.istft in fp32 on the CPU lose against the reference on the same inputs.  Then what must hold bit for bit, capture, and
the trainer's chain.
"""
import json
import os

import numpy as np
import pytest
import torch

import denoise_reference as D
import gate_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
NB = len(R.LENGTHS) + len(R.EXTRA)


def _modules(**kw):
    from efficient_tts_amd.denoise import NoiseProfile, SpectralGate
    return NoiseProfile(DEV, top_db=R.TOP_DB, min_frames=R.MIN_FRAMES), SpectralGate(DEV, top_db=R.TOP_DB, min_frames=R.MIN_FRAMES, **kw)


def _batch():
    pcm, audio, lengths = R.batch()
    return torch.from_numpy(pcm).to(DEV), torch.from_numpy(audio).to(DEV), torch.from_numpy(lengths).to(DEV)


def _same(a, b):
    """two dicts of `NoiseProfile` hold the same bits (NaN, the noise_db of an item without a noise frame, equals NaN)"""
    plain = lambda v: v.nan_to_num(nan=-1.0) if v.is_floating_point() else v
    return all(torch.equal(plain(a[k]), plain(b[k])) for k in a)


def _record(key, value):
    """how profiles/gate_error.json is produced: EFTS_WRITE_PROFILES=1 merges this test's figures into it"""
    if not os.environ.get("EFTS_WRITE_PROFILES"):
        return
    path = os.path.join(ROOT, "profiles", "gate_error.json")
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[key] = value
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def test_counts_equal_and_profile_within_four_times_the_fp32_yardstick():
    ref = R.reference_profiles()
    yard = R.profile_yardstick()
    pcm, audio, lengths = _batch()
    measure, _ = _modules()
    worst = 0.0
    for x in (audio, pcm):
        got = measure(x, lengths)
        assert got["profile"].shape == (NB, 513) and got["profile"].dtype == torch.float32 and got["noise_db"].dtype == torch.float64
        assert got["noise_frames"].dtype == torch.int32 and got["frames"].dtype == torch.int32
        assert got["frames"].tolist() == [p["frames"] for p in ref]
        assert got["noise_frames"].tolist() == [p["noise_frames"] for p in ref]                     # no item left out
        prof, db = got["profile"].cpu().numpy().astype(np.float64), got["noise_db"].cpu().numpy()
        for b, p in enumerate(ref):
            if p["noise_frames"] >= R.MIN_FRAMES:
                worst = max(worst, float(np.abs(prof[b] - p["profile"]).max()))
            else:
                assert not prof[b].any()                                                            # exactly 0, and K is still reported
            if p["noise_frames"]:
                assert abs(db[b] - p["noise_db"]) <= 1e-9
            else:
                assert np.isnan(db[b])
    scale = max(float(p["profile"].max()) for p in ref)
    print(f"profile: max |device - reference| = {worst:.3e}; fp32 torch.stft mean on the CPU: {yard:.3e}; bound 4 x = {4 * yard:.3e}; "
          f"largest profile value {scale:.3e}")
    _record("profile", {"device_max_abs_error": worst, "yardstick_fp32_torch_cpu_max_abs_error": yard, "bound": 4 * yard, "largest_value": scale,
                        "lengths": [int(n) for n in R.batch()[2]], "noise_frames": [p["noise_frames"] for p in ref]})
    assert 0.0 < yard < 1e-5 * scale                                   # the yardstick itself is an fp32 rounding error
    assert worst <= 4 * yard


def test_gate_within_four_times_the_fp32_yardstick():
    """the whole `SpectralGate` call (profile measured per item, short-of-noise items bypassed) and the call with one given row, at every
    strength and floor, fp32 and int16; the reference and the yardstick gate with the profile that the device was given or measured"""
    ref = R.reference_profiles()
    pcm, audio, lengths = _batch()
    _, host, n_host = R.batch()
    _, gate = _modules()
    bypass = [p["noise_frames"] < R.MIN_FRAMES for p in ref]
    shared = ref[7]["profile"].astype(np.float32)                      # the longest item's floor for everybody: nothing is bypassed
    worst = yard = 0.0
    for s in R.STRENGTHS:
        for fl in R.FLOORS:
            outs = []
            for x in (audio, pcm):
                out, stats = gate(x, lengths, strength=s, floor=fl, return_stats=True)
                assert stats["noise_frames"].tolist() == [p["noise_frames"] for p in ref]
                outs.append((out.cpu().numpy().astype(np.float64), stats["profile"].cpu().numpy(), bypass))
                out = gate(x, lengths, profile=torch.from_numpy(shared), strength=s, floor=fl)
                outs.append((out.cpu().numpy().astype(np.float64), np.tile(shared, (NB, 1)), [False] * NB))
            assert np.array_equal(outs[0][1], outs[2][1])              # int16 and fp32 measure the same profile
            for b in range(NB):
                n = int(n_host[b])
                x = host[b, :n]
                for k in (0, 1):                                        # measured, given: one reference and one yardstick each, for both dtypes
                    prof, skip = outs[k][1][b], outs[k][2][b]
                    want = R.gate(x, prof, s, fl, bypass=skip)
                    if n > 512 and not skip:
                        yard = max(yard, float(np.abs(R.gate_torch(x, prof, s, fl, torch.float32) - want).max()))
                    for got in (outs[k][0], outs[k + 2][0]):
                        assert not got[b, n:].any()
                        if n:
                            worst = max(worst, float(np.abs(got[b, :n] - want).max()))
    print(f"gate: max |device - reference| = {worst:.3e}; fp32 torch.stft / istft on the CPU: {yard:.3e}; bound 4 x = {4 * yard:.3e}")
    _record("gate", {"device_max_abs_error": worst, "yardstick_fp32_torch_cpu_max_abs_error": yard, "bound": 4 * yard,
                     "strengths": list(R.STRENGTHS), "floors": list(R.FLOORS), "dtypes": ["float32", "int16"]})
    assert 0.0 < yard < 1e-6                                           # an fp32 rounding error on signals of peak 0.5
    assert worst <= 4 * yard


def test_floor_zero_with_one_shared_row_gives_the_bits_of_the_bias_denoiser():
    from efficient_tts_amd import lib as L
    from efficient_tts_amd import ops as O
    from efficient_tts_amd.denoise import BiasDenoiser
    _, audio, lengths = _batch()
    _, gate = _modules()
    bias = D.bias_spectrum() * 0.01
    for s in (0.0, 0.5, 5.0):
        want = BiasDenoiser(DEV, bias, strength=s)(audio, lengths)
        assert torch.equal(gate(audio, lengths, profile=torch.from_numpy(bias), strength=s, floor=0.0), want)               # ld_profile = 0
        assert torch.equal(gate(audio, lengths, profile=torch.from_numpy(np.tile(bias, (NB, 1))), strength=s, floor=0.0), want)   # B equal rows
        assert not torch.equal(gate(audio, lengths, profile=torch.from_numpy(bias), strength=s, floor=0.5), want) or s == 0.0
    # the entry itself with an all-zero bypass array is the entry with none
    lib = L.load()
    out = torch.empty_like(audio)
    frames = torch.empty(NB, dtype=torch.int32, device=DEV)
    b = torch.from_numpy(bias).to(DEV)
    zeros = torch.zeros(NB, dtype=torch.int32, device=DEV)
    with O.stream_scope():
        L.check(lib.efts_spectral_gate(audio.data_ptr(), 0, 1.0, audio.shape[1], lengths.data_ptr(), audio.shape[1], gate._window(audio.device).data_ptr(),
                                       b.data_ptr(), 0, 0.5, 0.0, zeros.data_ptr(), out.data_ptr(), audio.shape[1], frames.data_ptr(), NB, O._stream()), "gate")
    assert torch.equal(out, BiasDenoiser(DEV, bias, strength=0.5)(audio, lengths))
    assert frames.tolist() == [p["frames"] for p in R.reference_profiles()]


def test_int16_input_gives_the_bits_of_its_fp32_twin():
    pcm, audio, lengths = _batch()
    measure, gate = _modules()
    a, b = measure(audio, lengths), measure(pcm, lengths)
    assert _same(a, b)
    assert torch.equal(gate(audio, lengths), gate(pcm, lengths))
    shared = a["profile"][7]
    assert torch.equal(gate(audio, lengths, profile=shared, strength=2.5, floor=0.0), gate(pcm, lengths, profile=shared, strength=2.5, floor=0.0))
    # another max_wav_value is another scale: fl32(sample / 32767) goes in, and comes out of a bypassed item
    from efficient_tts_amd.denoise import SpectralGate
    g2 = SpectralGate(DEV, max_wav_value=32767.0)
    twin = pcm.to(torch.float32) * torch.tensor(1.0 / 32767.0, dtype=torch.float32)
    assert torch.equal(g2(pcm, lengths), g2(twin, lengths))


def test_every_item_alone_elsewhere_and_with_nan_behind_it_gives_the_same_bits():
    pcm, audio, lengths = _batch()
    measure, gate = _modules()
    stats, out = measure(audio, lengths), gate(audio, lengths)
    assert _same(measure(audio, lengths), stats) and torch.equal(gate(audio, lengths), out)
    for b in range(NB):
        n = int(R.batch()[2][b])
        one = measure(audio[b:b + 1], lengths[b:b + 1])
        assert _same(one, {k: v[b:b + 1] for k, v in stats.items()}), b
        assert torch.equal(gate(audio[b:b + 1], lengths[b:b + 1])[0], out[b]), b
        if n > 512:                                                    # and in a buffer of its own size, with no lengths given
            assert torch.equal(gate(audio[b:b + 1, :n].contiguous())[0], out[b, :n]), b
            assert _same(measure(pcm[b:b + 1, :n].contiguous()), {k: v[b:b + 1] for k, v in stats.items()}), b
        assert float(out[b, n:].abs().max()) == 0.0                    # zeros lie behind len
    poisoned = audio.clone()
    for b in range(NB):
        poisoned[b, int(R.batch()[2][b]):] = float("nan")
    assert _same(measure(poisoned, lengths), stats) and torch.equal(gate(poisoned, lengths), out)
    perm = torch.tensor([11, 7, 0, 6, 10, 1, 5, 2, 9, 4, 3, 8], device=DEV)
    assert _same(measure(audio[perm].contiguous(), lengths[perm]), {k: v[perm] for k, v in stats.items()})
    assert torch.equal(gate(audio[perm].contiguous(), lengths[perm]), out[perm])


def test_bypassed_items_are_copied_bit_for_bit_and_the_threshold_is_min_frames():
    pcm, audio, lengths = _batch()
    ref = R.reference_profiles()
    _, gate = _modules()
    names = list(R.LENGTHS) + list(R.EXTRA)
    for x, want in ((audio, audio), (pcm, audio)):                     # int16: fl32(sample * pcm_scale), which is `audio`
        out, stats = gate(x, lengths, return_stats=True)
        for b, p in enumerate(ref):
            n = int(R.batch()[2][b])
            copied = torch.equal(out[b, :n], want[b, :n])
            if p["noise_frames"] < R.MIN_FRAMES or n <= 512:
                assert copied, names[b]
            else:
                assert not copied, names[b]
    by = dict(zip(names, range(NB)))
    assert ref[by["exact"]]["noise_frames"] == R.MIN_FRAMES and ref[by["short"]]["noise_frames"] == R.MIN_FRAMES - 1
    assert stats["noise_frames"][by["short"]].item() == R.MIN_FRAMES - 1 and not stats["profile"][by["short"]].any()
    for k in ("zeros", "tone", 0, 512, 513):
        assert torch.equal(out[by[k]], audio[by[k]])
    # one frame fewer asked for: the item that fell short is gated as well
    from efficient_tts_amd.denoise import SpectralGate
    lower = SpectralGate(DEV, top_db=R.TOP_DB, min_frames=R.MIN_FRAMES - 1)(audio, lengths)
    assert not torch.equal(lower[by["short"]], audio[by["short"]]) and torch.equal(lower[by["exact"]], out[by["exact"]])
    # with a profile given nothing is bypassed
    given = gate(audio, lengths, profile=stats["profile"][by["exact"]])
    assert not torch.equal(given[by["tone"]], audio[by["tone"]]) and torch.equal(given[by[512]], audio[by[512]])


def test_one_capture_replays_the_eager_bits_and_values_go_by_value():
    pcm, audio, lengths = _batch()
    _, gate = _modules()
    eager = gate(pcm, lengths, return_stats=True)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        gate(pcm, lengths)                                             # warm-up on the capture stream: window and workspace exist afterwards
    torch.cuda.current_stream().wait_stream(stream)
    from efficient_tts_amd import lib as L
    lib = L.load()
    real = {k: getattr(lib, k) for k in ("efts_noise_profile", "efts_spectral_gate")}
    seen = []

    def spy(name):
        def call(*args):
            seen.append((name, args[-1], torch.cuda.current_stream().cuda_stream, torch.cuda.is_current_stream_capturing()))
            return real[name](*args)
        return call
    graph = torch.cuda.CUDAGraph()
    for k in real:
        setattr(lib, k, spy(k))
    try:
        with torch.cuda.graph(graph):                                  # one stream, no side stream: the graph is a single chain
            out, stats = gate(pcm, lengths, return_stats=True)
    finally:
        for k, v in real.items():
            setattr(lib, k, v)
    assert [s[0] for s in seen] == ["efts_noise_profile", "efts_spectral_gate"] and all(s[1] == s[2] and s[3] for s in seen)
    out.zero_()
    stats["profile"].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[0]) and _same(stats, eager[1])
    # strength and floor are plain by-value arguments of the one launch: another pair is another call with the same device arguments
    a = gate(audio, lengths, strength=2.0, floor=0.0)
    b = gate(audio, lengths, strength=2.0, floor=0.3)
    assert not torch.equal(a, b) and not torch.equal(a, eager[0])
    assert gate.strength == 1.0 and gate.floor == 0.1 and torch.equal(gate(pcm, lengths), eager[0])


def test_trainer_chain_is_inert_without_a_gate_and_runs_the_four_modules_in_order():
    from efficient_tts_amd.bin.train import build_gate, build_loudness, build_trimmer
    from efficient_tts_amd.frontend import LogMelFrontend
    from efficient_tts_amd.resample import Resampler
    from efficient_tts_amd.trainer import EfficientTTSTrainer
    dev = torch.device("cuda:0")
    cfg = dict(outdir="/tmp", log_interval_steps=5, eval_interval_steps=0, save_interval_steps=10, train_max_steps=20, grad_norm=1.0,
               bucket_frames=0, bucket_phones=0, trim_silence=True, normalize_loudness=-23.0)
    t = EfficientTTSTrainer(steps=0, epochs=0, data_loader={}, sampler={}, model=torch.nn.Linear(2, 2), optimizer=None, scheduler=None, config=cfg,
                            device=dev)
    t.frontend = LogMelFrontend(dev)
    t.resampler = Resampler(dev, 24000, 22050)
    t.trimmer, t.loudness = build_trimmer(cfg, dev), build_loudness(cfg, dev)
    pcm, _, lengths = R.batch()
    keep = [5, 6, 7, 10]
    audio, lens = torch.from_numpy(pcm[keep]), torch.from_numpy(lengths[keep]).long()
    text, text_lengths = torch.ones(len(keep), 6, dtype=torch.long), torch.full((len(keep),), 6, dtype=torch.long)
    batch = (text, text_lengths, audio, lens)

    def by_hand(gate):
        x, n = t.resampler(audio.to(dev), lens.to(dev))
        if gate is not None:
            x = gate(x, n)
        x, n = t.trimmer(x, n)
        x = t.loudness(x, n)
        return t.frontend(x, n, max_frames=int(t.frontend.frames_of(n).max()))
    assert t.gate is None and build_gate(cfg, dev) is None             # the key absent: the path of before, bit for bit
    plain = t._stage(batch)
    want = by_hand(None)
    assert torch.equal(plain[2], want[0]) and torch.equal(plain[3], want[1])
    t.gate = build_gate(dict(cfg, denoise_corpus=True, denoise_floor=0.05), dev)
    assert t.gate.floor == 0.05
    gated = t._stage(batch)
    want = by_hand(t.gate)
    assert torch.equal(gated[2], want[0]) and torch.equal(gated[3], want[1])
    assert gated[2].shape != plain[2].shape or not torch.equal(gated[2], plain[2])
    assert torch.equal(gated[0].cpu(), text) and torch.equal(gated[1].cpu(), text_lengths)
