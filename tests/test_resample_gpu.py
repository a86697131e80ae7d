"""GPU (-m gpu): the sample-rate converter (efficient_tts_amd/resample.py, csrc/efts_resample.hip) against the float64 restatement of
tests/resample_reference.py, which evaluates h(tau) per output sample and never sees the product's table.

Inputs are uniform noise in [-1, 1], fixed seed.  Bound, derived and not tuned: an fp32 chain of K fused multiply-adds against exact sums
deviates by at most K * 2^-23 * max_p sum_k |h[p][k]| * max |x| (`resample_reference.bound`, computed from the formula's table: about 8e-5
for the largest K); the fp32 rounding of the taps (<= 6e-8 each) lies far inside it.  An indexing error is of the order of 0.1.
Samples that must be zero and results that must be bit-identical are asserted with ==.
"""
import numpy as np
import pytest
import torch
import yaml

import resample_reference as R
from efficient_tts_amd import lib as L
from efficient_tts_amd.resample import Resampler, resample_length, resample_table

pytestmark = pytest.mark.gpu

PAIRS = [(48000, 22050), (22050, 48000), (44100, 22050), (16000, 22050), (22050, 8000)]
LENGTHS = (4001, 2500, 37)
LD_IN = 4003                      # not a multiple of 4


@pytest.fixture(scope="module")
def dev():
    L.load()
    L.require_device()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def noise():
    rng = np.random.default_rng(20260)
    x = rng.uniform(-1.0, 1.0, size=(len(LENGTHS), LD_IN)).astype(np.float32)
    x.setflags(write=False)
    return x


def _call(dev, x, lengths, src, dst, quality, ld_out, pcm_scale=None):
    """efts_resample / efts_resample_pcm16 through the binding; the output row is pre-filled with a sentinel"""
    table, Lp, M, W = resample_table(src, dst, quality)
    xd = torch.from_numpy(np.array(x)).to(dev).contiguous()
    B, ld_in = xd.shape
    li = torch.tensor(lengths, dtype=torch.int32, device=dev)
    out = torch.full((B, ld_out), 7.0, dtype=torch.float32, device=dev)
    ol = torch.full((B,), -1, dtype=torch.int32, device=dev)
    td = table.to(dev)
    st = torch.cuda.current_stream().cuda_stream
    if pcm_scale is None:
        L.check(L.load().efts_resample(xd.data_ptr(), ld_in, li.data_ptr(), td.data_ptr(), Lp, M, W, out.data_ptr(), ld_out, ol.data_ptr(), B, st),
                "efts_resample")
    else:
        L.check(L.load().efts_resample_pcm16(xd.data_ptr(), ld_in, pcm_scale, li.data_ptr(), td.data_ptr(), Lp, M, W, out.data_ptr(), ld_out,
                                             ol.data_ptr(), B, st), "efts_resample_pcm16")
    torch.cuda.synchronize()
    return out.cpu().numpy(), ol.cpu().numpy()


@pytest.mark.parametrize("quality", ["best", "fast"])
@pytest.mark.parametrize("src,dst", PAIRS)
def test_parity_with_the_fp64_reference(dev, noise, src, dst, quality):
    ld_out = resample_length(LD_IN, src, dst) + 29                                    # larger than needed
    lengths = list(LENGTHS) + [0]
    x = np.concatenate([noise, noise[:1]], axis=0)                                    # the item of length 0 has samples behind it that must not be read
    out, ol = _call(dev, x, lengths, src, dst, quality, ld_out)
    tol = R.bound(src, dst, quality, peak=float(np.abs(noise).max()))
    worst = 0.0
    for b, n in enumerate(lengths):
        n_out = resample_length(n, src, dst)
        assert ol[b] == n_out == R.length(n, src, dst)
        ref = R.resample(x[b, :n], src, dst, quality)
        if n_out:
            worst = max(worst, float(np.abs(out[b, :n_out] - ref).max()))
        assert (out[b, n_out:] == 0.0).all()
    print(f"{src}->{dst} {quality}: max |device - fp64| {worst:.3e}, bound {tol:.3e}")
    assert worst <= tol
    assert ol[3] == 0 and (out[3] == 0.0).all()


def test_pcm16_entry_equals_the_float_entry(dev):
    rng = np.random.default_rng(7)
    pcm = rng.integers(-32768, 32768, size=(3, LD_IN)).astype(np.int16)
    ld_out = resample_length(LD_IN, 48000, 22050) + 5
    a, la = _call(dev, pcm, LENGTHS, 48000, 22050, "best", ld_out, pcm_scale=1.0 / 32768.0)
    b, lb = _call(dev, pcm.astype(np.float32) * np.float32(1.0 / 32768.0), LENGTHS, 48000, 22050, "best", ld_out)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(la, lb)
    y, n = Resampler(dev, 48000, 22050)(torch.from_numpy(pcm).to(dev), torch.tensor(LENGTHS))
    assert y.shape == (3, resample_length(LD_IN, 48000, 22050)) and n.tolist() == [resample_length(v, 48000, 22050) for v in LENGTHS]
    assert np.array_equal(y.cpu().numpy().view(np.uint32), a[:, :y.shape[1]].view(np.uint32))


@pytest.mark.parametrize("src,dst,quality", [(48000, 22050, "best"), (16000, 22050, "fast"), (22050, 8000, "best")])
def test_determinism_and_items_alone(dev, noise, src, dst, quality):
    ld_out = resample_length(LD_IN, src, dst) + 3
    a, _ = _call(dev, noise, LENGTHS, src, dst, quality, ld_out)
    b, _ = _call(dev, noise, LENGTHS, src, dst, quality, ld_out)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for i, n in enumerate(LENGTHS):
        alone, ln = _call(dev, noise[i:i + 1, :n].copy(), [n], src, dst, quality, resample_length(n, src, dst))
        assert ln[0] == resample_length(n, src, dst)
        assert np.array_equal(alone[0].view(np.uint32), a[i, :ln[0]].view(np.uint32))


def test_wide_positions(dev):
    """n M passes 2^31 inside one item: 14.7 M samples at 48000 -> 22050 (M = 320, the crossing at output 6 710 886)"""
    src, dst, n_in = 48000, 22050, 14_700_000
    g = torch.Generator().manual_seed(3)
    x = torch.rand(1, n_in, generator=g) * 2.0 - 1.0
    y, n = Resampler(dev, src, dst)(x.to(dev))
    n_out = resample_length(n_in, src, dst)
    assert int(n[0]) == n_out == y.shape[1]
    cross = 2 ** 31 // 320
    assert 1024 < cross < n_out - 4096
    tol = R.bound(src, dst, "best")
    xs = x[0].numpy()
    for lo in (cross - 1024, n_out - 2048):
        idx = np.arange(lo, lo + 2048)
        ref = R.resample(xs, src, dst, "best", outputs=idx)
        err = float(np.abs(y[0, lo:lo + 2048].cpu().numpy() - ref).max())
        print(f"outputs {lo} .. {lo + 2048}: max |device - fp64| {err:.3e}, bound {tol:.3e}")
        assert err <= tol


def test_trainer_stage_runs_the_resampler(dev):
    from efficient_tts_amd.frontend import LogMelFrontend
    from efficient_tts_amd.trainer import EfficientTTSTrainer
    cfg = dict(outdir="/tmp", log_interval_steps=5, eval_interval_steps=0, save_interval_steps=10, train_max_steps=20, grad_norm=1.0,
               bucket_frames=0, bucket_phones=0)
    t = EfficientTTSTrainer(steps=0, epochs=0, data_loader={}, sampler={}, model=torch.nn.Linear(2, 2), optimizer=None, scheduler=None, config=cfg,
                            device=dev)
    t.frontend = LogMelFrontend(dev)
    rng = np.random.default_rng(11)
    audio = torch.from_numpy(rng.integers(-20000, 20000, size=(3, 24000)).astype(np.int16))
    lengths = torch.tensor([24000, 17011, 9000])
    audio[1, 17011:] = 0
    audio[2, 9000:] = 0
    text, text_lengths = torch.randint(1, 70, (3, 12)), torch.tensor([12, 9, 7])
    # a 22 050 Hz batch without a resampler: the code of before
    mel0, ml0 = t._stage((text, text_lengths, audio, lengths))[2:]
    ref0, rl0 = t.frontend(audio, lengths)
    assert torch.equal(mel0, ref0) and torch.equal(ml0, rl0)
    # the same samples declared as a 48 kHz corpus
    t.resampler = Resampler(dev, 48000, 22050)
    out = t._stage((text, text_lengths, audio, lengths))
    conv, conv_lengths = Resampler(dev, 48000, 22050)(audio.to(dev), lengths.to(dev))
    ref, ref_lengths = t.frontend(conv, conv_lengths)
    assert conv_lengths.tolist() == [resample_length(int(n), 48000, 22050) for n in lengths]
    assert torch.equal(out[2], ref) and torch.equal(out[3], ref_lengths)
    assert torch.equal(out[3].cpu(), t.frontend.frames_of(conv_lengths).cpu())
    assert torch.equal(out[0].cpu(), text) and torch.equal(out[1].cpu(), text_lengths)


def test_inference_cli_sampling_rate(tmp_path):
    from scipy.io.wavfile import read
    from efficient_tts_amd import EfficientTTSCNN
    from efficient_tts_amd.bin.inference import main
    exp = tmp_path / "exp"
    exp.mkdir()
    phones = ["_"] + [f"P{i}" for i in range(1, 76)]
    (tmp_path / "phn.txt").write_text("\n".join(phones) + "\n")
    rng = np.random.default_rng(1)
    lines = [f"DUMMY/utt{n}.wav|" + " ".join(phones[int(i)] for i in rng.integers(1, 76, size=k)) for n, k in enumerate((9, 14, 11))]
    (tmp_path / "test.txt").write_text("\n".join(lines) + "\n")
    params = dict(num_symbols=76, dropout_rate=0.0, use_masking=True, use_weighted_masking=False, sigma=0.01)
    with open(exp / "config.yml", "w") as f:
        yaml.dump(dict(model_name="EfficientTTSCNN", model_params=params, dataset_params=dict(use_phnseq=True, phnset_path=str(tmp_path / "phn.txt"))), f)
    torch.manual_seed(0)
    m = EfficientTTSCNN(**params)
    with torch.no_grad():
        m.duration_predictor.linear.bias.fill_(1.5)              # a few frames per phoneme with random weights
    torch.save({"model": m.state_dict(), "steps": 7}, exp / "checkpoint-7steps.pkl")
    base = ["--checkpoint", str(exp / "checkpoint-7steps.pkl"), "--test_fid_scp", str(tmp_path / "test.txt"), "--verbose", "0",
            "--vocoder", "griffinlim", "--gl_iters", "2"]
    assert main(base + ["--outdir", str(tmp_path / "plain")]) == 0
    assert main(base + ["--outdir", str(tmp_path / "same"), "--sampling_rate", "22050"]) == 0
    assert main(base + ["--outdir", str(tmp_path / "r16"), "--sampling_rate", "16000"]) == 0
    assert main(base + ["--outdir", str(tmp_path / "r16b"), "--sampling_rate", "16000", "--batch_size", "3"]) == 0
    for n in range(3):
        name = f"utt{n}_7steps.wav"
        with open(tmp_path / "plain" / name, "rb") as f1, open(tmp_path / "same" / name, "rb") as f2:
            assert f1.read() == f2.read()
        sr0, a0 = read(str(tmp_path / "plain" / name))
        assert sr0 == 22050 and a0.shape[0] % 256 == 0
        for d in ("r16", "r16b"):
            sr, a = read(str(tmp_path / d / name))
            assert sr == 16000 and a.dtype == np.int16 and a.shape == (resample_length(a0.shape[0], 22050, 16000),)
