"""GPU (-m gpu): the command-line side of loudness normalisation on tiny wav files that the tests write -- `bin/loudness.py`'s table,
`bin/inference.py` with and without `--loudness`, and the training entry point refusing a recipe that sets the level twice.
"""
import numpy as np
import pytest
import torch
import yaml

import loudness_reference as R

pytestmark = pytest.mark.gpu


def test_loudness_tsv(tmp_path):
    from scipy.io.wavfile import write
    from efficient_tts_amd.bin.loudness import COLUMNS, main
    rng = np.random.default_rng(3)
    fs = 16000
    wavs = {"a": R._quantise(rng.uniform(-0.3, 0.3, size=fs)), "b": R._quantise(rng.uniform(-0.01, 0.01, size=fs + 777)),
            "c": np.zeros(fs // 2, np.int16), "d": R._quantise(rng.uniform(-0.02, 0.02, size=fs))}
    wavs["d"][::1000] = 30000                                         # clicks: the ceiling limits the gain
    (tmp_path / "wavs").mkdir()
    for k, v in wavs.items():
        write(str(tmp_path / "wavs" / f"{k}.wav"), fs, v)
    (tmp_path / "list.txt").write_text("".join(f"DUMMY/{k}.wav|some text\n" for k in wavs))
    assert main(["--filelist", str(tmp_path / "list.txt"), "--wav_path", str(tmp_path / "wavs"), "--outdir", str(tmp_path / "o"),
                 "--target", "-20", "--peak_ceiling", "0.5", "--batch_size", "3"]) == 0
    rows = [line.split("\t") for line in (tmp_path / "o" / "loudness.tsv").read_text().splitlines()]
    assert tuple(rows[0]) == COLUMNS == ("id", "seconds", "lufs", "gain_db", "limited") and [r[0] for r in rows[1:]] == list(wavs)
    for row, (k, v) in zip(rows[1:], wavs.items()):
        ref = R.measure(v, fs, target=-20.0, ceiling=0.5)
        assert float(row[1]) == pytest.approx(v.shape[0] / fs, abs=1e-4)
        assert int(row[4]) == (ref["flags"] >> 1) == (1 if k == "d" else 0)
        if ref["flags"] & 1:
            assert row[2] == "-inf" and float(row[3]) == 0.0
        else:
            assert float(row[2]) == pytest.approx(ref["lufs"], abs=1e-3) and float(row[3]) == pytest.approx(20.0 * np.log10(ref["gain"] * 32768.0), abs=1e-3)
    assert float(rows[1][3]) == pytest.approx(-20.0 - float(rows[1][2]), abs=2e-3)                   # unlimited: the gain is the distance to the target


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
        """stands in for the generator: seeded uniform noise of amplitude 0.1 (about -25.5 LUFS), T * 256 samples per item"""
        def vocoder(mel, lens=None):
            g = torch.Generator().manual_seed(int(mel.shape[2]))
            return (torch.rand(mel.shape[0], 1, mel.shape[2] * 256, generator=g) * 0.2 - 0.1).to(mel.device)
        return vocoder
    monkeypatch.setattr(I, "build_vocoder", build_vocoder)

    class Refuse:
        def __init__(self, *a, **k):
            raise AssertionError("no normaliser may be built without --loudness")
    real = I.LoudnessNormalizer
    monkeypatch.setattr(I, "LoudnessNormalizer", Refuse)
    assert I.main(base + ["--outdir", str(tmp_path / "plain")]) == 0   # without the flag nothing of the feature is even constructed
    monkeypatch.setattr(I, "LoudnessNormalizer", real)
    assert I.main(base + ["--outdir", str(tmp_path / "loud"), "--loudness", "-30"]) == 0
    assert I.main(base + ["--outdir", str(tmp_path / "loud2"), "--loudness", "-30", "--batch_size", "2"]) == 0
    for n in range(2):
        sr, a = read(str(tmp_path / "plain" / f"utt{n}_7steps.wav"))
        # ... and the file holds the vocoder's samples as they were: quantised as before, nothing in between
        noise = build_vocoder(None, None)(torch.zeros(1, 80, a.shape[0] // 256))[0, 0]
        assert np.array_equal(a, (noise.clamp(-1.0, 1.0) * 32767.0).round().to(torch.int16).numpy())
        _, b = read(str(tmp_path / "loud" / f"utt{n}_7steps.wav"))
        _, c = read(str(tmp_path / "loud2" / f"utt{n}_7steps.wav"))
        assert sr == 22050 and a.shape == b.shape == c.shape and a.shape[0] >= 8820 and a.shape[0] % 256 == 0
        before, after = R.measure(a, 22050)["lufs"], R.measure(b, 22050)["lufs"]
        print(f"utt{n}: {before:.3f} LUFS -> {after:.3f} LUFS")
        assert np.isfinite(before) and abs(before - -30.0) > 0.5     # the vocoder's own level is somewhere else
        assert abs(after - -30.0) <= 0.1                             # 16-bit quantisation at this level moves it by far less
        assert abs(R.measure(c, 22050)["lufs"] - -30.0) <= 0.1


def test_training_refuses_peak_and_loudness_together(tmp_path):
    from efficient_tts_amd.bin.train import build_loudness
    cfg = yaml.safe_load("normalize_peak: 0.95\nnormalize_loudness: -23.0\nfrontend_params: {sampling_rate: 22050}\n")
    with pytest.raises(ValueError, match="normalize_peak"):
        build_loudness(cfg, torch.device("cuda:0"))
    n = build_loudness(yaml.safe_load("normalize_loudness: -23.0\nloudness_peak_ceiling: 0.9\n"), torch.device("cuda:0"))
    x = torch.from_numpy(R._quantise(np.random.default_rng(0).uniform(-0.1, 0.1, size=(2, 11025)))).cuda()
    out, lufs, gains, flags, blocks = n(x, return_stats=True)
    assert out.shape == x.shape and not flags.any() and torch.isfinite(lufs).all()
