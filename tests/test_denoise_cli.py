"""GPU (-m gpu): the command-line side of the bias denoiser -- `bin/inference.py` with and without `--denoise` on a two-line list with a
random-weight generator, and `bin/vocoder_score.py --denoise` on tiny wav files that the test writes.
"""
import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu


def test_inference_cli_without_and_with_the_flag(tmp_path, monkeypatch):
    from scipy.io.wavfile import read
    from test_vocoder import CFG
    from efficient_tts_amd import EfficientTTSCNN
    from efficient_tts_amd.bin import inference as I
    from efficient_tts_amd.denoise import BiasDenoiser
    from efficient_tts_amd.vocoder import HiFiGANGenerator
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

    torch.manual_seed(5)
    gen = HiFiGANGenerator(CFG).to("cuda").eval()                    # random weights, the same generator for every run
    gen.remove_weight_norm()
    seen = []

    def build_vocoder(args, device):
        def vocoder(mel, lens=None):
            out = gen(mel) if lens is None else gen(mel, lens)
            if not bool((mel == mel.flatten()[0]).all()):              # (a constant mel: the blank one of from_vocoder)
                seen.append((out.detach().clone(), None if lens is None else lens.clone()))
            return out
        return vocoder
    monkeypatch.setattr(I, "build_vocoder", build_vocoder)

    class Refuse:
        @classmethod
        def from_vocoder(cls, *a, **k):
            raise AssertionError("no denoiser may be built without --denoise")
    monkeypatch.setattr(I, "BiasDenoiser", Refuse)
    assert I.main(base + ["--outdir", str(tmp_path / "plain")]) == 0   # without the flag nothing of the feature is even constructed
    assert I.main(base + ["--outdir", str(tmp_path / "plain2")]) == 0
    monkeypatch.setattr(I, "BiasDenoiser", BiasDenoiser)
    seen.clear()
    assert I.main(base + ["--outdir", str(tmp_path / "den"), "--denoise", "0.01"]) == 0
    singles = list(seen)
    seen.clear()
    assert I.main(base + ["--outdir", str(tmp_path / "den2"), "--denoise", "0.01", "--batch_size", "2"]) == 0
    batched = list(seen)
    assert len(singles) == 2 and len(batched) == 1
    d = BiasDenoiser.from_vocoder(gen, "cuda", strength=0.01)
    quantise = lambda v: (v.clamp(-1.0, 1.0) * 32767.0).round().to(torch.int16).cpu().numpy()
    audio2, lens2 = batched[0]
    want2 = d(audio2[:, 0].float(), lens2.to("cuda") * 256)
    for n in range(2):
        name = f"utt{n}_7steps.wav"
        a, a2 = (tmp_path / "plain" / name).read_bytes(), (tmp_path / "plain2" / name).read_bytes()
        b = (tmp_path / "den" / name).read_bytes()
        assert a == a2 and a != b                                      # inert without the flag; the flag changes the samples
        sr, plain = read(str(tmp_path / "plain" / name))
        assert sr == 22050 and np.array_equal(plain, quantise(singles[n][0][0, 0]))       # ... and the plain file is the vocoder's output
        _, got = read(str(tmp_path / "den" / name))
        assert np.array_equal(got, quantise(d(singles[n][0][0, 0][None].float())[0]))
        _, got2 = read(str(tmp_path / "den2" / name))
        k = int(lens2[n]) * 256
        assert got2.shape[0] == k and np.array_equal(got2, quantise(want2[n, :k]))


def test_vocoder_score_with_the_flag_scores_the_denoised_copy(tmp_path):
    from scipy.io.wavfile import write
    from efficient_tts_amd.bin import vocoder_score as V
    rng = np.random.default_rng(2)
    (tmp_path / "wavs").mkdir()
    t = np.arange(22050) / 22050.0
    for k, f0 in (("a", 180.0), ("b", 260.0)):
        x = 0.3 * np.sin(2 * np.pi * f0 * t) * (1.0 + 0.5 * np.sin(2 * np.pi * 3.0 * t)) + 0.01 * rng.standard_normal(t.shape[0])
        write(str(tmp_path / "wavs" / f"{k}.wav"), 22050, (x * 32767.0).round().astype(np.int16))
    (tmp_path / "list.txt").write_text("DUMMY/a.wav|x\nDUMMY/b.wav|y\n")
    base = ["--test_fid_scp", str(tmp_path / "list.txt"), "--wav_path", str(tmp_path / "wavs"), "--vocoder", "griffinlim", "--gl_iters", "2"]
    assert V.main(base + ["--outdir", str(tmp_path / "plain")]) == 0
    assert V.main(base + ["--outdir", str(tmp_path / "den"), "--denoise", "0.01"]) == 0
    plain, den = (tmp_path / "plain" / "mrstft.tsv").read_text().splitlines(), (tmp_path / "den" / "mrstft.tsv").read_text().splitlines()
    assert len(plain) == len(den) == 3 and [r.split("\t")[:2] for r in plain] == [r.split("\t")[:2] for r in den]
    for p, q in zip(plain, den):
        vp, vq = [float(v) for v in p.split("\t")[2:]], [float(v) for v in q.split("\t")[2:]]
        assert all(np.isfinite(vp)) and all(np.isfinite(vq)) and vp != vq
