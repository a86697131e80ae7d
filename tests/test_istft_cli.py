"""GPU (-m gpu): the command-line side of the iSTFTNet head -- `bin/inference.py --vocoder hifigan --vocoder_config ... --vocoder_checkpoint ...`
with a small C8C8I-shaped config (rates 8 x 8 under an N = 16, h = 4 head: 256 samples per frame) and a random-weight checkpoint with the
HiFi-GAN key set, both written by the test, in the three precisions.
"""
import json

import numpy as np
import pytest
import torch
import yaml

import istft_reference as IR

pytestmark = pytest.mark.gpu

C8C8I_SMALL = dict(resblock="1", upsample_rates=[8, 8], upsample_kernel_sizes=[16, 16], upsample_initial_channel=32, resblock_kernel_sizes=[3, 7],
                   resblock_dilation_sizes=[[1, 3], [1, 3]], num_mels=80, gen_istft_n_fft=16, gen_istft_hop_size=4)


def test_inference_cli_synthesises_through_a_c8c8i_config(tmp_path, monkeypatch):
    from scipy.io.wavfile import read
    from efficient_tts_amd import EfficientTTSCNN
    from efficient_tts_amd.bin import inference as I
    exp = tmp_path / "exp"
    exp.mkdir()
    phones = ["_"] + [f"P{i}" for i in range(1, 76)]
    (tmp_path / "phn.txt").write_text("\n".join(phones) + "\n")
    rng = np.random.default_rng(3)
    lines = [f"DUMMY/utt{n}.wav|" + " ".join(phones[int(i)] for i in rng.integers(1, 76, size=k)) for n, k in enumerate((12, 9))]
    (tmp_path / "test.txt").write_text("\n".join(lines) + "\n")
    params = dict(num_symbols=76, dropout_rate=0.0, use_masking=True, use_weighted_masking=False, sigma=0.01)
    with open(exp / "config.yml", "w") as f:
        yaml.dump(dict(model_name="EfficientTTSCNN", model_params=params, dataset_params=dict(use_phnseq=True, phnset_path=str(tmp_path / "phn.txt"))), f)
    torch.manual_seed(0)
    m = EfficientTTSCNN(**params)
    with torch.no_grad():
        m.duration_predictor.linear.bias.fill_(1.5)                  # a few frames per phoneme with random weights
    torch.save({"model": m.state_dict(), "steps": 7}, exp / "checkpoint-7steps.pkl")
    (tmp_path / "c8c8i.json").write_text(json.dumps(C8C8I_SMALL))
    torch.save({"generator": IR.fill(C8C8I_SMALL, 41)}, tmp_path / "g.pt")
    base = ["--checkpoint", str(exp / "checkpoint-7steps.pkl"), "--test_fid_scp", str(tmp_path / "test.txt"), "--verbose", "0", "--vocoder", "hifigan",
            "--vocoder_config", str(tmp_path / "c8c8i.json"), "--vocoder_checkpoint", str(tmp_path / "g.pt")]

    built, frames = [], []
    real = I.build_vocoder

    def build_vocoder(args, device):
        gen = real(args, device)
        built.append(gen)

        def vocoder(mel, lens=None):
            frames.append([mel.shape[2]] if lens is None else [int(v) for v in lens])
            return gen(mel) if lens is None else gen(mel, lens)
        return vocoder
    monkeypatch.setattr(I, "build_vocoder", build_vocoder)

    for precision, extra in (("bf16x3", []), ("fp32", ["--batch_size", "2"]), ("bf16", [])):
        frames.clear()
        out = tmp_path / precision
        assert I.main(base + ["--outdir", str(out), "--precision", precision] + extra) == 0
        gen = built[-1]
        assert gen.precision == precision and gen.hop == 256 and gen.conv_post.out_channels == 18
        counts = [n for call in frames for n in call]
        assert len(counts) == 2 and min(counts) > 0
        for n, k in enumerate(counts):
            sr, wav = read(str(out / f"utt{n}_7steps.wav"))
            assert sr == 22050 and wav.shape == (k * 256,)             # frames * hop samples on the 22050 Hz grid of 256-sample frames
            assert int(np.abs(wav).max()) > 0
