"""The command-line side of pitch scoring: `efficient_tts_amd.bin.score --f0` and `efficient_tts_amd.bin.inference --write_f0`.  Without a
GPU: the parsers and the refusal of `--f0` without a usable vocoder.  On the GPU (-m gpu): a tiny model with random weights, a three-line
list and Griffin-Lim at 4 iterations."""
import numpy as np
import pytest
import torch
import yaml

BASE = ["--checkpoint", "c.pkl", "--test_fid_scp", "t.txt", "--outdir", "o"]


def test_parsers_accept_the_new_flags():
    from efficient_tts_amd.bin import inference as I
    from efficient_tts_amd.bin import score as C
    a = C.get_parser().parse_args(BASE)
    assert (a.f0, a.vocoder, a.vocoder_config, a.vocoder_checkpoint, a.gl_iters, a.f0_min, a.f0_max, a.f0_threshold) == \
        (False, "hifigan", None, None, 32, 60.0, 600.0, 0.15)
    a = C.get_parser().parse_args(BASE + ["--f0", "--vocoder", "griffinlim", "--gl_iters", "4", "--f0_min", "80", "--f0_max", "400", "--f0_threshold", "0.2"])
    assert (a.f0, a.vocoder, a.gl_iters, a.f0_min, a.f0_max, a.f0_threshold) == (True, "griffinlim", 4, 80.0, 400.0, 0.2)
    a = C.get_parser().parse_args(BASE + ["--f0", "--vocoder", "hifigan", "--vocoder_config", "c.json", "--vocoder_checkpoint", "g.pt"])
    C.check_f0_args(a)
    assert C.build_vocoder is I.build_vocoder                   # the construction is shared, not copied
    assert I.get_parser().parse_args(BASE).write_f0 is False and I.get_parser().parse_args(BASE + ["--write_f0"]).write_f0 is True


def test_f0_without_a_usable_vocoder_is_refused():
    from efficient_tts_amd.bin import score as C
    for extra in ([], ["--vocoder", "hifigan"], ["--vocoder_checkpoint", "g.pt"]):
        with pytest.raises(ValueError, match="--f0 needs audio of the synthesis"):
            C.run_score(C.get_parser().parse_args(BASE + ["--f0"] + extra))            # before the device, the checkpoint or the list is touched
    a = C.get_parser().parse_args(BASE + ["--f0", "--vocoder", "griffinlim"])
    C.check_f0_args(a, {})
    with pytest.raises(ValueError, match="22050 Hz audio of 256 samples per frame"):
        C.check_f0_args(a, dict(sampling_rate=16000))
    with pytest.raises(ValueError):
        C.check_f0_args(C.get_parser().parse_args(BASE + ["--f0", "--vocoder", "griffinlim", "--f0_min", "20"]), {})


def _experiment(tmp_path):
    from scipy.io.wavfile import write
    from efficient_tts_amd import EfficientTTSCNN
    exp = tmp_path / "exp"
    exp.mkdir()
    phones = ["_"] + [f"P{i}" for i in range(1, 76)]
    (tmp_path / "phn.txt").write_text("\n".join(phones) + "\n")
    rng = np.random.default_rng(2)
    ids = [rng.integers(1, 76, size=k) for k in (9, 14, 6)]
    t = [np.arange(n) / 22050.0 for n in (9000, 12345, 7001)]
    pcm = [(9000.0 * np.sin(2 * np.pi * f * tt) + 4000.0 * np.sin(4 * np.pi * f * tt) + 300.0 * rng.standard_normal(tt.shape[0])).astype(np.int16)
           for f, tt in zip((140.0, 210.0, 175.0), t)]
    lines = []
    for n in range(3):
        write(str(tmp_path / f"utt{n}.wav"), 22050, pcm[n])
        lines.append(f"{tmp_path}/utt{n}.wav|" + " ".join(phones[int(i)] for i in ids[n]))
    (tmp_path / "test.txt").write_text("\n".join(lines) + "\n")
    params = dict(num_symbols=76, n_channels=256, symbol_embedding_dim=256, n_text_encoder_layer=1, n_mel_encoder_layer=1, n_decoder_layer=1,
                  dropout_rate=0.0, use_masking=True, use_weighted_masking=False, sigma=0.01)
    torch.manual_seed(0)
    m = EfficientTTSCNN(**params)
    with torch.no_grad():
        m.duration_predictor.linear.bias.fill_(1.5)              # a few frames per phoneme with random weights
    with open(exp / "config.yml", "w") as f:
        yaml.dump(dict(model_name="EfficientTTSCNN", model_params=params, dataset_params=dict(use_phnseq=True, phnset_path=str(tmp_path / "phn.txt"))), f)
    torch.save({"model": m.state_dict(), "steps": 7}, exp / "checkpoint-7steps.pkl")
    common = ["--checkpoint", str(exp / "checkpoint-7steps.pkl"), "--test_fid_scp", str(tmp_path / "test.txt")]
    return common, m, ids, pcm


@pytest.mark.gpu
def test_score_cli_with_and_without_f0(tmp_path, capsys):
    from efficient_tts_amd.bin.score import main
    from efficient_tts_amd.frontend import LogMelFrontend
    from efficient_tts_amd.score import MelCepstralDistortion
    common, m, ids, pcm = _experiment(tmp_path)
    dev = torch.device("cuda:0")
    assert main(common + ["--outdir", str(tmp_path / "plain")]) == 0
    plain_log = capsys.readouterr().out
    assert main(common + ["--outdir", str(tmp_path / "f0"), "--f0", "--vocoder", "griffinlim", "--gl_iters", "4"]) == 0
    f0_log = capsys.readouterr().out
    # without --f0: the bytes of the unchanged path -- the front-end, the free-running pass and the default scorer call, formatted as before
    model = m.to(dev).eval()
    model.remove_weight_norm()
    audio = torch.nn.utils.rnn.pad_sequence([torch.from_numpy(p) for p in pcm], batch_first=True)
    text = torch.nn.utils.rnn.pad_sequence([torch.from_numpy(i) for i in ids], batch_first=True)
    with torch.no_grad():
        rec, rec_len = LogMelFrontend(dev)(audio, torch.tensor([p.shape[0] for p in pcm]))
        syn, syn_len = model.inference_batch(text.to(dev), torch.tensor([len(i) for i in ids], device=dev), length_scale=1.0)[:2]
        out = MelCepstralDistortion(dev)(syn, syn_len, rec, rec_len)
    mcd = out["mcd"].tolist()
    expected = "".join(f"utt{n}\t{mcd[n]:.6f}\t{int(syn_len[n])}\t{int(rec_len[n])}\t{int(out['path_len'][n])}\n" for n in range(3))
    expected += f"mean\t{float(np.mean(mcd)):.6f}\n"
    assert (tmp_path / "plain" / "mcd.tsv").read_bytes() == expected.encode()
    assert plain_log == f"mean MCD over 3 of 3 utterances: {float(np.mean(mcd)):.4f} dB\n"
    # with --f0: the old columns unchanged, three more behind them
    old = [line.split("\t") for line in expected.splitlines()]
    new = [line.split("\t") for line in (tmp_path / "f0" / "mcd.tsv").read_text().splitlines()]
    assert [len(r) for r in new] == [8, 8, 8, 5] and [r[:len(o)] for r, o in zip(new, old)] == old
    for r in new[:3]:
        rmse, vuv, pairs = float(r[5]), float(r[6]), int(r[7])
        assert 0.0 <= vuv <= 1.0 and 0 <= pairs <= int(r[4])
        assert (np.isnan(rmse) and pairs == 0) or (np.isfinite(rmse) and rmse >= 0.0 and pairs > 0)
    assert f0_log.startswith(plain_log) and "mean F0 error" in f0_log and "voiced/unvoiced error" in f0_log


@pytest.mark.gpu
def test_inference_cli_writes_one_f0_line_per_frame(tmp_path):
    from scipy.io.wavfile import read
    from efficient_tts_amd.bin.inference import main
    common, _, _, _ = _experiment(tmp_path)
    out = tmp_path / "wav"
    assert main(common + ["--outdir", str(out), "--vocoder", "griffinlim", "--gl_iters", "4", "--batch_size", "2", "--write_f0", "--verbose", "0"]) == 0
    for n in range(3):                                           # a batch of two, then a single utterance: both paths of the script
        sr, wav = read(str(out / f"utt{n}_7steps.wav"))
        rows = [line.split("\t") for line in (out / f"utt{n}_7steps.f0.txt").read_text().splitlines()]
        assert sr == 22050 and len(rows) == wav.shape[0] // 256 > 0
        assert [int(r[0]) for r in rows] == list(range(len(rows)))
        assert all(float(r[1]) == pytest.approx(t * 256 / 22050, abs=1e-6) and (float(r[2]) == 0.0 or 60.0 <= float(r[2]) <= 631.0) for t, r in enumerate(rows))
    assert main(common + ["--outdir", str(tmp_path / "nof0"), "--vocoder", "griffinlim", "--gl_iters", "4", "--verbose", "0"]) == 0
    assert not list((tmp_path / "nof0").glob("*.f0.txt"))
