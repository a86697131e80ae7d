"""The command-line side of the waveform MCD: `bin/score.py --mcd_wave` and `bin/vocoder_score.py --mcd`.  Parsing and the column and row
plumbing run on the host, against the lines both tools wrote before the flags existed; one GPU case (-m gpu) scores the Griffin-Lim
copy-synthesis of two tiny wav files that the test writes, with and without the flag."""
import numpy as np
import pytest

from efficient_tts_amd.bin import score as C
from efficient_tts_amd.bin import vocoder_score as V

VBASE = ["--test_fid_scp", "t.txt", "--outdir", "o", "--vocoder", "griffinlim"]
CBASE = ["--checkpoint", "c.pkl", "--test_fid_scp", "t.txt", "--outdir", "o"]
NAN = float("nan")


def test_both_flags_are_off_by_default_and_change_no_other_argument():
    for mod, base, flag, key in ((V, VBASE, "--mcd", "mcd"), (C, CBASE, "--mcd_wave", "mcd_wave")):
        plain, flagged = mod.get_parser().parse_args(base), mod.get_parser().parse_args(base + [flag])
        assert getattr(plain, key) is False and getattr(flagged, key) is True
        assert {k: v for k, v in vars(plain).items() if k != key} == {k: v for k, v in vars(flagged).items() if k != key}
        with pytest.raises(SystemExit):                                # a switch: it takes no value
            mod.get_parser().parse_args(base + [flag + "=1"])
        assert flag in mod.__doc__
    V.check_args(V.get_parser().parse_args(VBASE + ["--mcd", "--stoi", "--denoise", "0.01"]))


def test_mcd_wave_needs_the_vocoder_switches_as_f0_does():
    for extra in ([], ["--vocoder", "hifigan"], ["--vocoder_checkpoint", "g.pt"]):
        with pytest.raises(ValueError, match="--mcd_wave needs audio of the synthesis"):
            C.run_score(C.get_parser().parse_args(CBASE + ["--mcd_wave"] + extra))         # before the device, the checkpoint or the list is touched
    with pytest.raises(ValueError, match="--f0 needs audio of the synthesis"):             # with both, the older flag still names itself
        C.run_score(C.get_parser().parse_args(CBASE + ["--f0", "--mcd_wave"]))
    a = C.get_parser().parse_args(CBASE + ["--mcd_wave", "--vocoder", "griffinlim"])
    C.check_f0_args(a)
    C.check_f0_args(a, {})
    C.check_f0_args(C.get_parser().parse_args(CBASE + ["--mcd_wave", "--vocoder", "griffinlim", "--f0_min", "20"]), {})      # no pitch search: its range is not checked
    with pytest.raises(ValueError, match="22050 Hz audio of 256 samples per frame"):
        C.check_f0_args(a, dict(sampling_rate=16000))
    C.check_f0_args(C.get_parser().parse_args(CBASE), dict(sampling_rate=16000))           # without either flag nothing is asked of the recipe


def test_score_lines_without_the_flag_are_what_they_were_and_with_it_gain_two_columns():
    rows = [("a", 5.123456789, 120, 118, 131), ("b", NAN, 0, 90, 0), ("c", 7.5, 80, 85, 90)]
    extra = [(35.25, 0.125, 60), (NAN, NAN, 0), (1200.0, 0.5, 7)]
    cuts = [(100, 20000), (0, 15000), (256, 18000)]
    # the lines as bin/score.py wrote them before --mcd_wave existed
    assert C.format_lines(rows) == ["a\t5.123457\t120\t118\t131", "b\tnan\t0\t90\t0", "c\t7.500000\t80\t85\t90", "mean\t6.311728"]
    assert C.format_lines(rows, extra) == ["a\t5.123457\t120\t118\t131\t35.2500\t0.125000\t60", "b\tnan\t0\t90\t0\tnan\tnan\t0",
                                           "c\t7.500000\t80\t85\t90\t1200.0000\t0.500000\t7", "mean\t6.311728\t617.6250\t0.312500\t22.3"]
    assert C.format_lines(rows, None, cuts) == ["a\t5.123457\t120\t118\t131\t100\t20000", "b\tnan\t0\t90\t0\t0\t15000", "c\t7.500000\t80\t85\t90\t256\t18000",
                                                "mean\t6.311728\t-\t-"]
    assert C.format_lines(rows, extra, cuts)[-1] == "mean\t6.311728\t617.6250\t0.312500\t22.3\t-\t-"
    assert C.format_lines([]) == ["mean\tnan"]
    wave = [(6.25, 140), (NAN, 0), (8.75, 97)]
    for other in ((None, None), (extra, None), (None, cuts), (extra, cuts)):
        before, after = C.format_lines(rows, *other), C.format_lines(rows, *other, wave=wave)
        assert [line[:len(b)] for line, b in zip(after, before)] == before                 # the columns in front are untouched
        assert [line[len(b):] for line, b in zip(after, before)] == ["\t6.250000\t140", "\tnan\t0", "\t8.750000\t97", "\t7.500000\t-"]
    assert C.format_lines(rows, wave=[(NAN, 0)] * 3)[-1].endswith("\tnan\t-")
    with pytest.raises(ValueError, match="one entry per row"):
        C.format_lines(rows, wave=wave[:2])


def test_vocoder_score_rows_without_the_flag_are_what_they_were_and_with_it_gain_two_columns():
    base = ["utt", "samples", "sc_1024_120_600", "log_mag_1024_120_600", "sc_2048_240_1200", "log_mag_2048_240_1200", "sc_512_50_240", "log_mag_512_50_240",
            "sc_mean", "log_mag_mean"]
    stoi_cols = ["stoi", "estoi", "stoi_kept_frames"]
    assert V.columns() == V.columns(mcd=False) == base and V.columns(stoi=True) == base + stoi_cols
    assert V.columns(mcd=True) == base + ["mcd_db", "mcd_frames"] and V.columns(stoi=True, mcd=True) == base + stoi_cols + ["mcd_db", "mcd_frames"]
    rows = [("a", 5000, [0.1, 0.2, 0.3], [1.0, 2.0, 3.0]), ("b", 900, [0.3, NAN, 0.5], [2.0, NAN, 4.0])]
    # the lines as bin/vocoder_score.py wrote them before --mcd existed
    plain = V.format_rows(rows)
    assert plain[0][0] == "a\t5000\t0.100000\t1.000000\t0.200000\t2.000000\t0.300000\t3.000000\t0.200000\t2.000000"
    assert plain[0][1] == "b\t900\t0.300000\t2.000000\tnan\tnan\t0.500000\t4.000000\tnan\tnan"
    assert plain[0][2] == "mean\t-\t0.200000\t1.500000\t0.200000\t2.000000\t0.400000\t3.500000\t0.200000\t2.000000"
    assert V.format_rows(rows, mcd=None) == plain and V.format_rows(rows, stoi=None, mcd=None) == plain
    stoi = [(0.75, 0.5, 31), (NAN, NAN, 3)]
    with_stoi = V.format_rows(rows, stoi=stoi)
    assert [line[len(b):] for line, b in zip(with_stoi[0], plain[0])] == ["\t0.750000\t0.500000\t31", "\tnan\tnan\t3", "\t0.750000\t0.500000\t-"]
    mcd = [(4.5, 20), (NAN, 0)]
    for before, kw in ((plain, {}), (with_stoi, dict(stoi=stoi))):
        after = V.format_rows(rows, mcd=mcd, **kw)
        assert after[1:-1] == before[1:] and after[-1] == 4.5           # the earlier means, then the new one
        assert [line[:len(b)] for line, b in zip(after[0], before[0])] == before[0]
        assert [line[len(b):] for line, b in zip(after[0], before[0])] == ["\t4.500000\t20", "\tnan\t0", "\t4.500000\t-"]
        assert all(len(line.split("\t")) == len(V.columns(stoi=bool(kw), mcd=True)) for line in after[0])
    assert V.format_rows(rows, mcd=[(NAN, 0)] * 2)[0][-1].endswith("\tnan\t-") and np.isnan(V.format_rows(rows, mcd=[(NAN, 0)] * 2)[-1])
    with pytest.raises(ValueError, match="one"):
        V.format_rows(rows, mcd=mcd[:1])
    with pytest.raises(ValueError, match="vocoder_checkpoint"):        # the flag changes no refusal
        V.run_score(V.get_parser().parse_args(["--test_fid_scp", "t.txt", "--outdir", "o", "--mcd"]))


@pytest.mark.gpu
def test_vocoder_score_with_the_flag_appends_the_distortion_and_without_it_writes_what_it_wrote(tmp_path, capsys):
    from scipy.io.wavfile import write
    rng = np.random.default_rng(3)
    (tmp_path / "wavs").mkdir()
    n = 11025                                                          # half a second: 44 frames
    t = np.arange(n) / 22050.0
    for k, f0 in (("a", 150.0), ("b", 210.0)):
        voice = sum(np.sin(2 * np.pi * h * f0 * t + h) / h for h in range(1, 16))
        x = 0.15 * voice * (0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t)) + 0.002 * rng.standard_normal(n)
        write(str(tmp_path / "wavs" / f"{k}.wav"), 22050, (x * 32767.0).round().astype(np.int16))
    (tmp_path / "list.txt").write_text("DUMMY/a.wav|x\nDUMMY/b.wav|y\n")
    base = ["--test_fid_scp", str(tmp_path / "list.txt"), "--wav_path", str(tmp_path / "wavs"), "--vocoder", "griffinlim", "--gl_iters", "4"]
    assert V.run_score(V.get_parser().parse_args(base + ["--outdir", str(tmp_path / "plain")])) is not None
    assert "MCD" not in capsys.readouterr().out
    V.run_score(V.get_parser().parse_args(base + ["--outdir", str(tmp_path / "mcd"), "--mcd"]))
    printed = capsys.readouterr().out
    plain, scored = (tmp_path / "plain" / "mrstft.tsv").read_text().splitlines(), (tmp_path / "mcd" / "mrstft.tsv").read_text().splitlines()
    assert len(plain) == len(scored) == 3
    assert all(len(r.split("\t")) == len(V.columns()) for r in plain)  # no such columns without the flag
    assert all(len(r.split("\t")) == len(V.columns(mcd=True)) for r in scored)
    assert ["\t".join(r.split("\t")[:len(V.columns())]) for r in scored] == plain              # the columns in front are what they were
    for r in scored[:2]:
        m, frames = r.split("\t")[-2:]
        assert 0.0 < float(m) < 30.0 and int(frames) == 1 + int(r.split("\t")[1]) // 256
    m_mean, dash = scored[2].split("\t")[-2:]
    assert dash == "-" and float(m_mean) == pytest.approx(np.mean([float(r.split("\t")[-2]) for r in scored[:2]]), abs=2e-6)
    assert "mean MCD" in printed


@pytest.mark.gpu
def test_score_cli_with_the_flag_appends_the_waveform_mcd_and_without_it_writes_what_it_wrote(tmp_path, capsys):
    from test_score_f0_cli import _experiment                          # a tiny model with random weights and three recordings
    common, _, _, _ = _experiment(tmp_path)
    assert C.main(common + ["--outdir", str(tmp_path / "plain")]) == 0
    plain_log = capsys.readouterr().out
    assert C.main(common + ["--outdir", str(tmp_path / "wave"), "--mcd_wave", "--vocoder", "griffinlim", "--gl_iters", "4", "--trim_silence"]) == 0
    wave_log = capsys.readouterr().out
    assert C.main(common + ["--outdir", str(tmp_path / "trim"), "--trim_silence"]) == 0
    capsys.readouterr()
    plain = [line.split("\t") for line in (tmp_path / "plain" / "mcd.tsv").read_text().splitlines()]
    trim = [line.split("\t") for line in (tmp_path / "trim" / "mcd.tsv").read_text().splitlines()]
    wave = [line.split("\t") for line in (tmp_path / "wave" / "mcd.tsv").read_text().splitlines()]
    assert [len(r) for r in plain] == [5, 5, 5, 2] and [len(r) for r in trim] == [7, 7, 7, 4] and [len(r) for r in wave] == [9, 9, 9, 6]
    assert [r[:len(o)] for r, o in zip(wave, trim)] == trim            # the columns in front are what they are without the flag
    for r in wave[:3]:
        m, n = float(r[-2]), int(r[-1])
        assert (np.isnan(m) and n == 0) or (0.0 < m < 60.0 and n >= max(int(r[2]), 1 + int(r[6]) // 256))      # a path is at least as long as either side
    assert wave[3][-1] == "-" and float(wave[3][-2]) == pytest.approx(np.nanmean([float(r[-2]) for r in wave[:3]]), abs=2e-6)
    assert "waveform MCD" in wave_log and "waveform MCD" not in plain_log
