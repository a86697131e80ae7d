"""`python -m efficient_tts_amd.bin.vocoder_score` -- multi-resolution STFT distance of a vocoder's copy-synthesis against the recordings.

    python -m efficient_tts_amd.bin.vocoder_score --test_fid_scp test.txt --outdir exp/vocoder/score \\
        --vocoder griffinlim|hifigan [--vocoder_config c.json --vocoder_checkpoint g.pt] [--gl_iters 32] [--precision bf16x3]
        [--batch_size 16] [--wav_path wavs/] [--denoise 0.01] [--stoi] [--mcd]

Copy-synthesis: recording -> log-mel (`LogMelFrontend`) -> vocoder (the `--vocoder` switches of `efficient_tts_amd.bin.inference`) -> audio,
compared with the recording over min(len) samples by `MultiResolutionSTFTDistance` at the reference's three resolutions.  No acoustic
checkpoint is involved.  Reads the `wav_path|...` list of `efficient_tts_amd.bin.inference` (only the path is used; 16-bit wav files at
22 050 Hz; a path that does not exist is looked up by its file name under --wav_path).  Writes outdir/mrstft.tsv -- utterance id, samples
compared, then sc and log_mag per resolution, then their means over the resolutions; the last line holds the means over the utterances that
have a value -- and prints those means.  An utterance too short for a resolution has nan there and in its own means.

sc is the spectral convergence ||mag_rec - mag_syn||_F / ||mag_rec||_F, log_mag the mean |ln mag_rec - ln mag_syn|; both are 0 for a perfect
copy.  The numbers judge `--precision`, `--gl_iters` and vocoder checkpoints against each other on the same recordings.

`--denoise S` (S > 0) passes the copy-synthesis through `efficient_tts_amd.denoise.BiasDenoiser` before it is scored, the bias measured once from
the vocoder's answer to a blank mel: the table then says whether a strength helps or eats the signal.

`--stoi` also scores every utterance's intelligibility with `efficient_tts_amd.stoi.ShortTimeIntelligibility` on the same (synthesis, recording,
samples) -- behind the denoiser where `--denoise` is given --, the recording as the clean signal: every line of mrstft.tsv gains the columns stoi,
estoi and stoi_kept_frames (the frames at 10 kHz left after silent-frame removal), the last line the means of the first two (and `-`), and
the two means are printed.  The spectral distances do not say whether the speech stays intelligible; these two do (1 for a perfect copy, nan
for an utterance with at most 30 kept frames).  Without the flag the file is byte for byte what it was.

`--mcd` also scores the mel-cepstral distortion that vocoder papers report, `efficient_tts_amd.mcep.WaveformMCD` in aligned mode (copy-synthesis
shares the recording's time axis: frame t against frame t, no warping) on the same (synthesis, recording, samples), behind the denoiser where
`--denoise` is given: order-24 all-pass-warped mel-cepstra of both waveforms by the periodogram route, every frame counted (no silence gating).
Every line gains the columns mcd_db and mcd_frames -- behind the `--stoi` columns when both are given --, the last line the mean of the first
(and `-`), and the mean is printed.  Without the flag the file is byte for byte what it was.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

from efficient_tts_amd.stft import DEFAULT_RESOLUTIONS

SAMPLING_RATE = 22050


def get_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="efficient_tts_amd.bin.vocoder_score", description=__doc__.splitlines()[0])
    p.add_argument("--test_fid_scp", type=str, required=True, help="utterance list: wav_path, optionally followed by |anything")
    p.add_argument("--outdir", type=str, required=True, help="where mrstft.tsv goes")
    p.add_argument("--vocoder", type=str, default="hifigan", choices=["hifigan", "griffinlim"], help="what turns the recordings' log-mels back into audio")
    p.add_argument("--vocoder_config", type=str, default=None, help="HiFi-GAN config.json (or an iSTFTNet one such as C8C8I: gen_istft_n_fft 16, gen_istft_hop_size 4 under upsample_rates [8, 8])")
    p.add_argument("--vocoder_checkpoint", type=str, default=None, help='HiFi-GAN checkpoint with a "generator" state_dict')
    p.add_argument("--gl_iters", type=int, default=32, help="Griffin-Lim iterations (--vocoder griffinlim; default 32)")
    p.add_argument("--precision", type=str, default="bf16x3", choices=["bf16x3", "bf16", "fp32"], help="MFMA operand mode of the vocoder")
    p.add_argument("--batch_size", type=int, default=16, help="utterances per call (default 16; every item is scored as if alone)")
    p.add_argument("--wav_path", type=str, default=None, help="directory searched, by file name, for a wav path that does not exist")
    p.add_argument("--denoise", type=float, default=None,
                   help="denoise the copy-synthesis before scoring: subtract this many times the vocoder's bias spectrum, for example 0.01 (default: off)")
    p.add_argument("--highpass_hz", type=float, default=None,
                   help="run a Butterworth high-pass at this cutoff over every recording before anything else, as `highpass_hz` in a recipe does")
    p.add_argument("--highpass_order", type=int, default=None, help="--highpass_hz: 2 (default) or 4")
    p.add_argument("--stoi", action="store_true", help="also score STOI and ESTOI of the copy-synthesis against the recording (columns stoi, estoi, stoi_kept_frames)")
    p.add_argument("--mcd", action="store_true", help="also score the mel-cepstral distortion of the copy-synthesis against the recording, frame by frame (columns mcd_db, mcd_frames)")
    return p


def check_args(args) -> None:
    """a generator with random weights has nothing to score: refused on the host, before anything is loaded"""
    if args.vocoder == "hifigan" and not (args.vocoder_checkpoint and args.vocoder_config):
        raise ValueError("--vocoder hifigan needs --vocoder_checkpoint and --vocoder_config (a generator with random weights has no copy-synthesis "
                         "to score); --vocoder griffinlim needs no weights")
    if args.batch_size < 1:
        raise ValueError("--batch_size must be >= 1")
    if args.denoise is not None and not (args.denoise > 0 and np.isfinite(args.denoise)):
        raise ValueError("--denoise must be a finite strength > 0 (leave the flag out for no denoiser)")
    build_highpass(args)


def build_highpass(args, max_wav_value: float = 32768.0, device=None):
    """the IIRFilter for the recordings, or None without --highpass_hz (checked on the host)"""
    from efficient_tts_amd.iir import build_chain
    return build_chain(device, SAMPLING_RATE, getattr(args, "highpass_hz", None), getattr(args, "highpass_order", None), max_wav_value=max_wav_value)


STOI_COLUMNS = ("stoi", "estoi", "stoi_kept_frames")
MCD_COLUMNS = ("mcd_db", "mcd_frames")


def _mean_of_finite(col) -> float:
    col = np.asarray(col, dtype=np.float64)
    return float(np.mean(col[np.isfinite(col)])) if np.isfinite(col).any() else float("nan")


def columns(resolutions=DEFAULT_RESOLUTIONS, stoi: bool = False, mcd: bool = False):
    """the columns of mrstft.tsv; `stoi`: with the three columns of --stoi behind them; `mcd`: with the two columns of --mcd behind those"""
    names = ["utt", "samples"]
    for n, h, w in resolutions:
        names += [f"sc_{n}_{h}_{w}", f"log_mag_{n}_{h}_{w}"]
    return names + ["sc_mean", "log_mag_mean"] + (list(STOI_COLUMNS) if stoi else []) + (list(MCD_COLUMNS) if mcd else [])


def format_rows(rows, resolutions=DEFAULT_RESOLUTIONS, stoi=None, mcd=None):
    """the lines of mrstft.tsv from (utt, samples, sc [R], log_mag [R]) per utterance, and the two means that the last line ends with.
    `stoi`: (stoi, estoi, kept frames) per utterance, in the rows' order: three more columns on every line (the last line: the means of the
    first two over the utterances that have a value, and `-`); the return value then ends with those two means.
    `mcd`: (mcd in dB, frames compared) per utterance: two more columns behind everything else (the last line: the mean of the first over
    the utterances that have a value, and `-`); the return value then ends with that mean."""
    if mcd is not None:
        if len(mcd) != len(rows):
            raise ValueError("mcd must hold one (mcd in dB, frames) per row")
        lines, *means = format_rows(rows, resolutions, stoi)
        for i, (m, frames) in enumerate(mcd):
            lines[i] += f"\t{float(m):.6f}\t{int(frames)}"
        m_mean = _mean_of_finite([v[0] for v in mcd])
        lines[-1] += f"\t{m_mean:.6f}\t-"
        return (lines, *means, m_mean)
    if stoi is not None:
        if len(stoi) != len(rows):
            raise ValueError("stoi must hold one (stoi, estoi, kept frames) per row")
        lines, sc_mean, lm_mean = format_rows(rows, resolutions)
        for i, (s, e, kept) in enumerate(stoi):
            lines[i] += "\t" + "\t".join([f"{float(s):.6f}", f"{float(e):.6f}", str(int(kept))])
        s_mean, e_mean = _mean_of_finite([v[0] for v in stoi]), _mean_of_finite([v[1] for v in stoi])
        lines[-1] += "\t" + "\t".join([f"{s_mean:.6f}", f"{e_mean:.6f}", "-"])
        return lines, sc_mean, lm_mean, s_mean, e_mean
    lines, table = [], []
    for utt, n, sc, lm in rows:
        vals = [v for pair in zip(sc, lm) for v in pair] + [float(np.mean(sc)), float(np.mean(lm))]       # (nan in a resolution: nan in the mean)
        table.append(vals)
        lines.append("\t".join([utt, str(int(n))] + [f"{v:.6f}" for v in vals]))
    table = np.asarray(table, dtype=np.float64).reshape(len(rows), 2 * len(resolutions) + 2)
    means = [float(np.mean(col[np.isfinite(col)])) if np.isfinite(col).any() else float("nan") for col in table.T]
    lines.append("\t".join(["mean", "-"] + [f"{v:.6f}" for v in means]))
    return lines, means[-2], means[-1]


def _read_paths(path: str):
    items = []
    with open(path) as handle:
        for line in handle:
            line = line.strip()
            if line:
                wav = line.split("|")[0]
                items.append((os.path.splitext(os.path.basename(wav))[0], wav))
    return items


def run_score(args):
    check_args(args)
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: efficient_tts_amd has no CPU path")
    from efficient_tts_amd.bin.inference import build_vocoder
    from efficient_tts_amd.bin._io import read_wav
    from efficient_tts_amd.frontend import LogMelFrontend
    from efficient_tts_amd.stft import MultiResolutionSTFTDistance
    device = torch.device("cuda")
    os.makedirs(args.outdir, exist_ok=True)
    frontend = LogMelFrontend(device)
    vocoder = build_vocoder(args, device)
    denoiser = None
    if args.denoise is not None:
        from efficient_tts_amd.denoise import BiasDenoiser
        denoiser = BiasDenoiser.from_vocoder(vocoder, device, strength=args.denoise)
    highpass = build_highpass(args, frontend.max_wav_value, device)
    scorer = MultiResolutionSTFTDistance(device, max_wav_value=frontend.max_wav_value)
    intelligibility = None
    if args.stoi:
        from efficient_tts_amd.stoi import ShortTimeIntelligibility
        intelligibility = ShortTimeIntelligibility(device, SAMPLING_RATE, max_wav_value=frontend.max_wav_value)
    distortion = None
    if args.mcd:
        from efficient_tts_amd.mcep import WaveformMCD
        distortion = WaveformMCD(device, sampling_rate=SAMPLING_RATE, max_wav_value=frontend.max_wav_value)
    items = _read_paths(args.test_fid_scp)
    rows, stoi_rows, mcd_rows = [], [], []
    for lo in range(0, len(items), args.batch_size):
        chunk = items[lo:lo + args.batch_size]
        wavs = [read_wav(path, args.wav_path, SAMPLING_RATE)[0] for _, path in chunk]
        audio = torch.nn.utils.rnn.pad_sequence(wavs, batch_first=True).to(device)
        wav_len = torch.tensor([w.shape[0] for w in wavs], device=device)
        with torch.no_grad():
            if highpass is not None:                         # the recordings as a run with `highpass_hz` trains on them: fp32 from here on
                audio = highpass(audio, wav_len)
            mel, mel_len = frontend(audio, wav_len)
            syn = vocoder(mel.transpose(1, 2).contiguous(), mel_len)[:, 0].float()
            if denoiser is not None:
                syn = denoiser(syn, (mel_len.to(wav_len.dtype) * frontend.hop).clamp(max=syn.shape[1]))
            n = torch.minimum(wav_len, mel_len.to(wav_len.dtype) * frontend.hop).clamp(max=min(syn.shape[1], audio.shape[1]))
            out = scorer(syn, audio, n)
            if intelligibility is not None:                  # the recording is the clean signal, the copy-synthesis the processed one
                si = intelligibility(audio, syn, n)
                stoi_rows += list(zip(si["stoi"].tolist(), si["estoi"].tolist(), si["kept"].tolist()))
            if distortion is not None:                       # one time axis: frame t of the copy-synthesis against frame t of the recording
                md = distortion(syn, n, audio, n, aligned=True)
                mcd_rows += list(zip(md["mcd"].tolist(), md["count"].tolist()))
        for (utt, _), k, sc, lm in zip(chunk, n.tolist(), out["sc"].tolist(), out["log_mag"].tolist()):
            rows.append((utt, k, sc, lm))
    if intelligibility is None:
        lines, sc_mean, lm_mean, *more = format_rows(rows, mcd=mcd_rows if distortion is not None else None)
    else:
        lines, sc_mean, lm_mean, stoi_mean, estoi_mean, *more = format_rows(rows, stoi=stoi_rows, mcd=mcd_rows if distortion is not None else None)
    with open(os.path.join(args.outdir, "mrstft.tsv"), "w") as handle:
        handle.write("\n".join(lines) + "\n")
    print(f"copy-synthesis of {len(rows)} utterances with {args.vocoder}: mean spectral convergence {sc_mean:.4f}, mean log-magnitude distance {lm_mean:.4f}")
    if intelligibility is not None:
        print(f"intelligibility of the copy-synthesis against the recordings: mean STOI {stoi_mean:.4f}, mean ESTOI {estoi_mean:.4f}")
    if distortion is not None:
        print(f"mel-cepstral distortion of the copy-synthesis against the recordings (order-24 mel-cepstra, frame by frame): mean MCD {more[0]:.4f} dB")
    return sc_mean, lm_mean


def main(argv=None) -> int:
    run_score(get_parser().parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
