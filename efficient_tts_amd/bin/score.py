"""`python -m efficient_tts_amd.bin.score` -- mel-cepstral distortion of a checkpoint's free-running synthesis against the recordings.

    python -m efficient_tts_amd.bin.score --checkpoint exp/efts/checkpoint-100000steps.pkl --test_fid_scp test.txt --outdir exp/efts/score \\
        [--config exp/efts/config.yml] [--batch_size 16] [--precision bf16x3] [--length_scale 1.0]
        [--f0 --vocoder griffinlim|hifigan [--vocoder_config c.json --vocoder_checkpoint g.pt] [--gl_iters 32] [--f0_min 60] [--f0_max 600] [--f0_threshold 0.15] [--f0_smooth]]
        [--trim_silence [--trim_top_db 40]] [--normalize_peak 0.95] [--max_pause_ms 300 [--pause_top_db 40]] [--mcd_wave] [--use_ema]

Reads the `wav_path|phonemes` list of `efficient_tts_amd.bin.inference` (16-bit wav files at the front-end's rate; a path that does not
exist is looked up by its file name under dataset_params.wav_path).  Per batch, on the device: the recordings' log-mels (`LogMelFrontend`
with the recipe's frontend_params), the free-running mels (`inference_batch`), and `MelCepstralDistortion` of synthesis against recording.
Writes outdir/mcd.tsv -- utterance id, MCD in dB, frames synthesised, frames recorded, length of the warping path; the last line is the
mean -- and prints the mean.  An utterance whose synthesis has no frames has no path: its line says nan and the mean leaves it out.

`--f0` adds the two pitch axes.  The synthesis is vocoded as `efficient_tts_amd.bin.inference` would (the same `--vocoder` switches), a YIN pitch
tracker (`efficient_tts_amd.pitch`) runs on the synthesis and on the recording, the MCD's own warping path is kept, and along it
`F0Error` gives the F0 error in cents over the cells voiced on both sides and the share of cells whose voicing differs.  mcd.tsv gets three more
columns behind its own -- f0_rmse_cents, vuv_error, voiced_pairs -- and the last line their means over the utterances that have a value.
`--f0_smooth` smooths both contours, synthesis and recording, across frames before the error is read (the tracker's Viterbi path over all lags
instead of YIN's frame-by-frame rule, whose octave errors of 1200 cents each otherwise dominate f0_rmse_cents).  Without `--f0` nothing changes.

`--trim_silence` and `--normalize_peak` treat the RECORDINGS as a training run with `trim_silence` / `normalize_peak` in its recipe treats them
(`efficient_tts_amd.trim.SilenceTrimmer` on the front-end's hop), before their log-mel and F0: the synthesis of a model trained on trimmed
recordings carries no silence at its ends, and the recordings it is scored against should not either.  mcd.tsv then ends every line with two
more columns, ref_trim_start and ref_trim_len (samples), and "-" in them on the line of the means.  Without the flags nothing changes.

`--max_pause_ms MS` (with `--pause_top_db`) cuts the pauses inside the RECORDINGS that are longer than MS down to it, as `max_pause_ms` in a
recipe does (`efficient_tts_amd.pauses.PauseShortener` at the front-end's rate and hop), behind `--trim_silence` and before their log-mel and F0.
It adds no column.  Without the flag nothing changes.

`--mcd_wave` adds the number that papers report: the synthesis is vocoded (the same `--vocoder` switches, required as for `--f0`) and
`efficient_tts_amd.mcep.WaveformMCD` scores it against the recording -- order-24 all-pass-warped mel-cepstra of the two waveforms along their own
warping path, behind `--trim_silence` / `--normalize_peak` where those are given; there is no per-frame silence gating.  Every line of mcd.tsv
ends with two more columns, mcd_wave_db and mcd_wave_path_len, the last line with the mean of the first (and `-`).  Without the flag nothing
changes.

`--use_ema` scores the averaged weights of the checkpoint (its "ema" entry: a run with `ema_decay` in its YAML writes one) instead of the
raw ones; a checkpoint without that entry is refused at start-up.  Without the flag nothing changes.

The numbers of the first column compare checkpoints of this project with each other (natural-log mels of this front-end); they are not
comparable to MCDs computed from SPTK cepstra of waveforms.  The `--mcd_wave` column is the literature's definition by the periodogram route.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

from efficient_tts_amd.bin._io import read_wav
from efficient_tts_amd.bin.inference import SAMPLING_RATE, USE_EMA_HELP, _read_list, build_vocoder, load_acoustic_model
from efficient_tts_amd.frontend import LogMelFrontend
from efficient_tts_amd.iir import build_chain
from efficient_tts_amd.pitch import PitchTracker, lag_range
from efficient_tts_amd.mcep import WaveformMCD
from efficient_tts_amd.pauses import PauseShortener
from efficient_tts_amd.score import F0Error, MelCepstralDistortion
from efficient_tts_amd.trim import SilenceTrimmer


def get_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="efficient_tts_amd.bin.score", description=__doc__.splitlines()[0])
    p.add_argument("--checkpoint", type=str, required=True, help="acoustic-model checkpoint (checkpoint-*steps.pkl)")
    p.add_argument("--test_fid_scp", type=str, required=True, help="utterance list: wav_path|phoneme sequence")
    p.add_argument("--outdir", type=str, required=True, help="where mcd.tsv goes")
    p.add_argument("--config", type=str, default=None, help="training config.yml (default: next to the checkpoint)")
    p.add_argument("--batch_size", type=int, default=16, help="utterances per call (default 16; every item is scored as if alone)")
    p.add_argument("--precision", type=str, default="bf16x3", choices=["bf16x3", "bf16", "fp32"], help="MFMA operand mode of the acoustic model")
    p.add_argument("--length_scale", type=float, default=1.0, help="multiplies every predicted duration (default 1.0)")
    p.add_argument("--f0", action="store_true", help="also score pitch along the MCD's warping path: F0 error in cents and voiced/unvoiced error")
    p.add_argument("--vocoder", type=str, default="hifigan", choices=["hifigan", "griffinlim"],
                   help="--f0: what turns the synthesised mel into audio (as efficient_tts_amd.bin.inference); hifigan needs --vocoder_checkpoint")
    p.add_argument("--vocoder_config", type=str, default=None, help="--f0: HiFi-GAN config.json (or an iSTFTNet one such as C8C8I: gen_istft_n_fft 16, gen_istft_hop_size 4 under upsample_rates [8, 8])")
    p.add_argument("--vocoder_checkpoint", type=str, default=None, help='--f0: HiFi-GAN checkpoint with a "generator" state_dict')
    p.add_argument("--gl_iters", type=int, default=32, help="--f0: Griffin-Lim iterations (--vocoder griffinlim; default 32)")
    p.add_argument("--f0_min", type=float, default=60.0, help="--f0: lowest fundamental searched, Hz (default 60)")
    p.add_argument("--f0_max", type=float, default=600.0, help="--f0: highest fundamental searched, Hz (default 600)")
    p.add_argument("--f0_threshold", type=float, default=0.15, help="--f0: YIN threshold on the normalised difference function (default 0.15)")
    p.add_argument("--f0_smooth", action="store_true", help="--f0: smooth both contours across frames (the cheapest path over the lags of all frames)")
    p.add_argument("--trim_silence", action="store_true", help="cut the silence at both ends of every recording before it is scored against")
    p.add_argument("--trim_top_db", type=float, default=40.0, help="--trim_silence: a frame this far under the loudest one is silence (default 40)")
    p.add_argument("--normalize_peak", type=float, default=None, help="bring every recording to this peak, in (0, 1], before it is scored against")
    p.add_argument("--max_pause_ms", type=float, default=None,
                   help="cut every pause inside a recording that is longer than this down to it before it is scored against, as `max_pause_ms` in a recipe does")
    p.add_argument("--pause_top_db", type=float, default=40.0, help="--max_pause_ms: a frame this far under the loudest one is quiet (default 40)")
    p.add_argument("--highpass_hz", type=float, default=None,
                   help="run a Butterworth high-pass at this cutoff over every recording before it is scored against, as `highpass_hz` in a recipe does")
    p.add_argument("--highpass_order", type=int, default=None, help="--highpass_hz: 2 (default) or 4")
    p.add_argument("--mcd_wave", action="store_true",
                   help="also score mel-cepstral distortion between the vocoded synthesis and the recording (needs the --vocoder switches, as --f0 does)")
    p.add_argument("--use_ema", action="store_true", help=USE_EMA_HELP.replace("synthesise", "score"))
    return p


def build_trimmer(args, hop: int, max_wav_value: float, device=None):
    """the SilenceTrimmer for the recordings, or None without --trim_silence / --normalize_peak"""
    if not args.trim_silence and args.normalize_peak is None:
        return None
    return SilenceTrimmer(device, hop_size=hop, top_db=args.trim_top_db, peak=args.normalize_peak, max_wav_value=max_wav_value, trim=args.trim_silence)


def build_pauses(args, rate: int, hop: int, max_wav_value: float, device=None):
    """the PauseShortener for the recordings, behind the trimmer as in training, or None without --max_pause_ms (checked on the host)"""
    if getattr(args, "max_pause_ms", None) is None:
        return None
    return PauseShortener(device, rate, max_pause_ms=args.max_pause_ms, hop_size=hop, top_db=args.pause_top_db, max_wav_value=max_wav_value)


def build_highpass(args, rate: int = SAMPLING_RATE, max_wav_value: float = 32768.0, device=None):
    """the IIRFilter for the recordings, in front of the trimmer as in training, or None without --highpass_hz (checked on the host)"""
    return build_chain(device, rate, getattr(args, "highpass_hz", None), getattr(args, "highpass_order", None), max_wav_value=max_wav_value)


def check_f0_args(args, front=None) -> None:
    """--f0 needs audio of the synthesis that means something: refused on the host, before anything is loaded"""
    if args.f0_smooth and not args.f0:
        raise ValueError("--f0_smooth smooths the contours that --f0 scores: give --f0 as well")
    mcd_wave = getattr(args, "mcd_wave", False)
    if not args.f0 and not mcd_wave:
        return
    flag = "--f0" if args.f0 else "--mcd_wave"
    if args.vocoder == "hifigan" and not (args.vocoder_checkpoint and args.vocoder_config):
        raise ValueError(f"{flag} needs audio of the synthesis: give --vocoder griffinlim, or --vocoder hifigan with --vocoder_checkpoint and "
                         f"--vocoder_config (a generator with random weights has no {'pitch' if args.f0 else 'spectrum'} to score)")
    if front is not None:
        rate, n_fft, hop = int(front.get("sampling_rate", SAMPLING_RATE)), int(front.get("n_fft", 1024)), int(front.get("hop_size", 256))
        if (rate, n_fft, hop) != (SAMPLING_RATE, 1024, 256):
            raise ValueError(f"{flag}: the vocoders produce {SAMPLING_RATE} Hz audio of 256 samples per frame; the recipe's front-end has "
                             f"sampling_rate {rate}, n_fft {n_fft}, hop_size {hop}")
        if args.f0:
            lag_range(rate, n_fft, args.f0_min, args.f0_max)


def _mean_of_finite(values) -> float:
    values = [v for v in values if np.isfinite(v)]
    return float(np.mean(values)) if values else float("nan")


def format_lines(rows, extra=None, cuts=None, wave=None):
    """the lines of mcd.tsv from (utt, mcd, frames synthesised, frames recorded, path length) per utterance; the last line holds the means.
    `extra`: (f0_rmse_cents, vuv_error, voiced_pairs) per utterance (--f0); `cuts`: (start, length) per recording (--trim_silence /
    --normalize_peak); `wave`: (mcd_wave_db, mcd_wave_path_len) per utterance (--mcd_wave).  Each adds its columns behind those before it."""
    for name, col in (("extra", extra), ("cuts", cuts), ("wave", wave)):
        if col is not None and len(col) != len(rows):
            raise ValueError(f"{name} must hold one entry per row")
    lines = []
    for i, (utt, m, a, b, n) in enumerate(rows):
        tail = f"\t{extra[i][0]:.4f}\t{extra[i][1]:.6f}\t{extra[i][2]}" if extra is not None else ""
        if cuts is not None:
            tail += f"\t{cuts[i][0]}\t{cuts[i][1]}"
        if wave is not None:
            tail += f"\t{float(wave[i][0]):.6f}\t{int(wave[i][1])}"
        lines.append(f"{utt}\t{m:.6f}\t{a}\t{b}\t{n}{tail}")
    tail = ""
    if extra is not None:
        tail = f"\t{_mean_of_finite([e[0] for e in extra]):.4f}\t{_mean_of_finite([e[1] for e in extra]):.6f}\t{_mean_of_finite([e[2] for e in extra]):.1f}"
    if cuts is not None:
        tail += "\t-\t-"
    if wave is not None:
        tail += f"\t{_mean_of_finite([w[0] for w in wave]):.6f}\t-"
    lines.append(f"mean\t{_mean_of_finite([r[1] for r in rows]):.6f}{tail}")
    return lines


def run_score(args) -> float:
    check_f0_args(args)
    build_highpass(args)
    build_pauses(args, SAMPLING_RATE, 256, 32768.0)   # a --max_pause_ms <= 0 is refused here, before anything is loaded
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: efficient_tts_amd has no CPU path")
    if not args.length_scale > 0:
        raise ValueError("--length_scale must be > 0")
    device = torch.device("cuda")
    os.makedirs(args.outdir, exist_ok=True)
    config, phn2idx, model = load_acoustic_model(args, device)
    front = config.get("frontend_params") or {}
    frontend = LogMelFrontend(device, **front)
    rate = int(front.get("sampling_rate", 22050))
    scorer = MelCepstralDistortion(device, num_mels=frontend.n_mels)
    check_f0_args(args, front)
    highpass = build_highpass(args, rate, frontend.max_wav_value, device)
    trimmer = build_trimmer(args, frontend.hop, frontend.max_wav_value, device)
    pauses = build_pauses(args, rate, frontend.hop, frontend.max_wav_value, device)
    if args.f0 or args.mcd_wave:
        vocoder = build_vocoder(args, device)
    if args.mcd_wave:
        wave_scorer = WaveformMCD(device, sampling_rate=rate, hop_size=frontend.hop, max_wav_value=frontend.max_wav_value)
    if args.f0:
        tracker = PitchTracker(device, sampling_rate=rate, n_fft=frontend.n_fft, hop_size=frontend.hop, fmin=args.f0_min, fmax=args.f0_max,
                               threshold=args.f0_threshold, max_wav_value=frontend.max_wav_value, smooth=args.f0_smooth)
        f0_error = F0Error(device)
    wav_dir = (config.get("dataset_params") or {}).get("wav_path")
    items = _read_list(args.test_fid_scp, phn2idx, with_paths=True)
    bs = max(1, int(args.batch_size))
    rows, extra, cuts, wave = [], [], [], []
    for lo in range(0, len(items), bs):
        chunk = items[lo:lo + bs]
        wavs = [read_wav(path, wav_dir, rate)[0] for _, _, path in chunk]
        audio = torch.nn.utils.rnn.pad_sequence(wavs, batch_first=True)
        ids = torch.nn.utils.rnn.pad_sequence([t for _, t, _ in chunk], batch_first=True)
        wav_len = torch.tensor([w.shape[0] for w in wavs])
        with torch.no_grad():
            if highpass is not None:               # DC and rumble out of the recordings, from zero state over each one's own samples: fp32 on the device
                audio = highpass(audio.to(device), wav_len)
            if trimmer is not None:                # the recordings as a run with these options trains on them: fp32 on the device, new lengths
                audio, wav_len, cut_start, _ = trimmer(audio.to(device), wav_len, return_bounds=True)
                cuts.extend(zip(cut_start.tolist(), wav_len.tolist()))
            if pauses is not None:                 # the long pauses inside the recordings cut down, as a run with `max_pause_ms` trains on them
                audio, wav_len = pauses(audio.to(device), wav_len)
            rec, rec_len = frontend(audio, wav_len)
            syn, syn_len = model.inference_batch(ids.to(device), torch.tensor([len(t) for _, t, _ in chunk], device=device),
                                                 length_scale=args.length_scale)[:2]
            out = scorer(syn, syn_len, rec, rec_len, return_path=True) if args.f0 else scorer(syn, syn_len, rec, rec_len)
            if args.f0 or args.mcd_wave:
                wav = vocoder(syn.transpose(1, 2).contiguous(), syn_len)[:, 0].float()
            if args.mcd_wave:                      # the vocoded synthesis against the recording (trimmed where the flags say so), along their own path
                wave_out = wave_scorer(wav, (syn_len * frontend.hop).clamp(max=wav.shape[1]), audio.to(device), wav_len)
                wave.extend(zip(wave_out["mcd"].tolist(), wave_out["count"].tolist()))
            if args.f0:
                f0_syn = tracker(wav, syn_len * frontend.hop, max_frames=syn.shape[1], short_ok=True)[0]
                f0_rec = tracker(audio, wav_len, max_frames=rec.shape[1])[0]
                pitch = f0_error(f0_syn, f0_rec, out["path"], out["path_len"])
                extra.extend(zip(pitch["f0_rmse_cents"].tolist(), pitch["vuv_error"].tolist(), pitch["voiced_pairs"].tolist()))
        for (utt, _, _), m, a, b, n in zip(chunk, out["mcd"].tolist(), syn_len.tolist(), rec_len.tolist(), out["path_len"].tolist()):
            rows.append((utt, m, a, b, n))
    scored = [r[1] for r in rows if np.isfinite(r[1])]
    mean = float(np.mean(scored)) if scored else float("nan")
    mean_of = lambda k: float(np.mean([e[k] for e in extra if np.isfinite(e[k])])) if any(np.isfinite(e[k]) for e in extra) else float("nan")
    with open(os.path.join(args.outdir, "mcd.tsv"), "w") as handle:
        handle.write("\n".join(format_lines(rows, extra if args.f0 else None, cuts if trimmer is not None else None, wave if args.mcd_wave else None)) + "\n")
    print(f"mean MCD over {len(scored)} of {len(rows)} utterances: {mean:.4f} dB")
    if args.f0:
        print(f"mean F0 error {mean_of(0):.2f} cents over {sum(np.isfinite(e[0]) for e in extra)} utterances with a voiced pair, "
              f"mean voiced/unvoiced error {mean_of(1):.4f}")
    if args.mcd_wave:
        print(f"mean waveform MCD (order-24 mel-cepstra, warped) over {sum(np.isfinite(w[0]) for w in wave)} of {len(rows)} utterances: "
              f"{_mean_of_finite([w[0] for w in wave]):.4f} dB")
    return mean


def main(argv=None) -> int:
    run_score(get_parser().parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
