"""`python -m efficient_tts_amd.bin.trim` -- what silence trimming and peak normalisation would do to a corpus, before training on it.

    python -m efficient_tts_amd.bin.trim --filelist train.txt --wav_path wavs --outdir exp/trim \\
        [--top_db 40] [--keep_frames 2] [--frame_length 1024] [--hop_size 256] [--normalize_peak 0.95] [--batch_size 16] [--write_wavs]
        [--max_pause_ms 300 [--pause_top_db 40]]

Reads a training file list (`audiopath|...`, one recording per line; the file name is looked up under --wav_path, 16-bit mono wav files),
runs the recordings through `efficient_tts_amd.trim.SilenceTrimmer` in batches -- the object that `trim_silence: true` / `normalize_peak`
in the training recipe put in front of the log-mel front-end, so --top_db, --keep_frames and --frame_length mean what `trim_top_db`,
`trim_keep_frames` and `trim_frame_length` mean there -- and writes outdir/trim.tsv:

    id  samples  start  new_samples  gain  seconds_removed

one line per recording under a header line (gain: what every kept sample was multiplied by, 1 / 32768 included; seconds at the file's own
rate), and prints the totals.  `--write_wavs` also writes the results to outdir/<id>.wav as 16-bit PCM (rounded to nearest, clipped),
to listen to a threshold before training on it.  There is no CPU mode.

`--max_pause_ms MS` also runs what the trimmer left through `efficient_tts_amd.pauses.PauseShortener` (what `max_pause_ms` in the recipe puts
behind the trimmer; --pause_top_db is its `pause_top_db`, the frame length and hop are those above, the rate is each batch's own) and appends
two columns to every line, pauses_cut and pause_seconds_removed; --write_wavs then writes the shortened audio.  Without the flag trim.tsv is
byte for byte what it was.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

from efficient_tts_amd.bin._io import read_wav
from efficient_tts_amd.pauses import PauseShortener
from efficient_tts_amd.trim import SilenceTrimmer


def get_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="efficient_tts_amd.bin.trim", description=__doc__.splitlines()[0])
    p.add_argument("--filelist", type=str, required=True, help="file list: audiopath|..., one recording per line")
    p.add_argument("--wav_path", type=str, required=True, help="directory of the wav files (looked up by file name)")
    p.add_argument("--outdir", type=str, required=True, help="where trim.tsv (and with --write_wavs the wav files) go")
    p.add_argument("--top_db", type=float, default=40.0, help="a frame this far under the loudest one is silence (default 40)")
    p.add_argument("--keep_frames", type=int, default=2, help="frames kept around the first and last sound frame (default 2)")
    p.add_argument("--frame_length", type=int, default=1024, help="512, 1024 or 2048 samples (default 1024)")
    p.add_argument("--hop_size", type=int, default=256, help="the front-end's hop (default 256)")
    p.add_argument("--normalize_peak", type=float, default=None, help="bring every recording to this peak, in (0, 1] (default: leave the level)")
    p.add_argument("--batch_size", type=int, default=16, help="recordings per call (default 16; every item is treated as if alone)")
    p.add_argument("--write_wavs", action="store_true", help="also write the trimmed recordings as 16-bit wav files")
    p.add_argument("--max_pause_ms", type=float, default=None, help="also cut every pause inside a recording that is longer than this down to it")
    p.add_argument("--pause_top_db", type=float, default=40.0, help="--max_pause_ms: a frame this far under the loudest one is quiet (default 40)")
    return p


def build_pauses(args, rate: int = 22050, device=None):
    """the PauseShortener behind the trimmer at `rate`, or None without --max_pause_ms (checked on the host)"""
    if getattr(args, "max_pause_ms", None) is None:
        return None
    return PauseShortener(device, rate, max_pause_ms=args.max_pause_ms, frame_length=args.frame_length, hop_size=args.hop_size, top_db=args.pause_top_db)


def _read_list(path: str):
    with open(path, encoding="utf-8") as handle:
        return [line.split("|")[0].strip() for line in handle if line.strip()]


def run_trim(args) -> float:
    from scipy.io.wavfile import write
    trimmer = SilenceTrimmer(None, frame_length=args.frame_length, hop_size=args.hop_size, top_db=args.top_db, keep_frames=args.keep_frames,
                             peak=args.normalize_peak)
    build_pauses(args)                         # a --max_pause_ms <= 0 is refused here, before any file is read
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: efficient_tts_amd has no CPU path")
    device = torch.device("cuda")
    shorteners = {}                            # rate -> PauseShortener (--max_pause_ms is a time, the plan counts hops)
    os.makedirs(args.outdir, exist_ok=True)
    names = _read_list(args.filelist)
    bs = max(1, int(args.batch_size))
    removed = kept = 0.0
    with open(os.path.join(args.outdir, "trim.tsv"), "w") as handle:
        handle.write("id\tsamples\tstart\tnew_samples\tgain\tseconds_removed" + ("\tpauses_cut\tpause_seconds_removed" if args.max_pause_ms is not None else "")
                     + "\n")
        for lo in range(0, len(names), bs):
            chunk = names[lo:lo + bs]
            wavs, rates = zip(*(read_wav(os.path.join(args.wav_path, os.path.basename(name))) for name in chunk))
            audio = torch.nn.utils.rnn.pad_sequence(list(wavs), batch_first=True).to(device)
            out, new_len, start, gain = trimmer(audio, torch.tensor([w.shape[0] for w in wavs]), return_bounds=True)
            new_len, start, gain = new_len.tolist(), start.tolist(), gain.tolist()
            cut = None
            if args.max_pause_ms is not None:
                if len(set(rates)) != 1:
                    raise ValueError(f"--max_pause_ms: the recordings of one batch must share a sampling rate, got {sorted(set(rates))}")
                shortener = shorteners.setdefault(rates[0], build_pauses(args, rates[0], device))
                out, short_len, stats = shortener(out, torch.tensor(new_len), return_stats=True)
                cut, gone, short_len = stats["pauses"].tolist(), stats["removed"].tolist(), short_len.tolist()
            pcm = torch.round(out * 32768.0).clamp(-32768, 32767).to(torch.int16).cpu().numpy() if args.write_wavs else None
            for i, name in enumerate(chunk):
                utt = os.path.splitext(os.path.basename(name))[0]
                n = int(wavs[i].shape[0])
                seconds = (n - new_len[i]) / rates[i]
                removed, kept = removed + seconds, kept + new_len[i] / rates[i]
                more = "" if cut is None else f"\t{cut[i]}\t{gone[i] / rates[i]:.4f}"
                handle.write(f"{utt}\t{n}\t{start[i]}\t{new_len[i]}\t{gain[i]:.9g}\t{seconds:.4f}{more}\n")
                if pcm is not None:
                    write(os.path.join(args.outdir, utt + ".wav"), rates[i], pcm[i, :new_len[i] if cut is None else short_len[i]])
    print(f"{len(names)} recordings: {removed:.2f} s removed, {kept:.2f} s kept")
    return removed


def main(argv=None) -> int:
    run_trim(get_parser().parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
