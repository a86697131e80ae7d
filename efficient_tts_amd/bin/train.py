"""`python -m efficient_tts_amd.bin.train` -- trains EFTS-CNN on MI355X from the reference recipe's files.

Drop-in for the command line and YAML schema of the reference entry point (nntts/bin/train.py:30-253), so the
recipe's `run.sh` and `egs/lj/conf/*.yaml` work unchanged:

    python -m efficient_tts_amd.bin.train --config conf.yaml --train_fid_scp train.txt --dev_fid_scp dev.txt \\
        --outdir exp/efts [--resume exp/efts/checkpoint-5000steps.pkl | --pretrain other.pkl] [--verbose 1]

Multi-GPU: one process per GPU, e.g. `python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1
-m efficient_tts_amd.bin.train ...`; RANK / LOCAL_RANK / WORLD_SIZE come from the environment and the backend
"nccl" is RCCL over xGMI.  The pieces named in the YAML (`dataset_type`, `collate_fn_type`, `model_name`,
`optimizer_type`, `scheduler_type`, `trainer_type`) are resolved in this package's registries
(efficient_tts_amd.datasets / models / optimizers / schedulers / trainers); the dataset yields waveforms and the
trainer computes log-mels on the GPU (efficient_tts_amd.frontend).  There is no CPU mode.
"""
from __future__ import annotations

import argparse
import logging
import os
import sys
from dataclasses import dataclass
from typing import Any, Dict, Optional

import torch
import yaml
from torch.utils.data import DataLoader
from torch.utils.data.distributed import DistributedSampler

import efficient_tts_amd as pkg
from efficient_tts_amd import datasets, models, optimizers, schedulers, trainers
from efficient_tts_amd.dist import DistributedEFTS
from efficient_tts_amd.ema import ParamEMA
from efficient_tts_amd.optim import FlatOptimizer
from efficient_tts_amd.frontend import LogMelFrontend
from efficient_tts_amd.resample import Resampler
from efficient_tts_amd.denoise import SpectralGate
from efficient_tts_amd.iir import IIRFilter, highpass_sos, preemphasis_sos
from efficient_tts_amd.loudness import LoudnessNormalizer
from efficient_tts_amd.pauses import PauseShortener
from efficient_tts_amd.trim import SilenceTrimmer

# (flags, kwargs) of the reference command line, kept as data so the parser and the docs cannot drift apart
_CLI = (
    (("--config",), dict(type=str, required=True, help="YAML recipe (egs/*/conf/*.yaml schema)")),
    (("--outdir",), dict(type=str, required=True, help="where config.yml and checkpoint-*steps.pkl go")),
    (("--train_fid_scp",), dict(type=str, default=None, help="training file list: audiopath|phoneme sequence")),
    (("--dev_fid_scp",), dict(type=str, default=None, help="validation file list")),
    (("--resume",), dict(type=str, default="", nargs="?", help="checkpoint to continue from (model, optimizer, schedule, counters)")),
    (("--pretrain",), dict(type=str, default="", nargs="?", help="checkpoint to take only the parameters from")),
    (("--verbose",), dict(type=int, default=1, help="0 warnings only, 1 info, 2 debug")),
    (("--rank", "--local_rank"), dict(type=int, default=None, help="local device index; normally LOCAL_RANK")),
)


def get_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog="efficient_tts_amd.bin.train", description=__doc__.splitlines()[0])
    for flags, kwargs in _CLI:
        parser.add_argument(*flags, **kwargs)
    return parser


@dataclass
class _Process:
    """where this process sits in the job (one process per GPU)"""
    rank: int
    local_rank: int
    world: int

    @property
    def distributed(self) -> bool:
        return self.world > 1

    @property
    def device(self) -> torch.device:
        return torch.device("cuda", self.local_rank)

    @staticmethod
    def from_env(cli_local_rank: Optional[int]) -> "_Process":
        env = os.environ
        local = cli_local_rank if cli_local_rank is not None else int(env.get("LOCAL_RANK", 0))
        return _Process(rank=int(env.get("RANK", 0)), local_rank=local, world=int(env.get("WORLD_SIZE", 1)))


def _setup_logging(verbose: int, quiet: bool) -> None:
    if quiet:                                   # every rank but 0 keeps silent, like the reference
        sys.stdout = open(os.devnull, "w")
    level = {0: logging.WARNING, 1: logging.INFO}.get(verbose, logging.DEBUG)
    logging.basicConfig(level=level, stream=sys.stdout, force=True,
                        format="%(asctime)s %(levelname)s %(name)s:%(lineno)d  %(message)s")


def _load_config(args: argparse.Namespace, proc: _Process) -> Dict[str, Any]:
    with open(args.config) as handle:
        config = yaml.safe_load(handle) or {}
    config.update(vars(args))                   # the reference merges the CLI into the recipe; trainer reads both
    config.update(rank=proc.rank, distributed=proc.distributed, world_size=proc.world,
                  version=getattr(pkg, "__version__", "0.1.0"))
    if proc.rank == 0:
        os.makedirs(args.outdir, exist_ok=True)
        with open(os.path.join(args.outdir, "config.yml"), "w") as handle:
            yaml.safe_dump(config, handle)
    for key in sorted(config):
        logging.info(f"config {key} = {config[key]}")
    return config


def _build_data(config: Dict[str, Any], args: argparse.Namespace, proc: _Process):
    make_dataset = getattr(datasets, config.get("dataset_type", "TextMelLoader"))
    params = config.get("dataset_params") or {}
    splits = {"train": make_dataset(meta_file=args.train_fid_scp, **params),
              "dev": make_dataset(meta_file=args.dev_fid_scp, **params)}
    collate = getattr(datasets, config.get("collate_fn_type", "TextMelCollate"))(**(config.get("collate_fn_params") or {}))
    samplers: Dict[str, Optional[DistributedSampler]] = {"train": None, "dev": None}
    if proc.distributed:
        samplers = {name: DistributedSampler(ds, num_replicas=proc.world, rank=proc.rank, shuffle=(name == "train"))
                    for name, ds in splits.items()}
    loaders = {name: DataLoader(ds, batch_size=int(config["batch_size"]), collate_fn=collate, sampler=samplers[name],
                                shuffle=samplers[name] is None, num_workers=int(config.get("num_workers", 0)),
                                pin_memory=bool(config.get("pin_memory", False)))
               for name, ds in splits.items()}
    for name, ds in splits.items():
        logging.info(f"{name}: {len(ds)} utterances")
    return loaders, samplers


def build_trimmer(config: Dict[str, Any], device=None) -> Optional[SilenceTrimmer]:
    """the SilenceTrimmer that the recipe asks for, on the front-end's hop; None when neither `trim_silence` nor `normalize_peak` is set.
    `trim_silence: true` (with `trim_top_db`, `trim_keep_frames`, `trim_frame_length`) cuts the quiet ends off every recording;
    `normalize_peak: 0.95` brings what is kept to that peak, with or without trimming."""
    trim, peak = bool(config.get("trim_silence", False)), config.get("normalize_peak")
    if isinstance(peak, bool):
        peak = 0.95 if peak else None
    if not trim and peak is None:
        return None
    front = config.get("frontend_params") or {}
    return SilenceTrimmer(device, frame_length=int(config.get("trim_frame_length", 1024)), hop_size=int(front.get("hop_size", 256)),
                          top_db=float(config.get("trim_top_db", 40.0)), keep_frames=int(config.get("trim_keep_frames", 2)),
                          peak=None if peak is None else float(peak), max_wav_value=float(front.get("max_wav_value", 32768.0)), trim=trim)


_PAUSE_KEYS = ("pause_top_db", "pause_frame_length", "pause_fade")


def build_pauses(config: Dict[str, Any], device=None) -> Optional[PauseShortener]:
    """the PauseShortener that the recipe asks for, at the front-end's rate and hop; None without `max_pause_ms`.  `max_pause_ms: 300` cuts
    every pause inside a recording that is longer than that down to it, behind the trimmer and in front of the level; `pause_top_db`
    (default 40.0) under the loudest frame is quiet, `pause_frame_length` (default 1024) is the energy frame and `pause_fade` (default 64)
    the samples of the linear fade into a joint.  A value <= 0, or one of the other keys without `max_pause_ms`, is refused."""
    limit = config.get("max_pause_ms")
    if limit is None:
        stray = [k for k in _PAUSE_KEYS if k in config]
        if stray:
            raise ValueError(f"{', '.join(stray)}: set without max_pause_ms")
        return None
    if isinstance(limit, bool) or not isinstance(limit, (int, float)) or not float(limit) > 0.0:
        raise ValueError(f"max_pause_ms must be a number > 0, got {limit!r}")
    front = config.get("frontend_params") or {}
    return PauseShortener(device, _front_rate(config), max_pause_ms=float(limit), frame_length=config.get("pause_frame_length", 1024),
                          hop_size=int(front.get("hop_size", 256)), top_db=float(config.get("pause_top_db", 40.0)),
                          fade=config.get("pause_fade", 64), max_wav_value=float(front.get("max_wav_value", 32768.0)))


_GATE_KEYS = ("denoise_strength", "denoise_floor", "denoise_top_db", "denoise_min_frames")


def build_gate(config: Dict[str, Any], device=None) -> Optional[SpectralGate]:
    """the SpectralGate that the recipe asks for; None without `denoise_corpus: true`.  Every recording is gated with the noise profile
    measured from its own quiet frames: `denoise_strength` (default 1.0) times the profile is subtracted from the magnitudes,
    `denoise_floor` (default 0.1) bounds the gain from below, `denoise_top_db` (default 40.0) under the loudest frame is quiet, and a recording
    with fewer than `denoise_min_frames` (default 8) quiet frames is left as it is.  One of these keys without `denoise_corpus` is refused."""
    on = config.get("denoise_corpus", False)
    if not isinstance(on, bool):
        raise ValueError(f"denoise_corpus must be true or false, got {on!r}")
    if not on:
        stray = [k for k in _GATE_KEYS if k in config]
        if stray:
            raise ValueError(f"{', '.join(stray)}: set without denoise_corpus: true")
        return None
    front = config.get("frontend_params") or {}
    return SpectralGate(device, strength=config.get("denoise_strength", 1.0), floor=config.get("denoise_floor", 0.1),
                        top_db=config.get("denoise_top_db", 40.0), min_frames=config.get("denoise_min_frames", 8),
                        max_wav_value=float(front.get("max_wav_value", 32768.0)))


def build_loudness(config: Dict[str, Any], device=None) -> Optional[LoudnessNormalizer]:
    """the LoudnessNormalizer that the recipe asks for, at the front-end's rate; None without `normalize_loudness`.
    `normalize_loudness: -23.0` brings every recording to that integrated loudness in LUFS (ITU-R BS.1770), `loudness_peak_ceiling`
    (default 0.99; null: none) bounds the peak that the gain may lead to.  Level is set once: together with `normalize_peak` it is refused."""
    target = config.get("normalize_loudness")
    if target is None or target is False:
        return None
    if isinstance(target, bool):
        target = -23.0
    if config.get("normalize_peak") not in (None, False):
        raise ValueError("normalize_loudness and normalize_peak both set the level of a recording: give one of them")
    front = config.get("frontend_params") or {}
    data = config.get("dataset_params") or {}
    rate = int(front.get("sampling_rate", data.get("sampling_rate", 22050)))
    ceiling = config.get("loudness_peak_ceiling", 0.99)
    return LoudnessNormalizer(device, rate, target_lufs=float(target), peak_ceiling=None if ceiling is None else float(ceiling),
                              max_wav_value=float(front.get("max_wav_value", 32768.0)))


def _front_rate(config: Dict[str, Any]) -> int:
    front = config.get("frontend_params") or {}
    data = config.get("dataset_params") or {}
    return int(front.get("sampling_rate", data.get("sampling_rate", 22050)))


def build_highpass(config: Dict[str, Any], device=None) -> Optional[IIRFilter]:
    """the IIRFilter that `highpass_hz` asks for, at the front-end's rate; None without the key.  `highpass_hz: 60` runs a Butterworth
    high-pass of `highpass_order` 2 (the default) or 4 over every recording, behind the resampler and in front of the spectral gate, so that
    the noise profile, the trim threshold and the loudness see no DC offset and no rumble.  A cutoff outside (0, rate / 2), another order, or
    an order without a cutoff is refused."""
    cutoff = config.get("highpass_hz")
    if cutoff is None:
        if "highpass_order" in config:
            raise ValueError("highpass_order: set without highpass_hz")
        return None
    front = config.get("frontend_params") or {}
    return IIRFilter(device, highpass_sos(_front_rate(config), cutoff, config.get("highpass_order", 2)),
                     max_wav_value=float(front.get("max_wav_value", 32768.0)))


def build_preemphasis(config: Dict[str, Any], device=None) -> Optional[IIRFilter]:
    """the IIRFilter that `preemphasis` asks for; None without the key.  `preemphasis: 0.97` runs y[n] = x[n] - 0.97 x[n - 1] over every
    recording as the last step in front of the log-mel front-end.  A coefficient outside [0, 1) is refused."""
    coef = config.get("preemphasis")
    if coef is None:
        return None
    front = config.get("frontend_params") or {}
    return IIRFilter(device, preemphasis_sos(coef), max_wav_value=float(front.get("max_wav_value", 32768.0)))


def build_ema(config: Dict[str, Any], optimizer=None) -> Optional[ParamEMA]:
    """the ParamEMA that the recipe asks for, attached to `optimizer`; None without `ema_decay`.  `ema_decay: 0.999` keeps an exponential
    moving average of the parameters beside the optimizer state, `ema_warmup` (default true) lets the decay ramp up as (1 + n) / (10 + n).
    It needs one of the fused optimizers of the registry: together with any other optimizer the key is refused.  Without an optimizer
    only the keys are checked."""
    decay, warmup = config.get("ema_decay"), config.get("ema_warmup", True)
    if decay is None:
        if "ema_warmup" in config:
            raise ValueError("ema_warmup: set without ema_decay")
        return None
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 < float(decay) < 1.0:
        raise ValueError(f"ema_decay must be a number in (0, 1), got {decay!r}")
    if not isinstance(warmup, bool):
        raise ValueError(f"ema_warmup must be true or false, got {warmup!r}")
    if optimizer is None:
        return None
    if not isinstance(optimizer, FlatOptimizer):
        raise ValueError(f"ema_decay needs one of the fused optimizers (optimizer_type Adam, AdamW or RAdam of efficient_tts_amd.optimizers), "
                         f"whose parameters live in one flat buffer: optimizer_type {config.get('optimizer_type', 'Adam')!r} built a "
                         f"{type(optimizer).__module__}.{type(optimizer).__name__}")
    return ParamEMA(optimizer, decay=float(decay), warmup=warmup)


def _build_trainer(config: Dict[str, Any], loaders, samplers, proc: _Process):
    device = proc.device
    net = getattr(models, config["model_name"])(**config["model_params"]).to(device)
    optimizer = getattr(optimizers, config.get("optimizer_type", "Adam"))(
        net, grad_norm=float(config.get("grad_norm", 1.0)), **config["optimizer_params"])
    ema = build_ema(config, optimizer)
    if ema is not None:
        logging.info(f"exponential moving average of the parameters: decay {ema.decay}" + (", warming up as (1 + n) / (10 + n)" if ema.warmup else "")
                     + "; checkpoints carry it as \"ema\", evaluations run on it")
    scheduler = None
    if config.get("scheduler_type"):
        scheduler = getattr(schedulers, config["scheduler_type"])(optimizer=optimizer, **(config.get("scheduler_params") or {}))
    model = DistributedEFTS(net) if proc.distributed else net
    logging.info(f"{model}")
    trainer_class = getattr(trainers, config.get("trainer_type", "EfficientTTSTrainer"))
    trainer = trainer_class(steps=0, epochs=0, data_loader=loaders, sampler=samplers, model=model, optimizer=optimizer,
                            scheduler=scheduler, config=config, device=device)
    front = config.get("frontend_params") or {}
    trainer.frontend = LogMelFrontend(device, **front)
    # a corpus at another rate than the front-end's is converted on the device, batch by batch (dataset_params.source_sampling_rate)
    data = config.get("dataset_params") or {}
    front_rate = int(front.get("sampling_rate", data.get("sampling_rate", 22050)))
    source_rate = data.get("source_sampling_rate")
    if source_rate is not None and int(source_rate) != front_rate:
        trainer.resampler = Resampler(device, int(source_rate), front_rate, quality=config.get("resample_quality", "best"),
                                      max_wav_value=float(front.get("max_wav_value", 32768.0)))
        logging.info(f"resampling {source_rate} -> {front_rate} Hz on the device ({trainer.resampler.quality})")
    trainer.highpass = build_highpass(config, device)
    if trainer.highpass is not None:
        logging.info(f"on the device, per recording: Butterworth high-pass of order {2 * trainer.highpass.sections} at {config['highpass_hz']} Hz")
    trainer.gate = build_gate(config, device)
    if trainer.gate is not None:
        g = trainer.gate
        logging.info(f"on the device, per recording: noise profile from the frames {g.top_db} dB under the loudest, {g.strength} x subtracted, "
                     f"gain floor {g.floor}, untouched under {g.min_frames} noise frames")
    trainer.trimmer = build_trimmer(config, device)
    if trainer.trimmer is not None:
        t = trainer.trimmer
        logging.info(f"on the device, per recording: " + (f"silence trimmed at {t.top_db} dB under the loudest frame, {t.keep_frames} frames kept" if t.trim
                                                           else "no trimming") + (f", peak set to {t.peak}" if t.peak is not None else ""))
    trainer.pauses = build_pauses(config, device)
    if trainer.pauses is not None:
        q = trainer.pauses
        logging.info(f"on the device, per recording: pauses over {q.max_pause_ms} ms ({q.chunks} hops, {q.top_db} dB under the loudest frame) cut "
                     f"down to that, {q.fade} samples of fade into the joint")
    trainer.loudness = build_loudness(config, device)
    if trainer.loudness is not None:
        n = trainer.loudness
        logging.info(f"on the device, per recording: integrated loudness set to {n.target_lufs} LUFS at {n.sampling_rate} Hz"
                     + (f", peak held under {n.peak_ceiling}" if n.peak_ceiling is not None else ""))
    trainer.preemphasis = build_preemphasis(config, device)
    if trainer.preemphasis is not None:
        logging.info(f"on the device, per recording: pre-emphasis {config['preemphasis']} in front of the log-mel front-end")
    return trainer


def main(argv=None) -> int:
    args = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: efficient_tts_amd has no CPU path")
    proc = _Process.from_env(args.rank)
    torch.cuda.set_device(proc.local_rank)
    if proc.distributed:
        torch.distributed.init_process_group(backend="nccl", init_method="env://", device_id=proc.device)
    _setup_logging(args.verbose, quiet=proc.rank != 0)
    config = _load_config(args, proc)
    build_loudness(config)                     # a recipe that sets the level twice is refused here, before any data is read
    build_gate(config)                         # likewise a gate key that is out of range or stands without `denoise_corpus`
    build_ema(config)                          # likewise an `ema_decay` outside (0, 1)
    build_highpass(config)                     # likewise a `highpass_hz` outside (0, rate / 2) or an order that is not 2 or 4
    build_preemphasis(config)                  # likewise a `preemphasis` outside [0, 1)
    build_pauses(config)                       # likewise a `max_pause_ms` <= 0 or a pause key that stands without it
    loaders, samplers = _build_data(config, args, proc)
    trainer = _build_trainer(config, loaders, samplers, proc)
    if args.pretrain:
        trainer.load_checkpoint(args.pretrain, load_only_params=True)
        logging.info(f"parameters initialised from {args.pretrain}")
    if args.resume:
        trainer.load_checkpoint(args.resume)
        logging.info(f"resumed from {args.resume} at step {trainer.steps}")
    try:
        trainer.run()
    except KeyboardInterrupt:                   # same courtesy as the reference: keep what was learnt so far
        path = os.path.join(config["outdir"], f"checkpoint-{trainer.steps}steps.pkl")
        trainer.save_checkpoint(path)
        logging.info(f"interrupted: state saved to {path}")
    finally:
        if proc.distributed:
            torch.distributed.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
