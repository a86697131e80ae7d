"""GPU (-m gpu): the exponential moving average of the parameters -- efts_ema_update alone against the float64 restatement of
tests/ema_reference.py, then `ParamEMA` (efficient_tts_amd/ema.py) through a training run (eager and as a replayed hipGraph), `applied()`,
the trainer's checkpoints and evaluation, and the command lines.

The bound is derived, not tuned.  One update is d = fl(p - e), e' = fl(w d + e): the subtraction loses at most 2^-24 |p - e|, the fma's one
rounding at most 2^-24 |e'|, and for w in [0, 1] both lie under 2^-24 (|p| + |e|): 2^-23 (|p| + |e|) per element and update
(ema_reference.bound).  Over a sequence the bounds add up and nothing more: the recurrence is a contraction (an error d in e becomes
(1 - w) d), so what earlier updates lost does not grow.

Measured on an MI355X, as the tests print it: one launch uses at most 0.84 of the bound (n = 2 M + 5, w = 0.9), 50 updates 0.015 of the summed
bounds, the 8- and 9-step training runs 0.16 - 0.20 of them."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import ema_reference as R

pytestmark = pytest.mark.gpu

# a tail only (1, 3); one vector, no tail (4); one block less one element, one block, one block + 1 (1023 / 1024 / 1025); several blocks
# + a tail of 0 mod 4 (4100); and one element more than 2048 blocks * 1024 elements + a vector: the only size at which the grid strides
SIZES = [1, 3, 4, 1023, 1024, 1025, 4100, 2048 * 1024 + 5]
WORDS = [0.0, 2.0 ** -10, 0.001, 0.9, 1.0]
SENTINEL, GUARD = -7.5, 64


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """seeded N(0, 1) parameters and averages, each element scaled by its own power of ten over six decades (1e-3 .. 1e3), so that
    |p| << |e|, |p| >> |e| and p close to e all occur"""
    gen = torch.Generator().manual_seed(4409 + n)
    p = (torch.randn(n, generator=gen) * 10.0 ** (6.0 * torch.rand(n, generator=gen) - 3.0)).numpy()
    e = (torch.randn(n, generator=gen) * 10.0 ** (6.0 * torch.rand(n, generator=gen) - 3.0)).numpy()
    if n >= 1024:
        e[5::7] = p[5::7] * np.float32(1.0 + 2.0 ** -12)     # ... and a share of averages that have all but converged
    p.setflags(write=False); e.setflags(write=False)
    return p, e


def _launch(e_buf, p, n, w):
    from efficient_tts_amd import lib as L, ops as P
    L.check(L.load().efts_ema_update(e_buf.data_ptr(), p.data_ptr(), n, w, P._stream()), "efts_ema_update")


def _device_update(n, w):
    """one launch on fresh buffers; the average lies in front of GUARD sentinel words.  Returns (average [n], guard [GUARD]) on the host"""
    p0, e0 = _inputs(n)
    dev = _dev()
    p = torch.from_numpy(p0.copy()).to(dev)
    buf = torch.full((n + GUARD,), SENTINEL, device=dev)
    buf[:n].copy_(torch.from_numpy(e0.copy()))
    _launch(buf, p, n, w)
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), torch.from_numpy(p0.copy()))          # the parameters are read only
    out = buf.cpu()
    return out[:n].numpy(), out[n:].numpy()


@pytest.mark.parametrize("w", WORDS)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_float64(n, w):
    p0, e0 = _inputs(n)
    wf = R.f32(w)
    got, guard = _device_update(n, wf)
    ref, bound = R.update(e0, p0, wf), R.bound(e0, p0)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"n {n} w {w}: worst err / bound {float((err / bound).max()):.3f}")
    assert np.isfinite(got).all() and bool((err <= bound).all()), float((err / bound).max())
    assert bool((guard == SENTINEL).all())                              # nothing behind n is written
    if w == 0.0:
        assert np.array_equal(got.view(np.uint32), e0.view(np.uint32))      # bit for bit
    if w == 1.0:
        assert np.array_equal(got.view(np.uint32), p0.view(np.uint32))      # exactly p
    if 0.0 < w < 1.0 and n >= 4:
        assert not np.array_equal(got, e0)                              # (the launch did something)
    again, _ = _device_update(n, wf)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))   # no atomics: two runs, equal bits


def test_argument_and_alignment_errors_on_device_buffers():
    from efficient_tts_amd import lib as L, ops as P
    lib, dev = L.load(), _dev()
    e, p = torch.zeros(64, device=dev), torch.ones(64, device=dev)
    st = P._stream()
    for bad in ((None, p.data_ptr(), 8, 0.5), (e.data_ptr(), None, 8, 0.5), (e.data_ptr(), p.data_ptr(), 0, 0.5), (e.data_ptr(), p.data_ptr(), -1, 0.5),
                (e.data_ptr(), p.data_ptr(), 8, -0.5), (e.data_ptr(), p.data_ptr(), 8, 1.0 + 2.0 ** -20), (e.data_ptr(), p.data_ptr(), 8, float("nan"))):
        assert lib.efts_ema_update(*bad, st) == -1, bad
    for bad in ((e.data_ptr() + 4, p.data_ptr(), 8, 0.5), (e.data_ptr(), p.data_ptr() + 8, 8, 0.5)):
        assert lib.efts_ema_update(*bad, st) == -3, bad
    with pytest.raises(ValueError, match="16-byte"):
        L.check(lib.efts_ema_update(e.data_ptr() + 4, p.data_ptr(), 8, 0.5, st), "efts_ema_update")
    torch.cuda.synchronize()
    assert bool((e == 0).all())                                         # a refused call launched nothing


def test_fifty_updates_against_the_float64_recurrence():
    """50 launches with warm-up on, so the word changes every call (0.9, 0.818.., ...), the parameters moving by a random walk: within
    the sum of the per-update bounds"""
    from efficient_tts_amd import lib as L
    n, steps, decay = 4100 + 3, 50, 0.999
    p0, e0 = _inputs(n)
    gen = torch.Generator().manual_seed(11)
    snaps = [p0]
    for _ in range(steps - 1):
        snaps.append((torch.from_numpy(snaps[-1].copy()) * (1.0 + 1e-2 * torch.randn(n, generator=gen))).numpy())
    dev = _dev()
    e = torch.from_numpy(e0.copy()).to(dev)
    arr, words = (C.c_float * 1)(), []
    for k, s in enumerate(snaps):
        L.check(L.load().efts_ema_hyper(decay, 1, k, arr), "efts_ema_hyper")
        words.append(arr[0])
        _launch(e, torch.from_numpy(s.copy()).to(dev), n, arr[0])
    torch.cuda.synchronize()
    assert words == [R.word(decay, True, k) for k in range(steps)] and len(set(words)) == steps
    ref, bound = R.run(e0, snaps, decay, True)
    err = np.abs(e.cpu().numpy().astype(np.float64) - ref)
    print(f"50 updates: worst err / summed bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all())
    # the check can tell: the recurrence without warm-up ends somewhere else entirely
    assert float(np.abs(R.run(e0, snaps, decay, False)[0] - ref).max()) > 1e3 * float(bound.max())


# ---------------------------------------------------------------------------------------------
# ParamEMA on the model
# ---------------------------------------------------------------------------------------------
NARROW = dict(num_symbols=76, n_channels=256, symbol_embedding_dim=256, dropout_rate=0.0, use_masking=True, sigma=0.01)
B, T1, T2 = 3, 40, 130


@functools.lru_cache(maxsize=None)
def _batches():
    gen = torch.Generator().manual_seed(B * 31 + T2)
    out = []
    for _ in range(2):
        out.append((torch.randint(0, 76, (B, T1), generator=gen), torch.randint(T1 // 2, T1 + 1, (B,), generator=gen),
                    torch.randn(B, T2, 80, generator=gen), torch.randint(T2 // 2, T2 + 1, (B,), generator=gen)))
    return out


def _fresh(decay=0.999, warmup=True, precision="bf16"):
    from efficient_tts_amd import EfficientTTSCNN
    from efficient_tts_amd.ema import ParamEMA
    from efficient_tts_amd.optim import EftsRAdam
    torch.manual_seed(1)
    m = EfficientTTSCNN(precision=precision, **NARROW).to(_dev()).train()
    opt = EftsRAdam(m, lr=1e-3, betas=(0.9, 0.99), eps=1e-9, weight_decay=1e-5, grad_norm=1.0)
    return m, opt, ParamEMA(opt, decay=decay, warmup=warmup)


def _check_against_recurrence(ema, e0, snaps, what):
    n = ema.opt.eng.numel
    ref, bound = R.run(e0[:n].cpu().numpy(), [s[:n].cpu().numpy() for s in snaps], ema.decay, ema.warmup)
    err = np.abs(ema.flat[:n].cpu().numpy().astype(np.float64) - ref)
    ok = bound > 0
    print(f"{what}: {len(snaps)} updates over {n} elements, worst err / summed bound {float((err[ok] / bound[ok]).max()):.4f}")
    assert bool((err <= bound).all()), what
    return ref


@pytest.mark.parametrize("graphed", [False, True])
def test_training_run_keeps_the_average(graphed):
    """8 steps on a 256-channel model at the shapes of test_graphed_radam_step_equals_the_eager_loop, eager and through GraphedStep: the
    device average against the float64 recurrence over THIS run's own parameter snapshots (two runs' gradients differ by the backward's
    float atomics, so each run is judged against itself), the host counters, and a replay behind an applied() block"""
    from efficient_tts_amd.optim import WarmupLR
    from efficient_tts_amd.step_graph import GraphedStep
    dev = _dev()
    batches = [tuple(t.to(dev) for t in b) for b in _batches()]
    m, opt, ema = _fresh()
    assert opt.ema is ema and ema.updates == 0 and ema.flat.data_ptr() != opt.flat_p.data_ptr() and ema.flat.shape == opt.flat_p.shape
    e0 = ema.flat.clone()
    assert torch.equal(e0[:opt.eng.numel], opt.flat_p[:opt.eng.numel])
    step = GraphedStep(m, opt, WarmupLR(opt, warmup_steps=50))
    snaps = []
    for i in range(8):
        a = batches[i % 2]
        step(*a) if graphed else step._eager(*a)
        snaps.append(opt.flat_p.clone())
    assert ema.updates == 8 and opt.t == 8 and step.replays == (7 if graphed else 0)
    ref = _check_against_recurrence(ema, e0, snaps, "graphed" if graphed else "eager")
    n = opt.eng.numel
    # the average is neither the first nor the last iterate: the parameters moved, and it lags them
    assert float(np.abs(ref - snaps[-1][:n].cpu().numpy()).max()) > 1e-5 and float(np.abs(ref - e0[:n].cpu().numpy()).max()) > 1e-5
    # an applied() block exchanges contents only: the captured step keeps its pointers and its tag, and replays
    ptr, before = opt.flat_p.data_ptr(), opt.flat_p.clone()
    with ema.applied():
        assert torch.equal(ema.flat, before) and opt.flat_p.data_ptr() == ptr
    assert torch.equal(opt.flat_p, before)
    step(*batches[0]) if graphed else step._eager(*batches[0])
    snaps.append(opt.flat_p.clone())
    assert ema.updates == 9 and step.replays == (8 if graphed else 0)
    assert not torch.equal(opt.flat_p, before)
    _check_against_recurrence(ema, e0, snaps, "behind applied()")


def test_applied_exchanges_and_restores_bit_for_bit():
    dev = _dev()
    batches = [tuple(t.to(dev) for t in b) for b in _batches()]
    m, opt, ema = _fresh(decay=0.9, precision="bf16x3")
    from efficient_tts_amd.step_graph import GraphedStep
    step = GraphedStep(m, opt, None)
    for i in range(3):
        step._eager(*batches[i % 2])
    m.eval()
    text, tl, mel, ml = batches[0]
    durations = torch.full((B, T1), 3)

    def forward():
        with torch.no_grad():
            return m(text=text, text_lengths=tl, speech=mel, speech_lengths=ml)[4].clone()

    def synth():
        with torch.no_grad():
            return m.inference_batch(text, tl, durations=durations)[0].clone()

    before, fwd, raw = opt.flat_p.clone(), forward(), synth()
    avg_before = ema.flat.clone()
    raw_sd = {k: v.clone() for k, v in m.state_dict().items()}
    with ema.applied():
        sd, inside = ema.state_dict(), m.state_dict()
        assert set(sd) == {"decay", "warmup", "updates", "model"} and (sd["decay"], sd["warmup"], sd["updates"]) == (0.9, True, 3)
        assert list(sd["model"]) == list(inside)
        for k in inside:
            assert torch.equal(sd["model"][k], inside[k]), k
        assert any(not torch.equal(inside[k], raw_sd[k]) for k in inside)
        avg = synth()
        assert avg.shape == raw.shape and bool(torch.isfinite(avg).all()) and not torch.equal(avg, raw)
        with pytest.raises(RuntimeError, match="nest"):
            with ema.applied():
                pass
        with pytest.raises(RuntimeError, match="applied"):
            ema.update()
    assert torch.equal(opt.flat_p, before) and torch.equal(ema.flat, avg_before) and ema.updates == 3
    assert torch.equal(forward(), fwd) and torch.equal(synth(), raw)
    # outside the block the entry holds the same averaged weights, and they load as any "model" entry does
    sd2 = ema.state_dict()
    for k in sd["model"]:
        assert torch.equal(sd2["model"][k], sd["model"][k]), k
    from efficient_tts_amd import EfficientTTSCNN
    other = EfficientTTSCNN(precision="bf16x3", **NARROW)
    other.load_state_dict({k: v.cpu() for k, v in sd2["model"].items()})
    # an exception inside the block still restores
    with pytest.raises(KeyError):
        with ema.applied():
            raise KeyError("x")
    assert torch.equal(opt.flat_p, before) and torch.equal(ema.flat, avg_before)
    # load_state_dict: restores, and names a key set that does not fit
    m2, opt2, ema2 = _fresh(decay=0.9, precision="bf16x3")
    ema2.load_state_dict(sd2)
    n = opt.eng.numel
    assert ema2.updates == 3 and torch.equal(ema2.flat[:n], ema.flat[:n])
    broken = dict(sd2, model={k: v for k, v in sd2["model"].items() if k != "mel_output_layer.bias"})
    with pytest.raises(ValueError, match="mel_output_layer.bias"):
        ema2.load_state_dict(broken)


def test_trainer_evaluates_on_the_average_and_checkpoints_it(tmp_path, caplog):
    """EfficientTTSTrainer with an attached ParamEMA: `_evaluate` publishes the averaged weights' losses and leaves flat_p bit for bit;
    save_checkpoint adds "ema", load_checkpoint restores it, starts it over (with a warning) from a checkpoint without one, and a run
    without the key ignores the entry"""
    import logging
    from efficient_tts_amd.trainer import EfficientTTSTrainer
    dev = _dev()
    batches = [tuple(t.to(dev) for t in b) for b in _batches()]
    config = dict(outdir=str(tmp_path), grad_norm=1.0, train_max_steps=100, log_interval_steps=0, eval_interval_steps=0, save_interval_steps=0)

    def trainer_of(m, opt):
        t = EfficientTTSTrainer(steps=0, epochs=0, data_loader={"train": [], "dev": [batches[0]]}, sampler=None, model=m, optimizer=opt,
                                scheduler=None, config=config, device=dev)
        t.published = {}
        t._publish = t.published.update
        return t

    m, opt, ema = _fresh(decay=0.9)
    tr = trainer_of(m, opt)
    assert tr.ema is ema
    for i in range(3):
        tr._train_step(batches[i % 2])
    before, avg = opt.flat_p.clone(), ema.flat.clone()
    tr._evaluate()
    assert torch.equal(opt.flat_p, before) and torch.equal(ema.flat, avg) and m.training
    on_avg = dict(tr.published)
    opt.ema = None                                   # the same pass on the raw weights
    tr._evaluate()
    opt.ema = ema
    assert set(on_avg) == set(tr.published) == {"eval/loss", "eval/mel_loss", "eval/dur_loss"}
    assert on_avg["eval/loss"] != tr.published["eval/loss"] and np.isfinite(on_avg["eval/loss"])
    with ema.applied():                              # ... and the published numbers are the averaged weights'
        m.eval()
        with torch.no_grad():
            want = float(m(text=batches[0][0], text_lengths=batches[0][1], speech=batches[0][2], speech_lengths=batches[0][3])[1]["loss"])
        m.train()
    raw_loss = tr.published["eval/loss"]
    print(f"eval/loss on the average {on_avg['eval/loss']:.6f}, recomputed {want:.6f}, on the raw weights {raw_loss:.6f}")
    assert abs(on_avg["eval/loss"] - want) <= 0.01 * abs(on_avg["eval/loss"] - raw_loss)
    path = tmp_path / "checkpoint-3steps.pkl"
    tr.save_checkpoint(str(path))
    sd = torch.load(path, map_location="cpu")
    assert set(sd) == {"model", "optimizer", "steps", "epochs", "ema"} and sd["ema"]["updates"] == 3
    assert set(sd["ema"]["model"]) == set(sd["model"])
    # resumed into a fresh run with the key
    m2, opt2, ema2 = _fresh(decay=0.9)
    tr2 = trainer_of(m2, opt2)
    tr2.load_checkpoint(str(path))
    n = opt.eng.numel
    assert ema2.updates == 3 and torch.equal(ema2.flat[:n], ema.flat[:n]) and torch.equal(opt2.flat_p[:n], opt.flat_p[:n])
    # a checkpoint without the entry: the average starts over from the loaded parameters, and the log says so
    plain = tmp_path / "plain.pkl"
    torch.save({k: v for k, v in sd.items() if k != "ema"}, plain)
    with caplog.at_level(logging.WARNING):
        tr2.load_checkpoint(str(plain))
    assert ema2.updates == 0 and torch.equal(ema2.flat[:n], opt2.flat_p[:n]) and "ema" in caplog.text
    # a run without the key ignores the entry and writes the reference's key set
    m3, opt3, ema3 = _fresh()
    opt3.ema = None
    tr3 = trainer_of(m3, opt3)
    tr3.load_checkpoint(str(path))
    tr3.save_checkpoint(str(tmp_path / "again.pkl"))
    assert set(torch.load(tmp_path / "again.pkl", map_location="cpu")) == {"model", "optimizer", "steps", "epochs"}


def test_cli_trains_resumes_and_synthesises_with_the_average(tmp_path):
    """python -m efficient_tts_amd.bin.train with `ema_decay: 0.9` (in the manner of test_cli_trains_and_resumes_with_the_new_optimizers),
    graphed, with an evaluation at steps 3 and 6; then bin/inference --use_ema on the result"""
    import yaml
    from efficient_tts_amd.bin.inference import main as synthesise
    from efficient_tts_amd.bin.train import main
    model_params = dict(num_symbols=76, dropout_rate=0.0, use_masking=True, use_weighted_masking=False, sigma=0.01)
    cfg = dict(dataset_type="SyntheticTextAudio", dataset_params=dict(n_items=12, min_phones=8, max_phones=16),
               collate_fn_type="TextMelCollate", model_name="EfficientTTSCNN", model_params=model_params,
               batch_size=4, pin_memory=False, num_workers=0, optimizer_type="RAdam",
               optimizer_params=dict(lr=1.0e-3, betas=[0.9, 0.99], eps=1.0e-9, weight_decay=1.0e-5), grad_norm=1.0,
               scheduler_type="WarmupLR", scheduler_params=dict(warmup_steps=4000), train_max_steps=6, save_interval_steps=3,
               eval_interval_steps=3, log_interval_steps=2, bucket_frames=32, bucket_phones=8, graph_steps=True, ema_decay=0.9)
    path, plain_path = tmp_path / "c.yaml", tmp_path / "plain.yaml"
    out, out2, out3 = tmp_path / "exp", tmp_path / "exp2", tmp_path / "exp3"
    with open(path, "w") as f:
        yaml.dump(cfg, f)
    with open(plain_path, "w") as f:
        yaml.dump({k: v for k, v in dict(cfg, train_max_steps=3).items() if k != "ema_decay"}, f)
    assert main(["--outdir", str(out), "--config", str(path), "--verbose", "0"]) == 0
    ck3, ck6 = out / "checkpoint-3steps.pkl", out / "checkpoint-6steps.pkl"
    sd3, sd6 = torch.load(ck3, map_location="cpu"), torch.load(ck6, map_location="cpu")
    assert set(sd6) == {"model", "optimizer", "scheduler", "steps", "epochs", "ema"} and sd6["steps"] == 6
    assert set(sd6["ema"]) == {"decay", "warmup", "updates", "model"}
    assert (sd6["ema"]["decay"], sd6["ema"]["warmup"], sd6["ema"]["updates"], sd3["ema"]["updates"]) == (0.9, True, 6, 3)
    assert list(sd6["ema"]["model"]) == list(sd6["model"])
    assert all(torch.isfinite(v).all() for v in sd6["ema"]["model"].values())
    assert all(v.shape == sd6["model"][k].shape for k, v in sd6["ema"]["model"].items())
    assert any(not torch.equal(sd6["ema"]["model"][k], sd6["model"][k]) for k in sd6["model"])
    # resumed from step 3
    assert main(["--outdir", str(out2), "--config", str(path), "--verbose", "0", "--resume", str(ck3)]) == 0
    sd2 = torch.load(out2 / "checkpoint-6steps.pkl", map_location="cpu")
    assert sd2["steps"] == 6 and sd2["ema"]["updates"] == 6 and not (out2 / "checkpoint-3steps.pkl").exists()
    # the same recipe without the key: the reference's five keys
    assert main(["--outdir", str(out3), "--config", str(plain_path), "--verbose", "0"]) == 0
    assert set(torch.load(out3 / "checkpoint-3steps.pkl", map_location="cpu")) == {"model", "optimizer", "scheduler", "steps", "epochs"}
    # synthesis: the mels of the averaged weights differ from the raw weights'.  (A few frames per phoneme from six steps of training: the
    # duration predictor's output bias is set in both entries, as tests/test_cli_data.py sets it.)
    for entry in (sd6["model"], sd6["ema"]["model"]):
        entry["duration_predictor.linear.bias"].fill_(1.5)
    syn = tmp_path / "syn"
    syn.mkdir()
    torch.save(sd6, syn / "checkpoint-6steps.pkl")
    phones = ["_"] + [f"P{i}" for i in range(1, 76)]
    (tmp_path / "phn.txt").write_text("\n".join(phones) + "\n")
    rng = np.random.default_rng(1)
    lines = [f"DUMMY/utt{n}.wav|" + " ".join(phones[int(i)] for i in rng.integers(1, 76, size=k)) for n, k in enumerate((9, 14))]
    (tmp_path / "test.txt").write_text("\n".join(lines) + "\n")
    with open(syn / "config.yml", "w") as f:
        yaml.dump(dict(model_name="EfficientTTSCNN", model_params=model_params, dataset_params=dict(use_phnseq=True, phnset_path=str(tmp_path / "phn.txt"))), f)
    base = ["--checkpoint", str(syn / "checkpoint-6steps.pkl"), "--test_fid_scp", str(tmp_path / "test.txt"), "--verbose", "0", "--no_vocoder"]
    assert synthesise(base + ["--outdir", str(tmp_path / "raw")]) == 0
    assert synthesise(base + ["--outdir", str(tmp_path / "avg"), "--use_ema"]) == 0
    for n in range(2):
        raw, avg = np.load(tmp_path / "raw" / f"utt{n}_6steps.npy"), np.load(tmp_path / "avg" / f"utt{n}_6steps.npy")
        assert raw.shape[1] == avg.shape[1] == 80 and raw.shape[0] > 0 and avg.shape[0] > 0 and np.isfinite(avg).all()
        assert raw.shape != avg.shape or not np.array_equal(raw, avg)
    # a checkpoint without the entry is refused, and the message says what would have written one
    torch.save({k: v for k, v in sd6.items() if k != "ema"}, syn / "checkpoint-6steps.pkl")
    with pytest.raises(ValueError, match="ema_decay"):
        synthesise(base + ["--outdir", str(tmp_path / "none"), "--use_ema"])
