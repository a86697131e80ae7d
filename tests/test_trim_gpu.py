"""GPU (-m gpu): the silence trimmer (efficient_tts_amd/trim.py, csrc/efts_trim.hip) against the numpy restatement of its definition in
tests/trim_reference.py, which never sees the product's code.

Nothing here has a tolerance.  int16: energies are integers and the decision is one fp64 multiply and compare, so bounds, gain and every
output sample are compared with ==.  fp32: tests/test_trim_cpu.py asserts that every frame of these inputs is at least 0.01 dB from the
threshold, ten times what any order of an fp32 sum of 2048 squares can be off by, so the bounds are compared with == as well, and the
samples bit for bit with float32(x) * g, g from the reference's exact peak.  Outputs are pre-filled with a sentinel; the padding behind
every item is full scale and the row behind the longest item is loud throughout.
"""
import numpy as np
import pytest
import torch

import trim_reference as R
from efficient_tts_amd import lib as L
from efficient_tts_amd.trim import SilenceTrimmer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    L.load()
    L.require_device()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def inputs():
    out = {np.int16: R.items(np.int16), np.float32: R.items(np.float32)}
    for v in out.values():
        v.setflags(write=False)
    return out


def _call(dev, x, lengths, W, H, top_db, keep_frames, peak, ld_out):
    """efts_trim / efts_trim_pcm16 through the binding; every output is pre-filled with a sentinel.  Returns the return code as well."""
    lib = L.load()
    xd = torch.from_numpy(np.array(x)).to(dev).contiguous()
    B, ld_in = xd.shape
    pcm = xd.dtype == torch.int16
    li = torch.tensor(lengths, dtype=torch.int32, device=dev)
    out = torch.full((B, ld_out), 7.0, dtype=torch.float32, device=dev)
    new_len = torch.full((B,), -1, dtype=torch.int32, device=dev)
    start = torch.full((B,), -1, dtype=torch.int32, device=dev)
    gain = torch.full((B,), -1.0, dtype=torch.float32, device=dev)
    ws = torch.empty(max(16, int(lib.efts_trim_workspace_bytes(B, ld_in, H, int(pcm)))), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    head = (xd.data_ptr(), ld_in, li.data_ptr(), W, H, R.ratio(top_db), keep_frames, 0.0 if peak is None else peak)
    tail = (out.data_ptr(), ld_out, new_len.data_ptr(), start.data_ptr(), gain.data_ptr(), ws.data_ptr(), B, st)
    rc = lib.efts_trim_pcm16(*head, 1.0 / 32768.0, *tail) if pcm else lib.efts_trim(*head, *tail)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), new_len.cpu().numpy(), start.cpu().numpy(), gain.cpu().numpy()


@pytest.mark.parametrize("peak", [0.95, None])
@pytest.mark.parametrize("W,H", R.PAIRS)
@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_equals_the_reference(dev, inputs, dtype, W, H, peak):
    x = inputs[dtype]
    ld_out = R.LD_IN + (5 if peak else 6)                           # 4008: rows 16-byte aligned; 4009: not
    rc, out, new_len, start, gain = _call(dev, x, R.LENGTHS, W, H, R.TOP_DB, 0, peak, ld_out)
    assert rc == 0
    for b, n in enumerate(R.LENGTHS):
        ref = R.trim(x[b, :n], W=W, H=H, top_db=R.TOP_DB, keep_frames=0, peak=peak)
        print(f"{np.dtype(dtype).name} W {W} H {H} peak {peak} item {b} len {n}: start {start[b]} ({ref['start']}) new_len {new_len[b]} "
              f"({ref['new_len']}) gain {gain[b]!r} ({ref['gain']!r})")
        assert (int(start[b]), int(new_len[b])) == (ref["start"], ref["new_len"])
        assert gain[b].view(np.uint32) == ref["gain"].view(np.uint32)
        assert np.array_equal(out[b, :ref["new_len"]].view(np.uint32), ref["out"].view(np.uint32))
        assert np.array_equal(out[b, ref["new_len"]:].view(np.uint32), np.zeros(ld_out - ref["new_len"], np.uint32))   # +0.0, up to ld_out


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_other_thresholds_and_keep_frames(dev, inputs, dtype):
    """30 dB cuts the 35 dB items as well, 50 dB cuts nothing; keep_frames 0 and one that clamps at both ends"""
    x = inputs[dtype]
    for top_db, keep in R.OTHER:
        rc, out, new_len, start, gain = _call(dev, x, R.LENGTHS, 1024, 256, top_db, keep, 1.0, R.LD_IN)
        assert rc == 0
        for b, n in enumerate(R.LENGTHS):
            ref = R.trim(x[b, :n], top_db=top_db, keep_frames=keep, peak=1.0)
            assert (int(start[b]), int(new_len[b]), gain[b].view(np.uint32)) == (ref["start"], ref["new_len"], ref["gain"].view(np.uint32))
            assert np.array_equal(out[b, :ref["new_len"]].view(np.uint32), ref["out"].view(np.uint32)) and not out[b, ref["new_len"]:].any()


@pytest.mark.parametrize("dtype", [torch.int16, torch.float32])
def test_items_alone_elsewhere_and_again(dev, inputs, dtype):
    x = torch.from_numpy(np.array(inputs[np.int16 if dtype == torch.int16 else np.float32])).to(dev)
    lengths = torch.tensor(R.LENGTHS)
    for W, H in ((1024, 256), (1024, 200)):
        t = SilenceTrimmer(dev, W, H, peak=0.95)
        batch = t(x, lengths, return_bounds=True)
        again = t(x, lengths, return_bounds=True)
        assert all(torch.equal(a, b) for a, b in zip(batch, again))
        assert batch[0].shape == x.shape and batch[1].dtype == batch[2].dtype == torch.int64 and batch[3].dtype == torch.float32
        order = [3, 5, 0, 4, 1, 2]                                   # every item at another position, behind another neighbour
        moved = t(x[order], lengths[order], return_bounds=True)
        for pos, b in enumerate(order):
            assert all(torch.equal(m[pos], a[b]) for m, a in zip(moved, batch))
        for b, n in enumerate(R.LENGTHS):
            alone = t(x[b:b + 1, :max(n, 1)].contiguous(), lengths[b:b + 1], return_bounds=True)        # its own row length: another T_max
            assert torch.equal(alone[0][0], batch[0][b, :max(n, 1)]) and all(torch.equal(a[0], c[b]) for a, c in zip(alone[1:], batch[1:]))


def test_nothing_switched_on_is_the_identity(dev, inputs):
    lengths = torch.tensor(R.LENGTHS)
    keep = torch.arange(R.LD_IN)[None, :] < lengths[:, None]
    t = SilenceTrimmer(dev, trim=False)
    pcm = torch.from_numpy(np.array(inputs[np.int16]))
    out, n, start, gain = t(pcm.to(dev), lengths, return_bounds=True)
    assert torch.equal(n.cpu(), lengths) and not start.any()
    assert torch.equal(out.cpu(), torch.where(keep, pcm.to(torch.float32) * (1.0 / 32768.0), torch.zeros(())))
    assert gain.cpu().tolist() == [1.0 / 32768.0 if v else 1.0 for v in R.LENGTHS]
    f = torch.from_numpy(np.array(inputs[np.float32]))
    out, n = t(f.to(dev), lengths)
    assert torch.equal(n.cpu(), lengths) and torch.equal(out.cpu(), torch.where(keep, f, torch.zeros(())))
    out, n = t(f.to(dev))                                          # no lengths: whole rows
    assert n.tolist() == [R.LD_IN] * len(R.LENGTHS) and torch.equal(out.cpu(), f)
    # normalisation alone: the bounds stay, the level is the reference's
    out, n, start, gain = SilenceTrimmer(dev, trim=False, peak=0.95)(pcm.to(dev), lengths, return_bounds=True)
    assert torch.equal(n.cpu(), lengths) and not start.any()
    for b, v in enumerate(R.LENGTHS):
        ref = R.trim(inputs[np.int16][b, :v], peak=0.95, trimming=False)
        assert gain[b].item() == float(ref["gain"]) and np.array_equal(out[b, :v].cpu().numpy(), ref["out"]) and not out[b, v:].any()


def test_refusal_before_any_launch(dev, inputs):
    rc, out, new_len, start, gain = _call(dev, inputs[np.int16], R.LENGTHS, 1024, 256, 40.0, 2, None, R.LD_IN - 1)
    assert rc == -2 and b"ld_out" in L.load().efts_last_error()                   # EFTS_ESHAPE
    assert (out == 7.0).all() and (new_len == -1).all() and (start == -1).all() and (gain == -1.0).all()
    rc = _call(dev, inputs[np.float32], R.LENGTHS, 1024, 256, 0.0, 2, None, R.LD_IN)[0]     # r = 1
    assert rc == -1                                                                # EFTS_EINVAL


def test_trainer_stage_runs_the_trimmer(dev):
    from efficient_tts_amd.datasets import SyntheticTextAudio, TextMelCollate
    from efficient_tts_amd.frontend import LogMelFrontend
    from efficient_tts_amd.trainer import EfficientTTSTrainer
    cfg = dict(outdir="/tmp", log_interval_steps=5, eval_interval_steps=0, save_interval_steps=10, train_max_steps=20, grad_norm=1.0,
               bucket_frames=0, bucket_phones=0)
    t = EfficientTTSTrainer(steps=0, epochs=0, data_loader={}, sampler={}, model=torch.nn.Linear(2, 2), optimizer=None, scheduler=None, config=cfg,
                            device=dev)
    t.frontend = LogMelFrontend(dev)
    ds = SyntheticTextAudio(n_items=3, min_phones=6, max_phones=12)
    silence = torch.zeros(2048, dtype=torch.int16)
    batch = TextMelCollate()([(text, torch.cat([silence, audio, silence])) for text, audio in ds])
    text, text_lengths, audio, lengths = batch
    # the keys absent: today's path
    assert t.trimmer is None
    mel0, ml0 = t._stage(batch)[2:]
    ref0, rl0 = t.frontend(audio, lengths)
    assert torch.equal(mel0, ref0) and torch.equal(ml0, rl0)
    # trim_silence: true
    from efficient_tts_amd.bin.train import build_trimmer
    t.trimmer = build_trimmer(dict(cfg, trim_silence=True), dev)
    out = t._stage(batch)
    cut = np.zeros(tuple(audio.shape), dtype=np.float32)
    new_len = []
    for b in range(audio.shape[0]):
        ref = R.trim(audio[b, :int(lengths[b])].numpy())
        assert 0 < ref["start"] <= 2048 and ref["start"] + ref["new_len"] < int(lengths[b])   # silence went at both ends
        cut[b, :ref["new_len"]] = ref["out"]
        new_len.append(ref["new_len"])
    new_len = torch.tensor(new_len)
    assert torch.equal(out[3].cpu(), t.frontend.frames_of(new_len))
    ref_mel, ref_frames = t.frontend(torch.from_numpy(cut).to(dev), new_len)
    assert torch.equal(out[2], ref_mel) and torch.equal(out[3], ref_frames) and out[2].shape[1] < mel0.shape[1]
    assert torch.equal(out[0].cpu(), text) and torch.equal(out[1].cpu(), text_lengths)
