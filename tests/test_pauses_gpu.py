"""GPU (-m gpu): the pause shortener (efficient_tts_amd/pauses.py, csrc/efts_pauses.hip) against the numpy restatement of its definition in
tests/pauses_reference.py, which never sees the product's code.

The plan has no tolerance: lengths, removed samples, pause counts and chunk_src are compared with ==.  int16 energies are integers; for the
fp32 items every test first asserts, on the CPU, that every frame lies at least 0.01 dB from the threshold by the reference's report -- far
more than any order of an fp32 sum of 2048 squares can be off by -- so the summation order cannot flip a decision.  Every output sample
outside a fade has the bits of its source sample (int16: of float32(sample) * float32(1 / 32768)), every sample behind new_len is +0.0.
A fade sample is one correctly rounded fma of the reference's own fp32 operands, the reference holds the same expression in float64: the
bound is 2^-24 |ref| + 2^-149, half an ulp of the result and the smallest subnormal.

Measured on an MI355X (profiles/pauses_error.json; EFTS_WRITE_PROFILES=1 merges the figures of a run into it): of the fade samples of all
cases none differs from the bits of the rounded reference.
"""
import json
import os

import numpy as np
import pytest
import torch

import pauses_reference as R
from efficient_tts_amd import lib as L
from efficient_tts_amd.pauses import PauseShortener

pytestmark = pytest.mark.gpu

SETTINGS = {(1024, 256): 7, (512, 64): 8}        # (W, H) -> items of R.LENGTHS in the batch: the 70 000-sample item runs at H = 64 alone
CASES = [(W, H, M, F) for (W, H) in SETTINGS for M in (1, 2, 7) for F in sorted({0, 64, H})]
PROFILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "pauses_error.json")


@pytest.fixture(scope="module")
def dev():
    L.load()
    L.require_device()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def inputs():
    """{(W, H, dtype): (x [count, n], lengths)}, read-only; the fp32 items' margin from the threshold is asserted here, before any comparison"""
    tile = R.plan_tile()
    out = {}
    for (W, H), count in SETTINGS.items():
        for dtype in (np.int16, np.float32):
            x, lengths = R.batch(W, H, dtype, tile, count)
            x.setflags(write=False)
            out[W, H, dtype] = (x, lengths)
        x, lengths = out[W, H, np.float32]
        for b, n in enumerate(lengths):
            margin = R.sound_flags(x[b, :n], W, H)[1]
            print(f"W {W} H {H} item {b} len {n}: fp32 margin {margin:.3f} dB")
            assert margin >= 0.01
    return out


def _shortener(dev, W, H, M, F, **kw):
    s = PauseShortener(dev, R.RATE, max_pause_ms=M * H * 1000.0 / R.RATE, frame_length=W, hop_size=H, top_db=R.TOP_DB, fade=F, **kw)
    assert s.chunks == M
    return s


def _run(s, x, lengths, dev):
    out, new_len, stats = s(torch.from_numpy(np.array(x)).to(dev), torch.tensor(lengths), return_stats=True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), new_len.cpu().numpy(), {k: v.cpu().numpy() for k, v in stats.items()}


def _record(case, fades, off):
    if not os.environ.get("EFTS_WRITE_PROFILES"):
        return
    report = {}
    if os.path.exists(PROFILE):
        with open(PROFILE) as f:
            report = json.load(f)
    report.setdefault("cases", {})[case] = {"fade_samples": int(fades), "not_the_bits_of_the_rounded_reference": int(off)}
    report["inputs"] = "tests/pauses_reference.py batch(): lengths (0, 1, 255, 256, 257, 12345, 40000) and at H = 64 also 70000"
    report["bound"] = "2^-24 |ref| + 2^-149 on fade samples; every other sample and every plan word: =="
    with open(PROFILE, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("W,H,M,F", CASES)
@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_equals_the_reference(dev, inputs, dtype, W, H, M, F):
    x, lengths = inputs[W, H, dtype]
    n_row = x.shape[1]
    t_max = -(-n_row // H)
    out, new_len, stats = _run(_shortener(dev, W, H, M, F), x, lengths, dev)
    assert out.shape == x.shape and out.dtype == np.float32 and stats["chunk_src"].shape == (len(lengths), t_max)
    fades = off = cut = 0
    for b, n in enumerate(lengths):
        ref = R.shorten(x[b, :n], W=W, H=H, top_db=R.TOP_DB, M=M, F=F)
        cut += ref["pauses"]
        assert (int(new_len[b]), int(stats["removed"][b]), int(stats["pauses"][b])) == (ref["new_len"], ref["removed"], ref["pauses"])
        assert stats["chunk_src"][b].tolist() == ref["chunk_src"] + [-1] * (t_max - len(ref["chunk_src"]))
        got, plain = out[b, :ref["new_len"]], ~ref["is_fade"]
        assert np.array_equal(got[plain].view(np.uint32), ref["out"][plain].astype(np.float32).view(np.uint32))
        assert not out[b, ref["new_len"]:].view(np.uint32).any()                # +0.0, up to the end of the row
        want = ref["out"][ref["is_fade"]]
        err = np.abs(got[ref["is_fade"]].astype(np.float64) - want)
        assert (err <= 2.0 ** -24 * np.abs(want) + 2.0 ** -149).all()
        fades += want.size
        off += int((got[ref["is_fade"]].view(np.uint32) != want.astype(np.float32).view(np.uint32)).sum())
        assert want.size == ref["pauses"] * F
    assert cut >= 4                                                             # (the case did shorten something)
    print(f"{np.dtype(dtype).name} W {W} H {H} M {M} F {F}: {cut} pauses cut, {fades} fade samples, {off} not the bits of the rounded reference")
    _record(f"{np.dtype(dtype).name} W{W} H{H} M{M} F{F}", fades, off)


@pytest.mark.parametrize("W,H", list(SETTINGS))
def test_int16_plans_as_its_fp32_twin(dev, inputs, W, H):
    for M in (1, 2, 7):
        s = _shortener(dev, W, H, M, 64)
        a = _run(s, *inputs[W, H, np.int16], dev)
        b = _run(s, *inputs[W, H, np.float32], dev)
        assert np.array_equal(a[1], b[1]) and all(np.array_equal(a[2][k], b[2][k]) for k in ("removed", "pauses", "chunk_src"))
        assert a[2]["removed"].sum() > 0


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_items_alone_elsewhere_and_again(dev, inputs, dtype):
    W, H = 512, 64
    x, lengths = inputs[W, H, dtype]
    x, lengths = torch.from_numpy(np.array(x)).to(dev), torch.tensor(lengths)
    s = _shortener(dev, W, H, 2, 64)

    def call(xs, ls):
        out, new_len, stats = s(xs, ls, return_stats=True)
        return out, new_len, stats["removed"], stats["pauses"], stats["chunk_src"]

    batch, again = call(x, lengths), call(x, lengths)
    assert all(torch.equal(a, b) for a, b in zip(batch, again))
    order = [3, 7, 0, 6, 1, 2, 4, 5]                                            # every item at another position, behind another neighbour
    moved = call(x[order], lengths[order])
    for pos, b in enumerate(order):
        assert all(torch.equal(m[pos], a[b]) for m, a in zip(moved, batch))
    for b, n in enumerate(lengths.tolist()):
        row = max(n, 1)                                                         # its own row length: another T_max, rows of 12 345 are not 16-byte aligned
        alone = call(x[b:b + 1, :row].contiguous(), lengths[b:b + 1])
        assert torch.equal(alone[0][0], batch[0][b, :row]) and all(torch.equal(a[0], c[b]) for a, c in zip(alone[1:4], batch[1:4]))
        t = alone[4].shape[1]
        assert torch.equal(alone[4][0], batch[4][b, :t]) and (batch[4][b, t:] == -1).all()
        behind = x[b:b + 1].clone()                                             # whatever lies behind it
        behind[:, n:] = 0
        assert all(torch.equal(a[0], c[b]) for a, c in zip(call(behind, lengths[b:b + 1]), batch))


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_graph_replay_gives_the_eager_bits(dev, inputs, dtype):
    W, H = 1024, 256
    x, lengths = inputs[W, H, dtype]
    x, lengths = torch.from_numpy(np.array(x)).to(dev), torch.tensor(lengths).to(dev)
    s = _shortener(dev, W, H, 2, 64)
    eager = s(x, lengths, return_stats=True)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        s(x, lengths)                                                           # (tables and workspace exist before the capture)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = s(x, lengths, return_stats=True)
    for t in (held[0], held[1], *held[2].values()):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(held[0], eager[0]) and torch.equal(held[1], eager[1]) and all(torch.equal(held[2][k], eager[2][k]) for k in eager[2])
    assert eager[2]["removed"].sum().item() > 0


@pytest.mark.parametrize("W,H", list(SETTINGS))
def test_a_limit_no_run_exceeds_is_the_identity(dev, inputs, W, H):
    s = PauseShortener(dev, R.RATE, max_pause_ms=60000.0, frame_length=W, hop_size=H, fade=64)
    for dtype in (np.int16, np.float32):
        x, lengths = inputs[W, H, dtype]
        out, new_len, stats = _run(s, x, lengths, dev)
        keep = np.arange(x.shape[1])[None, :] < np.array(lengths)[:, None]
        want = x.astype(np.float32) * np.float32(1.0 / 32768.0) if dtype == np.int16 else x
        assert np.array_equal(out.view(np.uint32), np.where(keep, want, np.float32(0.0)).view(np.uint32))
        assert new_len.tolist() == list(lengths) and not stats["removed"].any() and not stats["pauses"].any()
        for b, n in enumerate(lengths):
            t = -(-n // H)
            assert stats["chunk_src"][b, :t].tolist() == list(range(t)) and (stats["chunk_src"][b, t:] == -1).all()


def test_refusal_before_any_launch(dev, inputs):
    lib = L.load()
    x, lengths = inputs[1024, 256, np.float32]
    xd = torch.from_numpy(np.array(x)).to(dev)
    B, n = xd.shape
    li = torch.tensor(lengths, dtype=torch.int32, device=dev)
    out = torch.full((B, n), 7.0, device=dev)
    res = torch.full((3, B), -5, dtype=torch.int32, device=dev)
    src = torch.full((B, -(-n // 256)), -5, dtype=torch.int32, device=dev)
    table = torch.from_numpy(R.fade_table(64)).to(dev)
    ws = torch.empty(int(lib.efts_pauses_workspace_bytes(B, n, 256, 0)), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def call(W=1024, H=256, r=R.ratio(40.0), M=2, F=64, fade=table.data_ptr(), ld_out=n):
        return lib.efts_pauses(xd.data_ptr(), n, li.data_ptr(), W, H, r, M, F, fade, out.data_ptr(), ld_out, res[0].data_ptr(), res[1].data_ptr(),
                               res[2].data_ptr(), src.data_ptr(), ws.data_ptr(), B, st)

    assert call(M=0) == -2 and call(F=257) == -2 and call(F=-1) == -2 and call(W=1000) == -2 and call(H=255) == -2 and call(ld_out=n - 1) == -2   # EFTS_ESHAPE
    assert call(fade=None) == -1 and call(r=1.0) == -1                                                                                  # EFTS_EINVAL
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (res == -5).all() and (src == -5).all()
    assert call(F=0, fade=None) == 0                                             # no table without a fade
    torch.cuda.synchronize()
    assert res[0].tolist() == [R.shorten(x[b, :v], M=2, F=0)["new_len"] for b, v in enumerate(lengths)]


def test_trainer_stage_runs_the_shortener(dev):
    from efficient_tts_amd.bin.train import build_pauses
    from efficient_tts_amd.datasets import SyntheticTextAudio, TextMelCollate
    from efficient_tts_amd.frontend import LogMelFrontend
    from efficient_tts_amd.trainer import EfficientTTSTrainer
    cfg = dict(outdir="/tmp", log_interval_steps=5, eval_interval_steps=0, save_interval_steps=10, train_max_steps=20, grad_norm=1.0,
               bucket_frames=0, bucket_phones=0)
    t = EfficientTTSTrainer(steps=0, epochs=0, data_loader={}, sampler={}, model=torch.nn.Linear(2, 2), optimizer=None, scheduler=None, config=cfg,
                            device=dev)
    t.frontend = LogMelFrontend(dev)
    ds = SyntheticTextAudio(n_items=3, min_phones=6, max_phones=12)
    silence = torch.zeros(11025, dtype=torch.int16)                             # half a second in the middle of every item
    batch = TextMelCollate()([(text, torch.cat([audio[:audio.shape[0] // 2], silence, audio[audio.shape[0] // 2:]])) for text, audio in ds])
    text, text_lengths, audio, lengths = batch
    # the key absent: today's path
    assert t.pauses is None
    mel0, ml0 = t._stage(batch)[2:]
    ref0, rl0 = t.frontend(audio, lengths)
    assert torch.equal(mel0, ref0) and torch.equal(ml0, rl0)
    # max_pause_ms: 100
    t.pauses = build_pauses(dict(cfg, max_pause_ms=100), dev)
    out = t._stage(batch)
    short, short_len, stats = PauseShortener(dev, 22050, max_pause_ms=100.0)(audio.to(dev), lengths, return_stats=True)
    assert (stats["pauses"] >= 1).all() and (stats["removed"] >= 11025 - 256 * (t.pauses.chunks + 6)).all()
    for b in range(audio.shape[0]):
        ref = R.shorten(audio[b, :int(lengths[b])].numpy(), M=t.pauses.chunks)
        assert int(short_len[b]) == ref["new_len"] and int(stats["removed"][b]) == ref["removed"]
    ref_mel, ref_frames = t.frontend(short, short_len)
    assert torch.equal(out[2], ref_mel) and torch.equal(out[3], ref_frames) and out[2].shape[1] < mel0.shape[1]
    assert torch.equal(out[0].cpu(), text) and torch.equal(out[1].cpu(), text_lengths)
