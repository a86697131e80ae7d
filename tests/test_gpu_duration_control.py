"""GPU (-m gpu): duration control of free-running synthesis (length_scale / durations / target_frames / return_durations of
inference() and inference_batch(), the efts_duration_control kernel) and phoneme timings of recordings (align()), against the
oracle's inference(forced_delta=...) and forward()."""
import os

import numpy as np
import pytest
import torch

from oracle import efts_oracle as O

pytestmark = pytest.mark.gpu

# the bounds of test_inference_matches_reference_golden per precision: (mel max-abs, reconst_alpha max-abs)
BOUNDS = {"bf16x3": (1e-3, 1e-4), "fp32": (1e-4, 1e-5)}
SCALES = (0.5, 0.8, 1.25, 2.0)


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


_MODELS = {}


def _model(precision):
    if precision not in _MODELS:
        from efficient_tts_amd import EfficientTTSCNN
        from efficient_tts_amd import lib as L
        L.load()
        L.require_device()
        m = EfficientTTSCNN(num_symbols=76, dropout_rate=0.0, use_masking=True, use_weighted_masking=False, sigma=0.01, precision=precision)
        m.load_state_dict(O.fill_params())
        _MODELS[precision] = m.to(_dev()).eval()
    return _MODELS[precision]


@pytest.fixture(scope="module")
def params():
    return O.fill_params()


_ORACLE = {}


def _oracle(P, ids, key, forced=None):
    """oracle inference of ids [1, T1], cached by key (the predicted durations come from the key (n, None))"""
    if key not in _ORACLE:
        _ORACLE[key] = O.inference(P, ids, forced_delta=forced)
    return _ORACLE[key]


def _ids(g, n):
    return torch.from_numpy(g[f"ids{n}"])[None]


def _ragged(g, ns):
    seqs = [torch.from_numpy(g[f"ids{n}"]) for n in ns]
    text = torch.zeros(len(seqs), max(len(s) for s in seqs), dtype=torch.int64)
    for i, s in enumerate(seqs):
        text[i, :len(s)] = s
    return text, torch.tensor([len(s) for s in seqs])


# ------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize("T1", [37, 256, 700])
@pytest.mark.parametrize("method1", [True, False])
def test_kernel_without_controls_equals_duration_positions(T1, method1):
    from efficient_tts_amd import ops as P
    _model("bf16x3")
    dev = _dev()
    gen = torch.Generator().manual_seed(T1)
    B, ld = 5, T1 + 9
    dur = (torch.rand(B, ld, generator=gen) * 7).to(dev)
    tl = torch.tensor([T1, T1 // 2, 1, T1 - 3, 2], dtype=torch.int32, device=dev)
    e0, m0 = torch.empty(B, T1, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    P.duration_positions(dur, ld, tl, None, method1, e0, m0, B, T1)
    for frames in (None, torch.empty(B, T1, dtype=torch.int32, device=dev)):
        for scale in (None, torch.ones(B, device=dev)):
            e1, m1 = torch.full((B, T1), -7.0, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
            P.duration_control(dur, ld, tl, scale, None, None, method1, e1, m1, frames, B, T1)
            assert torch.equal(e0, e1) and torch.equal(m0, m1)


@pytest.mark.parametrize("T1", [40, 300])
@pytest.mark.parametrize("method1", [True, False])
def test_kernel_controls_target_and_frames(T1, method1):
    from efficient_tts_amd import ops as P
    _model("bf16x3")
    dev = _dev()
    gen = torch.Generator().manual_seed(3 * T1 + method1)
    B = 4
    dur = torch.rand(B, T1, generator=gen) * 6
    tl = torch.tensor([T1, T1 - 5, 7, T1 // 3], dtype=torch.int32)
    scale = torch.tensor([0.5, 1.0, 2.0, 1.3])
    over = torch.full((B, T1), -1.0)
    over[:, ::3] = torch.randint(0, 9, (B, (T1 + 2) // 3), generator=gen).float()
    target = torch.tensor([1000, 17, 50, 333], dtype=torch.int32)
    valid = torch.arange(T1)[None, :] < tl[:, None].long()
    d = torch.where(over >= 0, over, dur) * scale[:, None] * valid
    for tgt in (None, target):
        e = torch.empty(B, T1, device=dev)
        ml = torch.empty(B, dtype=torch.int32, device=dev)
        fr = torch.empty(B, T1, dtype=torch.int32, device=dev)
        P.duration_control(dur.to(dev), T1, tl.to(dev), scale.to(dev), over.to(dev), None if tgt is None else tgt.to(dev), method1,
                           e, ml, fr, B, T1)
        e, ml, fr = e.cpu(), ml.cpu(), fr.cpu()
        C = torch.cumsum(d.double(), 1)                                        # inclusive positions E
        tot = C.gather(1, tl.long()[:, None] - 1)[:, 0]
        f = torch.ones(B, dtype=torch.float64)
        if tgt is not None:
            f = tgt.double() / tot                                             # cumsum(d) * target / sum(d)
            assert torch.equal(ml, tgt)
        else:
            assert torch.equal(ml, torch.round(tot).int())
        want = (C if method1 else C - d.double()) * f[:, None]
        for b in range(B):
            n = int(tl[b])
            assert float((e[b, :n].double() - want[b, :n]).abs().max()) <= 1e-5 * float(tot[b] * f[b]) + 1e-5, (b, tgt)
        assert torch.equal(fr.sum(1).int(), ml)                                # frames add up to the mel length
        assert int((fr * ~valid).abs().sum()) == 0                            # 0 past the text length
        if method1:                                                            # rounded-boundary differences of the returned e
            r = torch.round(e)
            host = torch.diff(r, dim=1, prepend=torch.zeros(B, 1)).int() * valid
            assert torch.equal(fr, host)


def _scan_starts(x):
    """fp32 model of the kernel's block scan at one token per thread (T1 <= 256): the start value of every thread's chunk,
    (base + incl) - loc, with wave_scan_incl's shuffle-up adds in their order (efts_internal.h)"""
    N, T = x.shape
    loc = np.zeros((N, 256), np.float32)
    loc[:, :T] = x
    v = loc.copy()
    for w in range(4):
        seg = v[:, 64 * w:64 * w + 64]
        o = 1
        while o < 64:
            t = seg.copy()
            seg[:, o:] = seg[:, o:] + t[:, :-o]
            o <<= 1
    base = np.zeros((N, 256), np.float32)
    for w in range(1, 4):
        acc = np.zeros(N, np.float32)
        for i in range(w):
            acc = acc + v[:, 64 * i + 63]
        base[:, 64 * w:64 * w + 64] = acc[:, None]
    return ((base + v) - loc)[:, :T]


@pytest.mark.parametrize("with_target", [False, True])
def test_kernel_frames_telescope_at_half_integer_boundaries(with_target):
    """Continuous durations, one token per thread: the scan's value of a chunk boundary and the previous thread's sequential running
    sum can differ by an ulp, and where the boundary sits on x.5 they round apart.  The frames must still add up to the mel length
    and equal the differences of the rounded positions e the kernel wrote, on the rows where those two values round apart too."""
    from efficient_tts_amd import ops as P
    _model("bf16x3")
    dev = _dev()
    gen = torch.Generator().manual_seed(11)
    B, T1 = 4096, 200
    dur = torch.exp(torch.randn(B, T1, generator=gen) * 0.6 + 1.3)
    x = dur.numpy().astype(np.float32)
    st = _scan_starts(x)
    split = (np.rint(st[:, 1:]) != np.rint(st[:, :-1] + x[:, :-1])).any(1)   # a boundary the two values round apart
    hazard = np.nonzero(split)[0]
    assert len(hazard) >= 3, "the fixture lost its half-integer boundaries"
    tl = torch.full((B,), T1, dtype=torch.int32, device=dev)
    e = torch.empty(B, T1, device=dev)
    ml = torch.empty(B, dtype=torch.int32, device=dev)
    fr = torch.empty(B, T1, dtype=torch.int32, device=dev)
    tgt = torch.randint(200, 3000, (B,), generator=gen, dtype=torch.int32) if with_target else None
    P.duration_control(dur.to(dev), T1, tl, None, None, None if tgt is None else tgt.to(dev), True, e, ml, fr, B, T1)
    e, ml, fr = e.cpu(), ml.cpu(), fr.cpu()
    if tgt is not None:
        assert torch.equal(ml, tgt)
    else:
        assert torch.equal(ml, torch.round(e[:, -1]).int())
    assert torch.equal(fr.sum(1).int(), ml)
    host = torch.diff(torch.round(e), dim=1, prepend=torch.zeros(B, 1)).int()
    assert torch.equal(fr, host)
    assert torch.equal(fr[hazard], host[hazard]) and int(fr.min()) >= 0


def test_kernel_rejects_bad_items():
    from efficient_tts_amd import ops as P
    _model("bf16x3")
    dev = _dev()
    B, T1 = 3, 12
    dur = torch.ones(B, T1, device=dev)
    tl = torch.tensor([12, 12, 12], dtype=torch.int32, device=dev)
    e, ml = torch.empty(B, T1, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    fr = torch.empty(B, T1, dtype=torch.int32, device=dev)
    P.duration_control(dur, T1, tl, torch.tensor([1.0, 0.0, float("inf")], device=dev), None, None, True, e, ml, fr, B, T1)
    assert ml.tolist() == [12, -1, -1] and int(fr[1:].abs().sum()) == 0
    P.duration_control(dur * torch.tensor([[1.0], [0.0], [1.0]], device=dev), T1, tl, None, None,
                       torch.tensor([5, 5, 0], dtype=torch.int32, device=dev), True, e, ml, fr, B, T1)
    assert ml.tolist() == [5, -1, -1]
    over = torch.full((B, T1), 2.0, device=dev)
    over[2, 4] = -1.0                                                          # no prediction to fall back on
    P.duration_control(None, 0, tl, None, over, None, True, e, ml, fr, B, T1)
    assert ml.tolist() == [24, 24, -1]
    # a finite scale whose total does not fit the int32 mel length is rejected, not converted
    P.duration_control(dur, T1, tl, torch.tensor([1.0, 1e12, 3e38], device=dev), None, None, True, e, ml, fr, B, T1)
    assert ml.tolist() == [12, -1, -1] and int(fr[1:].abs().sum()) == 0
    m = _model("bf16x3")
    text = torch.ones(2, 9, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="rejected"):
        m.inference_batch(text, torch.tensor([9, 9], device=dev), length_scale=torch.tensor([1.0, 0.0], device=dev))


# ------------------------------------------------------------------ model API
def test_default_path_unchanged(golden_dir):
    g = _golden(golden_dir, "inference_lj")
    dev = _dev()
    m = _model("bf16x3")
    ids = _ids(g, 1).to(dev)
    for _ in range(3):                                                    # eager, capture, replay
        a = m.inference(ids)
        b = m.inference(ids, length_scale=1.0)
        c = m.inference(ids, length_scale=torch.ones(1), return_durations=True)   # the control kernel with a scale of 1
        for x, y, z in zip(a, b, c):
            assert torch.equal(x, y) and torch.equal(x, z)
        assert int(c[2].sum()) == a[0].shape[1]
    text, lens = _ragged(g, range(5))
    text, lens = text.to(dev), lens.to(dev)
    for _ in range(3):
        a = m.inference_batch(text, lens)
        b = m.inference_batch(text, lens, length_scale=1.0)
        c = m.inference_batch(text, lens, length_scale=torch.ones(5, device=dev), durations=-torch.ones(text.shape), return_durations=True)
        for x, y, z in zip(a, b, c):
            assert torch.equal(x, y) and torch.equal(x, z)
        assert torch.equal(c[3].sum(1), a[1])


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_length_scale_matches_oracle(golden_dir, params, precision):
    g = _golden(golden_dir, "inference_lj")
    dev = _dev()
    m = _model(precision)
    tol_mel, tol_alpha = BOUNDS[precision]
    for n in range(10):
        ids = _ids(g, n)
        delta = _oracle(params, ids, (n, None))["delta"]
        for s in SCALES:
            ref = _oracle(params, ids, (n, s), forced=s * delta)
            mel, ralpha, frames = m.inference(ids.to(dev), length_scale=s, return_durations=True)
            t2 = int(torch.round((s * delta).sum()))
            assert mel.shape[1] == t2 == ref["t2"] and int(frames.sum()) == t2, (n, s)
            assert float((mel.cpu() - ref["mel_pred"]).abs().max()) <= tol_mel, (n, s)
            assert float((ralpha.cpu() - ref["reconst_alpha"]).abs().max()) <= tol_alpha, (n, s)


def test_per_item_scale_equals_single_items(golden_dir):
    g = _golden(golden_dir, "inference_lj")
    dev = _dev()
    m = _model("bf16x3")
    ns = (1, 9, 4, 7)
    text, lens = _ragged(g, ns)
    scales = torch.tensor(SCALES)
    mel, ml, ralpha, frames = m.inference_batch(text.to(dev), lens.to(dev), length_scale=scales.to(dev), return_durations=True)
    assert torch.equal(frames.sum(1), ml)
    for i, n in enumerate(ns):
        one, ra1, fr1 = m.inference(_ids(g, n).to(dev), length_scale=float(scales[i]), return_durations=True)
        t2, k = one.shape[1], int(lens[i])
        assert int(ml[i]) == t2 and int(frames[i, k:].abs().sum()) == 0
        assert int((frames[i, :k] - fr1[0]).abs().max()) <= 1                   # (a boundary may round the other way)
        assert float((mel[i, :t2] - one[0]).abs().max()) <= 2e-4
        assert float(mel[i, t2:].abs().max()) == 0.0 if mel.shape[1] > t2 else True
        assert float((ralpha[i, :k, :t2] - ra1[0]).abs().max()) <= 1e-5


def test_duration_override_matches_oracle(golden_dir, params):
    g = _golden(golden_dir, "inference_lj")
    dev = _dev()
    m = _model("bf16x3")
    tol_mel, tol_alpha = BOUNDS["bf16x3"]
    gen = torch.Generator().manual_seed(7)
    for n in (0, 5):
        ids = _ids(g, n)
        delta = _oracle(params, ids, (n, None))["delta"]
        full = torch.randint(0, 6, ids.shape, generator=gen).float()
        part = full.clone()
        part[:, 1::2] = -1.0                                               # every other phoneme keeps its prediction
        for d, s in ((full, 1.0), (part, 1.0), (part, 0.8)):
            forced = torch.where(d >= 0, d, delta) * s
            ref = O.inference(params, ids, forced_delta=forced)
            mel, ralpha = m.inference(ids.to(dev), durations=d, length_scale=s)
            assert mel.shape[1] == ref["t2"] == int(torch.round(forced.sum()))
            assert float((mel.cpu() - ref["mel_pred"]).abs().max()) <= tol_mel
            assert float((ralpha.cpu() - ref["reconst_alpha"]).abs().max()) <= tol_alpha


def test_target_frames_are_exact(golden_dir):
    g = _golden(golden_dir, "inference_lj")
    dev = _dev()
    m = _model("bf16x3")
    text, lens = _ragged(g, (2, 3, 8))
    target = torch.tensor([77, 300, 41])
    mel, ml, ralpha, frames = m.inference_batch(text.to(dev), lens.to(dev), target_frames=target.to(dev), return_durations=True)
    assert ml.cpu().tolist() == target.tolist() and mel.shape[1] == 300
    assert frames.sum(1).cpu().tolist() == target.tolist()
    # B = 1: a target together with a scale (the scale then cancels) and fixed phonemes
    ids = _ids(g, 6).to(dev)
    a, _, fa = m.inference(ids, target_frames=123, return_durations=True)
    b, _, fb = m.inference(ids, target_frames=123, length_scale=1.7, return_durations=True)
    assert a.shape[1] == b.shape[1] == 123 and int(fa.sum()) == int(fb.sum()) == 123
    assert float((a - b).abs().max()) <= 1e-3


def test_controls_replay_one_phase1_graph(golden_dir):
    g = _golden(golden_dir, "inference_lj")
    dev = _dev()
    m = _model("bf16x3")
    text, lens = _ragged(g, (1, 4))
    text, lens = text.to(dev), lens.to(dev)
    m.graphs = True
    key = ("text", 2, -(-text.shape[1] // m.T1_BUCKET) * m.T1_BUCKET, "ctl", (True, False, False))
    m._infer_cache.entries.pop(key, None)
    before = m._infer_cache.captures
    outs, graphs = [], []
    for s in (0.7, 0.9, 1.3):
        outs.append(m.inference_batch(text, lens, length_scale=s))
        graphs.append(m._infer_cache.entries[key].graph)
    ent = m._infer_cache.entries[key]
    assert ent.calls == 3 and graphs[0] is None and graphs[1] is not None and graphs[2] is graphs[1]   # captured once, replayed
    # the cache's own count: one phase-1 capture; phase 2 (keyed by the mel-length bucket) captures a bucket on its second sighting
    buckets = [-(-mel.shape[1] // m.T2_BUCKET) for mel, _, _ in outs]
    assert m._infer_cache.captures - before == 1 + sum(1 for v in set(buckets) if buckets.count(v) >= 2)
    m.graphs = False
    try:
        for s, (mel, ml, ralpha) in zip((0.7, 0.9, 1.3), outs):
            mel0, ml0, ralpha0 = m.inference_batch(text, lens, length_scale=s)
            assert torch.equal(ml, ml0)
            assert float((mel - mel0).abs().max()) <= 2e-4 and float((ralpha - ralpha0).abs().max()) <= 1e-5
    finally:
        m.graphs = True


# ------------------------------------------------------------------ align()
def test_align_matches_forward_and_resynthesises(golden_dir, params):
    g = _golden(golden_dir, "fwd_tiny")
    dev = _dev()
    m = _model("bf16x3")
    args = [torch.from_numpy(g[k]) for k in ("text", "text_lengths", "speech", "speech_lengths")]
    out = m.align(*[a.to(dev) for a in args])
    assert set(out) == {"e", "durations", "frames", "imv"}
    assert float((out["e"].cpu() - torch.from_numpy(g["e"])).abs().max()) <= 1e-2
    ref = O.forward(params, *args)
    assert float((out["imv"].cpu() - ref["imv"]).abs().max()) <= 2e-3
    with torch.no_grad():
        imv_fwd = m(*[a.to(dev) for a in args])[2]
    assert float((out["imv"] - imv_fwd).abs().max()) <= 1e-6                  # the launches of forward() up to the IMV
    e_ref = ref["e"]
    delta_e = torch.cat([e_ref[:, :1], e_ref[:, 1:] - e_ref[:, :-1]], dim=1)   # efficient_tts.py:204 (delta_e_method_1)
    dur, frames = out["durations"].cpu(), out["frames"].cpu()
    for b, n in enumerate(args[1].tolist()):
        assert float((dur[b, :n] - delta_e[b, :n]).abs().max()) <= 2e-2
        assert float(dur[b, n:].abs().max()) == 0.0 if n < dur.shape[1] else True
        assert int(frames[b].sum()) == int(torch.round(dur[b].double().sum())) == int(torch.round(out["e"][b, n - 1].cpu()))
        assert int(frames[b, n:].abs().sum()) == 0
        mel, _ = m.inference(args[0][b:b + 1, :n].to(dev), durations=dur[b:b + 1, :n])
        assert mel.shape[1] == int(torch.round(dur[b].double().sum()))


# ------------------------------------------------------------------ the synthesis script
def test_cli_writes_durations(tmp_path):
    import yaml
    from efficient_tts_amd import EfficientTTSCNN
    from efficient_tts_amd.bin.inference import main
    exp = tmp_path / "exp"
    exp.mkdir()
    phones = ["_"] + [f"P{i}" for i in range(1, 76)]
    (tmp_path / "phn.txt").write_text("\n".join(phones) + "\n")
    rng = np.random.default_rng(2)
    lines = [f"DUMMY/utt{n}.wav|" + " ".join(phones[int(i)] for i in rng.integers(1, 76, size=k)) for n, k in enumerate((9, 14, 11))]
    (tmp_path / "test.txt").write_text("\n".join(lines) + "\n")
    params = dict(num_symbols=76, dropout_rate=0.0, use_masking=True, use_weighted_masking=False, sigma=0.01)
    with open(exp / "config.yml", "w") as f:
        yaml.dump(dict(model_name="EfficientTTSCNN", model_params=params,
                       dataset_params=dict(use_phnseq=True, phnset_path=str(tmp_path / "phn.txt"))), f)
    torch.manual_seed(0)
    m = EfficientTTSCNN(**params)
    with torch.no_grad():
        m.duration_predictor.linear.bias.fill_(1.5)
    torch.save({"model": m.state_dict(), "steps": 7}, exp / "checkpoint-7steps.pkl")
    base = ["--checkpoint", str(exp / "checkpoint-7steps.pkl"), "--test_fid_scp", str(tmp_path / "test.txt"), "--verbose", "0",
            "--no_vocoder", "--write_durations"]
    lengths = {}
    for tag, extra in (("s1", []), ("slow", ["--length_scale", "1.6"]), ("slowb", ["--length_scale", "1.6", "--batch_size", "3"])):
        out = tmp_path / tag
        assert main(base + ["--outdir", str(out)] + extra) == 0
        for n, line in enumerate(lines):
            mel = np.load(out / f"utt{n}_7steps.npy")
            rows = [r.split("\t") for r in (out / f"utt{n}_7steps.durations.txt").read_text().splitlines()]
            assert [r[1] for r in rows] == line.split("|")[1].split()
            counts = [int(r[3]) for r in rows]
            starts = [int(r[2]) for r in rows]
            assert sum(counts) == mel.shape[0] and starts == list(np.cumsum([0] + counts[:-1]))
            assert abs(float(rows[-1][4]) - starts[-1] * 256 / 22050) <= 1e-5
            lengths[tag, n] = mel.shape[0]
    for n in range(len(lines)):
        assert lengths["slow", n] == lengths["slowb", n] and lengths["slow", n] > lengths["s1", n]
