"""GPU (-m gpu): the scorer (efficient_tts_amd/score.py, csrc/efts_score.hip) against the float64 restatement of tests/score_reference.py.

Shapes (Tx, Ty) sit on each side of every boundary of efts_dtw, derived from the kernel's constants DTW_THREADS = 256 threads,
DTW_ROWS = 4 rows per lane (a band of DTW_BAND = 1024 rows; a thread's last row may be partial) and a ring refill every 256 columns.

Three input classes.  Exact: one non-zero coordinate holding multiples of 1/8 in [-16, 16] drawn from five values, so ties are frequent
and every fp32 operation is exact: cost and path_len must EQUAL the reference.  Known warp: K base frames 4 N(0, 1) repeated a_k times in
x and b_k times in y (min(a_k, b_k) = 1, at most 4) plus 0.01 N(0, 1) noise; the reference's on-path margin is first asserted above
1000 gamma, so no choice on the path can flip under fp32 error: path_len must equal the reference's (= sum of max(a_k, b_k)) and the cost
lie within gamma.  Random: Gaussian random walks, unrelated or loosely warped; near-ties on the path are unavoidable, so only
max(Tx, Ty) <= path_len <= Tx + Ty - 1 and the cost within gamma are asserted.

gamma = 2 (Tx + Ty + D + 3) 2^-24 relative to the reference cost, derived (score_reference.gamma), not tuned; an indexing error shows
at 1e-2 or worse.  Each test prints its worst error as a fraction of gamma.
"""
import numpy as np
import pytest
import torch
import yaml

import score_reference as R
from efficient_tts_amd import lib as L
from efficient_tts_amd import score as S

pytestmark = pytest.mark.gpu

DTW_THREADS, DTW_ROWS = 256, 4
DTW_BAND = DTW_THREADS * DTW_ROWS
SHAPES = [(1, 1), (1, 7), (5, 1), (63, 65), (64, 64), (65, 130), (257, 130), (9, 255), (7, 257), (6, 513),
          (DTW_BAND - 1, 1030), (DTW_BAND, 260), (DTW_BAND + 1, 1031), (2 * DTW_BAND + 2, 700)]
DIMS = (13, 1, 32, 20)                    # 13 and 20 leave a zero-padded tail in the kernel's D' = 16 and D' = 32 forms
SENTINEL = -7.0


@pytest.fixture(scope="module")
def dev():
    L.load()
    L.require_device()
    return torch.device("cuda:0")


def _run(dev, xs, ys, ld=None, t_pad=0):
    """efts_dtw on lists of [T, D] arrays: rows beyond an item's length (and the columns beyond D of a wider row) are NaN, the outputs
    pre-filled with a sentinel"""
    B, D = len(xs), xs[0].shape[1]
    ld = D if ld is None else ld

    def pad(items):
        T = max(max(v.shape[0] for v in items), 1) + t_pad
        buf = np.full((B, T, ld), np.nan, dtype=np.float32)
        for b, v in enumerate(items):
            buf[b, :v.shape[0], :D] = v
        return torch.from_numpy(buf).to(dev), torch.tensor([v.shape[0] for v in items], dtype=torch.int32, device=dev), T
    x, xl, Tx = pad(xs)
    y, yl, Ty = pad(ys)
    cost = torch.full((B,), SENTINEL, dtype=torch.float32, device=dev)
    plen = torch.full((B,), -1, dtype=torch.int32, device=dev)
    L.check(L.load().efts_dtw(x.data_ptr(), ld, Tx * ld, xl.data_ptr(), Tx, y.data_ptr(), ld, Ty * ld, yl.data_ptr(), Ty, D, cost.data_ptr(),
                              plen.data_ptr(), B, torch.cuda.current_stream().cuda_stream), "efts_dtw")
    torch.cuda.synchronize()
    return cost.cpu().numpy(), plen.cpu().numpy()


def _within_gamma(what, cost, ref, tx, ty, d):
    g = R.gamma(tx, ty, d)
    rel = abs(float(cost) - ref) / ref
    print(f"{what}: device {float(cost)!r} reference {ref!r} relative error {rel:.3e} = {rel / g:.4f} gamma (gamma {g:.3e})")
    assert rel <= g


@pytest.mark.parametrize("n,shape", list(enumerate(SHAPES)))
def test_exact_inputs_equal_the_reference(dev, n, shape):
    tx, ty = shape
    d = DIMS[n % 4]
    rng = np.random.default_rng(100 + n)
    values = rng.integers(-128, 129, size=5) / 8.0
    x, y = np.zeros((tx, d), np.float32), np.zeros((ty, d), np.float32)
    x[:, d // 2], y[:, d // 2] = rng.choice(values, tx), rng.choice(values, ty)
    ref_cost, ref_len, margin = R.dtw(x, y)
    cost, plen = _run(dev, [x], [y], ld=d + 3 if n % 3 == 1 else None)
    print(f"exact {tx} x {ty}, D {d}: cost {cost[0]!r} path_len {plen[0]} (reference {ref_cost!r}, {ref_len}; on-path margin {margin})")
    assert float(cost[0]) == ref_cost and int(plen[0]) == ref_len


@pytest.mark.parametrize("K,d", [(40, 13), (150, 13), (300, 13), (97, 32), (64, 1)])
def test_known_warp(dev, K, d):
    rng = np.random.default_rng(K)
    base = 4.0 * rng.normal(size=(K, d))
    long_side = rng.integers(0, 2, size=K)
    reps = rng.integers(1, 5, size=K)
    a, b = np.where(long_side == 0, reps, 1), np.where(long_side == 1, reps, 1)
    x = (np.repeat(base, a, axis=0) + 0.01 * rng.normal(size=(a.sum(), d))).astype(np.float32)
    y = (np.repeat(base, b, axis=0) + 0.01 * rng.normal(size=(b.sum(), d))).astype(np.float32)
    tx, ty = x.shape[0], y.shape[0]
    ref_cost, ref_len, margin = R.dtw(x, y)
    g = R.gamma(tx, ty, d)
    print(f"known warp K {K} D {d}: {tx} x {ty}, on-path margin {margin:.3e} = {margin / g:.0f} gamma")
    assert margin > 1000.0 * g
    assert ref_len == int(np.maximum(a, b).sum())
    cost, plen = _run(dev, [x], [y])
    assert int(plen[0]) == ref_len
    _within_gamma(f"known warp K {K} D {d}", cost[0], ref_cost, tx, ty, d)


@pytest.mark.parametrize("n,shape", [(n, s) for n, s in enumerate(SHAPES) if s[0] > 1 and s[1] > 1])
def test_random_walks(dev, n, shape):
    tx, ty = shape
    d = DIMS[n % 4]
    rng = np.random.default_rng(200 + n)
    x = np.cumsum(rng.normal(size=(tx, d)), axis=0).astype(np.float32)
    unrelated = np.cumsum(rng.normal(size=(ty, d)), axis=0).astype(np.float32)
    # loosely warped: y follows x along a jittered monotone map of its rows, plus noise
    pos = np.sort(rng.uniform(0, tx - 1, size=ty))
    warped = (x[np.round(pos).astype(int)] + 0.3 * rng.normal(size=(ty, d))).astype(np.float32)
    cost, plen = _run(dev, [x, x], [unrelated, warped], ld=d + 1 if n % 2 else None)
    for b, (name, y) in enumerate((("unrelated", unrelated), ("warped", warped))):
        ref_cost, _, margin = R.dtw(x, y)
        assert max(tx, ty) <= int(plen[b]) <= tx + ty - 1
        _within_gamma(f"random {name} {tx} x {ty} D {d} (on-path margin {margin:.2e})", cost[b], ref_cost, tx, ty, d)


@pytest.mark.parametrize("n_mels,n_coef,ld", [(80, 13, 80), (128, 32, 131), (20, 5, 20)])
def test_mel_cepstrum(dev, n_mels, n_coef, ld):
    rng = np.random.default_rng(n_mels)
    T, lengths = 70, [70, 33, 0, 1]
    mel = np.full((len(lengths), T, ld), np.nan, dtype=np.float32)
    for b, n in enumerate(lengths):
        mel[b, :n, :n_mels] = rng.uniform(-11.6, 2.0, size=(n, n_mels))
    md = torch.from_numpy(mel).to(dev)
    out = S.mel_cepstrum(md[:, :, :n_mels], torch.tensor(lengths), n_coef).cpu().numpy()
    assert out.shape == (len(lengths), T, n_coef)
    table = R.table(n_mels, n_coef)
    tol = n_mels * 2.0 ** -24 * np.abs(table).sum(axis=1).max() * 11.6
    worst = 0.0
    for b, n in enumerate(lengths):
        assert (out[b, n:] == 0.0).all()
        if n:
            worst = max(worst, float(np.abs(out[b, :n] - R.mel_cepstrum(mel[b, :n, :n_mels], n_coef)).max()))
    print(f"mel_cepstrum {n_mels} -> {n_coef}: max |device - fp64| {worst:.3e}, bound {tol:.3e}")
    assert worst <= tol


PAIRS5 = [(DTW_BAND + 76, 300), (5, 700), (257, 130), (64, 64), (1, 9)]


@pytest.fixture(scope="module")
def ragged(dev):
    rng = np.random.default_rng(77)
    xs = [np.cumsum(rng.normal(size=(tx, 13)), axis=0).astype(np.float32) for tx, _ in PAIRS5]
    ys = [np.cumsum(rng.normal(size=(ty, 13)), axis=0).astype(np.float32) for _, ty in PAIRS5]
    return xs, ys, _run(dev, xs, ys, ld=16)


def test_bit_identity_in_a_batch_alone_and_again(dev, ragged):
    xs, ys, (cost, plen) = ragged
    again = _run(dev, xs, ys, ld=16)
    assert np.array_equal(cost.view(np.uint32), again[0].view(np.uint32)) and np.array_equal(plen, again[1])
    for b in range(len(xs)):
        c1, n1 = _run(dev, [xs[b]], [ys[b]])
        assert c1.view(np.uint32)[0] == cost.view(np.uint32)[b] and n1[0] == plen[b]
        _within_gamma(f"ragged item {b}", cost[b], R.dtw(xs[b], ys[b])[0], xs[b].shape[0], ys[b].shape[0], 13)


def test_empty_items_and_the_limit(dev, ragged):
    xs, ys, (cost, plen) = ragged
    empty = np.zeros((0, 13), np.float32)
    c, n = _run(dev, [xs[2], empty, xs[3], xs[4]], [ys[2], ys[1], ys[3], empty], ld=16)
    assert np.isnan(c[1]) and n[1] == 0 and np.isnan(c[3]) and n[3] == 0
    assert c.view(np.uint32)[0] == cost.view(np.uint32)[2] and n[0] == plen[2] and c.view(np.uint32)[2] == cost.view(np.uint32)[3] and n[2] == plen[3]
    # a padded length above the limit: the error, and nothing runs
    import re
    with open(L.HERE + "/../include/efts_abi.h") as f:
        limit = int(re.search(r"#define EFTS_DTW_MAX_FRAMES (\d+)", f.read()).group(1))
    x = torch.zeros(1, limit + 1, 13, device=dev)
    y = torch.zeros(1, 8, 13, device=dev)
    one, eight = torch.tensor([1], dtype=torch.int32, device=dev), torch.tensor([8], dtype=torch.int32, device=dev)
    out_c = torch.full((1,), SENTINEL, device=dev)
    out_n = torch.full((1,), -1, dtype=torch.int32, device=dev)
    for a, al, ta, b_, bl, tb in ((x, one, limit + 1, y, eight, 8), (y, eight, 8, x, one, limit + 1)):
        rc = L.load().efts_dtw(a.data_ptr(), 13, ta * 13, al.data_ptr(), ta, b_.data_ptr(), 13, tb * 13, bl.data_ptr(), tb, 13, out_c.data_ptr(),
                               out_n.data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
        assert rc == -2 and b"frames" in L.load().efts_last_error()
    torch.cuda.synchronize()
    assert float(out_c[0]) == SENTINEL and int(out_n[0]) == -1
    with pytest.raises(ValueError, match="efts_dtw"):
        S.dtw(x, one, y, eight)
    # ... and the limit itself is served
    c, n = S.dtw(x[:, :limit], torch.tensor([limit]), y, eight)
    assert float(c[0]) == 0.0 and int(n[0]) == limit


def test_mel_cepstral_distortion(dev):
    rng = np.random.default_rng(9)
    T = 100
    mel = torch.from_numpy(rng.uniform(-11.6, 2.0, size=(2, T, 80)).astype(np.float32)).to(dev)
    lengths = torch.tensor([T, 61])
    scorer = S.MelCepstralDistortion(dev)
    out = scorer(mel, lengths, mel, lengths)
    assert set(out) == {"mcd", "cost", "path_len", "frames_ratio"} and all(v.is_cuda for v in out.values())
    assert out["mcd"].tolist() == [0.0, 0.0] and out["path_len"].tolist() == [T, 61] and out["frames_ratio"].tolist() == [1.0, 1.0]
    assert out["path_len"].dtype == torch.int32 and out["cost"].dtype == torch.float32
    # an item without frames has no path: NaN and 0, its neighbour unchanged
    out = scorer(mel, torch.tensor([T, 0]), mel, lengths)
    assert out["mcd"][0].item() == 0.0 and out["path_len"].tolist() == [T, 0]
    assert all(bool(torch.isnan(out[k][1])) for k in ("mcd", "cost", "frames_ratio"))
    # every third frame doubled: the only path of cost 0 visits each frame of the longer side once
    idx = torch.tensor([i for t in range(T) for i in ([t, t] if t % 3 == 2 else [t])], device=dev)
    longer = mel[:, idx]
    n_long = [T + T // 3, 61 + 61 // 3]
    out = scorer(mel, lengths, longer, torch.tensor(n_long))
    assert out["mcd"].tolist() == [0.0, 0.0] and out["path_len"].tolist() == n_long
    assert out["frames_ratio"].tolist() == pytest.approx([T / n_long[0], 61 / n_long[1]], rel=1e-6)
    # the figure itself: (10 / ln 10) sqrt(2) cost / path_len of the two cepstra against the float64 restatement
    other = torch.from_numpy(rng.uniform(-11.6, 2.0, size=(2, 90, 80)).astype(np.float32)).to(dev)
    out = scorer(mel, lengths, other, torch.tensor([90, 44]))
    ca, cb = S.mel_cepstrum(mel, lengths).cpu().numpy(), S.mel_cepstrum(other, torch.tensor([90, 44])).cpu().numpy()
    for b, (na, nb) in enumerate(((T, 90), (61, 44))):
        ref_cost, ref_len, _ = R.dtw(ca[b, :na], cb[b, :nb])
        _within_gamma(f"mcd item {b}", out["cost"][b], ref_cost, na, nb, 13)
        assert max(na, nb) <= int(out["path_len"][b]) <= na + nb - 1
        assert float(out["mcd"][b]) == pytest.approx(R.MCD_DB * float(out["cost"][b]) / int(out["path_len"][b]), rel=1e-6)


def _tiny_model(dev=None):
    from efficient_tts_amd import EfficientTTSCNN
    params = dict(num_symbols=76, n_channels=256, symbol_embedding_dim=256, n_text_encoder_layer=1, n_mel_encoder_layer=1, n_decoder_layer=1,
                  dropout_rate=0.0, use_masking=True, use_weighted_masking=False, sigma=0.01)
    torch.manual_seed(0)
    m = EfficientTTSCNN(**params)
    with torch.no_grad():
        m.duration_predictor.linear.bias.fill_(1.5)              # a few frames per phoneme with random weights
    return params, (m if dev is None else m.to(dev))


def test_trainer_publishes_mcd_only_when_asked(dev):
    from efficient_tts_amd.trainer import EfficientTTSTrainer
    _, model = _tiny_model(dev)
    rng = np.random.default_rng(3)
    text, text_lengths = torch.from_numpy(rng.integers(1, 76, size=(2, 12))), torch.tensor([12, 9])
    text[1, 9:] = 0
    mel = torch.from_numpy(rng.uniform(-11.6, 2.0, size=(2, 64, 80)).astype(np.float32))
    mel[1, 50:] = 0.0
    batch = (text, text_lengths, mel, torch.tensor([64, 50]))
    cfg = dict(outdir="/tmp", log_interval_steps=5, eval_interval_steps=0, save_interval_steps=10, train_max_steps=20, grad_norm=1.0)
    seen = {}
    for extra in ({}, {"eval_mcd": True}):
        t = EfficientTTSTrainer(steps=0, epochs=0, data_loader={"dev": [batch]}, sampler={}, model=model, optimizer=None, scheduler=None,
                                config=dict(cfg, **extra), device=dev)
        got = {}
        t._publish = got.update
        t._evaluate()
        seen[bool(extra)] = got
    assert set(seen[False]) == {"eval/loss", "eval/mel_loss", "eval/dur_loss"}
    assert set(seen[True]) == set(seen[False]) | {"eval/mcd_db", "eval/frames_ratio"}
    assert all(seen[True][k] == seen[False][k] for k in seen[False])
    assert np.isfinite(seen[True]["eval/mcd_db"]) and seen[True]["eval/mcd_db"] > 0.0 and np.isfinite(seen[True]["eval/frames_ratio"])
    assert seen[True]["eval/frames_ratio"] > 0.0


def test_score_cli(dev, tmp_path, capsys):
    from scipy.io.wavfile import write
    from efficient_tts_amd.bin.score import main
    from efficient_tts_amd.frontend import LogMelFrontend
    exp = tmp_path / "exp"
    exp.mkdir()
    phones = ["_"] + [f"P{i}" for i in range(1, 76)]
    (tmp_path / "phn.txt").write_text("\n".join(phones) + "\n")
    rng = np.random.default_rng(1)
    ids = [rng.integers(1, 76, size=k) for k in (9, 14)]
    pcm = [rng.integers(-8000, 8000, size=n).astype(np.int16) for n in (9000, 12345)]
    lines = []
    for n in range(2):
        write(str(tmp_path / f"utt{n}.wav"), 22050, pcm[n])
        lines.append(f"{tmp_path}/utt{n}.wav|" + " ".join(phones[int(i)] for i in ids[n]))
    (tmp_path / "test.txt").write_text("\n".join(lines) + "\n")
    params, m = _tiny_model()
    with open(exp / "config.yml", "w") as f:
        yaml.dump(dict(model_name="EfficientTTSCNN", model_params=params, dataset_params=dict(use_phnseq=True, phnset_path=str(tmp_path / "phn.txt"))), f)
    torch.save({"model": m.state_dict(), "steps": 7}, exp / "checkpoint-7steps.pkl")
    assert main(["--checkpoint", str(exp / "checkpoint-7steps.pkl"), "--test_fid_scp", str(tmp_path / "test.txt"), "--outdir", str(tmp_path / "out")]) == 0
    rows = [line.split("\t") for line in (tmp_path / "out" / "mcd.tsv").read_text().splitlines()]
    assert [r[0] for r in rows] == ["utt0", "utt1", "mean"] and [len(r) for r in rows] == [5, 5, 2]
    # the same figures from a direct call
    model = m.to(dev).eval()
    model.remove_weight_norm()
    audio = torch.zeros(2, 12345, dtype=torch.int16)
    for n in range(2):
        audio[n, :pcm[n].shape[0]] = torch.from_numpy(pcm[n])
    text = torch.zeros(2, 14, dtype=torch.long)
    for n in range(2):
        text[n, :ids[n].shape[0]] = torch.from_numpy(ids[n])
    with torch.no_grad():
        rec, rec_len = LogMelFrontend(dev)(audio, torch.tensor([9000, 12345]))
        syn, syn_len = model.inference_batch(text.to(dev), torch.tensor([9, 14], device=dev), length_scale=1.0)[:2]
        out = S.MelCepstralDistortion(dev)(syn, syn_len, rec, rec_len)
    for n in range(2):
        assert rows[n][1:] == [f"{float(out['mcd'][n]):.6f}", str(int(syn_len[n])), str(int(rec_len[n])), str(int(out["path_len"][n]))]
        assert np.isfinite(float(rows[n][1])) and float(rows[n][1]) > 0.0
    mean = float(np.mean([float(v) for v in out["mcd"].tolist()]))
    assert rows[2][1] == f"{mean:.6f}" and f"{mean:.4f} dB" in capsys.readouterr().out
