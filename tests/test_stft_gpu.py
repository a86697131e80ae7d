"""GPU (-m gpu): the STFT magnitudes and the multi-resolution STFT distance (efficient_tts_amd/stft.py, csrc/efts_stft.hip) against the numpy
float64 restatement of their definition in tests/stft_reference.py, which never sees the product's code.

Tolerances.  The sums (num, den, l1): nothing fixed in advance.  The yardstick is measured here, on these inputs: the same sums through
torch.stft in fp32 on the CPU against the float64 restatement; the kernel's relative error must stay within 4 x the largest such error (the
factor pays for the different summation order).  The magnitudes, cell by cell: an fp32 FFT of N points is off by at most about
log2(N) eps times the 2-norm of the spectrum in every bin (Higham, Accuracy and Stability of Numerical Algorithms, 24.2), the window product,
the untangling of the two frames of a transform and the square root add a few eps of the same norm and of the magnitude itself, and
sqrt(max(., 1e-7)) does not amplify an error of |X|: |mag - ref| <= eps (log2 N + 4) ||X_t||_2 + 4 eps ref, eps = 2^-23.

Measured on an MI355X (profiles/mrstft_error.json; EFTS_MRSTFT_ERROR_JSON=<path> writes the file anew): see test_distance_against_float64.
"""
import json
import os

import numpy as np
import pytest
import torch

import stft_reference as R
from efficient_tts_amd import lib as L
from efficient_tts_amd.stft import MultiResolutionSTFTDistance, STFTMagnitude

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
# the default (H, W) of the three default sizes; W = N with H = N / 4; an odd hop with an odd window, on the smallest and the largest transform
MAG_CASES = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240), (256, 64, 256), (256, 37, 201), (2048, 333, 1001))


@pytest.fixture(scope="module")
def dev():
    L.load()
    L.require_device()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def inputs():
    x, y = R.batch(fill=99)                     # garbage behind every length
    ref = R.distance(x, y, R.LENGTHS)
    for v in (x, y, *ref.values()):
        v.setflags(write=False)
    return x, y, ref


@pytest.fixture(scope="module")
def yardstick(inputs):
    """the largest relative error of num, den, l1 when the reference's formula runs through torch.stft in fp32 on the CPU, on these inputs"""
    x, y, ref = inputs
    worst = 0.0
    for b, n in enumerate(R.LENGTHS):
        xf = torch.from_numpy(x[b:b + 1, :n].copy())
        yf = torch.from_numpy(y[b:b + 1, :n].astype(np.float32) / np.float32(R.MAX_WAV))
        for r, (N, H, W) in enumerate(R.DEFAULT):
            if ref["cells"][b, r] == 0:
                continue
            win = torch.from_numpy(R.window(W))
            mags = []
            for s in (xf, yf):
                spec = torch.stft(s, N, H, W, win, return_complex=True)
                mags.append(torch.sqrt(torch.clamp(spec.real ** 2 + spec.imag ** 2, min=1e-7)))
            mx, my = mags
            got = [float(((my - mx) ** 2).sum()), float((my ** 2).sum()), float((torch.log(my) - torch.log(mx)).abs().sum())]
            err = [abs(g - w) / w for g, w in zip(got, ref["sums"][b, r])]
            print(f"fp32 torch.stft item {b} resolution {(N, H, W)}: relative error of num, den, l1 {err[0]:.2e} {err[1]:.2e} {err[2]:.2e}")
            worst = max(worst, *err)
    return worst


def _items(N, dtype):
    """the smallest items that reach every branch: one sample over the reflection limit, 4 N + 3, and one AT the limit (no frames)"""
    lengths = (N // 2 + 1, 4 * N + 3, N // 2)
    rng = np.random.default_rng(N)
    pcm = rng.integers(-32768, 32767, (3, 4 * N + 3)).astype(np.int16)            # garbage behind the lengths
    for b, n in enumerate(lengths):
        pcm[b, :n] = R.signal(n, 10 * N + b)[1]
    return lengths, pcm if dtype == np.int16 else pcm.astype(np.float32) / np.float32(R.MAX_WAV)


@pytest.mark.parametrize("N,H,W", MAG_CASES)
def test_transform_alone(dev, N, H, W):
    lengths, pcm = _items(N, np.int16)
    f32 = _items(N, np.float32)[1]
    op = STFTMagnitude(dev, N, H, W)
    li = torch.tensor(lengths)
    mag, frames = op(torch.from_numpy(pcm).to(dev), li)
    mag_f, frames_f = op(torch.from_numpy(f32).to(dev), li)
    mag, mag_f = mag.cpu().numpy(), mag_f.cpu().numpy()
    assert mag.shape == (3, 1 + (4 * N + 3) // H, N // 2 + 1)
    assert frames.tolist() == frames_f.tolist() == [R.frame_count(n, N, H) for n in lengths] and frames[2] == 0
    assert np.array_equal(mag.view(np.uint32), mag_f.view(np.uint32))             # int16 PCM == the same values as fp32
    worst = 0.0
    for b, n in enumerate(lengths):
        ref = R.magnitudes(pcm[b, :n], N, H, W)
        T = ref.shape[0]
        assert not mag[b, T:].any()                                               # rows at and beyond the item's count
        if T == 0:
            continue
        # ||X_t||_2 over all N bins from the N / 2 + 1 kept ones (the clamp only adds to it)
        norm = np.sqrt(2.0 * (ref ** 2).sum(axis=1) - ref[:, 0] ** 2 - ref[:, -1] ** 2)
        tol = EPS * (np.log2(N) + 4) * norm[:, None] + 4 * EPS * ref
        ratio = np.abs(mag[b, :T] - ref) / tol
        worst = max(worst, float(ratio.max()))
        print(f"N {N} H {H} W {W} item {b} len {n}: {T} frames, largest |mag - ref| / bound {ratio.max():.3f}, "
              f"largest relative error {np.max(np.abs(mag[b, :T] - ref) / ref):.2e}")
        assert (ratio <= 1.0).all()                                               # every cell
    assert worst > 0.0


def _run(dev, x, y, lengths, **kw):
    out = MultiResolutionSTFTDistance(dev, **kw)(torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(y)).to(dev), torch.tensor(lengths))
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_distance_against_float64(dev, inputs, yardstick):
    """Measured on an MI355X (profiles/mrstft_error.json): the fp32 torch.stft yardstick on these inputs is 1.25e-07 (l1 of the 1025-sample item
    at 2048), the bound 5.0e-07; the kernel's largest relative error is 1.7e-07 (l1 of the 1025-sample item at 512), over num 1.8e-08 ..
    1.6e-07, over den 3.1e-08 .. 1.3e-07, over l1 9.3e-09 .. 1.7e-07."""
    x, y, ref = inputs
    got = _run(dev, x, y, R.LENGTHS)
    assert got["sums"].dtype == np.float64 and got["cells"].dtype == np.int64 and got["sums"].shape == (3, 3, 3)
    assert np.array_equal(got["cells"], ref["cells"])                              # no cell left out
    assert got["cells"][1, 1] == 0 and np.isnan(got["sc"][1, 1]) and np.isnan(got["log_mag"][1, 1])
    assert np.isnan(got["sc"]).sum() == 1 and np.isnan(got["log_mag"]).sum() == 1 and not got["sums"][1, 1].any()
    bound = 4.0 * yardstick
    print(f"yardstick (fp32 torch.stft, largest relative error) {yardstick:.3e}, bound {bound:.3e}")
    worst = 0.0
    errors = {}
    for b in range(3):
        for r, res in enumerate(R.DEFAULT):
            if ref["cells"][b, r] == 0:
                continue
            err = np.abs(got["sums"][b, r] - ref["sums"][b, r]) / ref["sums"][b, r]
            errors[f"item{b}_{res[0]}_{res[1]}_{res[2]}"] = [float(e) for e in err]
            print(f"item {b} resolution {res}: relative error of num, den, l1 {err[0]:.2e} {err[1]:.2e} {err[2]:.2e}; clamped {ref['clamped'][b, r]:.3f}")
            worst = max(worst, float(err.max()))
    if os.environ.get("EFTS_MRSTFT_ERROR_JSON"):
        with open(os.environ["EFTS_MRSTFT_ERROR_JSON"], "w") as f:
            json.dump({"inputs": "tests/stft_reference.py batch(), lengths (1025, 1024, 4099), x fp32 against y int16, default resolutions",
                       "yardstick_fp32_torch_stft_cpu_max_rel_error": yardstick, "bound_4x": bound, "kernel_max_rel_error": worst,
                       "kernel_rel_error_num_den_l1": errors}, f, indent=1)
            f.write("\n")
    assert worst <= bound
    ok = ~np.isnan(ref["sc"])
    np.testing.assert_allclose(got["sc"][ok], ref["sc"][ok], rtol=bound, atol=0)               # sqrt halves a relative error
    np.testing.assert_allclose(got["log_mag"][ok], ref["log_mag"][ok], rtol=bound, atol=0)


def test_exact_properties(dev, inputs):
    x, y, _ = inputs
    yf = y.astype(np.float32) / np.float32(R.MAX_WAV)
    base = _run(dev, x, y, R.LENGTHS)
    bits = lambda o: (o["sums"].tobytes(), o["cells"].tobytes())
    # two runs
    assert bits(_run(dev, x, y, R.LENGTHS)) == bits(base)
    # int16 y == the same values as fp32; and an int16 x likewise
    assert bits(_run(dev, x, yf, R.LENGTHS)) == bits(base)
    x16 = np.round(x * np.float32(R.MAX_WAV)).astype(np.int16)
    assert bits(_run(dev, x16, y, R.LENGTHS)) == bits(base)
    # x identical to y: no distance at all, and den unchanged
    same = _run(dev, yf, y, R.LENGTHS)
    assert not same["sums"][..., 0].any() and not same["sums"][..., 2].any()
    assert np.array_equal(same["sums"][..., 1], base["sums"][..., 1])
    ok = same["cells"] > 0
    assert (same["sc"][ok] == 0).all() and (same["log_mag"][ok] == 0).all()
    # every item alone == inside the batch of three (whose rows hold garbage behind the lengths)
    for b, n in enumerate(R.LENGTHS):
        one = _run(dev, x[b:b + 1, :n], y[b:b + 1, :n], (n,))
        assert one["sums"].tobytes() == base["sums"][b:b + 1].tobytes() and np.array_equal(one["cells"], base["cells"][b:b + 1])
        alone = _run(dev, x[b:b + 1], y[b:b + 1], (n,))                            # the same row, its garbage included
        assert alone["sums"].tobytes() == base["sums"][b:b + 1].tobytes()


def test_batch_loss(dev, yardstick):
    lengths = (4099, 4099)
    x, y = R.batch(lengths, seed=5)
    want = R.batch_loss(R.distance(x, y, lengths))
    scorer = MultiResolutionSTFTDistance(dev)
    out = scorer(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
    sc, mag = scorer.batch_loss(out)
    print(f"batch_loss {float(sc)!r} {float(mag)!r} against {want!r}")
    assert abs(float(sc) - want[0]) <= 4.0 * yardstick * want[0] and abs(float(mag) - want[1]) <= 4.0 * yardstick * want[1]


def test_command_line(dev, tmp_path):
    from scipy.io.wavfile import write

    from efficient_tts_amd.bin import vocoder_score as V
    names = []
    for i in range(2):
        pcm = R.signal(11025 + 300 * i, 40 + i)[1]
        write(str(tmp_path / f"utt{i}.wav"), 22050, pcm)
        names.append(f"utt{i}.wav|ignored")
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    out = tmp_path / "out"
    assert V.main(["--test_fid_scp", str(tmp_path / "list.txt"), "--outdir", str(out), "--vocoder", "griffinlim", "--gl_iters", "4", "--wav_path", str(tmp_path)]) == 0
    lines = (out / "mrstft.tsv").read_text().splitlines()
    assert len(lines) == 3 and [line.split("\t")[0] for line in lines] == ["utt0", "utt1", "mean"]
    for line in lines:
        cells = line.split("\t")
        assert len(cells) == len(V.columns())
        vals = np.array([float(v) for v in cells[2:]])
        assert np.isfinite(vals).all() and (vals > 0).all()
    assert int(lines[0].split("\t")[1]) == 11025 // 256 * 256 and lines[2].split("\t")[1] == "-"
