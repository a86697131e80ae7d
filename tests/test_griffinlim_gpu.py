"""GPU (-m gpu): the Griffin-Lim vocoder (efficient_tts_amd/griffinlim.py, csrc/efts_griffinlim.hip) against the float64 restatement
of tests/griffinlim_reference.py.

Kernels alone.  efts_gl_init / efts_gl_synthesis / efts_gl_analysis / efts_gl_overlap_add are called through `efficient_tts_amd.lib`
with torch tensors as buffers.  Kernel and reference get the SAME float32 inputs (the reference upcasts them).  Metric and bound are
those of tests/test_bwd_kernels_gpu.py: `_rel` = max |got - ref| / max |ref| over the tensor; the same restatement evaluated in
float32 on the CPU deviates from float64 by `e32`, and the kernel must be within max(8 * e32, 2e-6).  Values that must be exactly zero,
untouched or bit-identical are asserted with ==.  Frames at or beyond an item's length are never written: the buffers are filled
with a sentinel first.

Trajectory.  1, 2 and 4 iterations from init="zero" on the audio, the loop run on given float32 magnitudes so that only the loop is
compared; bound 8 * e32(n), e32(n) the float32 twin's deviation after the same n iterations.  Measured on the CPU, 8 * e32(n) stays
below 1e-2 of the signal's peak for every test signal and n in {1, 2, 4} (largest: 8 * 6.5e-4 = 5.2e-3 at n = 4), so no n is dropped.

The float64 reference reproduces a padded signal on every sample but the first four and last three, where the window sum lies under
the 1e-8 floor (tests/test_griffinlim_cpu.py); the round trip on the GPU is therefore compared with the reference's round trip, which
behaves the same way there.

Measured on one MI355X: cases and the worst `kernel error / e32` of each check (error / e32 of that case):

    check                          cases  worst err / e32
    efts_gl_synthesis                 48  1.60  (1x5 random[0]: 2.1e-07 / 1.3e-07)
    efts_gl_analysis.Y                48  1.32  (3x64 signal[1]: 1.3e-07 / 1.0e-07)
    efts_gl_analysis.prev             48  1.32  (3x64 signal[1]: 1.3e-07 / 1.0e-07)
    efts_gl_analysis.X                48  6.19  (3x3 random[0]: 5.7e-06 / 9.2e-07)
    efts_gl_overlap_add.padded        48  1.00  (1x1 random[0]: 3.7e-08 / 3.7e-08)
    efts_gl_overlap_add.audio         48  1.76  (3x5 random[2]: 1.4e-07 / 8.1e-08)
    efts_gl_init                       4  0.32  (1x5[0]: 7.7e-08 / 2.4e-07)
    round trip                         4  2.00  (9.3 s: 2.9e-04 / 1.5e-04)
    trajectory n=1                     4  1.47  (0.3 s n=1: 1.0e-04 / 7.1e-05)
    trajectory n=2                     4  1.30  (0.3 s n=2: 1.6e-04 / 1.2e-04)
    trajectory n=4                     4  1.41  (9.3 s n=4: 8.5e-04 / 6.0e-04)

Every ratio is below 8; no factor was widened.  Quality, chain consistency and mel inversion on the same run:

    SC 0.3 s: device 32 iterations 0.18769, 1 iteration 0.42559; float64 reference 0.18828; ratio 0.9969
    SC 1.1 s: device 32 iterations 0.19055, 1 iteration 0.46668; float64 reference 0.19132; ratio 0.9960
    SC 2.4 s: device 32 iterations 0.10500, 1 iteration 0.73901; float64 reference 0.10453; ratio 1.0045
    SC 9.3 s: device 32 iterations 0.15363, 1 iteration 0.67054; float64 reference 0.15361; ratio 1.0001
    chain 0.3 s: mean |logmel(vocoder(mel)) - mel| device 0.33790, float64 reference 0.33339, ratio 1.0135
    chain 1.1 s: mean |logmel(vocoder(mel)) - mel| device 0.27025, float64 reference 0.27250, ratio 0.9917
    chain 2.4 s: mean |logmel(vocoder(mel)) - mel| device 0.10785, float64 reference 0.10790, ratio 0.9995
    chain 9.3 s: mean |logmel(vocoder(mel)) - mel| device 0.24839, float64 reference 0.24841, ratio 0.9999
    mel inversion fp32: max |M - M64| / max |M64| = 2.055e-07
    mel inversion bf16x3: max |M - M64| / max |M64| = 7.748e-06
"""
import numpy as np
import pytest
import torch

import griffinlim_reference as R
from kernel_check import _call, _dev, _st, load_lib

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 8.0, 2e-6
SIGNALS = [(0.3, 1), (1.1, 2), (2.4, 3), (9.3, 4)]          # (seconds, seed): 26, 95, 207 and 801 frames
SENTINEL = 777.0


@pytest.fixture(scope="module")
def lib():
    return load_lib()


# `_rel` and `_check` stay this file's own.  They are not kernel_check's: the references here are complex and reach down to exact zeros, so
# the denominator is guarded by 1e-30, not 1e-12; a complex reference is compared as complex; the trajectories are bounded by 8 * e32
# alone (`factor_only`) and read the returned e32; and there is no COND cap, whose place the trajectory test's own 1e-2 condition takes.
def _rel(a, b):
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30)


def _check(kernel, case, got, ref64, ref32, factor_only=False):
    """got against the float64 reference, bounded by the float32 twin's own error: max(8 * e32, 2e-6), or 8 * e32 alone"""
    got = got.detach().cpu()
    got = (torch.view_as_complex(got.contiguous()) if got.shape != ref64.shape else got).to(ref64.dtype)
    e32 = _rel(ref32.to(ref64.dtype), ref64)
    err = _rel(got, ref64)
    ratio = err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0
    print(f"RATIO {kernel} {case} err={err:.3e} e32={e32:.3e} ratio={ratio:.2f}")
    assert torch.isfinite(torch.view_as_real(got) if got.is_complex() else got).all()
    bound = FACTOR * e32 if factor_only else max(FACTOR * e32, FLOOR)
    assert err <= bound, f"{kernel} {case}: error {err:.3e} vs float64, float32 twin {e32:.3e}"
    return e32


# ------------------------------------------------------------------------------------------------ the kernels, called directly
def _window():
    return torch.hann_window(R.N_FFT, dtype=torch.float32).to(_dev())


def _ri(x: torch.Tensor) -> torch.Tensor:
    """complex [..] -> float32 (re, im) on the device"""
    return torch.view_as_real(x.to(torch.complex64)).contiguous().to(_dev())


def k_synthesis(lib, spec_ri, lens, wf=None):
    B, T = spec_ri.shape[:2]
    if wf is None:
        wf = torch.full((B, T, R.N_FFT), SENTINEL, dtype=torch.float32, device=_dev())
    _call("efts_gl_synthesis", lib.efts_gl_synthesis(spec_ri.data_ptr(), lens.data_ptr(), _window().data_ptr(), wf.data_ptr(), B, T, 1024, 256, _st()))
    return wf


def k_analysis(lib, lens, B, T, wf=None, signal=None, mag=None, prev=None, momentum=0.0, out=None):
    if out is None:
        out = torch.full((B, T, R.BINS, 2), SENTINEL, dtype=torch.float32, device=_dev())
    _call("efts_gl_analysis", lib.efts_gl_analysis(None if wf is None else wf.data_ptr(), None if signal is None else signal.data_ptr(),
                                                   0 if signal is None else signal.shape[1], lens.data_ptr(), _window().data_ptr(),
                                                   None if mag is None else mag.data_ptr(), None if prev is None else prev.data_ptr(), out.data_ptr(),
                                                   momentum, B, T, 1024, 256, _st()))
    return out


def k_overlap_add(lib, wf, lens, start, n_out):
    B, T = wf.shape[:2]
    out = torch.full((B, n_out), SENTINEL, dtype=torch.float32, device=_dev())
    _call("efts_gl_overlap_add", lib.efts_gl_overlap_add(wf.data_ptr(), lens.data_ptr(), _window().data_ptr(), out.data_ptr(), n_out, start, n_out,
                                                         B, T, 1024, 256, _st()))
    return out


def gpu_loop(lib, mag32, lens_list, n_iter, momentum=0.99, mode=0, seed=0):
    """the loop of GriffinLimVocoder._run on given magnitudes [B, T, 513] float32 -> audio [B, 256 T]"""
    B, T = mag32.shape[:2]
    mag = mag32.contiguous().to(_dev())
    lens = torch.tensor(lens_list, dtype=torch.int32, device=_dev())
    spec = torch.zeros(B, T, R.BINS, 2, dtype=torch.float32, device=_dev())
    prev = torch.zeros_like(spec)
    wf = torch.zeros(B, T, R.N_FFT, dtype=torch.float32, device=_dev())
    _call("efts_gl_init", lib.efts_gl_init(mag.data_ptr(), spec.data_ptr(), prev.data_ptr(), B, T, mode, seed, _st()))
    for _ in range(n_iter):
        k_synthesis(lib, spec, lens, wf)
        k_analysis(lib, lens, B, T, wf=wf, mag=mag, prev=prev, momentum=momentum, out=spec)
    k_synthesis(lib, spec, lens, wf)
    return k_overlap_add(lib, wf, lens, R.PAD, R.HOP * T).cpu()


def _lengths(B, T):
    return [T] if B == 1 else [T, max(1, T // 2), max(1, T - 1)]


def _spectra(B, T, kind):
    """[B, T, 513] complex128 whose values are float32-representable: random, or the spectra of a test signal"""
    if kind == "random":
        g = torch.Generator().manual_seed(100 * B + T)
        X = torch.complex(torch.randn(B, T, R.BINS, generator=g), torch.randn(B, T, R.BINS, generator=g))
    else:
        X = torch.stack([R.analysis(R.reflect_pad(R.voiced(max(T, 2) * R.HOP / R.SR, 10 * b + T))[:R.padded_len(T)]) for b in range(B)])
    return X.to(torch.complex64).to(torch.complex128)


CASES = [(B, T, kind) for T in (1, 2, 3, 5, 64, 801) for B in (1, 3) for kind in ("random", "signal")]


# ------------------------------------------------------------------------------------------------ 1. each kernel alone
@pytest.mark.parametrize("B,T,kind", CASES)
def test_synthesis_kernel_vs_fp64(lib, B, T, kind):
    X = _spectra(B, T, kind)
    lens = _lengths(B, T)
    wf = k_synthesis(lib, _ri(X), torch.tensor(lens, dtype=torch.int32, device=_dev())).cpu()
    for b, n in enumerate(lens):
        _check("efts_gl_synthesis", f"{B}x{T} {kind}[{b}]", wf[b, :n], R.windowed_frames(X[b, :n]), R.windowed_frames(X[b, :n].to(torch.complex64)))
        assert (wf[b, n:] == SENTINEL).all()


@pytest.mark.parametrize("B,T,kind", CASES)
def test_analysis_projection_kernel_vs_fp64(lib, B, T, kind):
    X = _spectra(B, T, kind)
    lens = _lengths(B, T)
    g = torch.Generator().manual_seed(7 * B + T)
    wf32 = torch.stack([R.windowed_frames(X[b]) for b in range(B)]).float()               # the kernel's input, consistent frames
    prev = (X.abs().mean() * torch.complex(torch.randn(B, T, R.BINS, generator=g), torch.randn(B, T, R.BINS, generator=g))).to(torch.complex64)
    mag32 = (X.abs() * (0.5 + torch.rand(B, T, R.BINS, generator=g, dtype=torch.float64))).float()
    a = 0.99
    lens_d = torch.tensor(lens, dtype=torch.int32, device=_dev())
    prev_d = _ri(prev)
    live = (torch.arange(T, device=_dev())[None, :] < lens_d[:, None])[:, :, None, None]
    prev_d = torch.where(live, prev_d, torch.full_like(prev_d, SENTINEL)).contiguous()
    out = k_analysis(lib, lens_d, B, T, wf=wf32.to(_dev()), mag=mag32.to(_dev()), prev=prev_d, momentum=a).cpu()
    plain = k_analysis(lib, lens_d, B, T, wf=wf32.to(_dev())).cpu()
    prev_out = prev_d.cpu()
    for b, n in enumerate(lens):
        ref = {}
        for dt in (torch.float64, torch.float32):
            Y = R.analysis(R.overlap_add(wf32[b, :n].to(dt)))
            ref[dt] = (Y, R.project(Y, prev[b, :n].to(R.cplx(dt)), mag32[b, :n].to(dt), a))
        case = f"{B}x{T} {kind}[{b}]"
        _check("efts_gl_analysis.Y", case, plain[b, :n], ref[torch.float64][0], ref[torch.float32][0])
        _check("efts_gl_analysis.prev", case, prev_out[b, :n], ref[torch.float64][0], ref[torch.float32][0])
        _check("efts_gl_analysis.X", case, out[b, :n], ref[torch.float64][1], ref[torch.float32][1])
        assert (out[b, n:] == SENTINEL).all() and (plain[b, n:] == SENTINEL).all() and (prev_out[b, n:] == SENTINEL).all()


@pytest.mark.parametrize("B,T,kind", CASES)
def test_overlap_add_kernel_vs_fp64(lib, B, T, kind):
    X = _spectra(B, T, kind)
    lens = _lengths(B, T)
    wf32 = torch.stack([R.windowed_frames(X[b]) for b in range(B)]).float()
    lens_d = torch.tensor(lens, dtype=torch.int32, device=_dev())
    audio = k_overlap_add(lib, wf32.to(_dev()), lens_d, R.PAD, R.HOP * T).cpu()
    full = k_overlap_add(lib, wf32.to(_dev()), lens_d, 0, R.padded_len(T)).cpu()
    for b, n in enumerate(lens):
        y64, y32 = R.overlap_add(wf32[b, :n].double()), R.overlap_add(wf32[b, :n])
        case = f"{B}x{T} {kind}[{b}]"
        _check("efts_gl_overlap_add.padded", case, full[b, :R.padded_len(n)], y64, y32)
        _check("efts_gl_overlap_add.audio", case, audio[b, :R.HOP * n], R.trim(y64), R.trim(y32))
        assert (audio[b, R.HOP * n:] == 0).all() and (full[b, R.padded_len(n):] == 0).all()


@pytest.mark.parametrize("B,T", [(1, 5), (3, 64)])
def test_init_kernel(lib, B, T):
    g = torch.Generator().manual_seed(T)
    mag = (torch.rand(B, T, R.BINS, generator=g) + 0.1).to(_dev())
    spec, prev = torch.full((B, T, R.BINS, 2), SENTINEL, device=_dev()), torch.full((B, T, R.BINS, 2), SENTINEL, device=_dev())
    _call("efts_gl_init", lib.efts_gl_init(mag.data_ptr(), spec.data_ptr(), prev.data_ptr(), B, T, 0, 5, _st()))
    assert torch.equal(spec[..., 0], mag) and (spec[..., 1] == 0).all() and (prev == 0).all()
    _call("efts_gl_init", lib.efts_gl_init(mag.data_ptr(), spec.data_ptr(), prev.data_ptr(), B, T, 1, 5, _st()))
    for b in range(B):
        m = mag[b].cpu()
        _check("efts_gl_init", f"{B}x{T}[{b}]", spec[b], R.initial_spectrum(m.double(), "random", 5), R.initial_spectrum(m, "random", 5))
    spec2 = torch.empty_like(spec)
    _call("efts_gl_init", lib.efts_gl_init(mag.data_ptr(), spec2.data_ptr(), prev.data_ptr(), B, T, 1, 6, _st()))
    assert not torch.equal(spec, spec2)


# ------------------------------------------------------------------------------------------------ 2. round trip
@pytest.mark.parametrize("seconds,seed", SIGNALS)
def test_round_trip_reproduces_the_padded_signal(lib, seconds, seed):
    y32 = R.reflect_pad(R.voiced(seconds, seed)).float()
    T = (y32.shape[0] - 2 * R.PAD) // R.HOP
    lens = torch.tensor([T], dtype=torch.int32, device=_dev())
    Y = k_analysis(lib, lens, 1, T, signal=y32[None].contiguous().to(_dev()))
    back = k_overlap_add(lib, k_synthesis(lib, Y, lens), lens, 0, R.padded_len(T)).cpu()[0]
    ref64, ref32 = R.synthesis(R.analysis(y32.double())), R.synthesis(R.analysis(y32))
    _check("round trip", f"{seconds} s", back, ref64, ref32)
    assert float((ref64 - y32.double())[4:-3].abs().max()) <= 1e-12          # (and the reference's round trip is the signal itself)


# ------------------------------------------------------------------------------------------------ 3. trajectory
@pytest.mark.parametrize("seconds,seed", SIGNALS)
def test_trajectory_vs_fp64(lib, seconds, seed):
    M32 = R.mel_to_magnitude(R.logmel(R.voiced(seconds, seed))).float()
    T = M32.shape[0]
    for n in (1, 2, 4):
        y64, y32 = R.trim(R.griffinlim(M32.double(), n_iter=n)), R.trim(R.griffinlim(M32, n_iter=n))
        got = gpu_loop(lib, M32[None], [T], n)[0]
        e32 = _check("trajectory", f"{seconds} s n={n}", got, y64, y32, factor_only=True)
        assert FACTOR * e32 <= 1e-2, "this n should have been dropped from the test (see the module docstring)"


# ------------------------------------------------------------------------------------------------ 4. / 5. quality, chain consistency
@pytest.mark.parametrize("seconds,seed", SIGNALS)
def test_quality_after_32_iterations(seconds, seed):
    from efficient_tts_amd.griffinlim import GriffinLimVocoder
    lm = R.logmel(R.voiced(seconds, seed))
    M = R.mel_to_magnitude(lm)
    mel = lm.float()[None].to(_dev())
    sc_ref = R.spectral_convergence(R.trim(R.griffinlim(M, n_iter=32)), M)
    a32 = GriffinLimVocoder(_dev(), n_iter=32)(mel)[0, 0].cpu().double()
    a1 = GriffinLimVocoder(_dev(), n_iter=1)(mel)[0, 0].cpu().double()
    sc32, sc1 = R.spectral_convergence(a32, M), R.spectral_convergence(a1, M)
    print(f"SC {seconds} s: device 32 iterations {sc32:.5f}, 1 iteration {sc1:.5f}; float64 reference {sc_ref:.5f}; ratio {sc32 / sc_ref:.4f}")
    assert a32.shape == (R.HOP * lm.shape[1],) and torch.isfinite(a32).all()
    assert sc32 <= 1.05 * sc_ref
    assert sc32 < sc1


@pytest.mark.parametrize("seconds,seed", SIGNALS)
def test_chain_consistency_with_the_front_end(seconds, seed):
    from efficient_tts_amd.frontend import LogMelFrontend
    from efficient_tts_amd.griffinlim import GriffinLimVocoder
    audio = R.voiced(seconds, seed)
    fe = LogMelFrontend(_dev())
    mel, frames = fe(audio.float()[None].to(_dev()), torch.tensor([audio.shape[0]]))
    out = GriffinLimVocoder(_dev())(mel.transpose(1, 2).contiguous(), frames)
    mel2, frames2 = fe(out[:, 0].contiguous(), torch.tensor([audio.shape[0]]))
    assert int(frames2[0]) == int(frames[0]) == mel.shape[1]
    dev_mad = float((mel2 - mel).abs().mean())
    lm = mel[0].t().cpu().double()
    ref_mad = float((R.logmel(R.vocode(lm)) - lm).abs().mean())
    print(f"chain {seconds} s: mean |logmel(vocoder(mel)) - mel| device {dev_mad:.5f}, float64 reference {ref_mad:.5f}, ratio {dev_mad / ref_mad:.4f}")
    assert dev_mad <= 1.05 * ref_mad


# ------------------------------------------------------------------------------------------------ 6. ragged = single, determinism, graphs
@pytest.mark.parametrize("init", ["zero", "random"])
def test_ragged_batch_equals_single_items_and_runs_are_bit_identical(init):
    from efficient_tts_amd.griffinlim import GriffinLimVocoder
    lms = [R.logmel(R.voiced(s, seed)).float() for s, seed in ((0.75, 11), (0.3, 12), (0.52, 13))]
    lens = [m.shape[1] for m in lms]
    T = max(lens)
    mel = torch.randn(3, 80, T)                                        # what lies behind an item's length must not matter
    for b, m in enumerate(lms):
        mel[b, :, :lens[b]] = m
    mel, lens_t = mel.to(_dev()), torch.tensor(lens, device=_dev())
    voc = GriffinLimVocoder(_dev(), n_iter=8, init=init, seed=3, graphs=False)
    batch = voc(mel, lens_t)
    assert batch.shape == (3, 1, R.HOP * T)
    for b in range(3):
        single = voc(mel[b:b + 1, :, :lens[b]].contiguous())
        assert torch.equal(batch[b, 0, :R.HOP * lens[b]], single[0, 0])
        assert (batch[b, 0, R.HOP * lens[b]:] == 0).all()
    assert torch.equal(voc(mel, lens_t), batch)                        # run twice = same bits
    vg = GriffinLimVocoder(_dev(), n_iter=8, init=init, seed=3, graphs=True)
    outs = [vg(mel, lens_t) for _ in range(4)]                         # eager, captured, replayed, replayed
    assert vg._graph_cache.captures == 1
    for o in outs:
        assert torch.equal(o, batch)                                   # graph replay = eager
    if init == "random":
        assert not torch.equal(GriffinLimVocoder(_dev(), n_iter=8, init=init, seed=4, graphs=False)(mel, lens_t), batch)


# ------------------------------------------------------------------------------------------------ 7. mel inversion
@pytest.mark.parametrize("precision,bound", [("fp32", 1e-5), ("bf16x3", 1e-3)])
def test_mel_inversion_vs_numpy_fp64(precision, bound):
    from efficient_tts_amd.griffinlim import GriffinLimVocoder
    lms = [R.logmel(R.voiced(s, seed)).float() for s, seed in ((0.75, 11), (0.3, 12), (9.3, 4))]
    T = max(m.shape[1] for m in lms)
    mel = torch.zeros(3, 80, T)
    for b, m in enumerate(lms):
        mel[b, :, :m.shape[1]] = m
    got = GriffinLimVocoder(_dev(), precision=precision).magnitude(mel.to(_dev())).cpu().double().numpy()
    pinv = np.linalg.pinv(R.filterbank().astype(np.float64))
    ref = np.maximum(np.einsum("fm,bmt->btf", pinv, np.exp(mel.double().numpy())), 1e-5)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"mel inversion {precision}: max |M - M64| / max |M64| = {err:.3e}")
    assert got.shape == (3, T, 513) and err <= bound


# ------------------------------------------------------------------------------------------------ 8. command line
def test_inference_cli_with_griffinlim(tmp_path, capsys):
    import yaml
    from scipy.io.wavfile import read
    from efficient_tts_amd import EfficientTTSCNN
    from efficient_tts_amd.bin.inference import main
    exp = tmp_path / "exp"
    exp.mkdir()
    phones = ["_"] + [f"P{i}" for i in range(1, 76)]
    (tmp_path / "phn.txt").write_text("\n".join(phones) + "\n")
    rng = np.random.default_rng(1)
    lines = [f"DUMMY/utt{n}.wav|" + " ".join(phones[int(i)] for i in rng.integers(1, 76, size=k)) for n, k in enumerate((9, 14, 11))]
    (tmp_path / "test.txt").write_text("\n".join(lines) + "\n")
    params = dict(num_symbols=76, dropout_rate=0.0, use_masking=True, use_weighted_masking=False, sigma=0.01)
    with open(exp / "config.yml", "w") as f:
        yaml.dump(dict(model_name="EfficientTTSCNN", model_params=params, dataset_params=dict(use_phnseq=True, phnset_path=str(tmp_path / "phn.txt"))), f)
    torch.manual_seed(0)
    m = EfficientTTSCNN(**params)
    with torch.no_grad():
        m.duration_predictor.linear.bias.fill_(1.5)              # a few frames per phoneme with random weights
    torch.save({"model": m.state_dict(), "steps": 7}, exp / "checkpoint-7steps.pkl")
    base = ["--checkpoint", str(exp / "checkpoint-7steps.pkl"), "--test_fid_scp", str(tmp_path / "test.txt"), "--verbose", "0", "--vocoder", "griffinlim"]
    assert main(base + ["--outdir", str(tmp_path / "w1"), "--batch_size", "1"]) == 0
    assert main(base + ["--outdir", str(tmp_path / "w3"), "--batch_size", "3", "--gl_iters", "32"]) == 0
    assert main(base + ["--outdir", str(tmp_path / "mel"), "--no_vocoder"]) == 0
    log = capsys.readouterr()
    assert "RANDOM weights" not in log.out + log.err
    for n in range(3):
        sr, a = read(str(tmp_path / "w1" / f"utt{n}_7steps.wav"))
        _, b = read(str(tmp_path / "w3" / f"utt{n}_7steps.wav"))
        mel = np.load(tmp_path / "mel" / f"utt{n}_7steps.npy")
        assert sr == 22050 and a.dtype == np.int16 and a.shape == (mel.shape[0] * 256,) and mel.shape[1] == 80
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals(lib):
    from efficient_tts_amd.griffinlim import GriffinLimVocoder
    for kw in (dict(n_fft=2048, win_size=2048), dict(n_fft=512, win_size=512), dict(n_iter=-1), dict(momentum=1.0), dict(momentum=-0.01)):
        with pytest.raises(ValueError):
            GriffinLimVocoder(_dev(), **kw)
    voc = GriffinLimVocoder(_dev())
    with pytest.raises(ValueError):
        voc(torch.zeros(1, 79, 8, device=_dev()))
    with pytest.raises(RuntimeError):
        voc(torch.zeros(1, 80, 8))
    # the C entries refuse before any launch
    buf = torch.zeros(2 * 4 * R.BINS * 2 + 1, device=_dev())
    lens = torch.tensor([4, 4], dtype=torch.int32, device=_dev())
    w = _window()
    assert lib.efts_gl_synthesis(buf.data_ptr(), lens.data_ptr(), w.data_ptr(), buf.data_ptr(), 2, 4, 512, 256, _st()) == -2
    assert lib.efts_gl_synthesis(buf.data_ptr() + 4, lens.data_ptr(), w.data_ptr(), buf.data_ptr(), 2, 4, 1024, 256, _st()) == -3
    assert lib.efts_gl_synthesis(None, lens.data_ptr(), w.data_ptr(), buf.data_ptr(), 2, 4, 1024, 256, _st()) == -1
    assert lib.efts_gl_analysis(buf.data_ptr(), None, 0, lens.data_ptr(), w.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1.0, 2, 4, 1024, 256, _st()) == -1
    assert lib.efts_gl_analysis(buf.data_ptr(), buf.data_ptr(), 4096, lens.data_ptr(), w.data_ptr(), None, None, buf.data_ptr(), 0.5, 2, 4, 1024, 256, _st()) == -1
    assert lib.efts_gl_analysis(None, buf.data_ptr(), 100, lens.data_ptr(), w.data_ptr(), None, None, buf.data_ptr(), 0.5, 2, 4, 1024, 256, _st()) == -2
    assert lib.efts_gl_overlap_add(buf.data_ptr(), lens.data_ptr(), w.data_ptr(), buf.data_ptr(), 1024, 384, 1025, 2, 4, 1024, 256, _st()) == -2
    assert lib.efts_gl_init(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 2, 0, 0, 0, _st()) == -2
    assert lib.efts_gl_init(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 2, 4, 2, 0, _st()) == -1
