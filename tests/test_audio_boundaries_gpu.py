"""GPU (-m gpu): the audio kernels past one workgroup, one chunk and one scan turn per item.  Each case is the smallest item that crosses the
boundary, in a ragged batch whose other items end before it, with garbage (NaN, full scale, -32768) behind every length, against the float64
reference of its family under that family's existing bound.  tests/test_audio_boundaries_cpu.py holds the conditions on the inputs.

The audit: every constant of the audio kernels that bounds what one workgroup, one chunk or one scan turn takes, the smallest shape that
crosses it, and the test that does.  [new] = a case of this module; the others were crossed before.

    kernel (csrc/)                          constant                                     smallest crossing shape          crossed by
    stoi_energy_kernel (efts_stoi.hip)      SI_E_WAVES * SI_E_ITER = 32 frames / wg      F = 33 (4480 samples)            test_stoi_gpu (F = 182)
    stoi_select_kernel                      256 frames per scan turn (:87)               F = 257 (33 024 samples)         [new] test_stoi_..[scan]
    stoi_spectra_kernel                     SI_S_GROUPS * SI_S_ITER = 32 frames / wg     K = 34                           test_stoi_gpu (K about 90)
    stoi_segment_kernel                     SI_G_GROUPS = 8 segments / wg                M = 9                            test_stoi_gpu (M about 60)
    stoi_reduce_kernel                      SI_CHUNK = 512 segments per step             M = 513 (69 632 dense samples)   [new] test_stoi_..[reduce]
    stft_kernel<256 / 512 / 1024>           2 UPB = 256 / 128 / 64 frames / wg           T = 2 UPB + 1                    [new] test_stft_magnitudes_..
    stft_kernel<2048>                       2 UPB = 32 frames / wg                       T = 33                           test_stft_gpu (35 frames at (2048, 240))
    stft_kernel<512, DIST>                  128 frames / wg                              T = 129                          [new] test_stft_distance_.. (9 and 17 wg)
    stft_reduce_kernel                      ST_CHUNK = 1024 frames per step              T = 1025 (51 200 at hop 50)      [new] test_stft_distance_..
    logspec_project_kernel (efts_mcep.hip)  2 LP_UPB = 128 frames / wg                   T = 129                          [new] test_logspec_project_..
    frame_dist_kernel                       FD_CHUNK = 1024 frames per step              n = 1025                         [new] test_frame_dist_..
    trim_energy_kernel<S, true>             F = 45 / 64 / 21 / 57 frames / wg            F H + 1 samples                  [new] test_trim_.. (energy_plus_1)
    trim_energy_kernel<S, false>            the same F                                   F H + 1 samples                  test_pauses_gpu (70 000 samples)
    trim_bounds_kernel                      TR_THREADS = 256 frames per turn             first / last sound frame > 256   [new] test_trim_.. (*_past_turn)
    trim_copy_kernel                        TR_COPY = 4096 outputs / wg                  new_len = 4097                   [new] test_trim_.. (copy_*)
    pauses: scans and copy (efts_pauses.hip) EFTS_PAUSES_TILE = 256 chunks, PA_COPY = 4096 T = 257; 4097 outputs           test_pauses_gpu (both sides of the tile)
    loud_filter_kernel (efts_loudness.hip)  64 segments of 512 samples / wg              32 769 samples                   test_loudness_gpu (66 150, 96 000 samples)
    loud_decide_kernel                      LD_THREADS = 256 per turn of four loops: segments' peaks, sub-blocks, blocks of either gate
                                                                                         257 segments (131 073 samples); 260 sub-blocks of 100 ms = 257 blocks
                                                                                         (208 000 samples at 8000 Hz)     [new] test_loudness_..
    loud_scale_kernel                       LD_COPY = 4096 outputs / wg                  4097 samples                     test_loudness_gpu (every batch)
    resample_kernel (efts_resample.hip)     RS_NB = 512 outputs / wg                     513 outputs                      test_resample_gpu (4001 samples in)
    Griffin-Lim (efts_griffinlim.hip)       GL_WAVES = 2 frame pairs / wg, 256 samples / wg in synthesis    5 frames      test_griffinlim_gpu (every case)
    yin_kernel (efts_pitch.hip)             G = 4 * (1024 / W) = 8 or 16 frames / wg     G + 1 frames                     test_pitch_gpu (5999 samples: 24 and 47 frames)
    mel_cepstrum_kernel (efts_score.hip)    MC_ROWS = 32 rows / wg                       33 frames                        test_score_gpu (T = 70)
    dtw_kernel, dtw_path                    DTW_BAND = 1024 rows, ring refill at 256 columns, BT_STEPS = 64            test_score_gpu, test_dtw_path_gpu (1023 .. 2049; 255 .. 513)
    f0_path_error_kernel                    F0_THREADS = 256 cells per turn              257 cells                        test_dtw_path_gpu (n = 300)
    denoise / gate / noise profile          DN_RUN = NP_RUN = 16 hops per wave, 4 waves  17 and 65 hops                   test_denoise_gpu, test_gate_gpu (both sides of a run)
    limiter (efts_limiter.hip)              EFTS_LIMITER_CHUNK = 2048 samples / wg       2049 samples                     test_limiter_gpu (both sides of the chunk)
    IIR (efts_iir.hip)                      EFTS_IIR_SEGMENT = 256 samples / thread, 64 segments / wg                     test_iir_gpu (both sides of segment and span)
    istft_head (efts_istft_head.hip)        EFTS_ISTFT_RUN = 1024 samples / wg = FR hops  FR + 1 frames                    test_istft_head_gpu (FR - 1, FR, FR + 1, 3 FR + 1)
    pitch Viterbi (efts_pitch_viterbi.hip)  VIT_BT_ROWS = 256 frames per back-pointer chunk                               test_pitch_viterbi_gpu (both sides of the chunk)

Bounds.  STOI, STFT distance and logspec_project: four times an fp32 CPU yardstick measured on the same inputs, printed with the device's
worst error by each test; EFTS_WRITE_PROFILES=1 writes them to profiles/audio_boundaries_error.json.  STFT magnitudes: the a-priori per-cell
bound of tests/test_stft_gpu.py.  efts_frame_dist: the derived bound in its test's docstring (the derivation closed; no yardstick).  Trimmer:
exact.  Loudness: the fixed bounds of tests/test_loudness_gpu.py.  The speech_like STOI item that reaches K = 543 is 152 320 samples long, the longest input here.

Measured on an MI355X (profiles/audio_boundaries_error.json), device's worst error / fp32 CPU yardstick / bound: STOI scan batch 6.15e-6 /
1.56e-6 / 6.24e-6 (fp32) and 2.27e-6 / 6.95e-7 / 2.78e-6 (int16) -- the worst is ESTOI of the 182-frame neighbour, which never leaves the
first turn: close to the bound, and no boundary's doing.  That item's ESTOI is badly conditioned: in float64 on the CPU, moving every
sample of x and y by a random relative 2^-24 -- half an fp32 rounding -- moves it by 1e-7 .. 3.3e-6, so a few fp32 roundings along the
device's chain account for the figure; fp32 numpy loses 9.3e-7 on it.  (Every seed of the reference modules was searched against the CPU
conditions of tests/test_audio_boundaries_cpu.py alone, before the first device run.) --; STOI reduce batch 9.6e-7 / 3.52e-6 / 1.41e-5 and 3.7e-8 / 2.46e-7 / 9.8e-7;
STFT distance 7.8e-8 / 1.80e-7 / 7.2e-7 relative; logspec_project 3.9e-7 / 6.96e-7 / 2.78e-6 at hop 256 and 9.5e-7 / 6.81e-7 / 2.72e-6 at
hop 120.  STFT magnitudes: at most 0.31 of the per-cell bound (0.025 in the second workgroup).  efts_frame_dist: at most 3.6e-6 against
bounds of 3e-4 .. 6e-4 (1.2e-8 .. 4e-8 against 1.4e-6 .. 1.9e-6 at n = 5).  Loudness: at most 3.6e-15 LU from
the reference (bound 1e-6 LU), gains, flags and block counts equal.  No case found a wrong kernel.

Each of these value-only breaks of a scratch copy of csrc/ (no load or store moves: every changed index stays below the one it replaces)
fails here, at the case named, while the kernel's earlier GPU test passes unless noted:
    `kb[base + off + before]` -> `kb[off + before]` in stoi_select_kernel: test_stoi_..[scan] (the counts stay; the scores are off by 0.06) and [reduce]
    `p[2L * c0 + i]` -> `p[i]` in stoi_reduce_kernel: test_stoi_..[reduce] (scores off by 0.07)
    `p[3L * c0 + i]` -> `p[i]` in stft_reduce_kernel: test_stft_distance_past_the_first_chunk_of_frames (sums off by 9e-3 relative)
    `s0 = t0 * H - N / 2` -> `(t0 % (2 * C::UPB)) * H - N / 2` in stft_kernel: test_stft_magnitudes_..[256 / 512 / 1024], item 2 at frame 256 /
        128 / 64 (test_stft_gpu.py's test_transform_alone[2048-240-1200] fails too: at 2048 it had reached the second workgroup before)
    the same change of `s0` in logspec_project_kernel: test_logspec_project_around_the_second_workgroup
    `xb + (long)(c0 + i) * ldx` -> `xb + (long)i * ldx` in frame_dist_kernel: test_frame_dist_..[25], [24] at n = 1025 (1023 and 1024 pass)
    `(long)f0 * H - pad` -> `-pad` in trim_energy_kernel's staging: test_trim_..[every case] at energy_plus_1: new_len 7680 for 7681
    `e[t]` -> `e[t % TR_THREADS]` in trim_bounds_kernel's search: test_trim_..[every case] at first_sound_past_turn
    `(long)start + o0` -> `(long)start` in trim_copy_kernel's staging: test_trim_..[every case] at output 4096 of energy_full
    `seg_peak[.. + s]` -> `seg_peak[.. + s % LD_THREADS]` in loud_decide_kernel: test_loudness_..[int16-0.5], [float32-0.5] at segments_257
    `sb[j] .. sb[j + 3]` -> the same at `j % LD_THREADS` in both gate loops of loud_decide_kernel: test_loudness_..[every case] at blocks_257
The last one and the one in trim_energy_kernel also fail test_trim_gpu.py's test_trainer_stage_runs_the_trimmer, whose int16 recordings are
longer than one workgroup of launches A and C; the other tests of test_trim_gpu.py pass with all three.
"""
import json
import os

import numpy as np
import pytest
import torch

import loudness_reference as LD
import mcep_reference as MC
import stft_reference as ST
import stoi_reference as SI
import trim_reference as TR
from kernel_check import _call, _st, load_lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _profile(key, value):
    """with EFTS_WRITE_PROFILES set: profiles/audio_boundaries_error.json gains (or replaces) one entry"""
    if not os.environ.get("EFTS_WRITE_PROFILES"):
        return
    path = os.path.join(ROOT, "profiles", "audio_boundaries_error.json")
    report = {}
    if os.path.exists(path):
        with open(path) as f:
            report = json.load(f)
    report[key] = value
    with open(path, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")


# ---- 1. STOI

@pytest.mark.parametrize("which", ["scan", "reduce"])
def test_stoi_past_the_first_scan_turn_and_the_first_chunk_of_segments(lib, which):
    """the bounds of tests/test_stoi_gpu.py: counts and the NaN pattern exactly, both scores within four times what stoi(dtype=float32) loses
    against float64 on these inputs"""
    from efficient_tts_amd.stoi import ShortTimeIntelligibility
    s = ShortTimeIntelligibility(DEV, 10000)
    x, y, lengths, names = SI.boundary_batch(which)
    li = torch.from_numpy(np.array(lengths)).to(DEV)
    report = {}
    for pcm16 in (False, True):
        ref, yard = SI.boundary_reference(which, pcm16), SI.boundary_yardstick(which, pcm16)
        xs, ys = (SI.boundary_pcm16(x, lengths), SI.boundary_pcm16(y, lengths)) if pcm16 else (x, y)
        out = s(torch.from_numpy(np.array(xs)).to(DEV), torch.from_numpy(np.array(ys)).to(DEV), li)
        got = {k: out[k].cpu().numpy() for k in ("stoi", "estoi", "frames", "kept", "segments")}
        worst = 0.0
        for b, r in enumerate(ref):
            assert (int(got["frames"][b]), int(got["kept"][b]), int(got["segments"][b])) == (r["frames"], r["kept"], r["segments"]), (pcm16, names[b])
            for k in ("stoi", "estoi"):
                assert not np.isnan(r[k]) and not np.isnan(got[k][b]), (pcm16, names[b], k)
                err = abs(float(got[k][b]) - r[k])
                print(f"{which} int16 {pcm16} {names[b]} {k}: device {float(got[k][b]):.9f} reference {r[k]:.9f} |difference| {err:.3e}")
                worst = max(worst, err)
        print(f"{which} int16 {pcm16}: max |device - reference| = {worst:.3e}; the definition in fp32 numpy on the CPU: {yard:.3e}; bound 4 x = {4 * yard:.3e}")
        report["int16" if pcm16 else "fp32"] = {"device_max_abs_error": worst, "yardstick_fp32_numpy_cpu_max_abs_error": yard, "bound": 4 * yard}
    _profile(f"stoi_{which}", dict(report, lengths=[int(n) for n in lengths]))
    for v in report.values():
        assert 0.0 < v["yardstick_fp32_numpy_cpu_max_abs_error"] < 1e-5
        assert v["device_max_abs_error"] <= v["bound"]


# ---- 2. STFT magnitudes and distance

@pytest.mark.parametrize("N,H,W", ST.BOUNDARY_MAG)
def test_stft_magnitudes_around_the_second_workgroup(lib, N, H, W):
    """the per-cell a-priori bound of tests/test_stft_gpu.py: |mag - ref| <= eps (log2 N + 4) ||X_t||_2 + 4 eps ref, eps = 2^-23"""
    from efficient_tts_amd.stft import STFTMagnitude
    lengths = ST.boundary_mag_lengths(N, H)
    per = ST.FRAMES_PER_WORKGROUP[N]
    f32, _ = ST.boundary_batch(lengths, 300 + N)                        # NaN behind every item
    pcm, _ = ST.boundary_batch(lengths, 300 + N, fp32_x=False)          # -32768 behind every item
    op = STFTMagnitude(DEV, N, H, W)
    li = torch.tensor(lengths)
    mag, frames = op(torch.from_numpy(pcm).to(DEV), li)
    mag_f, frames_f = op(torch.from_numpy(f32).to(DEV), li)
    mag, mag_f = mag.cpu().numpy(), mag_f.cpu().numpy()
    assert mag.shape == (4, per + 2, N // 2 + 1)
    assert frames.tolist() == frames_f.tolist() == [per - 1, per, per + 1, per + 2]
    assert np.array_equal(mag.view(np.uint32), mag_f.view(np.uint32))   # int16 PCM == the same values as fp32
    for b, n in enumerate(lengths):
        ref = ST.magnitudes(pcm[b, :n], N, H, W)
        T = ref.shape[0]
        assert not mag[b, T:].any()                                     # rows at and beyond the item's count
        norm = np.sqrt(2.0 * (ref ** 2).sum(axis=1) - ref[:, 0] ** 2 - ref[:, -1] ** 2)
        tol = EPS * (np.log2(N) + 4) * norm[:, None] + 4 * EPS * ref
        ratio = np.abs(mag[b, :T] - ref) / tol
        t_bad = int(np.argmax(ratio.max(axis=1)))
        print(f"N {N} H {H} W {W} item {b} len {n}: {T} frames, largest |mag - ref| / bound {ratio.max():.3f} (frame {t_bad}); "
              f"in the second workgroup {ratio[per:].max() if T > per else 0.0:.3f}")
        assert (ratio <= 1.0).all(), (b, t_bad)
        assert ratio.max() > 0.0


@pytest.fixture(scope="module")
def dist_inputs():
    lengths = ST.boundary_dist_lengths()
    x, y = ST.boundary_batch(lengths, 700)
    ref = ST.distance(x, y, lengths, (ST.BOUNDARY_DIST,))
    for v in (x, y, *ref.values()):
        v.setflags(write=False)
    return lengths, x, y, ref


def _torch_stft_yardstick(lengths, x, y, ref, N, H, W):
    """the rule of tests/test_stft_gpu.py: the largest relative error of num, den, l1 through torch.stft in fp32 on the CPU, on these inputs"""
    worst = 0.0
    win = torch.from_numpy(ST.window(W))
    for b, n in enumerate(lengths):
        xf = torch.from_numpy(x[b:b + 1, :n].copy())
        yf = torch.from_numpy(y[b:b + 1, :n].astype(np.float32) / np.float32(ST.MAX_WAV))
        mags = []
        for s in (xf, yf):
            spec = torch.stft(s, N, H, W, win, return_complex=True)
            mags.append(torch.sqrt(torch.clamp(spec.real ** 2 + spec.imag ** 2, min=1e-7)))
        mx, my = mags
        got = [float(((my - mx) ** 2).sum()), float((my ** 2).sum()), float((torch.log(my) - torch.log(mx)).abs().sum())]
        err = [abs(g - w) / w for g, w in zip(got, ref["sums"][b, 0])]
        print(f"fp32 torch.stft item {b} len {n}: relative error of num, den, l1 {err[0]:.2e} {err[1]:.2e} {err[2]:.2e}")
        worst = max(worst, *err)
    return worst


def test_stft_distance_past_the_first_chunk_of_frames(lib, dist_inputs):
    """the rule of test_distance_against_float64: num, den and l1 within four times the fp32 torch.stft yardstick on these inputs; cells exact"""
    from efficient_tts_amd.stft import MultiResolutionSTFTDistance
    lengths, x, y, ref = dist_inputs
    N, H, W = ST.BOUNDARY_DIST
    yard = _torch_stft_yardstick(lengths, x, y, ref, N, H, W)
    out = MultiResolutionSTFTDistance(DEV, (ST.BOUNDARY_DIST,))(torch.from_numpy(np.array(x)).to(DEV), torch.from_numpy(np.array(y)).to(DEV),
                                                               torch.tensor(lengths))
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.array_equal(got["cells"], ref["cells"]) and got["cells"][:, 0].tolist() == [T * (N // 2 + 1) for T in ST.BOUNDARY_DIST_FRAMES]
    bound, worst, errors = 4.0 * yard, 0.0, {}
    for b, n in enumerate(lengths):
        err = np.abs(got["sums"][b, 0] - ref["sums"][b, 0]) / ref["sums"][b, 0]
        errors[f"len{n}"] = [float(e) for e in err]
        print(f"item {b} len {n} ({ST.BOUNDARY_DIST_FRAMES[b]} frames): relative error of num, den, l1 {err[0]:.2e} {err[1]:.2e} {err[2]:.2e}")
        worst = max(worst, float(err.max()))
    print(f"yardstick (fp32 torch.stft, largest relative error) {yard:.3e}, bound 4 x = {bound:.3e}, device's largest relative error {worst:.3e}")
    _profile("stft_distance", {"resolution": list(ST.BOUNDARY_DIST), "lengths": list(lengths), "yardstick_fp32_torch_stft_cpu_max_rel_error": yard,
                               "bound": bound, "device_max_rel_error": worst, "device_rel_error_num_den_l1": errors})
    assert 0.0 < yard < 1e-5
    assert worst <= bound
    # fp32 x against int16 y above; both as int16 give the same bits
    x16 = np.full(x.shape, -32768, dtype=np.int16)
    for b, n in enumerate(lengths):
        x16[b, :n] = np.round(x[b, :n] * np.float32(ST.MAX_WAV)).astype(np.int16)
    again = MultiResolutionSTFTDistance(DEV, (ST.BOUNDARY_DIST,))(torch.from_numpy(x16).to(DEV), torch.from_numpy(np.array(y)).to(DEV), torch.tensor(lengths))
    assert again["sums"].cpu().numpy().tobytes() == got["sums"].tobytes()


# ---- 3. waveform mel-cepstra

def test_logspec_project_around_the_second_workgroup(lib):
    """the bound of tests/test_mcep_gpu.py: four times what the same definition in fp32 on the CPU loses against float64 on these inputs"""
    from efficient_tts_amd.mcep import MelCepstrum
    report = {}
    for name, pcm16, H, W in MC.BOUNDARY_CONFIGS:
        ref, yard = MC.boundary_reference(pcm16, H, W), MC.boundary_yardstick(pcm16, H, W)
        assert all(low >= 1e-5 for _, low in ref)
        x, lengths = MC.boundary_batch(pcm16, H)
        mc, frames = MelCepstrum(DEV, hop_size=H, win_length=W)(torch.from_numpy(np.array(x)).to(DEV), torch.from_numpy(np.array(lengths)).to(DEV))
        assert mc.shape == (4, 1 + x.shape[1] // H, MC.ORDER) == (4, 130, MC.ORDER) and frames.tolist() == [127, 128, 129, 130]
        got = mc.cpu().numpy().astype(np.float64)
        assert not np.isnan(got).any()
        worst = 0.0
        for b, (r, _) in enumerate(ref):
            assert not got[b, len(r):].any()                           # rows at and beyond T are 0
            err = np.abs(got[b, :len(r)] - r).max(axis=1)
            print(f"{name} item {b} ({len(r)} frames): max |device - reference| {err.max():.3e} (frame {int(err.argmax())}); from frame 128 on "
                  f"{err[128:].max() if len(r) > 128 else 0.0:.3e}")
            worst = max(worst, float(err.max()))
        print(f"{name}: max |device - reference| = {worst:.3e}; the definition in fp32 on the CPU: {yard:.3e}; bound 4 x = {4 * yard:.3e}")
        report[name] = {"device_max_abs_error": worst, "yardstick_fp32_torch_cpu_max_abs_error": yard, "bound": 4 * yard,
                        "lengths": [int(n) for n in lengths]}
    _profile("logspec_project", report)
    for v in report.values():
        assert 0.0 < v["yardstick_fp32_torch_cpu_max_abs_error"] < 1e-4
        assert v["device_max_abs_error"] <= v["bound"]


@pytest.mark.parametrize("D", MC.DIST_DIMS)
def test_frame_dist_past_the_first_chunk_of_frames(lib, D):
    """`efts_frame_dist` alone on synthetic frames, n = min(Ta, Tb) = 1023, 1024, 1025, 2049 and 5, NaN in every row at and beyond a count.

    The bound is derived, not measured (u = 2^-24).  Per frame frame_dist_kernel rounds in fp32: the D differences (1 + e, |e| <= u each, so
    their squares carry (1 + e)^2), the D fused additions of the sum of squares (a factor within 1 +- gamma_D of every term, gamma_k =
    k u / (1 - k u)), and the square root, which halves the relative error of its argument and adds at most one ulp = 2 u of its own.  All
    terms are non-negative, so frame t's distance comes out within (gamma_(D + 2) / 2 + 2 u) d_t <= (D / 2 + 4) u d_t of the exact d_t.
    The frames are then added in float64 in frame order: n 2^-53 relative, and the reference adds in the same order.  So
        |cost - reference| <= ((D / 2 + 4) 2^-24 + n 2^-53) * sum_t d_t,
    which lies below the n D 2^-24 that an fp32 sum over the frames would need.  `count` is exact."""
    x, xf, y, yf = MC.dist_frames(D)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    xl, yl = torch.from_numpy(xf).to(DEV), torch.from_numpy(yf).to(DEV)
    B = x.shape[0]
    cost = torch.full((B,), -1.0, dtype=torch.float64, device=DEV)
    count = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    _call("efts_frame_dist", lib.efts_frame_dist(xd.data_ptr(), xd.stride(1), xd.stride(0), xl.data_ptr(), x.shape[1], yd.data_ptr(), yd.stride(1),
                                                 yd.stride(0), yl.data_ptr(), y.shape[1], D, cost.data_ptr(), count.data_ptr(), B, _st()))
    torch.cuda.synchronize()
    cost, count = cost.cpu().numpy(), count.cpu().numpy()
    assert count.tolist() == list(MC.DIST_COUNTS)
    for b, n in enumerate(MC.DIST_COUNTS):
        ref, ref_n = MC.aligned_cost(x[b, :xf[b]].astype(np.float64), y[b, :yf[b]].astype(np.float64))
        assert ref_n == n
        bound = ((D / 2 + 4) * 2.0 ** -24 + n * 2.0 ** -53) * ref
        print(f"D {D} n {n}: cost {cost[b]:.9f} reference {ref:.9f} |difference| {abs(cost[b] - ref):.3e} bound {bound:.3e}")
        assert abs(cost[b] - ref) <= bound, (D, n)


# ---- 4. trimmer

def _trim(lib, x, lengths, W, H, peak, ld_out):
    """efts_trim / efts_trim_pcm16 through the binding, as tests/test_trim_gpu.py calls them; every output is pre-filled with a sentinel and the
    output row is followed by sentinel rows of its own"""
    xd = torch.from_numpy(np.array(x)).to(DEV).contiguous()
    B, ld_in = xd.shape
    pcm = xd.dtype == torch.int16
    li = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    out = torch.full((B + 1, ld_out), 7.0, dtype=torch.float32, device=DEV)
    new_len = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    start = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    gain = torch.full((B,), -1.0, dtype=torch.float32, device=DEV)
    ws = torch.empty(max(16, int(lib.efts_trim_workspace_bytes(B, ld_in, H, int(pcm)))), dtype=torch.uint8, device=DEV)
    head = (xd.data_ptr(), ld_in, li.data_ptr(), W, H, TR.ratio(TR.TOP_DB), TR.BOUNDARY_KEEP, 0.0 if peak is None else peak)
    tail = (out.data_ptr(), ld_out, new_len.data_ptr(), start.data_ptr(), gain.data_ptr(), ws.data_ptr(), B, _st())
    rc = lib.efts_trim_pcm16(*head, 1.0 / 32768.0, *tail) if pcm else lib.efts_trim(*head, *tail)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), new_len.cpu().numpy(), start.cpu().numpy(), gain.cpu().numpy()


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("peak", [0.95, None])
@pytest.mark.parametrize("W,H", TR.BOUNDARY_PAIRS)
@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_trim_past_one_workgroup_of_every_launch(lib, dtype, W, H, peak, aligned):
    """the bounds of tests/test_trim_gpu.py: start and new_len exactly, the gain from the reference's exact peak, every sample float32(x) * g
    bit for bit, +0.0 behind new_len up to ld_out, the sentinel intact beyond"""
    x, lengths = TR.boundary_items(W, H, dtype)
    ld_out = x.shape[1] + (5 if aligned else 6)                        # rows 16-byte aligned (float4 stores), and not (dword stores)
    assert (ld_out % 4 == 0) == aligned
    rc, out, new_len, start, gain = _trim(lib, x, lengths, W, H, peak, ld_out)
    assert rc == 0
    for b, (name, n) in enumerate(zip(TR.BOUNDARY_NAMES, lengths)):
        ref = TR.trim(x[b, :n], W=W, H=H, top_db=TR.TOP_DB, keep_frames=TR.BOUNDARY_KEEP, peak=peak)
        print(f"{np.dtype(dtype).name} W {W} H {H} peak {peak} {name} len {n}: start {start[b]} ({ref['start']}) new_len {new_len[b]} "
              f"({ref['new_len']}) gain {gain[b]!r} ({ref['gain']!r})")
        assert (int(start[b]), int(new_len[b])) == (ref["start"], ref["new_len"]), name
        assert gain[b].view(np.uint32) == ref["gain"].view(np.uint32), name
        same = out[b, :ref["new_len"]].view(np.uint32) == ref["out"].view(np.uint32)
        assert same.all(), (name, int(np.argmin(same)))
        assert np.array_equal(out[b, ref["new_len"]:].view(np.uint32), np.zeros(ld_out - ref["new_len"], np.uint32)), name     # +0.0, up to ld_out
    assert (out[len(lengths)] == 7.0).all()                            # the sentinel behind the last row


# ---- 5. loudness: the one constant the audit found uncrossed

@pytest.mark.parametrize("ceiling", [None, 0.5])
@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_loudness_past_the_first_turn_of_the_decision_loops(lib, dtype, ceiling):
    """the bounds of tests/test_loudness_gpu.py: lufs within 1e-6 LU, the gain within 4e-7 relative, flags and both block counts exactly, every
    sample float32(x) * the device's gain bit for bit, +0.0 behind every length"""
    from efficient_tts_amd.loudness import LoudnessNormalizer
    from test_loudness_gpu import GAIN_RTOL, LUFS_TOL
    case = LD.boundary_case(ceiling)
    x = case["x"] if dtype == np.int16 else LD.as_float(case["x"])
    ref = LD.reference(case, dtype)
    n = LoudnessNormalizer(DEV, case["fs"], target_lufs=case["target"], peak_ceiling=ceiling)
    res = n(torch.from_numpy(np.array(x)).to(DEV), torch.tensor(case["lengths"]), return_stats=True)
    torch.cuda.synchronize()
    out, lufs, gains, flags, blocks = (t.cpu().numpy() for t in res)
    for b, (name, v, r) in enumerate(zip(LD.BOUNDARY_NAMES, case["lengths"], ref)):
        d_lufs, d_gain = abs(lufs[b] - r["lufs"]), abs(float(gains[b]) / float(r["gain"]) - 1.0)
        print(f"ceiling {ceiling} {np.dtype(dtype).name} {name} len {v}: {lufs[b]:.9f} LUFS (ref {r['lufs']:.9f}, off {d_lufs:.3g} LU) gain {gains[b]!r} "
              f"(ref {r['gain']!r}, off {d_gain:.3g}) flags {flags[b]} ({r['flags']}) blocks {tuple(blocks[b])} ({r['blocks']})")
        assert d_lufs <= LUFS_TOL, name
        assert tuple(int(k) for k in blocks[b]) == r["blocks"], name
        assert int(flags[b]) == r["flags"], name
        assert d_gain <= GAIN_RTOL, name
        want = x[b, :v].astype(np.float32) * gains[b]
        assert np.array_equal(out[b, :v].view(np.uint32), want.view(np.uint32)), name
        assert np.array_equal(out[b, v:].view(np.uint32), np.zeros(x.shape[1] - v, np.uint32)), name
        if ceiling is not None:
            assert float(np.abs(out[b]).max()) <= ceiling, name
