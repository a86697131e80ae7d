"""No GPU: the inputs of tests/test_audio_boundaries_gpu.py.  Every item must cross the boundary it was built for -- the frame, kept, segment,
chunk and turn counts are asserted against the constants, which are read from csrc/ (include/efts_abi.h exports none of them) -- and must meet
the margin condition of its family's existing CPU test, with no item left out.  Only the references run here."""
import math
import os
import re

import numpy as np
import pytest

import loudness_reference as LD
import mcep_reference as MC
import stft_reference as ST
import stoi_reference as SI
import trim_reference as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(name):
    with open(os.path.join(ROOT, "efficient_tts_amd", "csrc", name)) as f:
        return f.read()


def _const(src, name):
    return int(re.search(r"\b%s = (\d+)" % name, src).group(1))


# ---- STOI

def test_stoi_constants_are_those_of_the_kernels():
    src = _src("efts_stoi.hip")
    assert _const(src, "SI_CHUNK") == 512                              # csrc/efts_stoi.hip:41
    assert "for (int c0 = 0; c0 < F; c0 += 256)" in src                # the scan turn of stoi_select_kernel, csrc/efts_stoi.hip:87
    assert _const(src, "SI_SEG") == SI.SEGMENT


@pytest.mark.parametrize("pcm16", [False, True])
def test_stoi_scan_items_cross_the_second_turn_with_a_carried_base_that_is_no_frame_index(pcm16):
    x, y, lengths, names = SI.boundary_batch("scan")
    assert lengths.tolist() == [32896, 33024, 38528, 23424] and names == ("F256", "F257", "F300", "F182")
    ref = SI.boundary_reference("scan", pcm16)
    xs = SI.boundary_pcm16(x, lengths).astype(np.float32) / np.float32(32768.0) if pcm16 else x
    for b, (n, r) in enumerate(zip(lengths, ref)):
        keep = SI.keep_flags(xs[b, :n])
        print(f"int16 {pcm16} {names[b]}: frames {r['frames']} kept {r['kept']} (before frame 256: {int(keep[:256].sum())}, dropped there "
              f"{int((~keep[:256]).sum())}; from 256 on: {int(keep[256:].sum())}) segments {r['segments']} margin {r['margin_db']:.4f} dB")
        assert r["margin_db"] >= 0.01                                  # the cap of tests/test_stoi_cpu.py
        assert r["frames"] == SI.SCAN_FRAMES[b] == len(keep) and r["kept"] == int(keep.sum()) and r["segments"] == r["kept"] - 30 > 0
        assert math.ceil(r["frames"] / 256) == (1, 2, 2, 1)[b]         # turns of the scan
        assert (~keep[:256]).sum() >= 1 and keep[:256].sum() >= 1      # the base carried into the second turn is below 256
        if r["frames"] > 256:
            assert keep[256:].sum() >= 1 and keep[r["frames"] - 1]     # kept frames on both sides of frame 256 (F = 257: frame 256 itself)
        else:
            assert keep[r["frames"] - 1] == (b == 0)                   # the full turn's last lane holds a kept frame
    assert np.isnan(x[0, lengths[0]:]).all() and np.isnan(y[3, lengths[3]:]).all()


@pytest.mark.parametrize("pcm16", [False, True])
def test_stoi_reduce_items_cross_the_second_and_third_chunk(pcm16):
    x, y, lengths, names = SI.boundary_batch("reduce")
    assert lengths[:3].tolist() == [69504, 69632, 135168]
    ref = SI.boundary_reference("reduce", pcm16)
    for b, r in enumerate(ref):
        print(f"int16 {pcm16} {names[b]}: samples {lengths[b]} frames {r['frames']} kept {r['kept']} segments {r['segments']} margin {r['margin_db']:.4f} dB")
        assert r["margin_db"] >= 0.01
    assert [r["segments"] for r in ref[:4]] == [512, 513, 1025, 513] == list(SI.REDUCE_SEGMENTS[:4])
    assert [math.ceil(r["segments"] / 512) for r in ref] == [1, 2, 3, 2, 1]
    assert all(r["kept"] == r["frames"] for r in ref[:3])              # the dense items: no silent frame
    assert ref[3]["kept"] == 543 and 0.3 * ref[3]["frames"] < ref[3]["kept"] < 0.7 * ref[3]["frames"]
    assert 0 < ref[4]["segments"] < 512
    for r in ref:                                                      # noise that grows along the item: no score near 1, none near 0
        assert 0.05 < r["estoi"] < 0.95 and 0.05 < r["stoi"] < 0.95


def test_stoi_fast_truncation_is_the_slow_one():
    base = SI.speech_like(SI.LD, 7)
    for K in (30, 31, 60):
        assert SI.truncate_to_kept_fast(base, K) == SI.truncate_to_kept(base, K)
    full = SI.speech_like(160000, SI.REDUCE_SEEDS[3])
    n = SI.truncate_to_kept_fast(full, 543)
    assert n == SI.boundary_batch("reduce")[2][3]
    assert SI.stoi(full[:n], full[:n])["kept"] == 543 and SI.stoi(full[:n - SI.HOP], full[:n - SI.HOP])["kept"] == 542


def test_stoi_yardsticks_are_fp32_rounding_errors():
    for which in ("scan", "reduce"):
        for pcm16 in (False, True):
            yard = SI.boundary_yardstick(which, pcm16)
            print(f"{which} int16 {pcm16}: fp32 numpy yardstick {yard:.3e}")
            assert 0.0 < yard < 1e-5


# ---- STFT

def test_stft_constants_are_those_of_the_kernels():
    src = _src("efts_stft.hip")
    it = _const(src, "ST_ITER")
    for N, per in ST.FRAMES_PER_WORKGROUP.items():
        m, p, waves = (int(v) for v in re.search(r"st_geo<%d>\s*\{ static constexpr int M = (\d+), P = (\d+), WAVES = (\d+);" % N, src).groups())
        assert 2 * waves * (64 // (m * p)) * it == per                 # 2 UPB, csrc/efts_stft.hip:40
    assert _const(src, "ST_CHUNK") == ST.REDUCE_CHUNK


def test_stft_items_sit_around_the_second_workgroup_and_the_second_and_third_chunk():
    for N, H, W in ST.BOUNDARY_MAG:
        per = ST.FRAMES_PER_WORKGROUP[N]
        lengths = ST.boundary_mag_lengths(N, H)
        assert [ST.frame_count(n, N, H) for n in lengths] == [per - 1, per, per + 1, per + 2]
        assert (N, H, W) in ((256, 64, 256),) + ST.DEFAULT             # hops the project already uses
    assert ST.boundary_mag_lengths(256, 64) == (16256, 16320, 16384, 16448)
    N, H, W = ST.BOUNDARY_DIST
    lengths = ST.boundary_dist_lengths()
    assert lengths == (51150, 51200, 102400, 6450)
    T = [ST.frame_count(n, N, H) for n in lengths]
    assert T == [1024, 1025, 2049, 130] and [math.ceil(t / ST.REDUCE_CHUNK) for t in T] == [1, 2, 3, 1]
    assert [math.ceil(t / ST.FRAMES_PER_WORKGROUP[N]) for t in T] == [8, 9, 17, 2]
    x, y = ST.boundary_batch(ST.boundary_mag_lengths(256, 64), 300)
    assert np.isnan(x[0, 16256:]).all() and (y[0, 16256:] == -32768).all() and not np.isnan(x[3]).any()
    x16, _ = ST.boundary_batch(ST.boundary_mag_lengths(256, 64), 300, fp32_x=False)
    assert np.array_equal(x16[0, :16256].astype(np.float32) / np.float32(32768.0), x[0, :16256]) and (x16[0, 16256:] == -32768).all()


# ---- waveform mel-cepstra

def test_mcep_constants_are_those_of_the_kernels():
    src = _src("efts_mcep.hip")
    assert 2 * _const(src, "LP_WAVES") * _const(src, "LP_ITER") == MC.FRAMES_PER_WORKGROUP and "LP_UPB = LP_WAVES * LP_ITER" in src
    assert _const(src, "FD_CHUNK") == MC.DIST_CHUNK and _const(src, "FD_MAX_DIM") == 32


def test_mcep_items_sit_around_the_second_workgroup_and_stay_off_the_clamp():
    for name, pcm16, H, W in MC.BOUNDARY_CONFIGS:
        x, lengths = MC.boundary_batch(pcm16, H)
        assert [ST.frame_count(int(n), MC.N, H) for n in lengths] == [127, 128, 129, 130]
        assert all(H * (T - 1) <= n < H * T for n, T in zip(lengths, MC.BOUNDARY_FRAMES))
        ref = MC.boundary_reference(pcm16, H, W)
        print(f"{name}: lengths {lengths.tolist()}, smallest power cell {min(low for _, low in ref):.3e}")
        assert [len(r) for r, _ in ref] == [127, 128, 129, 130]
        assert all(low >= 1e-5 for _, low in ref)                      # the condition of tests/test_mcep_gpu.py: 100 x above the clamp
        bad = x[0, lengths[0]:]
        assert (bad == -32768).all() if pcm16 else np.isnan(bad).all()
    a, b = MC.boundary_batch(False, 256), MC.boundary_batch(True, 256)
    assert np.array_equal(a[0][2, :a[1][2]], b[0][2, :b[1][2]].astype(np.float32) / np.float32(32768.0))


def test_mcep_frame_pairs_sit_around_the_second_and_third_chunk():
    assert MC.DIST_DIMS == (25, 24) and all(D <= 32 for D in MC.DIST_DIMS)
    for D in MC.DIST_DIMS:
        x, xf, y, yf = MC.dist_frames(D)
        n = np.minimum(xf, yf)
        assert n.tolist() == [1023, 1024, 1025, 2049, 5] and [math.ceil(v / MC.DIST_CHUNK) for v in n] == [1, 1, 2, 3, 1]
        assert (xf != yf).all() and (xf < yf).any() and (xf > yf).any()          # either side is the shorter one
        for b in range(len(n)):
            assert np.isnan(x[b, xf[b]:]).all() and np.isnan(y[b, yf[b]:]).all() and not np.isnan(x[b, :xf[b]]).any() and not np.isnan(y[b, :yf[b]]).any()
            d = MC.frame_distances(x[b, :xf[b]].astype(np.float64), y[b, :yf[b]].astype(np.float64))
            assert len(d) == n[b] and d.min() > 0 and d[-1] > 2 * d[0]          # the distance grows along the item


# ---- trimmer

def test_trim_constants_are_those_of_the_kernels():
    src = _src("efts_trim_energy.h")
    assert (_const(src, "TR_THREADS"), _const(src, "TR_COPY")) == (TR.SCAN_TURN, TR.COPY_BLOCK)
    assert (_const(src, "TR_SPAN_MAX"), _const(src, "TR_F_MAX")) == (12288, 64)
    assert "max(1, min(TR_F_MAX, (TR_SPAN_MAX - W) / H + 1))" in src   # csrc/efts_trim_energy.h:106
    assert [TR.energy_frames(W, H) for W, H in TR.BOUNDARY_PAIRS] == [45, 64, 21, 57, 56]
    assert TR.BOUNDARY_PAIRS[:4] == TR.PAIRS and "t += TR_THREADS" in _src("efts_trim.hip")


@pytest.mark.parametrize("W,H", TR.BOUNDARY_PAIRS)
def test_trim_items_cross_every_boundary_and_keep_their_distance_from_the_threshold(W, H):
    pcm, lengths = TR.boundary_items(W, H, np.int16)
    x, lengths32 = TR.boundary_items(W, H, np.float32)
    assert lengths == lengths32 and pcm.shape[1] % 8 == 3 and (pcm.shape[1] + 5) % 4 == 0 and (pcm.shape[1] + 6) % 4 != 0
    F = TR.energy_frames(W, H)
    res = {}
    for b, (name, n) in enumerate(zip(TR.BOUNDARY_NAMES, lengths)):
        assert (pcm[b, n:] == 32767).all()
        r = TR.trim(x[b, :n], W=W, H=H, keep_frames=TR.BOUNDARY_KEEP, peak=0.95)
        q = TR.trim(pcm[b, :n], W=W, H=H, keep_frames=TR.BOUNDARY_KEEP, peak=0.95)
        print(f"W {W} H {H} {name} len {n}: start {r['start']} new_len {r['new_len']} margin {r['margin_db']:.4f} dB")
        assert r["margin_db"] >= 0.01 and q["margin_db"] >= 0.01       # the condition of tests/test_trim_cpu.py
        assert (r["start"], r["new_len"]) == (q["start"], q["new_len"])
        res[name] = dict(r, n=n, T=-(-n // H))
    # launch A: exactly one workgroup's frames, and one frame more whose energy decides new_len and whose chunk holds the peak
    full, plus = res["energy_full"], res["energy_plus_1"]
    assert (full["n"], full["T"], plus["n"], plus["T"]) == (F * H, F, F * H + 1, F + 1)
    assert full["start"] + full["new_len"] == F * H and plus["start"] + plus["new_len"] == F * H + 1 and plus["start"] > 0
    assert plus["gain"] == np.float32(0.95) / np.float32(30000 * 2.0 ** -15) == full["gain"]
    # launch B: the first and the last sound frame in the second turn of the strided loops
    first, last = res["first_sound_past_turn"], res["last_sound_past_turn"]
    assert first["T"] > TR.SCAN_TURN and first["start"] // H > TR.SCAN_TURN and first["start"] % H == 0 and first["start"] > 256 * H
    assert last["T"] > TR.SCAN_TURN and last["start"] // H < 8 and last["start"] + last["new_len"] < last["n"]
    assert (last["start"] + last["new_len"]) // H - 1 > TR.SCAN_TURN
    # launch C: one output under a workgroup, exactly one, one over, and a third workgroup
    assert [res[k]["new_len"] for k in ("copy_4095", "copy_4096", "copy_4097", "copy_8293")] == [4095, 4096, 4097, 8293]
    assert all(res[k]["start"] > 0 for k in ("copy_4095", "copy_4096", "copy_4097", "copy_8293"))
    assert first["new_len"] < TR.COPY_BLOCK or W == 2048
    if H == 202:
        assert all(res[k]["start"] % 4 == 2 for k in ("copy_4095", "copy_4096", "copy_4097", "copy_8293"))     # no multiple of 4 (fp32) or 8 (int16)


# ---- loudness

def test_loudness_constants_are_those_of_the_kernels():
    with open(os.path.join(ROOT, "include", "efts_abi.h")) as f:
        assert int(re.search(r"#define EFTS_LOUDNESS_SEGMENT (\d+)", f.read()).group(1)) == LD.SEGMENT == 512
    src = _src("efts_loudness.hip")
    assert _const(src, "LD_THREADS") == LD.DECIDE_TURN                 # csrc/efts_loudness.hip:24
    assert src.count("+= LD_THREADS") >= 4                             # the sub-blocks, the segments' peaks and both gates: :115, :122, :132, :142


@pytest.mark.parametrize("ceiling", [None, 0.5])
def test_loudness_items_cross_the_second_turn_of_every_loop_and_keep_their_distance_from_the_gates(ceiling):
    case = LD.boundary_case(ceiling)
    h, turn = case["fs"] // 10, LD.DECIDE_TURN
    assert (case["fs"], h) == (8000, 800) and case["lengths"] == [131073, 207200, 208000, 208923, 40000]
    counts = [(-(-n // LD.SEGMENT), n // h, max(n // h - 3, 0)) for n in case["lengths"]]          # segments, sub-blocks, blocks
    assert counts == [(257, 163, 160), (405, 259, 256), (407, 260, 257), (409, 261, 258), (79, 50, 47)]
    assert [tuple(math.ceil(c / turn) for c in item) for item in counts] == [(2, 1, 1), (2, 2, 1), (2, 2, 2), (2, 2, 2), (1, 1, 1)]
    for dtype in (np.int16, np.float32):
        x = case["x"] if dtype == np.int16 else LD.as_float(case["x"])
        ref = LD.reference(case, dtype)
        for b, (name, n, r) in enumerate(zip(LD.BOUNDARY_NAMES, case["lengths"], ref)):
            print(f"ceiling {ceiling} {np.dtype(dtype).name} {name} len {n}: {r['lufs']:.4f} LUFS, blocks {r['blocks']} of {len(r['z'])}, flags {r['flags']}, "
                  f"margin {r['margin_lu']:.4f} LU, ceiling margin {r['ceiling_margin']:.4g}")
            assert r["margin_lu"] >= 0.01 and r["ceiling_margin"] >= 1e-3         # the conditions of tests/test_loudness_cpu.py
            assert len(r["z"]) == counts[b][2] and r["flags"] == (0 if ceiling is None else 2)
            assert (case["x"][b, n:] == 32767).all()
            peak_at = int(np.argmax(np.abs(x[b, :n].astype(np.float64))))
            if name in ("segments_257", "blocks_258_late"):            # the peak in a segment of the second turn
                assert peak_at // LD.SEGMENT >= turn
            else:
                assert peak_at // LD.SEGMENT < turn
        late, others = ref[3], LD.measure(x[3, :256 * h], case["fs"], case["target"], ceiling)
        assert late["lufs"] > others["lufs"] + 0.3                     # the sub-blocks from 256 on move the loudness by 3e5 x the tolerance
        assert ref[2]["blocks"][0] == 257 and ref[3]["blocks"][0] == 258 and ref[3]["blocks"][1] > ref[2]["blocks"][1]
        gamma_r = 0.1 * late["z"][late["z"] > LD.GAMMA_A].mean()
        assert (late["z"][256:] > gamma_r).all() and ref[2]["z"][256] > LD.GAMMA_A       # blocks of the second turn pass the gates they meet
