"""GPU (-m gpu): the six entry points of csrc/efts_frontend.hip, each alone, against the float64 restatement in tests/frontend_reference.py (which
never sees the product's code).  tests/test_frontend_reference_cpu.py pins that reference and proves, without a device, the conditions these
tests rely on (no compared cell near the clamp, every `_check` case conditioned, every filterbank on the side of the table limit named here).

Bounds.  Whole filterbanks: `kernel_check._check`, per item -- max |got - ref64| / max |ref64| within 8 x the error of the stage's fp32
transcription on the CPU (torch.stft for the transform), floor 2e-6.  Operand planes: element by element, |got - ref64| <= r |ref64| +
2^-24 |ref64|, r = 2^-8 (bf16) or 2^-16 (bf16x3), the 2^-24 for the one fp32 product sample x window.

Bin by bin (one-hot filterbanks; derived, not measured).  An fp32 FFT of N points is off by at most about log2(N) eps ||X_t||_2 in every bin
(Higham, Accuracy and Stability of Numerical Algorithms, 24.2; tests/test_stft_gpu.py), the window product, the untangling of the two frames of a
transform and the square root add a few eps of the same norm and of the magnitude: tol_mag = eps (log2 N + 4) ||X_t||_2 + 4 eps ref, eps = 2^-23,
ref = sqrt(|X|^2 + 1e-9).  x -> max(x, 1e-5) is 1-Lipschitz and log has slope 1 / x, so the magnitude's error reaches the output as
tol_mag / max(ref, 1e-5); v_log_f32 / logf (log2 within an ulp or two of a value up to 17), the product with ln 2 and the rounding of ln 2 itself
add at most 4 eps (1 + |log|):
    |out - log(max(ref, 1e-5))| <= tol_mag / max(ref, 1e-5) + 4 eps (1 + |log max(ref, 1e-5)|)       for EVERY cell.
For the radix recombination X[f] = sum_p W^(p f) Y_p[f mod M] the transform's part is R complex multiply-adds instead: their error is at most
eps (R + c) sum_p |Y_p[g]|, and sum_p |Y_p[g]| <= sqrt(R) (sum_p |Y_p[g]|^2)^(1/2) <= sqrt(R) ||X||_2 / sqrt(R) (Parseval: the R sub-transforms
together hold ||X||_2^2 / R), so the same formula holds with log2 N replaced by R.  A whole (non-negative) filter: the magnitudes' bounds
weighted by the filter plus eps (n + 2) of the sum for its n products and additions (frontend_reference.mel_cell_bound); every cell of the fused
kernel's whole-bank tests is held to it as well.

Two things the definition forces.  (1) Through a one-hot filter silence reads sqrt(1e-9) = 3.2e-5, which is ABOVE the clamp: the silent item
must give log(sqrt(1e-9)) within 2 ulp there, and log(1e-5) within 2 ulp through every whole filterbank (weights sum to less than 0.16).
(2) The ragged spans come as two banks (frontend_reference.ragged_bank): one-lane 27 and four-lane 144 together need 4096 > 2560 floats.

Measured on an MI355X: profiles/frontend_error.json (EFTS_FRONTEND_ERROR_JSON=<path> writes it anew); the largest ratio against each bound, per
kernel, is in that file and printed as RATIO / CELL lines: planes 0.99 (bf16) and 0.49 (bf16x3) of the storage resolution; efts_logmel 0.07 of
its `_check` bound; efts_logmel_dit 0.12 (fast) / 0.22 (general) of `_check` and 0.11 of the per-cell bound; the fused kernel 0.86 of `_check`
(its error is 0.5 .. 2 x that of fp32 torch.stft), 0.12 of the per-bin bound, 0.11 of the per-filter bound; clamp values within 1.7 ulp.

What notices what (scratch builds, one wrong-value change at a time): tw2s[2][5] off by 1e-4 fails test_fused_whole_banks and
test_fused_persistent_loop, NOT test_fused_bin_by_bin -- the worst-case per-bin bound (the kernel sits at 0.12 of it) is 14 eps ||X||_2 and the
change moves a bin by less; the yardstick of `_check` is what sees it, and tests/test_frontend.py does not.  Dropping `sgn` in the fast radix
kernel fails test_logmel_dit_alone, 2 (L - 1) - s -> 2 L - 1 - s in frame_pack_kernel fails test_frame_pack_planes.
"""
import json
import os

import numpy as np
import pytest
import torch

import frontend_reference as R
from kernel_check import COND, FACTOR, FLOOR, _call, _check, _dev, _rel, _st, load_lib, unpack_plane

pytestmark = pytest.mark.gpu

RES = {1: 2.0 ** -8, 2: 2.0 ** -16}
LOG_CLAMP = float(np.log(1e-5))
RECORD = {}


@pytest.fixture(scope="module")
def lib():
    lib = load_lib()
    yield lib
    path = os.environ.get("EFTS_FRONTEND_ERROR_JSON")
    if path:
        with open(path, "w") as f:
            json.dump({"what": "largest error / bound per kernel (tests/test_frontend_kernels_gpu.py); check = kernel_check._check per item, "
                               "cell = the derived per-cell bound, plane = the storage resolution of an operand plane, ulp2 = 2 ulp of the clamp value",
                       "ratios": RECORD}, f, indent=1, sort_keys=True)
            f.write("\n")


def _note(kernel, bound, ratio):
    d = RECORD.setdefault(kernel, {})
    d[bound] = max(d.get(bound, 0.0), float(ratio))


def _chk(kernel, case, got, ref64, ref32):
    """kernel_check._check, and its ratio against the bound for the record"""
    got, ref64 = torch.as_tensor(got), torch.as_tensor(ref64)
    _check(kernel, case, got, ref64, ref32)
    e32 = _rel(ref32.detach().double().reshape(ref64.shape), ref64)
    _note(kernel, "check", _rel(got.detach().cpu().double().reshape(ref64.shape), ref64) / min(max(FACTOR * e32, FLOOR), COND))


def _cells(kernel, case, got, want, bound):
    """every cell within its own bound"""
    ratio = np.abs(got.astype(np.float64) - want) / bound
    print(f"CELL {kernel} {case} largest |out - ref| / bound {ratio.max():.3f} over {ratio.size} cells")
    _note(kernel, "cell", ratio.max())
    assert np.isfinite(got).all() and (ratio <= 1.0).all(), f"{kernel} {case}: {int((ratio > 1).sum())} cells over their bound, worst {ratio.max():.2f}"


def _ulp2(kernel, case, got, value):
    """within 2 ulp (of fp32) of `value`"""
    got = np.asarray(got, dtype=np.float64)
    if got.size == 0:
        return
    ulp = float(np.spacing(np.float32(abs(value))))
    worst = float(np.abs(got - value).max()) / (2 * ulp)
    _note(kernel, "ulp2", worst)
    assert worst <= 1.0, f"{kernel} {case}: {worst * 2:.2f} ulp from {value}"


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _nan(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


# ---------------------------------------------------------------------------------------------------------------- a. the frame planes
def _plane_bits(pl, rows, n_fft, split):
    """uint8 [rows][ld] -> int16 [rows, split, n_fft]: the bf16 bit patterns of the hi (and lo) half of every element"""
    w = pl.cpu().view(torch.int16).view(rows, -1)
    if split == 1:
        return w[:, :n_fft].reshape(rows, 1, n_fft)
    return w[:, :2 * n_fft].reshape(rows, n_fft // 32, 2, 32).permute(0, 2, 1, 3).reshape(rows, 2, n_fft)


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("n_fft,hop,radices", [(1024, 256, (2, 4, 8, 16)), (512, 128, (2, 4))])
def test_frame_pack_planes(lib, n_fft, hop, radices, split):
    """efts_frame_pack and efts_frame_pack_dit: the decoded plane against the float64 frames, element by element; rows at and past an item's
    frame count (guard rows included) zero bit for bit; the de-interleaved plane = the natural one under the column permutation, bit for bit"""
    from efficient_tts_amd.ops import Rows
    dev = _dev()
    pad = (n_fft - hop) // 2
    lengths = (pad + 1, 4 * n_fft + 3, 2 * hop + 1)
    its = [(str(L),) + R.signal(L, 200 + i) for i, L in enumerate(lengths)]
    _, f32, _ = R.batch(its)
    nfr = [L // hop for L in lengths]
    B, T = 3, max(nfr)
    Tp = Rows(B, T).Tp
    assert Tp > T
    ref = np.zeros((B, Tp, n_fft))
    for b, (_, pcm, _) in enumerate(its):
        ref[b, :nfr[b]] = R.frames(pcm, n_fft, hop)
    audio, li, win = _d(f32, dev), _d(np.array(lengths, dtype=np.int32), dev), _d(R.window(n_fft), dev)
    ld = n_fft * 2 * split
    live = np.zeros((B, Tp), dtype=bool)
    for b in range(B):
        live[b, :nfr[b]] = True

    def run(radix):
        pl = torch.full((B * Tp, ld), 0xFF, dtype=torch.uint8, device=dev)          # bf16 0xFFFF: NaN
        if radix is None:
            _call("efts_frame_pack", lib.efts_frame_pack(audio.data_ptr(), audio.shape[1], li.data_ptr(), win.data_ptr(), pl.data_ptr(), ld, B, T, Tp,
                                                         n_fft, hop, split, _st()))
        else:
            _call("efts_frame_pack_dit", lib.efts_frame_pack_dit(audio.data_ptr(), audio.shape[1], li.data_ptr(), win.data_ptr(), pl.data_ptr(), ld, B, T,
                                                                 Tp, n_fft, hop, split, radix, _st()))
        torch.cuda.synchronize()
        return pl

    def against_ref(kernel, case, pl, want):
        got = unpack_plane(pl, B, Tp, Tp, n_fft, split).numpy().astype(np.float64)
        assert np.isfinite(got).all()
        tol = (RES[split] + 2.0 ** -24) * np.abs(want)
        err = np.abs(got - want)
        nz = want != 0
        ratio = float((err[nz] / tol[nz]).max())
        print(f"CELL {kernel} {case} largest |got - ref| / (r |ref|) {ratio:.3f}")
        _note(kernel + f".split{split}", "plane", ratio)
        assert (err <= tol).all()
        assert not pl.cpu().view(B, Tp, ld)[torch.from_numpy(~live)].any()              # bit for bit

    nat = run(None)
    against_ref("efts_frame_pack", f"n_fft={n_fft} split={split}", nat, ref)
    nat_bits = _plane_bits(nat, B * Tp, n_fft, split)
    for radix in radices:
        dit = run(radix)
        col = R.deinterleave_index(n_fft, radix)
        against_ref("efts_frame_pack_dit", f"n_fft={n_fft} split={split} radix={radix}", dit, R.deinterleave(ref, radix))
        assert torch.equal(_plane_bits(dit, B * Tp, n_fft, split)[:, :, col], nat_bits)


# ---------------------------------------------------------------------------------------------------------------- b, c. the log-mel kernels alone
B3, T5, TP7 = 3, 5, 7
FRAMES3 = (5, 2, 0)


def _rows_buffer(rows32, ld, dev):
    """[5, c] float32 -> device [B3 * TP7, ld]: rows t < frames[b] of item b hold the data, everything else NaN"""
    buf = np.full((B3, TP7, ld), np.nan, dtype=np.float32)
    for b, n in enumerate(FRAMES3):
        buf[b, :n, :rows32.shape[1]] = rows32[:n]
    return _d(buf.reshape(B3 * TP7, ld), dev)


def _expect_rows(rows):
    """[5, n_mels] -> [B3, T5, n_mels] with zeros at and past frames[b]"""
    out = np.zeros((B3, T5, rows.shape[1]))
    for b, n in enumerate(FRAMES3):
        out[b, :n] = rows[:n]
    return out


def _stage_banks(n_fft, mels):
    nb = n_fft // 2 + 1
    banks = [(f"slaney{m}", R.slaney(m, 8000.0, n_fft=n_fft)) for m in mels]
    banks = [(n, b, R.ranges_of(b)) for n, b in banks]
    return banks + [(f"ragged{w}",) + R.ragged_bank(w, nb) for w in (0, 1)]


def _stage_check(kernel, case, out, want64, want32, rng):
    """a whole-bank case of a stage kernel: `_check` on the live rows of item 0, bit-equal rows in item 1, log(1e-5) within 2 ulp on the zero row
    and in every empty filter, zeros at and past frames[b], nothing left of the NaN pre-fill"""
    out = out.cpu().numpy()
    assert np.isfinite(out).all()
    _chk(kernel, case, out[0], want64, want32)
    assert np.array_equal(out[1, :2].view(np.uint32), out[0, :2].view(np.uint32))
    assert not out[1, 2:].any() and not out[2].any()
    _ulp2(kernel, case + " zero row", out[0, 4], LOG_CLAMP)
    _ulp2(kernel, case + " empty filters", out[0][:, rng[:, 1] == rng[:, 0]], LOG_CLAMP)


@pytest.mark.parametrize("n_bins", [513, 257])
def test_logmel_alone(lib, n_bins):
    """efts_logmel on a spectrum whose answer is known: the float64 reference spectrum cast to fp32 (ref64 is computed from the rounded values)"""
    dev = _dev()
    n_fft = 2 * (n_bins - 1)
    spec = np.fft.rfft(R.stage_frames(n_fft), axis=1)
    re, im = spec.real.astype(np.float32), spec.imag.astype(np.float32)
    ld = 2 * n_bins + 6
    sd = _rows_buffer(np.concatenate([re, im], axis=1), ld, dev)
    fr = _d(np.array(FRAMES3, dtype=np.int32), dev)
    mag = np.sqrt(re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2 + R.MAG_EPS)
    for name, basis, rng in _stage_banks(n_fft, (80, 130, 1)):
        n_mels = basis.shape[0]
        out, bd, rd = _nan((B3, T5, n_mels), dev), _d(basis, dev), _d(rng, dev)
        _call("efts_logmel", lib.efts_logmel(sd.data_ptr(), ld, bd.data_ptr(), rd.data_ptr(), fr.data_ptr(), out.data_ptr(), B3, T5, TP7, n_bins, n_mels, _st()))
        torch.cuda.synchronize()
        want64 = R.log_clamp(R.mel_energy(mag, basis))
        want32 = R.logmel_of_spectrum32(torch.from_numpy(re), torch.from_numpy(im), basis)
        _stage_check("efts_logmel", f"n_bins={n_bins} {name}", out, want64, want32, rng)


# (n_fft, radix, ld_spec, kernel, mel counts of the Slaney banks): the fast kernel takes 1024 points, radix 2 / 4 / 8, n_mels <= 128 and rows of whole
# float4s; everything else the general one
DIT_CASES = [(1024, 2, 1028, "fast", (80, 128)), (1024, 4, 1024, "fast", (80, 128)), (1024, 8, 1028, "fast", (80, 128)),
             (1024, 16, 1028, "general", (80,)), (1024, 4, 1026, "general", (80,)), (1024, 2, 1024, "general", (129,)),
             (512, 2, 516, "general", (80,)), (512, 4, 512, "general", (80,))]


@pytest.mark.parametrize("n_fft,radix,ld,kernel,mels", DIT_CASES, ids=[f"{c[0]}-r{c[1]}-ld{c[2]}-{c[3]}-{c[4][-1]}" for c in DIT_CASES])
def test_logmel_dit_alone(lib, n_fft, radix, ld, kernel, mels):
    """efts_logmel_dit on radix rows whose answer is known (the reference's, cast to fp32, twiddles likewise): whole banks under `_check`, every bin
    through the one-hot banks under the per-cell bound with R multiply-adds -- bins 0 and N / 2 and g = 0, M / 2, M / 2 +- 1 of every residue class
    included.  21 rows: not a multiple of the fast kernel's 16 rows per block."""
    dev = _dev()
    n_bins = n_fft // 2 + 1
    rows = R.radix_rows(R.stage_frames(n_fft), radix).astype(np.float32)
    tw = R.twiddles(radix, n_fft).astype(np.float32)
    X = R.recombine(rows, radix, tw)
    mag = R.magnitude(X)
    xr, xi = R.recombine32(rows, radix, tw)
    sd, twd = _rows_buffer(rows, ld, dev), _d(tw, dev)
    fr = _d(np.array(FRAMES3, dtype=np.int32), dev)
    assert B3 * TP7 == 21

    def which(n_mels):
        return "efts_logmel_dit." + ("fast" if n_fft == 1024 and n_mels <= 128 and ld % 4 == 0 and radix in (2, 4, 8) else "general")

    assert which(mels[-1]) == "efts_logmel_dit." + kernel
    name = which(80)                                             # the ragged and the one-hot banks have 80 filters

    def run(basis, rng):
        n_mels = basis.shape[0]
        out, bd, rd = _nan((B3, T5, n_mels), dev), _d(basis, dev), _d(rng, dev)
        _call("efts_logmel_dit", lib.efts_logmel_dit(sd.data_ptr(), ld, bd.data_ptr(), rd.data_ptr(), fr.data_ptr(), twd.data_ptr(), out.data_ptr(), B3, T5, TP7,
                                                     n_bins, n_mels, radix, _st()))
        torch.cuda.synchronize()
        return out

    banks = _stage_banks(n_fft, mels) if mels[-1] <= 128 else [b for b in _stage_banks(n_fft, mels) if b[0].startswith("slaney")]
    if name.endswith("fast"):
        banks.append(("fat",) + R.fat_bank())                    # 2560 weights > LM_CB: read from memory
    for bank, basis, rng in banks:
        want64 = R.log_clamp(R.mel_energy(mag, basis))
        _stage_check(which(basis.shape[0]), f"n_fft={n_fft} radix={radix} ld={ld} {bank}", run(basis, rng), want64, R.logmel_of_spectrum32(xr, xi, basis), rng)
    want, bound = R.log_clamp(mag), R.cell_bound(mag, radix)
    seen = np.zeros(n_bins, dtype=int)
    got = np.full((T5, n_bins, 2), np.nan, dtype=np.float32)
    for basis, rng in R.onehot_banks(80, n_bins):
        out = run(basis, rng).cpu().numpy()
        live = rng[:, 1] > rng[:, 0]
        assert not out[1, 2:].any() and not out[2].any()
        _ulp2(name, "one-hot, empty filters", out[0][:, ~live], LOG_CLAMP)
        for m in np.nonzero(live)[0]:
            got[:, rng[m, 0], int(m >= R.FF_WIDE)] = out[0, :, m]
            seen[rng[m, 0]] += 1
    assert (seen == 2).all()
    for k in range(2):
        _cells(name, f"n_fft={n_fft} radix={radix} ld={ld} one-hot pass {k}", got[:, :, k], want, bound)


# ---------------------------------------------------------------------------------------------------------------- d, e. the fused kernel
@pytest.fixture(scope="module")
def fused():
    """the items, their batch (32767 / NaN behind every length) and the float64 magnitudes of every item -- shared, read-only"""
    its = R.items()
    pcm, f32, lengths = R.batch(its)
    mags = [R.magnitude(R.spectrum(p)) for _, p, _ in its]
    for a in (pcm, f32, *mags):
        a.setflags(write=False)
    return dict(items=its, pcm=pcm, f32=f32, lengths=lengths, frames=[L // R.HOP for L in lengths], mags=mags)


def _run_fused(lib, dev, pcm, f32, lengths, basis, rng, T):
    """both entry points on the same samples: identical bits; returns the output [B, T, n_mels] on the host"""
    B, n_mels = len(lengths), basis.shape[0]
    li, win, bd, rd = _d(np.array(lengths, dtype=np.int32), dev), _d(R.window(R.N_FFT), dev), _d(basis, dev), _d(rng, dev)
    a16, a32 = _d(pcm, dev), _d(f32, dev)
    o16, o32 = _nan((B, T, n_mels), dev), _nan((B, T, n_mels), dev)
    _call("efts_logmel_fft", lib.efts_logmel_fft(a32.data_ptr(), a32.shape[1], li.data_ptr(), win.data_ptr(), bd.data_ptr(), rd.data_ptr(), o32.data_ptr(), B, T,
                                                 R.N_FFT, R.HOP, n_mels, _st()))
    _call("efts_logmel_fft_pcm16", lib.efts_logmel_fft_pcm16(a16.data_ptr(), a16.shape[1], 1.0 / R.MAX_WAV, li.data_ptr(), win.data_ptr(), bd.data_ptr(),
                                                             rd.data_ptr(), o16.data_ptr(), B, T, R.N_FFT, R.HOP, n_mels, _st()))
    torch.cuda.synchronize()
    o16, o32 = o16.cpu().numpy(), o32.cpu().numpy()
    assert np.isfinite(o32).all()
    assert np.array_equal(o16.view(np.uint32), o32.view(np.uint32))                       # int16 PCM == the same values as fp32
    return o32


@pytest.mark.parametrize("extra", [0, 3])
def test_fused_bin_by_bin(lib, fused, extra):
    """efts_logmel_fft / efts_logmel_fft_pcm16: every |X[f]|, f = 0 .. 512, of every frame read out through one-hot filters, once in a one-lane slot
    and once in a four-lane slot, each cell under the derived bound"""
    dev = _dev()
    B, T = len(fused["lengths"]), max(fused["frames"]) + extra
    got = np.full((B, T, 513, 2), np.nan, dtype=np.float32)
    seen = np.zeros(513, dtype=int)
    for basis, rng in R.onehot_banks(80, 513):
        out = _run_fused(lib, dev, fused["pcm"], fused["f32"], fused["lengths"], basis, rng, T)
        live = rng[:, 1] > rng[:, 0]
        for b, n in enumerate(fused["frames"]):
            assert not out[b, n:].any()                                                   # rows at and past the item's count
            _ulp2("efts_logmel_fft", "one-hot, empty filters", out[b, :n][:, ~live], LOG_CLAMP)
        for m in np.nonzero(live)[0]:
            got[:, :, rng[m, 0], int(m >= R.FF_WIDE)] = out[:, :, m]
            seen[rng[m, 0]] += 1
    assert (seen == 2).all()
    for b, (name, _, _) in enumerate(fused["items"]):
        mag, n = fused["mags"][b], fused["frames"][b]
        assert mag.shape[0] == n
        for k, slot in enumerate(("one-lane", "four-lane")):
            _cells(f"efts_logmel_fft.{slot}", f"T={T} item {name}", got[b, :n, :, k], R.log_clamp(mag), R.cell_bound(mag, 10))
            if b == R.SILENT:                                                             # sqrt(1e-9), above the clamp
                _ulp2(f"efts_logmel_fft.{slot}", "silence", got[b, :n, :, k], float(np.log(np.sqrt(R.MAG_EPS))))


@pytest.mark.parametrize("bank", R.BANK_NAMES)
def test_fused_whole_banks(lib, fused, bank):
    """the fused kernel with whole filterbanks -- three Slaney banks and the two ragged ones in its LDS table, (64, 11025) read from memory --
    against float64, per item under `_check` (yardstick: the fp32 torch.stft transcription) and per cell under mel_cell_bound"""
    dev = _dev()
    basis, rng = dict(R.whole_banks())[bank]
    assert (R.fused_table_floats(rng) <= R.FF_CB) == (bank != "slaney64_11025")
    empty = rng[:, 1] == rng[:, 0]
    for extra in (0, 3):
        T = max(fused["frames"]) + extra
        out = _run_fused(lib, dev, fused["pcm"], fused["f32"], fused["lengths"], basis, rng, T)
        for b, (name, pcm, f32) in enumerate(fused["items"]):
            mag, n = fused["mags"][b], fused["frames"][b]
            assert not out[b, n:].any()
            want = R.log_clamp(R.mel_energy(mag, basis))
            if (name, bank) not in R.ILL_CONDITIONED:
                _chk("efts_logmel_fft", f"{bank} T={T} item {name}", out[b, :n], want, R.logmel32(f32, basis))
            _cells("efts_logmel_fft.bank", f"{bank} T={T} item {name}", out[b, :n], want, R.mel_cell_bound(mag, basis, 10))
            _ulp2("efts_logmel_fft", f"{bank} empty filters", out[b, :n][:, empty], LOG_CLAMP)
            if b == R.SILENT:
                _ulp2("efts_logmel_fft", f"{bank} silence", out[b, :n], LOG_CLAMP)


def test_fused_persistent_loop(lib):
    """more frame pairs than the launch has waves (3 x CUs blocks of 4 waves): every wave works through several pairs, re-using its LDS buffer"""
    dev = _dev()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    B = R.persistent_batch_size(cus)
    assert B * ((R.PERSISTENT_T + 1) // 2) > 12 * cus and B <= R.PERSISTENT_MAX_B
    its = R.persistent_items(B)
    pcm, f32, lengths = R.batch(its)
    basis, rng = R.slaney_bank(80, 8000.0)
    out = _run_fused(lib, dev, pcm, f32, lengths, basis, rng, R.PERSISTENT_T)
    for b, (name, p, f) in enumerate(its):
        n = len(p) // R.HOP
        mag = R.magnitude(R.spectrum(p))
        want = R.log_clamp(R.mel_energy(mag, basis))
        assert not out[b, n:].any()
        _chk("efts_logmel_fft.persistent", f"B={B} item {name}", out[b, :n], want, R.logmel32(f, basis))
        _cells("efts_logmel_fft.persistent", f"B={B} item {name}", out[b, :n], want, R.mel_cell_bound(mag, basis, 10))
