"""GPU (-m gpu): every kernel of the forward alignment chain alone against a float64 reference of the same operation.

The exports below are called directly through `efficient_tts_amd.lib` with torch tensors as buffers -- no model, no golden file:

    efts_attn_soft_index  efts_imv_scan  efts_aligned_positions  efts_duration_target  efts_imv_align  efts_reconst_alpha

Reference, metric and bound are those of tests/test_bwd_kernels_gpu.py (tests/kernel_check.py): the float64 evaluation of the twins in
tests/bwd_reference.py on the SAME float32 inputs, `_rel` = max |got - ref| / max |ref|, and the kernel within max(8 * e32, 2e-6) of it,
where e32 is the error of the float32 torch transcription; 8 * e32 <= 2e-4 is asserted for every case (and, without a device, by
tests/test_fwd_reference_cpu.py).  Inputs and references of every case come from tests/fwd_cases.py.  Every output buffer is prefilled
with 7.0 (planes with 0xAB bytes); what must be exactly zero, untouched or bit-identical is asserted with ==.

efts_imv_align is compared with float64 here IN ADDITION to tests/test_align_gpu.py, which compares it bit for bit with the three
kernels it fuses: the two share one algorithm, so only a reference that is not that algorithm can see a mistake they share.

Measured on one MI355X (table in the format of the backward file: the worst `kernel error / e32` over the cases whose bound is the
8 * e32 branch, and the worst error where the 2e-6 floor is the bound):

    kernel                         cases  worst err / e32 (e32 > 2.5e-7)                                   worst err under the 2e-6 floor
    efts_attn_soft_index.soft_idx     16  -                                                                1.7e-07  (2x203x300 ld=203)
    efts_attn_soft_index.alpha        16  -                                                                7.0e-08  (2x203x300 ld=203)
    efts_imv_scan                     49  -                                                                4.7e-07  (hard T2=4100[item 2])
    efts_aligned_positions.e          10  0.61  (2x203x300: 1.5e-07 / 2.5e-07)                             1.4e-07  (2x63x97)
    efts_aligned_positions.lde        10  1.01  (2x64x130: 1.9e-06 / 1.9e-06)                              3.4e-07  (3x5x64)
    efts_duration_target               8  -                                                                9.1e-08  (3x1 method1=False)
    efts_imv_align.imv                16  -                                                                5.4e-07  (2x128x4100 method1=True)
    efts_imv_align.e                  16  0.75  (2x203x1500 method1=True: 3.7e-07 / 4.9e-07)               1.4e-07  (4x100x124 method1=True)
    efts_imv_align.lde                16  0.83  (4x100x124 method1=True: 2.2e-06 / 2.7e-06)                8.9e-08  (3x1x33 method1=True)
    efts_reconst_alpha.fp32           14  0.44  (2x300x333 inference: 1.3e-07 / 3.0e-07)                   1.4e-07  (2x33x65 inference)
    efts_reconst_alpha.plane2         28  -                                                                4.8e-06  (2x33x65 inference alpha_out=False)
    efts_reconst_alpha.plane3         28  0.44  (2x300x333 inference alpha_out=False: 1.3e-07 / 3.0e-07)   1.4e-07  (2x33x65 inference alpha_out=False)
    fwd_chain                          8  1.03  (imv 2x128x800: 5.1e-07 / 4.9e-07)                         1.9e-07  (soft_idx 2x128x800)

Every fp32 ratio is at or below 1.0: the kernels' `__expf` does not show against the float32 transcription at these inputs (the
weights that carry mass have arguments within about -10 of the maximum), so no kernel was changed and no bound was derived.  The two
plane rows are held to the bound plus the format's resolution (2^-16 of the largest value for format 2, nothing for format 3), which is
what the format-2 row's larger figure is (that row: the worst error of all cases).  `fwd_chain` is test_forward_alignment_chain_vs_fp64 (4 stages x 2 shapes), under the capped bound.
"""
import pytest
import torch

import fwd_cases as F
from kernel_check import _call, _check, _dev, _st, load_lib, unpack_plane

pytestmark = pytest.mark.gpu

SIGMA, SIGMA_E, OFFSET = F.SIGMA, F.SIGMA_E, F.OFFSET


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _full(shape, dev):
    return torch.full(shape, 7.0, device=dev)


# =====================================================================================================================
# efts_attn_soft_index
# =====================================================================================================================
def _run_attn(lib, scores, ld, tl, ml, B, T1, T2, with_alpha):
    dev = scores.device
    sidx = _full((B, T2), dev)
    alpha = _full((B, T1, T2), dev) if with_alpha else None
    _call("efts_attn_soft_index", lib.efts_attn_soft_index(scores.data_ptr(), ld, tl.data_ptr(), ml.data_ptr(), sidx.data_ptr(),
                                                           None if alpha is None else alpha.data_ptr(), B, T1, T2, _st()))
    return sidx, alpha


@pytest.mark.parametrize("ldx", [0, 3])
@pytest.mark.parametrize("B,T1,T2", F.ATTN_SHAPES)
def test_attn_soft_index_vs_fp64(lib, B, T1, T2, ldx):
    """efts_attn_soft_index: masked softmax over the keys of one frame and the expected key index.  One wave per (b, j), 64 keys per
    pass: one key, 5, 9, 37, 63 / 64 / 65 around the wave, 203; B * T2 mod 4 (frames per block) = 3, 0, 0, 1, 2, 0, 0, 0."""
    dev = _dev()
    cs = F.attn_case(B, T1, T2, ldx)
    tm, mm = cs["tm"], cs["mm"]
    sc, tl, ml = cs["scores"].to(dev), cs["tl"].to(dev), cs["ml"].to(dev)
    sidx0, _ = _run_attn(lib, sc, cs["ld"], tl, ml, B, T1, T2, False)
    sidx1, alpha = _run_attn(lib, sc, cs["ld"], tl, ml, B, T1, T2, True)
    torch.cuda.synchronize()
    case = f"{B}x{T1}x{T2} ld={cs['ld']}"
    _check("efts_attn_soft_index.soft_idx", case, sidx0, *cs["refs"]["soft_idx"])
    _check("efts_attn_soft_index.alpha", case, alpha, *cs["refs"]["alpha"])
    sidx0, sidx1, alpha = sidx0.cpu(), sidx1.cpu(), alpha.cpu()
    assert torch.equal(sidx0.view(torch.int32), sidx1.view(torch.int32))             # alpha_out does not change one bit of the soft index
    assert bool((sidx0[~mm] == 0).all())                                             # padded frames: exactly 0
    assert bool((alpha.transpose(1, 2)[~mm] == 0).all()) and bool((alpha[~tm] == 0).all())
    assert float((alpha.double().sum(1)[mm] - 1.0).abs().max()) <= 1e-5              # live columns sum to 1


# =====================================================================================================================
# efts_imv_scan
# =====================================================================================================================
def _run_imv_scan(lib, cs, T2):
    dev = _dev()
    d = [cs[k].to(dev) for k in ("sidx", "tl", "ml")]
    imv = _full((cs["B"], T2), dev)
    _call("efts_imv_scan", lib.efts_imv_scan(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), imv.data_ptr(), cs["B"], T2, _st()))
    torch.cuda.synchronize()
    return imv.cpu()


def _imv_properties(imv, cs, ref64):
    """what imv_generator guarantees whatever the rounding: 0 past mel_len, monotone over the live frames, text_len - 1 at the last one"""
    for b in range(cs["B"]):
        n, scale = int(cs["ml"][b]), float(cs["tl"][b]) - 1.0
        assert bool((imv[b, n:] == 0).all())
        live = imv[b, :n]
        assert bool((live[1:] >= live[:-1]).all())
        if float(ref64[b].abs().max()) > 0:
            assert abs(float(live[-1]) - scale) <= 1e-6 * scale
        else:
            assert bool((live == 0).all())


@pytest.mark.parametrize("T2", F.IMV_T2)
def test_imv_scan_vs_fp64(lib, T2):
    """efts_imv_scan: relu-diff, cumsum, mask, max-normalise, times text_len - 1.  One wave per item, ceil(T2 / 64) frames per lane:
    segments of 1 (T2 <= 64, lanes empty below), 2 (65 ... 128; at 65 lanes 33 ... 63 are empty), 3 (129: lanes 43 ... 63 empty), 4, 13, 65."""
    cs = F.imv_case(T2)
    imv = _run_imv_scan(lib, cs, T2)
    ref64, ref32 = cs["refs"]["imv"]
    _check("efts_imv_scan", f"T2={T2}", imv, ref64, ref32)
    _imv_properties(imv, cs, ref64)
    assert bool((imv[1] == 0).all()) and bool((imv[2] == 0).all())                    # one frame; one token


@pytest.mark.parametrize("T2", F.IMV_T2)
def test_imv_scan_clamp_mask_and_plateau(lib, T2):
    """The inputs the ragged batch does not hold (fwd_cases.imv_hard_case): a soft index that decreases everywhere gives exact zeros through
    the 1e-8 clamp (no 0 / 0), frames past mel_len do not reach the maximum, a plateau stays a plateau, large exact partial sums."""
    cs = F.imv_hard_case(T2)
    imv = _run_imv_scan(lib, cs, T2)
    ref64, ref32 = cs["refs"]["imv"]
    _check("efts_imv_scan", f"hard T2={T2}", imv, ref64, ref32)
    for b in range(1, 4):                                                             # per item: one item's error must not hide behind another's range
        if float(ref64[b].abs().max()) > 0:
            _check("efts_imv_scan", f"hard T2={T2}[item {b}]", imv[b], ref64[b], ref32[b])
    _imv_properties(imv, cs, ref64)
    assert bool((imv[0] == 0).all()) and bool((ref64[0] == 0).all())                  # decreasing everywhere: exact zeros, no NaN


# =====================================================================================================================
# efts_aligned_positions, efts_duration_target
# =====================================================================================================================
@pytest.mark.parametrize("B,T1,T2", F.EPOS_SHAPES)
def test_aligned_positions_vs_fp64(lib, B, T1, T2):
    """efts_aligned_positions: e_i = sum_j softmax_j(-sigma_e (pi_j - i)^2) j over the live frames, one wave per token and 4 tokens per block
    (T1 mod 4 = 1, 1, 1, 1, 3, 0, 1, 3, 0, 3), with and without the method-1 duration target appended."""
    dev = _dev()
    cs = F.epos_case(B, T1, T2)
    imv, tl, ml = cs["imv"].to(dev), cs["tl"].to(dev), cs["ml"].to(dev)
    e0, e1, lde = _full((B, T1), dev), _full((B, T1), dev), _full((B, T1), dev)
    _call("efts_aligned_positions", lib.efts_aligned_positions(imv.data_ptr(), tl.data_ptr(), ml.data_ptr(), SIGMA_E, OFFSET, e0.data_ptr(), None,
                                                               B, T1, T2, _st()))
    _call("efts_aligned_positions", lib.efts_aligned_positions(imv.data_ptr(), tl.data_ptr(), ml.data_ptr(), SIGMA_E, OFFSET, e1.data_ptr(),
                                                               lde.data_ptr(), B, T1, T2, _st()))
    torch.cuda.synchronize()
    case = f"{B}x{T1}x{T2}"
    _check("efts_aligned_positions.e", case, e0, *cs["refs"]["e"])
    _check("efts_aligned_positions.lde", case, lde, *cs["refs"]["lde"])
    e0, e1, lde = e0.cpu(), e1.cpu(), lde.cpu()
    assert torch.equal(e0.view(torch.int32), e1.view(torch.int32))
    assert bool((e0[~cs["tm"]] == 0).all()) and bool((lde[~cs["tm"]] == 0).all())     # padded tokens: exactly 0


@pytest.mark.parametrize("method1", [True, False])
@pytest.mark.parametrize("B,T1", F.DUR_SHAPES)
def test_duration_target_vs_fp64(lib, B, T1, method1):
    """efts_duration_target: log(e_i - e_{i-1} + offset) with e_{-1} = 0 (method 1), log(e_{i+1} - e_i + offset) with e_{text_len} = mel_len"""
    dev = _dev()
    cs = F.dur_case(B, T1, method1)
    e, tl, ml = cs["e"].to(dev), cs["tl"].to(dev), cs["ml"].to(dev)
    lde = _full((B, T1), dev)
    _call("efts_duration_target", lib.efts_duration_target(e.data_ptr(), tl.data_ptr(), ml.data_ptr(), OFFSET, int(method1), lde.data_ptr(), B, T1, _st()))
    torch.cuda.synchronize()
    _check("efts_duration_target", f"{B}x{T1} method1={method1}", lde, *cs["refs"]["lde"])
    assert bool((lde.cpu()[~cs["tm"]] == 0).all())


# =====================================================================================================================
# efts_imv_align
# =====================================================================================================================
def _run_imv_align(lib, sidx, tl, ml, method1, B, T1, T2):
    dev = sidx.device
    imv, e, lde = _full((B, T2), dev), _full((B, T1), dev), _full((B, T1), dev)
    _call("efts_imv_align", lib.efts_imv_align(sidx.data_ptr(), tl.data_ptr(), ml.data_ptr(), SIGMA_E, OFFSET, int(method1), imv.data_ptr(),
                                               e.data_ptr(), lde.data_ptr(), B, T1, T2, _st()))
    return imv, e, lde


@pytest.mark.parametrize("method1", [True, False])
@pytest.mark.parametrize("B,T1,T2", F.ALIGN_SHAPES)
def test_imv_align_vs_fp64(lib, B, T1, T2, method1):
    """efts_imv_align: IMV, e and the duration target of either method from the soft index in one launch, each against the float64 composition
    imv_from_soft_index -> aligned_positions -> duration_target (e32: the same composition in float32)."""
    dev = _dev()
    cs = F.align_case(B, T1, T2, method1)
    imv, e, lde = _run_imv_align(lib, cs["sidx"].to(dev), cs["tl"].to(dev), cs["ml"].to(dev), method1, B, T1, T2)
    torch.cuda.synchronize()
    case = f"{B}x{T1}x{T2} method1={method1}"
    _check("efts_imv_align.imv", case, imv, *cs["refs"]["imv"])
    _check("efts_imv_align.e", case, e, *cs["refs"]["e"])
    _check("efts_imv_align.lde", case, lde, *cs["refs"]["lde"])
    imv, e, lde = imv.cpu(), e.cpu(), lde.cpu()
    assert bool((imv[~cs["mm"]] == 0).all()) and bool((e[~cs["tm"]] == 0).all()) and bool((lde[~cs["tm"]] == 0).all())


def test_imv_align_exact_integers(lib):
    """A soft index of small integers (fwd_cases.align_exact_case): every quantity of the scan is exact in float32 in any association, so the
    lane-segmented scan must give the float32 transcription's IMV bit for bit."""
    dev = _dev()
    cs = F.align_exact_case()
    B, T1, T2 = cs["B"], cs["T1"], cs["T2"]
    imv, _, _ = _run_imv_align(lib, cs["sidx"].to(dev), cs["tl"].to(dev), cs["ml"].to(dev), True, B, T1, T2)
    d = [cs[k].to(dev) for k in ("sidx", "tl", "ml")]
    imv2 = _full((B, T2), dev)
    _call("efts_imv_scan", lib.efts_imv_scan(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), imv2.data_ptr(), B, T2, _st()))
    torch.cuda.synchronize()
    assert torch.equal(imv.cpu(), cs["imv32"])
    assert torch.equal(imv2.cpu(), cs["imv32"])


# =====================================================================================================================
# efts_reconst_alpha
# =====================================================================================================================
def _run_reconst(lib, e, tl, ml, B, T1, T2, with_alpha, split, pad_ldp=0):
    """alpha_out [B, T1, T2] and / or the plane [B * T2p][ldp bytes] of format `split` (None: no plane); T2p = T2 + 2 leaves two gap rows per item"""
    dev = e.device
    kp = (T1 + 31) // 32 * 32
    T2p, ldp = T2 + 2, kp * 4 + pad_ldp
    alpha = _full((B, T1, T2), dev) if with_alpha else None
    pl = torch.full((B * T2p, ldp), 0xAB, dtype=torch.uint8, device=dev) if split else None
    _call("efts_reconst_alpha", lib.efts_reconst_alpha(e.data_ptr(), None if tl is None else tl.data_ptr(), None if ml is None else ml.data_ptr(), SIGMA,
                                                       None if alpha is None else alpha.data_ptr(), None if pl is None else pl.data_ptr(), ldp,
                                                       B, T1, T2, T2p, split or 2, _st()))
    return alpha, pl, kp, T2p, ldp


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("B,T1,T2", F.RALPHA_SHAPES)
def test_reconst_alpha_vs_fp64(lib, B, T1, T2, masked):
    """efts_reconst_alpha: alpha'[i][j] = softmax_i(-sigma (q_j - e_i)^2) as fp32 [B, T1, T2] and / or as the K-major operand plane of format
    2 or 3.  64 frames per block (T2 = 31, 64, 65, 70, 211, 333, 5), the keys over 4 waves and in tiles of 32 (T1 = 1, 16, 31, 33, 37, 256, 300:
    300 is past what efts_expand takes, so this kernel is the only path there); masked (training) and unmasked (inference) form."""
    dev = _dev()
    cs = F.ralpha_case(B, T1, T2, masked)
    ref64, ref32 = cs["refs"]["ralpha"]
    tm, mm = cs["tm"], cs["mm"]
    e = cs["e"].to(dev)
    tl, ml = (cs["tl"].to(dev), cs["ml"].to(dev)) if masked else (None, None)
    case = f"{B}x{T1}x{T2} {'masked' if masked else 'inference'}"
    first = None
    for with_alpha, split in ((True, None), (False, 2), (False, 3), (True, 2), (True, 3)):
        alpha, pl, kp, T2p, ldp = _run_reconst(lib, e, tl, ml, B, T1, T2, with_alpha, split, pad_ldp=128 if T1 == 37 else 0)
        torch.cuda.synchronize()
        if alpha is not None:
            alpha = alpha.cpu()
            if first is None:
                first = alpha
                _check("efts_reconst_alpha.fp32", case, alpha, ref64, ref32)
                assert bool((alpha[~tm] == 0).all()) and bool((alpha.transpose(1, 2)[~mm] == 0).all())   # i >= text_len, j >= mel_len: exactly 0
            else:
                assert torch.equal(alpha.view(torch.int32), first.view(torch.int32))      # a plane next to it changes no bit of alpha_out
        if pl is not None:
            got = unpack_plane(pl, B, T2p, T2, kp, split).transpose(1, 2)                 # [B, kp, T2]
            _check(f"efts_reconst_alpha.plane{split}", f"{case} alpha_out={with_alpha}", got[:, :T1], ref64, ref32, extra=2.0 ** -16 if split == 2 else 0.0)
            assert bool((got[:, T1:] == 0).all())                                         # key padding T1 .. roundup(T1, 32) - 1: exactly 0
            assert bool((got[:, :T1][~tm] == 0).all()) and bool((got[:, :T1].transpose(1, 2)[~mm] == 0).all())
            if split == 3 and alpha is not None:
                assert torch.equal(got[:, :T1].contiguous().view(torch.int32), alpha.view(torch.int32))   # format 3 holds the unrounded value
            raw = pl.cpu().view(B, T2p, ldp)
            assert bool((raw[:, T2:] == 0xAB).all()) and bool((raw[:, :, kp * 4:] == 0xAB).all())   # gap rows and bytes past the chunks: untouched


# =====================================================================================================================
# the whole forward block
# =====================================================================================================================
@pytest.mark.parametrize("B,T1,T2", F.CHAIN_SHAPES)
def test_forward_alignment_chain_vs_fp64(lib, B, T1, T2):
    """efts_attn_soft_index -> efts_imv_align -> efts_reconst_alpha back to back on the device, every stage fed by the kernel before it, against
    the float64 block (scores -> alpha -> soft index -> pi -> e -> alpha'); e32 is the whole block in float32.  As in the backward chain test the
    inputs keep 1e-4 between neighbouring soft indices so that no relu decision can differ, and the bound is the capped one of `_check(chain=True)`:
    float32 itself does not meet the single-stage condition once the stages are composed."""
    dev = _dev()
    cs = F.chain_case(B, T1, T2)
    assert float(cs["refs"]["soft_idx"][0].diff(dim=1).abs()[cs["mm"][:, 1:]].min()) >= 1e-4
    sc, tl, ml = cs["scores"].to(dev), cs["tl"].to(dev), cs["ml"].to(dev)
    sidx, _ = _run_attn(lib, sc, T1, tl, ml, B, T1, T2, False)
    imv, e, _ = _run_imv_align(lib, sidx, tl, ml, True, B, T1, T2)
    ralpha, _, _, _, _ = _run_reconst(lib, e, tl, ml, B, T1, T2, True, None)
    torch.cuda.synchronize()
    for name, got in (("soft_idx", sidx), ("imv", imv), ("e", e), ("ralpha", ralpha)):
        _check("fwd_chain", f"{name} {B}x{T1}x{T2}", got, *cs["refs"][name], chain=True)
