"""No device: the host side of tests/test_gemm_kernels_gpu.py -- the operand encoders against the layout include/efts_abi.h documents, the
reference against float64 conv1d, the conditioning of every case of the table, and the tiling predicate against the table."""
import pytest
import torch

import gemm_reference as R
from kernel_check import conditioned

IDS = [c.name for c in R.CASES]


# ------------------------------------------------------------------------------------------------------------ encoders
@pytest.mark.parametrize("split", [1, 2, 3])
@pytest.mark.parametrize("K", [24, 32, 64, 80, 130])
def test_encoder_layout_matches_the_header(split, K):
    """element (row, k) sits where "MFMA operand planes" says: format 1 [Kp] bf16 with Kp = roundup(K, 64); format 2 [Kp / 32][hi32 | lo32]
    with Kp = roundup(K, 32), hi = RNE_bf16(x), lo = RNE_bf16(x - hi); format 3 [Kp] fp32 with Kp = roundup(K, 32); K padding is zero"""
    rows = 5
    x = torch.randn(rows, K, generator=torch.Generator().manual_seed(K * 10 + split)) * 3.0
    kp = (K + 63) // 64 * 64 if split == 1 else (K + 31) // 32 * 32
    rb = kp * 2 if split == 1 else kp * 4
    assert R.kp_of(K, split) == kp and R.row_bytes(K, split) == rb and rb % 128 == 0
    ld = rb + 16
    pl = R.encode_rows(x, split, ld, fill=R.CANARY)
    assert pl.shape == (rows, ld) and pl.dtype == torch.uint8
    assert bool((pl[:, rb:] == R.CANARY).all())
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    seen = torch.zeros(rb, dtype=torch.bool)
    for r in range(rows):
        for k in range(K):
            if split == 1:
                o = 2 * k
                assert torch.equal(pl[r, o:o + 2].view(torch.bfloat16), hi[r, k:k + 1])
                seen[o:o + 2] = True
            elif split == 3:
                o = 4 * k
                assert torch.equal(pl[r, o:o + 4].view(torch.float32), x[r, k:k + 1])
                seen[o:o + 4] = True
            else:
                o = (k // 32) * 128 + (k % 32) * 2
                assert torch.equal(pl[r, o:o + 2].view(torch.bfloat16), hi[r, k:k + 1])
                assert torch.equal(pl[r, o + 64:o + 66].view(torch.bfloat16), lo[r, k:k + 1])
                seen[o:o + 2] = True
                seen[o + 64:o + 66] = True
            assert R.byte_offsets(k, split)[0] == o
    assert float(pl[:, :rb][:, ~seen].float().abs().max() if bool((~seen).any()) else 0.0) == 0.0      # K padding
    assert torch.equal(R.element_bytes(K, split, ld)[:rb], seen) and not bool(R.element_bytes(K, split, ld)[rb:].any())


@pytest.mark.parametrize("split", [1, 2, 3])
@pytest.mark.parametrize("K", [24, 32, 64, 80, 130])
def test_encode_decode_is_the_identity_on_representable_values(split, K):
    g = torch.Generator().manual_seed(K + split)
    x = torch.randn(7, K, generator=g)
    if split == 1:
        x = x.bfloat16().float()
    elif split == 2:                                       # hi + lo with lo a bf16 below half an ulp of hi (an ulp of hi is at least 2^-9 |hi|)
        hi = x.bfloat16().float()
        x = hi + (hi * 2.0 ** -11 * (2.0 * torch.rand(7, K, generator=g) - 1.0)).bfloat16().float()
        assert torch.equal(x.bfloat16().float(), hi)
    back = R.decode_rows(R.encode_rows(x, split, R.row_bytes(K, split) + 32, fill=R.CANARY), K, split)
    assert torch.equal(back[:, :K], x) and float(back[:, K:].abs().max() if back.shape[1] > K else 0.0) == 0.0
    h, l = R.decode_rows(R.encode_rows(x, split), K, split, parts=True)
    assert torch.equal((h + l)[:, :K], x)
    if split == 2:
        assert torch.equal(h[:, :K], x.bfloat16().float())
    w = torch.randn(6, K, 3, generator=g)                   # weights: [cout][cin][taps] -> [taps][cout][ld]
    wp = R.encode_weight(w, split, R.row_bytes(K, split) + 32, fill=R.CANARY)
    assert wp.shape == (3, 6, R.row_bytes(K, split) + 32)
    for t in range(3):
        assert torch.equal(wp[t], R.encode_rows(w[:, :, t], split, R.row_bytes(K, split) + 32, fill=R.CANARY))
    dw = R.decode_weight(wp, K, split)
    want = w if split == 3 else (w.bfloat16().float() if split == 1 else w.bfloat16().float() + (w - w.bfloat16().float()).bfloat16().float())
    assert torch.equal(dw[:, :, :K], want.permute(2, 0, 1))


# ------------------------------------------------------------------------------------------------------------ reference
def _conv_check(case):
    """reference(case) against float64 conv1d on the decoded values, per item of the row space"""
    op = R.operands(case)
    ref64, _, bound = R.reference(case)
    T, gap, l0, l1 = case.items
    Tp = T + gap
    xd = R.decode_rows(op.a[0, R.A_GUARD_LO:R.A_GUARD_LO + case.m], case.K, case.split).double()[:, :case.K]
    wd = R.decode_weight(op.b[0, :case.taps * case.n].view(case.taps, case.n, case.ldb), case.K, case.split).double()[:, :, :case.K]
    x = xd.view(2, Tp, case.K)[:, :T].transpose(1, 2)                                  # [2][K][T]: two independent zero-padded convolutions
    z = torch.nn.functional.conv1d(x, wd.permute(1, 2, 0), op.bias.double() if case.bias else None, padding=(case.taps - 1) // 2 * case.dil,
                                   dilation=case.dil).transpose(1, 2)                  # [2][T][n]
    if case.resid:
        z = z + op.resid[0, :case.m, :case.n].double().view(2, Tp, case.n)[:, :T]
    lens = torch.tensor([l0, l1])
    z = z * (torch.arange(T)[None, :] < lens[:, None]).double()[..., None]
    got = ref64[0, 0].view(2, Tp, case.n)
    scale = float(z.abs().max())
    # format 2: the decoded value is hi + lo, and the kernel's three products leave lo*lo out: |lo| <= 2^-8 |hi|, so at most 2^-16 sum |a||w|
    mag = torch.nn.functional.conv1d(x.abs(), wd.permute(1, 2, 0).abs(), padding=(case.taps - 1) // 2 * case.dil, dilation=case.dil).transpose(1, 2)
    tol = 1e-12 * scale + (2.0 ** -16 * mag if case.split == 2 else 0.0)
    assert bool(((got[:, :T] - z).abs() <= tol).all())
    assert float(got[:, T:].abs().max()) == 0.0                                        # gap rows: masked
    assert bool((bound >= 0).all())


@pytest.mark.parametrize("case", [c for c in R.CASES if c.items], ids=[c.name for c in R.CASES if c.items])
def test_reference_is_conv1d_on_a_two_item_row_space(case):
    """every tap count and dilations above 1, on two items with gap rows and a ragged second item"""
    _conv_check(case)


def test_reference_cases_cover_every_tap_count_and_dilation():
    conv = [c for c in R.CASES if c.items and c.split == 1]
    assert {c.taps for c in conv} == {1, 3, 5, 7, 9, 11} and max(c.dil for c in conv) > 1


def test_reference_format2_sums_three_terms():
    """hi*hi + hi*lo + lo*hi, and NOT (hi + lo) * (hi + lo): the difference is the lo*lo term, which the reference must not contain"""
    case = next(c for c in R.CASES if c.name == "dil-bf16x3-t7-d3")
    op = R.operands(case)
    ref64 = R.reference(case)[0][0, 0]
    ah, al = R.decode_rows(op.a[0], case.K, 2, parts=True)
    wh, wl = R.decode_weight(op.b[0, :case.taps * case.n].view(case.taps, case.n, case.ldb), case.K, 2, parts=True)
    three = torch.zeros(case.m, case.n, dtype=torch.float64)
    four = torch.zeros(case.m, case.n, dtype=torch.float64)
    for k in range(case.taps):
        r0 = R.A_GUARD_LO + (k - case.pad) * case.dil
        h, l = ah[r0:r0 + case.m].double(), al[r0:r0 + case.m].double()
        three += h @ wh[k].double().T + h @ wl[k].double().T + l @ wh[k].double().T
        four += (h + l) @ (wh[k] .double() + wl[k].double()).T
    want = (three + op.bias.double() + op.resid[0, :case.m, :case.n].double()) * op.mask[0, :case.m, None].double()
    assert float((ref64 - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float((three - four).abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------------------ conditioning
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_every_case_is_conditioned(case):
    """8 * e32 <= 2e-4 for the fp32 output and for the value the plane encodes: the bound of kernel_check._check means something"""
    for plane in ((False, True) if case.has_plane and case.plane_act else (False,)):
        ref64, ref32, bound = R.reference(case, plane)
        ok, e32 = conditioned(ref64, ref32)
        assert ok, f"{case.name}: e32 = {e32:.3e}"
        assert ref64.dtype == torch.float64 and ref32.dtype == torch.float32 and ref64.shape == (case.batch2, case.batch, case.m, case.n)
        assert bool(torch.isfinite(ref64).all()) and bool(torch.isfinite(bound).all())
        # the float32 transcription itself obeys the a-priori bound (it is one of the summation orders the bound covers)
        assert bool(((ref32.double() - ref64).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------------------ accepts
def test_table_size():
    assert 120 <= len(R.CASES) <= 170


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_accepts_agrees_with_the_table(case):
    assert case.tilings and any(R.accepts(case, t) for t in R.EXPLICIT)
    for t in case.tilings:
        assert R.accepts(case, t), f"{case.name} is listed for {R.TILING_NAME[t]}"
    for t in case.refused:
        assert not R.accepts(case, t), f"{case.name} must be refused by {R.TILING_NAME[t]}"
    assert R.accepts(case, R.AUTO)


def test_every_tiling_has_its_edges_in_the_table():
    """what section "Cases" of the issue lists per kernel is in the table and accepted by that kernel"""
    by = {t: [c for c in R.CASES if t in c.tilings] for t in R.EXPLICIT}
    rows = lambda t, taps: {c.m for c in by[t] if c.name.startswith("row-") and c.taps == taps}
    assert {1, 123, 124, 125, 249} <= rows(R.GENERIC, 5) and {1, 123, 124, 125, 249} <= rows(R.NARROW, 5)
    assert {1, 253, 254, 255, 509} <= rows(R.RESIDENT, 3)
    assert {63, 64, 65, 129} <= rows(R.SMALLM, 5)
    assert {110, 252, 362, 504} <= rows(R.WIDE, 5)
    refused_wide = {c.m for c in R.CASES if R.WIDE in c.refused and c.name.startswith("row-")}
    assert refused_wide == {109, 253}
    cols = lambda t: {c.n for c in by[t] if c.name.startswith("col-")}
    assert {4, 28, 32, 36, 60, 64, 68, 124, 128, 132} <= cols(R.GENERIC) & cols(R.NARROW) & cols(R.WIDE)
    assert {4, 28, 32, 36, 60, 64} <= cols(R.RESIDENT) and {32, 96} <= cols(R.SMALLM)
    assert any(c.n == 36 and R.SMALLM in c.refused for c in R.CASES)
    for t in R.RING:                                       # every ring kernel on the scalar epilogue: odd ldo, tail, unaligned pointer
        assert any(not c.vec_ok and c.ldo_ % 4 for c in by[t]) and any(c.out_off for c in by[t])
    assert any(c.n % 4 and c.vec_ok for c in by[R.GENERIC]) and any(c.n % 4 and c.vec_ok for c in by[R.WIDE])
    assert {c.taps for c in by[R.GENERIC]} == {1, 3, 5, 7, 9, 11} and {c.taps for c in by[R.NARROW]} == {1, 3, 5, 7, 11}
    assert any(c.taps == 9 and R.NARROW in c.refused for c in R.CASES)
    assert {(3, 1), (7, 3), (11, 5), (11, 6), (3, 32)} <= {(c.taps, c.dil) for c in by[R.RESIDENT]}
    assert {c.nchunk for c in by[R.NARROW] if c.taps == 1} >= {1, 2, 3, 4, 5} - {5} and any(c.K == 320 for c in R.CASES)
    assert any(c.batch == 3 for c in R.CASES) and any(c.batch2 == 3 for c in R.CASES)
    assert all(R.GENERIC in c.tilings for c in R.CASES if c.split == 3) and any(c.split == 3 for c in R.CASES)
