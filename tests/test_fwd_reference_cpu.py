"""CPU: every case of tests/test_fwd_kernels_gpu.py and tests/test_act_kernels_gpu.py is conditioned well enough for its bound.

The bound of kernel_check._check is max(8 * e32, 2e-6), where e32 is the error of the float32 torch transcription against float64.
It only means something while 8 * e32 <= 2e-4, which `_check` asserts next to the kernel's error.  Here the same input makers and the
same two transcriptions (tests/fwd_cases.py) run without a device and that condition alone is asserted, so that an ill-conditioned
input is found before a GPU is spent on it.  Where a case could not meet it the inputs were changed, not the constants:
  * the inference form of efts_reconst_alpha gets items that span T1 x T2 (fwd_cases.ralpha_case says why);
  * f' of Tanh and Sigmoid is measured in two bands instead of three (fwd_cases.GRAD_BANDS_SATURATING says why).
"""
import pytest
import torch

import fwd_cases as F
from kernel_check import COND, FACTOR, conditioned


def _assert_conditioned(case, refs):
    for name, (r64, r32) in refs.items():
        assert r64.dtype == torch.float64 and r32.dtype == torch.float32
        assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all()), f"{case} {name}"
        ok, e32 = conditioned(r64, r32)
        assert ok, f"{case} {name}: e32 = {e32:.3e}, {FACTOR} * e32 > {COND}"


@pytest.mark.parametrize("B,T1,T2", F.ATTN_SHAPES)
def test_attn_soft_index_cases(B, T1, T2):
    for ldx in (0, 3):
        _assert_conditioned(f"{B}x{T1}x{T2}", F.attn_case(B, T1, T2, ldx)["refs"])


@pytest.mark.parametrize("T2", F.IMV_T2)
def test_imv_scan_cases(T2):
    _assert_conditioned(f"T2={T2}", F.imv_case(T2)["refs"])
    cs = F.imv_hard_case(T2)
    _assert_conditioned(f"hard T2={T2}", cs["refs"])
    r64, r32 = cs["refs"]["imv"]
    for b in range(1, 4):
        if float(r64[b].abs().max()) > 0:
            _assert_conditioned(f"hard T2={T2}[item {b}]", {"imv": (r64[b], r32[b])})
    assert float(r64[0].abs().max()) == 0.0                                         # the inputs are what the docstring says they are
    if T2 >= 63:
        assert bool((cs["sidx"][1, int(cs["ml"][1]):].diff() > 0).any()) and float(r64[1].max()) == float(cs["tl"][1]) - 1.0
        assert int((r64[2] == r64[2].max()).sum()) >= 3


@pytest.mark.parametrize("B,T1,T2", F.EPOS_SHAPES)
def test_aligned_positions_cases(B, T1, T2):
    _assert_conditioned(f"{B}x{T1}x{T2}", F.epos_case(B, T1, T2)["refs"])


@pytest.mark.parametrize("method1", [True, False])
@pytest.mark.parametrize("B,T1", F.DUR_SHAPES)
def test_duration_target_cases(B, T1, method1):
    cs = F.dur_case(B, T1, method1)
    _assert_conditioned(f"{B}x{T1} method1={method1}", cs["refs"])
    e, tm = cs["e"], cs["tm"]
    assert bool((e[:, 1:] > e[:, :-1])[tm[:, 1:]].all()) and bool((e[:, 0] > 0).all())        # positive differences
    last = e.gather(1, (cs["tl"].long() - 1)[:, None])[:, 0]
    assert bool((last < cs["ml"]).all())


@pytest.mark.parametrize("method1", [True, False])
@pytest.mark.parametrize("B,T1,T2", F.ALIGN_SHAPES)
def test_imv_align_cases(B, T1, T2, method1):
    _assert_conditioned(f"{B}x{T1}x{T2} method1={method1}", F.align_case(B, T1, T2, method1)["refs"])


def test_imv_align_exact_case_is_exact():
    """the integer soft index: float32 and float64 transcriptions agree to the one rounding of the final product"""
    cs = F.align_exact_case()
    mm = F.R.non_pad_mask(cs["ml"], cs["T2"])
    r64 = F.R.imv_from_soft_index(cs["sidx"].double(), mm, cs["tl"])
    assert torch.equal(cs["imv32"], r64.float())
    assert bool((cs["sidx"] == cs["sidx"].round()).all()) and float(cs["sidx"].abs().max()) < 2 ** 12


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("B,T1,T2", F.RALPHA_SHAPES)
def test_reconst_alpha_cases(B, T1, T2, masked):
    _assert_conditioned(f"{B}x{T1}x{T2} masked={masked}", F.ralpha_case(B, T1, T2, masked)["refs"])


@pytest.mark.parametrize("B,T1,T2", F.CHAIN_SHAPES)
def test_chain_cases(B, T1, T2):
    """the chain's bound is capped instead (test_forward_alignment_chain_vs_fp64): only its first stage is held to the condition here"""
    cs = F.chain_case(B, T1, T2)
    _assert_conditioned(f"chain {B}x{T1}x{T2}", {"soft_idx": cs["refs"]["soft_idx"]})
    assert float(cs["refs"]["soft_idx"][0].diff(dim=1).abs()[cs["mm"][:, 1:]].min()) >= 1e-4


ACT_PARAMS = [pytest.param(n, p, id=F.act_id(n, p)) for n, p in F.act_list()]


def test_the_activation_list_is_the_variants_list_plus_defaults():
    names = F.act_list()
    assert len(names) == 24 and len({F.act_id(n, p) for n, p in names}) == 24
    from efficient_tts_amd import lib as L
    assert all(L.actfn(n, p) is not None for n, p in names)
    assert {L.actfn(n, p)[0] for n, p in names} == set(range(19))                   # every id of the library


@pytest.mark.parametrize("name,params", ACT_PARAMS)
def test_activation_cases(name, params):
    shapes = [(r, c, "grid") for r, c in F.ACT_SHAPES] + [F.RANDOM_SHAPE + ("random",)]
    for rows, c, kind in shapes:
        cs = F.act_case(name, params, rows, c, kind)
        z = cs["z"]
        case = f"{F.act_id(name, params)} {rows}x{c} {kind}"
        for which, pairs in (("apply", [F.act_apply_refs(cs, r, m) for r in (False, True) for m in (False, True)]),
                             ("grad", [F.act_grad_refs(cs, m) for m in (False, True)])):
            for r64, r32 in pairs:
                for label, sel in F.band_masks(z, F.act_bands(name, which)):
                    if bool(sel.any()):
                        _assert_conditioned(f"{case} {which} {label}", {which: (r64[sel], r32[sel])})
        if kind == "grid" and rows * c >= 600:                                       # the whole grid is in the tensor: both sides of every breakpoint
            for b in F.act_breakpoints(name, params):
                b32 = float(torch.tensor(b, dtype=torch.float32))
                assert bool(((z.double() - b32).abs() == 2.0 ** -10).sum() >= 2) and not bool((z.double() == b32).any() and b != 0.0)
            assert bool((z.abs() == 88.0).any()) and bool((z == 0).sum() >= 2)
        # the column sums behind dbias
        for m in (False, True):
            _assert_conditioned(f"{case} dbias", {"dbias": F.act_dbias_refs(cs, m)})
