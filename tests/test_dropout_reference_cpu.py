"""CPU: tests/dropout_reference.py pinned -- the inputs of tests/test_dropout_kernels_gpu.py to the condition of kernel_check's bound, every
host mask to a state in which an exact keep-set comparison can fail (kept and dropped elements in every column group, the binomial
share), the inputs to a state in which the keep set can be read off an output (no kept element that looks dropped) -- and the refusals
the dropout arguments of efts_gemm, efts_act_apply and efts_act_grad answer without a device (the pointers are never dereferenced)."""
import ctypes as C

import numpy as np
import pytest
import torch

import dropout_reference as D
import gemm_reference as G
from kernel_check import conditioned
from train_pack_reference import drop_params, keep_scale

EINVAL = -1
X = 0x1000


# ---------------------------------------------------------------------------------------------------------------------
# the bound's condition: FACTOR * e32 <= COND for every reduction of the GPU file
# ---------------------------------------------------------------------------------------------------------------------
def test_every_reduction_is_conditioned():
    n = 0
    for name, ref64, ref32 in D.reduction_cases():
        ok, e32 = conditioned(ref64, ref32)
        assert ok, f"{name}: inputs too ill-conditioned for the bound to mean anything (e32 = {e32:.3e})"
        n += 1
    assert n == len(D.LN_CASES) * (2 + 3 + 5 + 5) + 2 * len(D.act_cases())


# ---------------------------------------------------------------------------------------------------------------------
# the host masks
# ---------------------------------------------------------------------------------------------------------------------
def test_the_case_tables_cover_what_they_name():
    ps = {d.p for d in D.GEMM_CASES}
    assert ps == set(D.DROP_PS) and {d.seed for d in D.GEMM_CASES} == set(D.DROP_SEEDS) and max(D.DROP_SEEDS) >= 2 ** 31
    assert {(d.case.taps, d.case.m) for d in D.GEMM_CASES} >= {(1, 130), (5, 362), (1, 7)}
    assert {d.case.n for d in D.GEMM_CASES} == {128, 256, 320, 80}
    assert {d.case.ldo_ - d.case.n for d in D.GEMM_CASES} == {0, 8}
    for sp in (1, 2):
        assert any(d.case.split == sp and G.WIDE in d.tilings for d in D.GEMM_CASES)
    assert all(d.tilings == (G.GENERIC, G.AUTO) and d.case.taps == 1 for d in D.GEMM_CASES if d.case.split == 3)
    assert all(d.sign == (d.case.n % 128 == 0) and d.case.batch == 1 and d.case.act == G.ACT_LEAKY for d in D.GEMM_CASES)
    assert {c[1] for c in D.LN_CASES} == {256, 512, 2048} and {c[0] for c in D.LN_CASES} == {1, 7, 9, 130}
    assert {c[2] for c in D.LN_CASES} == set(D.DROP_PS) and any(c[4] is None for c in D.LN_CASES)
    assert {(c[2], c[3]) for c in D.act_cases()} == {tuple(s) for s in D.F.ACT_SHAPES}
    assert {c[4] for c in D.act_cases()} == set(D.DROP_PS) and len(D.act_cases()) == 4 * len(D.F.ACT_SHAPES)


def test_every_host_mask_has_kept_and_dropped_elements_and_the_binomial_share():
    """an empty or a full mask would let an exact keep-set comparison pass trivially"""
    n = 0
    for name, p, keep in D.mask_cases():
        _, inv_keep = drop_params(p)
        assert set(np.unique(keep.numpy())) <= {np.float32(0.0), inv_keep}, name
        rows, c = keep.shape
        for c0 in range(0, c, 128):
            grp = keep[:, c0:c0 + 128]
            if grp.numel() >= 64:
                assert bool((grp == 0).any()) and bool((grp != 0).any()), f"{name}: column group {c0 // 128} is all kept or all dropped"
        if keep.numel() >= 4096:
            kept = float((keep != 0).double().mean())
            sigma = (p * (1 - p) / keep.numel()) ** 0.5
            assert abs(kept - (1 - p)) <= 4 * sigma, (name, kept, 1 - p, sigma)
        n += 1
    assert n == len(D.GEMM_CASES) + len(D.LN_CASES) + len(D.act_cases())


def test_the_seed_wrap_cases_wrap_and_the_device_word_changes_the_mask():
    wraps = [c for c in D.LN_CASES if c[4] is not None and c[3] + c[4] >= 2 ** 32]
    assert len(wraps) >= 1 and all(c[4] == D.WRAP_ADD for c in wraps)
    idx = np.arange(4096)
    for rows, c, p, seed, add in wraps:
        got = D.ln_keep_scale(seed, add, idx, p)
        assert np.array_equal(got, keep_scale(seed + add - 2 ** 32, idx, p))           # the uint32 sum, not the integer one
    for case in D.LN_CASES:
        rows, c, p, seed, add = case
        if add is not None and rows * c >= 1024:
            assert not torch.equal(D.ln_keep(case), D.ln_keep(case, add=None)), D.ln_id(case)
    assert np.array_equal(D.ln_keep_scale(77, None, idx, 0.25), keep_scale(77, idx, 0.25))


# ---------------------------------------------------------------------------------------------------------------------
# the keep set can be read off the outputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", D.GEMM_CASES, ids=[d.name for d in D.GEMM_CASES])
def test_gemm_inputs_no_kept_element_looks_dropped(d):
    """The GPU file calls an element dropped iff the output equals resid * rowmask bit for bit.  A kept element could only look so if its
    scaled activated value vanished next to the residual (below half a spacing of it, 1e-7): in the float32 transcription none does, and
    no activated value is 0.  The contraction can not be drawn away from 0 as an input can, so the GPU file asserts the same of the
    kernel's own activated values before it reads a keep set.  The row mask has live rows, and dead ones where there is more than one row tile."""
    r = D.gemm_reference(d)
    live = r.mask != 0
    assert bool(live.any()) and (d.case.m < 130 or bool((~live).any()))
    assert bool((r.a64 != 0).all()) and bool((r.a32 != 0).all())
    looks_dropped = (r.a32 * r.keep + r.resid).view(torch.int32) == r.resid.contiguous().view(torch.int32)
    assert torch.equal(looks_dropped, r.keep == 0), f"{d.name}: a kept element of the float32 transcription equals its residual"
    ok, e32 = conditioned(r.ref64, r.ref32)
    assert ok, (d.name, e32)


@pytest.mark.parametrize("case", D.LN_CASES, ids=D.ln_id)
def test_layernorm_inputs_no_kept_element_is_zero(case):
    """kept elements of live rows stay away from 0 by far more than the kernel's error on them (2e-6 of a value of order 1)"""
    i = D.ln_inputs(case[0], case[1])
    y64, y32 = D.ln_forward(case)["rows"]
    kept = (D.ln_keep(case) != 0) & (i.rm != 0)[:, None]
    assert float(y64[kept].abs().min()) >= 4e-6 and bool((y32[kept] != 0).all())
    assert bool((y64[~kept] == 0).all())
    assert float(i.beta.abs().min()) > 0
    assert case[0] == 1 or (bool((i.rm == 0).any()) and bool((i.rm != 0).any()))


@pytest.mark.parametrize("case", D.act_cases(), ids=D.act_case_id)
def test_act_inputs_no_kept_element_looks_dropped(case):
    i = D.act_inputs(case[2], case[3])
    keep = D.act_keep(case)
    live = (i.rm != 0)[:, None]
    for use_resid in (False, True):
        r = D.act_reference(case, use_resid, True)
        y32, dz32 = r["y"][1], r["dz"][1]
        # (without a residual a dropped element is f(z) * 0 = +-0: compared as a value; with one, bit for bit)
        looks_dropped = y32.view(torch.int32) == (i.resid * i.rm[:, None]).view(torch.int32) if use_resid else y32 == 0
        assert torch.equal(looks_dropped | ~live, (keep == 0) | ~live)
        assert torch.equal((dz32 == 0) | ~live, (keep == 0) | ~live)
        d64 = r["dz"][0]
        assert float(d64[(keep != 0) & live].abs().min()) > 1e-9


# ---------------------------------------------------------------------------------------------------------------------
# refusals (no device work)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from efficient_tts_amd import build as B
    from efficient_tts_amd import lib as L
    B.build(verbose=False)
    return L.load()


def _gemm(lib, **kw):
    """efts_gemm on a well-formed one-tap 130 x 128 launch with dropout, changed by `kw`: (return code, message)"""
    from efficient_tts_amd import lib as L
    g = L.GemmArgs()
    g.a, g.lda, g.b, g.ldb, g.b_tap_stride = X, 128, X, 128, 128 * 128
    g.split, g.taps, g.m, g.n, g.nchunk, g.batch = 1, 1, 130, 128, 1, 1
    g.alpha, g.act, g.slope, g.dilation = 1.0, G.ACT_LEAKY, 0.1, 1
    g.out_f32, g.ldo = X, 128
    g.drop_p, g.drop_seed = 0.25, 77
    g.tiling = G.GENERIC
    for k, v in kw.items():
        setattr(g, k, v)
    rc = lib.efts_gemm(C.byref(g), None)
    return rc, lib.efts_last_error()


def test_gemm_refuses_dropout_it_has_no_form_of(lib):
    rc, msg = _gemm(lib, batch=2, a_batch_stride=1 << 16, out_batch_stride=1 << 16)
    assert rc == EINVAL and b"dropout needs batch 1" in msg
    for p in (1.0, 1.5):
        rc, msg = _gemm(lib, drop_p=p)
        assert rc == EINVAL and b"drop_p must be in [0, 1)" in msg
    rc, msg = _gemm(lib, n=130, ldo=132)
    assert rc == EINVAL and b"n % 4 == 0" in msg
    for tiling, extra in ((G.NARROW, {}), (G.RESIDENT, dict(taps=3, n=64, ldo=64)), (G.SMALLM, dict(taps=5))):
        rc, msg = _gemm(lib, tiling=tiling, **extra)
        assert rc == EINVAL and b"dropout needs the generic or wide tiling" in msg, (tiling, rc, msg)       # (each shape suits its tiling)
    rc, msg = _gemm(lib, n=96, ldo=96, rowmask=X, sqerr_target=X, ld_target=96, target_batch_stride=130 * 96, sqerr_part=X)
    assert rc == EINVAL and b"sqerr_part needs" in msg and b"dropout" in msg


@pytest.mark.parametrize("p", [1.0, 2.0])
def test_act_kernels_refuse_a_drop_p_of_one_or_more(lib, p):
    assert lib.efts_act_apply(X, None, None, 1, 0.0, 0.0, X, None, 0, 1, 8, 32, p, 7, None) == EINVAL
    assert b"efts_act_apply" in lib.efts_last_error() and b"drop_p must be in [0, 1)" in lib.efts_last_error()
    assert lib.efts_act_grad(X, X, None, 1, 0.0, 0.0, X, None, 0, 1, None, 8, 32, p, 7, None) == EINVAL
    assert b"efts_act_grad" in lib.efts_last_error() and b"drop_p must be in [0, 1)" in lib.efts_last_error()
