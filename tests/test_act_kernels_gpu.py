"""The general activations (csrc/efts_act.hip) alone: f and f' of every activation id against torch's own module in float64.

GPU tests (marked gpu) call efts_act_apply and efts_act_grad directly through `efficient_tts_amd.lib` for the 20 (name, params) entries of
ACTS in tests/test_gpu_variants.py and the defaults ELU(), CELU(), Softplus(), Hardtanh(); the three tests at the end check refusals and
need no device.

Input.  A deterministic float32 grid (fwd_cases.act_grid): 512 points in (-8, 8), the tails +-{12, 19.5, 20.5, 30, 60, 88}, +-0, and
both sides, at 2^-10, of every breakpoint of the activation (0 for ReLU / LeakyReLU / ELU / CELU / SELU, +-3 for Hardswish and Hardsigmoid,
min_val and max_val for Hardtanh, 0 and 6 for ReLU6, threshold / beta for Softplus, 20 for Mish); no point is on a breakpoint other than 0,
where torch and the kernels take the same side by definition (z > 0).  The grid is laid into [rows, c] in a fixed stride; one more tensor is
3 * randn.  Shapes (1, 4), (63, 124), (64, 128), (65, 132), (130, 512): efts_act_grad works in blocks of 64 rows x 128 columns.

Reference.  getattr(torch.nn, name)(**params) in float64 on the CPU and torch autograd of it; e32 is the same module in float32.
Metric and bound are tests/kernel_check.py's, applied per band of |z| (<= 1, (1, 8], > 8) so that the tails do not set the scale for the
core; f' of Tanh and Sigmoid uses two bands (fwd_cases.GRAD_BANDS_SATURATING says why).  A plane is held to the same bound plus its format's
resolution: 2^-8 (bf16), 2^-16 (bf16x3); a format-3 plane is the fp32 output bit for bit.  Everything must be finite, z = +-88 included.

Measured on one MI355X (the worst `kernel error / e32` over the cases whose bound is the 8 * e32 branch, and the worst error where the
2e-6 floor is the bound):

    kernel                 cases  worst err / e32 (e32 > 2.5e-7)                                      worst err under the 2e-6 floor
    efts_act_apply.fp32     1536  -                                                                   3.0e-07  (Tanhshrink 65x132 random resid=0 mask=0 |z|<=1)
    efts_act_apply.plane1    384  -                                                                   3.7e-03  (Softplus 65x132 random |z|<=1)
    efts_act_apply.plane2    384  -                                                                   6.8e-06  (Tanh 130x512 grid |z|>8)
    efts_act_grad.dz         748  1.00  (SiLU 63x124 grid mask=0 1<|z|<=8: 3.0e-07 / 3.0e-07)         2.5e-07  (Mish 130x512 grid mask=1 1<|z|<=8)
    efts_act_grad.dbias      288  0.60  (GELU_approximatetanh 64x128 grid mask=0: 1.6e-07 / 2.7e-07)  2.8e-07  (Mish 130x512 grid mask=1)
    efts_act_grad.plane1     374  -                                                                   3.6e-03  (LogSigmoid 130x512 grid 1<|z|<=8)
    efts_act_grad.plane2     374  -                                                                   7.1e-06  (Identity 64x128 grid 1<|z|<=8)

Every fp32 figure is below the 2e-6 floor or at ratio 1.0 and nothing was widened.  The plane rows are held to the bound plus the
format's resolution (2^-8 of the band's largest value for format 1, 2^-16 for format 2), which is what their figures are: 3.7e-3 <
2^-8 = 3.9e-3, 7.1e-6 < 2^-16 = 1.5e-5; these rows give the worst error of all cases.
"""
import pytest
import torch

import fwd_cases as F
from kernel_check import _call, _check, _dev, _st, load_lib, unpack_plane

ACT_PARAMS = [pytest.param(n, p, id=F.act_id(n, p)) for n, p in F.act_list()]
SHAPE_PARAMS = [pytest.param(r, c, "grid", id=f"{r}x{c}") for r, c in F.ACT_SHAPES] + [pytest.param(*F.RANDOM_SHAPE, "random", id="random")]
RES = {1: 2.0 ** -8, 2: 2.0 ** -16, 3: 0.0}


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _plane(rows, c, dev):
    kp = (c + 31) // 32 * 32
    return torch.full((rows, kp * 4), 0xAB, dtype=torch.uint8, device=dev), kp


def _banded(kernel, case, z, bands, got, ref64, ref32, extra=0.0):
    got = got.detach().cpu()
    for label, sel in F.band_masks(z, bands):
        if bool(sel.any()):
            _check(kernel, f"{case} {label}", got[sel], ref64[sel], ref32[sel], extra=extra)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,c,kind", SHAPE_PARAMS)
@pytest.mark.parametrize("name,params", ACT_PARAMS)
def test_act_apply_vs_fp64(lib, name, params, rows, c, kind):
    """efts_act_apply: y = (resid + f(z)) * rowmask as fp32, with and without the residual and the row mask, and as a plane of format 1, 2, 3"""
    from efficient_tts_amd import lib as L
    dev = _dev()
    act, p0, p1 = L.actfn(name, params)
    cs = F.act_case(name, params, rows, c, kind)
    z, bands = cs["z"], F.act_bands(name, "apply")
    zd, rd, md = cs["z"].to(dev), cs["resid"].to(dev), cs["rm"].to(dev)
    case = f"{F.act_id(name, params)} {rows}x{c} {kind}"
    dead = cs["rm"] == 0

    def run(use_resid, use_mask, split):
        y = torch.full((rows, c), 7.0, device=dev)
        pl, kp = _plane(rows, c, dev) if split else (None, 0)
        _call("efts_act_apply", lib.efts_act_apply(zd.data_ptr(), rd.data_ptr() if use_resid else None, md.data_ptr() if use_mask else None, act, p0, p1,
                                                   y.data_ptr(), None if pl is None else pl.data_ptr(), kp * 4, split or 1, rows, c, 0.0, 0, _st()))
        torch.cuda.synchronize()
        return y.cpu(), pl, kp

    for use_resid in (False, True):
        for use_mask in (False, True):
            y, _, _ = run(use_resid, use_mask, None)
            ref64, ref32 = F.act_apply_refs(cs, use_resid, use_mask)
            _banded("efts_act_apply.fp32", f"{case} resid={int(use_resid)} mask={int(use_mask)}", z, bands, y, ref64, ref32)
            if use_mask:
                assert bool((y[dead] == 0).all())                                     # masked rows: exactly 0
    ref64, ref32 = F.act_apply_refs(cs, True, True)
    for split in (1, 2, 3):
        y, pl, kp = run(True, True, split)
        got = unpack_plane(pl, 1, rows, rows, kp, split)[0, :, :c]
        if split == 3:
            assert torch.equal(got.contiguous().view(torch.int32), y.view(torch.int32))
        else:
            _banded(f"efts_act_apply.plane{split}", case, z, bands, got, ref64, ref32, extra=RES[split])
        assert bool((got[dead] == 0).all())
        assert torch.isfinite(got).all()


@pytest.mark.gpu
@pytest.mark.parametrize("rows,c,kind", SHAPE_PARAMS)
@pytest.mark.parametrize("name,params", ACT_PARAMS)
def test_act_grad_vs_fp64(lib, name, params, rows, c, kind):
    """efts_act_grad: dZ = G * rowmask * f'(z) as fp32 and as a plane of format 1 and 2; the column sums of dZ ADDED to dbias (one atomic per column
    and 64-row block: 130 rows are three blocks, the last of 2 rows; c = 4, 124, 132 end inside a 128-column group, whose other columns get nothing)."""
    from efficient_tts_amd import lib as L
    dev = _dev()
    act, p0, p1 = L.actfn(name, params)
    cs = F.act_case(name, params, rows, c, kind)
    z, bands = cs["z"], F.act_bands(name, "grad")
    zd, gd, md = cs["z"].to(dev), cs["up"].to(dev), cs["rm"].to(dev)
    case = f"{F.act_id(name, params)} {rows}x{c} {kind}"
    dead = cs["rm"] == 0

    def run(use_mask, split, with_dbias):
        dz = torch.full((rows, c), 7.0, device=dev)
        pl, kp = _plane(rows, c, dev) if split else (None, 0)
        db = cs["db0"].clone().to(dev) if with_dbias else None
        _call("efts_act_grad", lib.efts_act_grad(gd.data_ptr(), zd.data_ptr(), md.data_ptr() if use_mask else None, act, p0, p1, dz.data_ptr(),
                                                 None if pl is None else pl.data_ptr(), kp * 4, split or 1, None if db is None else db.data_ptr(),
                                                 rows, c, 0.0, 0, _st()))
        torch.cuda.synchronize()
        return dz.cpu(), pl, kp, None if db is None else db.cpu()

    for use_mask in (False, True):
        dz, _, _, db = run(use_mask, None, True)
        ref64, ref32 = F.act_grad_refs(cs, use_mask)
        _banded("efts_act_grad.dz", f"{case} mask={int(use_mask)}", z, bands, dz, ref64, ref32)
        _check("efts_act_grad.dbias", f"{case} mask={int(use_mask)}", db[:c], *F.act_dbias_refs(cs, use_mask))
        assert torch.equal(db[c:], cs["db0"][c:])                                     # columns >= c of the last group: no write
        if use_mask:
            assert bool((dz[dead] == 0).all())
        dz0, _, _, _ = run(use_mask, None, False)
        assert torch.equal(dz0.view(torch.int32), dz.view(torch.int32))               # dbias = NULL: the same dz bit for bit
    for split in (1, 2):
        dz1, pl, kp, _ = run(True, split, True)
        assert torch.equal(dz1.view(torch.int32), dz.view(torch.int32))
        got = unpack_plane(pl, 1, rows, rows, kp, split)[0, :, :c]
        _banded(f"efts_act_grad.plane{split}", case, z, bands, got, ref64, ref32, extra=RES[split])
        assert bool((got[dead] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# argument checks (no device work; the pointers are never dereferenced)
# ---------------------------------------------------------------------------------------------------------------------
EINVAL, ESHAPE = -1, -2
X = 0x1000


@pytest.fixture(scope="module")
def cpu_lib():
    from efficient_tts_amd import build as B
    from efficient_tts_amd import lib as L
    B.build(verbose=False)
    return L.load()


@pytest.mark.parametrize("act", [-1, 19, 1000])
def test_act_kernels_refuse_an_unknown_activation(cpu_lib, act):
    assert cpu_lib.efts_act_apply(X, None, None, act, 0.0, 0.0, X, None, 0, 1, 8, 32, 0.0, 0, None) == EINVAL
    assert b"efts_act_apply" in cpu_lib.efts_last_error() and b"activation" in cpu_lib.efts_last_error()
    assert cpu_lib.efts_act_grad(X, X, None, act, 0.0, 0.0, X, None, 0, 1, None, 8, 32, 0.0, 0, None) == EINVAL
    assert b"efts_act_grad" in cpu_lib.efts_last_error() and b"activation" in cpu_lib.efts_last_error()


@pytest.mark.parametrize("rows,c", [(8, 30), (8, 1), (8, 0), (0, 32), (8, -4)])
def test_act_kernels_refuse_bad_shapes(cpu_lib, rows, c):
    assert cpu_lib.efts_act_apply(X, None, None, 1, 0.0, 0.0, X, None, 0, 1, rows, c, 0.0, 0, None) == ESHAPE
    assert b"multiple of 4" in cpu_lib.efts_last_error()
    assert cpu_lib.efts_act_grad(X, X, None, 1, 0.0, 0.0, X, None, 0, 1, None, rows, c, 0.0, 0, None) == ESHAPE
    assert b"multiple of 4" in cpu_lib.efts_last_error()


def test_act_kernels_refuse_formats_they_have_no_form_of(cpu_lib):
    assert cpu_lib.efts_act_grad(X, X, None, 1, 0.0, 0.0, None, X, 128, 3, None, 8, 32, 0.0, 0, None) == EINVAL      # training has no fp32 planes
    assert b"split" in cpu_lib.efts_last_error()
    for split in (0, 4):
        assert cpu_lib.efts_act_apply(X, None, None, 1, 0.0, 0.0, None, X, 128, split, 8, 32, 0.0, 0, None) == EINVAL
        assert b"split" in cpu_lib.efts_last_error()
        assert cpu_lib.efts_act_grad(X, X, None, 1, 0.0, 0.0, None, X, 128, split, None, 8, 32, 0.0, 0, None) == EINVAL
        assert b"split" in cpu_lib.efts_last_error()
    assert cpu_lib.efts_act_apply(X, None, None, 1, 0.0, 0.0, None, None, 0, 1, 8, 32, 0.0, 0, None) == EINVAL          # no output at all
    assert b"null" in cpu_lib.efts_last_error()
