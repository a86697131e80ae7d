"""GPU (-m gpu): every launch that draws a train-mode Dropout mask, alone, against the host's mask element by element.

    efts_gemm (EPI_DROP: generic, wide, AUTO)   efts_layernorm_rows   efts_layernorm_dot   efts_layernorm_bwd   efts_act_apply   efts_act_grad
    and the forward / backward pairs the engine uses (with efts_act_bwd_dropout modes 1 and 4)

called directly through `efficient_tts_amd.lib` on the cases of tests/dropout_reference.py (pinned without a device by
tests/test_dropout_reference_cpu.py, which also asserts the condition of the bound for every sum below and that every host mask has kept
and dropped elements).  No launch stores its mask: forward and backward each draw it from (seed, element index), every launch spelling the
index out for itself; a slip on one side leaves every kept share right and the gradients silently wrong.  So the KEEP SET of every launch
is read off its output -- an element is dropped iff the output is bit for bit what the launch writes for a zero, (0 + resid) * rowmask --
and must equal keep_scale(seed, row * n + col, p) == 0 of the host with ZERO mismatches; the first mismatching (row, col) is reported.

Every output lies between canary bytes and is compared whole.  Exact: keep sets, sign words (those of the activated value BEFORE dropout:
byte for byte the drop-free launch's and the host's), the p = 0.5 values of efts_gemm ((2 a + resid) * rowmask in float32, a = the kernel's
own activated value from a launch without residual, mask and dropout: the scale 2 rounds nothing, contracted or not), the tilings among each
other, a repeated launch, the plane bytes against the host encoding of the launch's own fp32 result.  Everything else: float64 through
kernel_check._check (FACTOR, FLOOR, COND = 8, 2e-6, 2e-4; a decoded plane plus its format's resolution), efts_gemm also per element to the
a-priori bound of gemm_reference carried through the three extra steps.  Nothing widened, no new constant.

The backward references are torch autograd, in float64, of the masked forward.  efts_layernorm_bwd has no output whose zeros are the mask
(dz mixes a row's elements), so its pair test feeds it one row of dy at a time into a zeroed dbeta: dbeta is then dy[row] * mask[row] exactly.

Measured on one MI355X (the worst `kernel error / e32` over the cases whose bound is the 8 * e32 branch, and the worst error where the
2e-6 floor is the bound):

    kernel and output                   cases  worst err / e32 (e32 > 2.5e-7)                              worst err under the 2e-6 floor
    efts_gemm.drop                         48  -                                                           2.0e-07  (bf16x3 t5 m362 n80 p0.25)
    efts_gemm.drop.plane1                  18  -                                                           2.8e-03  (bf16 t1 m130 n128 p0.5)
    efts_gemm.drop.plane2                  20  -                                                           5.9e-06  (bf16x3 t1 m130 n320 p0.5)
    efts_gemm.drop.plane3                  10  -                                                           1.9e-07  (fp32 t1 m130 n80 p0.5)
    efts_layernorm_rows.drop               12  -                                                           1.8e-07  (9x512 p0.5)
    efts_layernorm_rows.drop.plane2        12  -                                                           6.3e-06  (9x512 p0.5)
    efts_layernorm_dot.drop.mode0          12  3.70  (1x512 p0.1: 2.9e-06 / 7.7e-07)                       1.4e-07  (9x256 p0.25)
    efts_layernorm_dot.drop.mode1          12  5.70  (1x512 p0.1: 3.2e-06 / 5.7e-07)                       3.8e-07  (130x256 p0.5)
    efts_layernorm_bwd.drop.dz             36  -                                                           1.9e-07  (ddur 1x256 p0.5)
    efts_layernorm_bwd.drop.dgamma         36  -                                                           2.4e-07  (ddur 130x512 p0.1)
    efts_layernorm_bwd.drop.dbeta          36  -                                                           1.6e-07  (ddur 130x512 p0.1)
    efts_layernorm_bwd.drop.dbias          36  -                                                           1.9e-07  (dy 130x2048 p0.25)
    efts_layernorm_bwd.drop.dw             24  0.47  (ddur_rowmask 130x512 p0.1: 1.3e-07 / 2.7e-07)        2.0e-07  (ddur 9x2048 p0.1)
    efts_layernorm_bwd.drop.db             24  -                                                           2.3e-07  (ddur_rowmask 130x256 p0.5)
    efts_act_apply.drop                    80  -                                                           1.1e-07  (SiLU 130x512 p0.25 resid=0 mask=1)
    efts_act_grad.drop.dz                  40  -                                                           1.2e-07  (SiLU 130x512 p0.25 mask=1)
    efts_act_grad.drop.dbias               40  -                                                           1.7e-07  (SiLU 65x132 p0.1 mask=1)
    largest e32 of a case: 9.8e-07

Every case meets the bound: nothing is held to the a-priori bound alone and nothing was widened.  The two ratios above 1 are the single-row
efts_layernorm_dot cases (one output number: the metric is relative to it alone, and the wave's butterfly sum is ordered otherwise than
torch's); the plane rows are held to the bound plus the format's resolution, which is what their figures are (2.8e-3 < 2^-8, 6.3e-6 < 2^-16).
Exact and without a mismatch: the keep sets of 48 + 20 efts_gemm launches, 12 + 12 + 2 efts_layernorm_rows ones, 80 efts_act_apply and 40
efts_act_grad ones, the sign words of 24 launches, the p = 0.5 values of 8 cases on every tiling, the four pairs.

Each of these one-line breaks fails here (first failing case, file order; tried one at a time on a scratch copy):
  1. `(unsigned)p.n` -> `(unsigned)p.ldo` in the EPI_DROP index: test_gemm_dropout_vs_host_mask[drop-bf16x3-t5-m362-n128-ldo136-p0.5-s2654435769]
     (17805 of 35712 elements, the first at (1, 0));
  2. `t.m0 +` removed from it: test_gemm_dropout_vs_host_mask[drop-bf16-t5-m362-n128-ldo128-p0.25-s77] (the first at (124, 3): the second row tile);
  3. `t.col` -> `t.c4` in it: test_gemm_dropout_vs_host_mask[drop-bf16-t5-m362-n256-ldo264-p0.5-s77] (the first at (1, 128): the second column tile);
  4. `e0 + 2` -> `e0 + 1` in layernorm_kernel: test_layernorm_forward_dropout_vs_host_mask[1x256-p0.5-s77-addNone] (26 of 256, the first at (0, 10));
  5. `seed_add ? *seed_add : 0u` -> `0u` in layernorm_bwd_kernel only: test_layernorm_bwd_dropout_vs_fp64[7x256-p0.1-s2654435769-add5-dy] (dz off by 0.5);
  6. `* dms[e]` removed from the `aw` accumulation: test_layernorm_bwd_dropout_vs_fp64[1x256-p0.5-s77-addNone-ddur] (dw off by 0.63);
  7. the drop_thresh block of act_grad_kernel removed: test_act_apply_and_grad_dropout_vs_host_mask[Identity-1x4-p0.1-s77] (dz off by 0.1);
  8. drop_scale after the residual add in act_apply_kernel: test_act_apply_and_grad_dropout_vs_host_mask[Identity-1x4-p0.1-s77] (resid=1: off by 0.09).
"""
import pytest
import torch

import dropout_reference as D
import gemm_reference as G
import train_pack_reference as T
from kernel_check import _call, _check, _dev, _st, load_lib
from test_gemm_kernels_gpu import _Outputs, _check_plane_bytes, _device_operands, _launch, _plane_values
from test_train_pack_kernels_gpu import Out, _bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _same_set(got, want, sel, what):
    """boolean [rows][c] `got` (the kernel's dropped set) equals `want` (the host's) wherever `sel`; reports the first mismatch"""
    bad = (got != want) & sel
    if bool(bad.any()):
        r, c = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {int(sel.sum())} elements differ from the host mask, the first at (row, col) = ({r}, {c}): "
                             f"the kernel {'dropped' if bool(got[r, c]) else 'kept'} it")


def _rows(sel, c):
    return sel[:, None].expand(-1, c)


# ---------------------------------------------------------------------------------------------------------------------
# efts_gemm
# ---------------------------------------------------------------------------------------------------------------------
class _Sign:
    """sign words [m][n / 8] between OUT_GUARD canary rows"""

    def __init__(self, c):
        self.c, self.ld = c, c.n // 8
        self.t = torch.full((c.m + 2 * G.OUT_GUARD, self.ld), G.CANARY, dtype=torch.uint8, device=_dev())
        self.ptr = self.t.data_ptr() + G.OUT_GUARD * self.ld

    def collect(self):
        raw, g = self.t.cpu(), G.OUT_GUARD
        assert bool((raw[:g] == G.CANARY).all()) and bool((raw[g + self.c.m:] == G.CANARY).all()), f"{self.c.name}: sign words outside rows [0, m)"
        return raw[g:g + self.c.m].clone()


def _gemm_run(lib, c, ops, tiling, drop=None, sign=False):
    """one launch of `c` -> (fp32 [m][n], plane bytes [1][m][ldob] or None, sign bytes [m][n / 8] or None); every canary checked"""
    o = _Outputs(c, _dev())
    s = _Sign(c) if sign else None

    def hook(g):
        if drop is not None:
            g.drop_p, g.drop_seed = drop
        if s is not None:
            g.sign_mask = s.ptr
    _launch(lib, c, ops, o, tiling, hook)
    torch.cuda.synchronize()
    f, p, _ = o.collect()
    return f[0, 0], p, None if s is None else s.collect()


def _gemm_dropped(d, r, f, a, seed, what):
    """the dropped set of fp32 output `f` on live rows, after asserting that it can be read: no kept element of the kernel's own activated
    value `a` is so small that adding it leaves the residual where it is"""
    keep = r.keep if seed == d.seed else D.gemm_keep(d, seed)
    live = _rows(r.mask != 0, d.case.n)
    kept = (keep != 0) & live
    assert bool(((a.double().abs() * keep.double())[kept] > 2 * G._ulp(r.resid.double())[kept]).all()), f"{what}: a kept value below two spacings of its residual"
    got = _bits(f).view(f.shape) == _bits(r.resid * r.mask[:, None]).view(f.shape)
    _same_set(got, keep == 0, live, what)
    assert bool((f[~live] == 0).all()), f"{what}: a dead row is not 0"
    return got & live


@pytest.mark.parametrize("d", D.GEMM_CASES, ids=[d.name for d in D.GEMM_CASES])
def test_gemm_dropout_vs_host_mask(lib, d):
    c, r = d.case, D.gemm_reference(d)
    ops = _device_operands(c, _dev())
    live = _rows(r.mask != 0, c.n)
    res = G.storage_resolution(c.osplit)
    seen = {}
    for tiling in d.tilings:
        tag = f"efts_gemm[{G.TILING_NAME[tiling]}]"
        what = f"{d.name} {tag}"
        f0, _, s0 = _gemm_run(lib, c, ops, tiling, None, d.sign)                      # drop_p = 0
        f1, p1, s1 = _gemm_run(lib, c, ops, tiling, (d.p, d.seed), d.sign)
        a, _, _ = _gemm_run(lib, d.plain, ops, tiling)                                # the kernel's own activated value
        assert bool((a != 0).all())
        assert torch.equal(_bits(f0).view(f0.shape)[live], _bits((a + r.resid) * r.mask[:, None]).view(f0.shape)[live]), f"{what}: drop_p = 0 is not (a + resid) * rowmask"
        # 1. the keep set
        _gemm_dropped(d, r, f1, a, d.seed, what)
        # 2. the values
        if d.p == 0.5:
            want = (r.keep * a + r.resid) * r.mask[:, None]                           # keep is 2 or 0: the product is exact
            assert torch.equal(_bits(f1).view(f1.shape)[live], _bits(want).view(f1.shape)[live]), f"{what}: p = 0.5 is not (2 a + resid) * rowmask bit for bit"
        _check(tag + ".drop", d.name, f1, r.ref64, r.ref32)
        assert bool(((f1.double() - r.ref64).abs() <= r.bound).all()), f"{what}: an element misses the a-priori bound"
        _check_plane_bytes(c, p1, f1[None], "the plane")
        _check(tag + f".drop.plane{c.osplit}", d.name, _plane_values(p1, c)[0, 0], r.ref64, r.ref32, extra=res)
        # 4. the sign words: those of the activated value before dropout
        if d.sign:
            assert torch.equal(s1, s0), f"{what}: the sign words change with dropout"
            assert torch.equal(s0, T.sign_words(a > 0)), f"{what}: the sign words are not those of the activated value"
        seen[tiling] = (f1, p1)
    # 3. the tilings agree bit for bit
    first = d.tilings[0]
    for tiling in d.tilings[1:]:
        assert torch.equal(_bits(seen[tiling][0]), _bits(seen[first][0])) and torch.equal(seen[tiling][1], seen[first][1]), \
            f"{d.name}: {G.TILING_NAME[tiling]} differs from {G.TILING_NAME[first]} with dropout on"
    # 5. the same seed twice: equal bits; another seed: the host's keep set for that seed, and another one
    again, pa, _ = _gemm_run(lib, c, ops, first, (d.p, d.seed))
    assert torch.equal(_bits(again), _bits(seen[first][0])) and torch.equal(pa, seen[first][1])
    other = next(s for s in D.DROP_SEEDS if s != d.seed)
    f2, _, _ = _gemm_run(lib, c, ops, first, (d.p, other))
    a, _, _ = _gemm_run(lib, d.plain, ops, first)
    set2 = _gemm_dropped(d, r, f2, a, other, f"{d.name} seed {other}")
    assert not torch.equal(set2, (r.keep == 0) & live)


# ---------------------------------------------------------------------------------------------------------------------
# efts_layernorm_rows / efts_layernorm_dot / efts_layernorm_bwd
# ---------------------------------------------------------------------------------------------------------------------
def _ln_device(rows, c):
    i = D.ln_inputs(rows, c)
    dev = _dev()
    return i, {k: getattr(i, k).to(dev) for k in ("x", "gamma", "beta", "rm", "w", "b", "dy", "ddur")}


def _word(add):
    """the device word behind drop_seed_add, written in stream order; None: no word"""
    from efficient_tts_amd import ops as O
    if add is None:
        return None
    w = torch.zeros(1, dtype=torch.int32, device=_dev())
    O.store_words(w, [add])
    return w


def _ln_rows(lib, t, rows, c, p, seed, word, y=None, plane=None, ld=0, split=1):
    _call("efts_layernorm_rows", lib.efts_layernorm_rows(t["x"].data_ptr(), t["gamma"].data_ptr(), t["beta"].data_ptr(), D.LN_EPS, t["rm"].data_ptr(),
                                                         None if y is None else y.ptr, None if plane is None else plane.ptr, ld, rows, c, split, p, seed,
                                                         None if word is None else word.data_ptr(), _st()))


@pytest.mark.parametrize("case", D.LN_CASES, ids=D.ln_id)
def test_layernorm_forward_dropout_vs_host_mask(lib, case):
    """efts_layernorm_rows as fp32 and as a format-2 plane, efts_layernorm_dot in mode 0 and 1: the mask of (drop_seed + *drop_seed_add) on
    LN * gamma + beta, before the row mask and the dot.  Dropped elements are exactly 0, kept ones are not; dead rows are exactly 0"""
    rows, c, p, seed, add = case
    i, t = _ln_device(rows, c)
    fwd, keep = D.ln_forward(case), D.ln_keep(case)
    word = _word(add)
    live = _rows(i.rm != 0, c)
    name = D.ln_id(case)
    y = Out(rows * c * 4)
    _ln_rows(lib, t, rows, c, p, seed, word, y=y)
    got = y.f32().view(rows, c)
    _same_set(got == 0, keep == 0, live, f"efts_layernorm_rows {name}")
    assert bool((got[~live] == 0).all())
    _check("efts_layernorm_rows.drop", name, got, *fwd["rows"])
    ld = G.row_bytes(c, 2) + 16
    pl = Out(rows * ld)
    _ln_rows(lib, t, rows, c, p, seed, word, plane=pl, ld=ld, split=2)
    raw = pl.bytes().view(rows, ld)
    assert bool((raw[:, G.row_bytes(c, 2):] == G.CANARY).all())
    dec = G.decode_rows(raw, c, 2)[:, :c]
    _same_set(dec == 0, keep == 0, live, f"efts_layernorm_rows plane {name}")
    assert bool((dec[~live] == 0).all())
    _check("efts_layernorm_rows.drop.plane2", name, dec, *fwd["rows"], extra=G.storage_resolution(2))
    for mode in (0, 1):
        out = Out(rows * 4)
        _call("efts_layernorm_dot", lib.efts_layernorm_dot(t["x"].data_ptr(), t["gamma"].data_ptr(), t["beta"].data_ptr(), D.LN_EPS, t["w"].data_ptr(),
                                                           t["b"].data_ptr(), t["rm"].data_ptr(), mode, D.DOT_OFFSET, out.ptr, rows, c, p, seed,
                                                           None if word is None else word.data_ptr(), _st()))
        o = out.f32()
        _check(f"efts_layernorm_dot.drop.mode{mode}", name, o, *fwd[f"dot{mode}"])
        assert bool((o[i.rm == 0] == 0).all())


def test_layernorm_reads_the_seed_word_in_stream_order(lib):
    """word <- a; launch; word <- b; launch, with nothing between them but the stream: the two masks are the host's for a and for b"""
    from efficient_tts_amd import ops as O
    case = D.LN_STREAM_CASE
    rows, c, p, seed, _ = case
    i, t = _ln_device(rows, c)
    live = _rows(i.rm != 0, c)
    adds = (5, D.WRAP_ADD)
    word = torch.zeros(1, dtype=torch.int32, device=_dev())
    outs = []
    for add in adds:
        O.store_words(word, [add])
        y = Out(rows * c * 4)
        _ln_rows(lib, t, rows, c, p, seed, word, y=y)
        outs.append(y)
    sets = []
    for add, y in zip(adds, outs):
        got = y.f32().view(rows, c)
        _same_set(got == 0, D.ln_keep(case, add=add) == 0, live, f"efts_layernorm_rows word {add}")
        sets.append((got == 0) & live)
    assert not torch.equal(*sets)


@pytest.mark.parametrize("form", D.LN_FORMS)
@pytest.mark.parametrize("case", D.LN_CASES, ids=D.ln_id)
def test_layernorm_bwd_dropout_vs_fp64(lib, case, form):
    """dz, and dgamma, dbeta, dbias, dw, db ACCUMULATED into non-zero buffers, against float64 autograd of the masked forward, with the
    (seed, seed_add) of the forward case: the mask multiplies dy (hence dgamma, dbeta) and the dw term"""
    rows, c, p, seed, add = case
    i, t = _ln_device(rows, c)
    ref = D.ln_backward(case, form)
    word = _word(add)
    acc = {k: Out(v.numel() * 4, v) for k, v in i.init.items() if k in ref}
    dz = Out(rows * c * 4)
    ptr = lambda k: acc[k].ptr if k in acc else None                                   # noqa: E731
    dy = form == "dy"
    _call("efts_layernorm_bwd", lib.efts_layernorm_bwd(
        t["x"].data_ptr(), t["gamma"].data_ptr(), t["beta"].data_ptr(), D.LN_EPS, t["dy"].data_ptr() if dy else None, None if dy else t["ddur"].data_ptr(),
        None if dy else t["w"].data_ptr(), None if form == "ddur" else t["rm"].data_ptr(), dz.ptr, None, 0, 1, ptr("dgamma"), ptr("dbeta"), ptr("dbias"),
        ptr("dw"), ptr("db"), rows, c, p, seed, None if word is None else word.data_ptr(), _st()))
    name = f"{form} {D.ln_id(case)}"
    got = dz.f32().view(rows, c)
    _check("efts_layernorm_bwd.drop.dz", name, got, *ref["dz"])
    assert bool((got[i.rm == 0] == 0).all())
    for k in acc:
        _check(f"efts_layernorm_bwd.drop.{k}", name, acc[k].f32(), *ref[k])


# ---------------------------------------------------------------------------------------------------------------------
# efts_act_apply / efts_act_grad
# ---------------------------------------------------------------------------------------------------------------------
def _act_apply(lib, act, z, resid, rm, rows, c, p, seed):
    y = Out(rows * c * 4)
    _call("efts_act_apply", lib.efts_act_apply(z.data_ptr(), None if resid is None else resid.data_ptr(), None if rm is None else rm.data_ptr(), *act, y.ptr,
                                               None, 0, 1, rows, c, p, seed, _st()))
    return y.f32().view(rows, c)


def _act_grad(lib, act, up, z, rm, db0, rows, c, p, seed):
    dz, db = Out(rows * c * 4), Out(c * 4, db0)
    _call("efts_act_grad", lib.efts_act_grad(up.data_ptr(), z.data_ptr(), None if rm is None else rm.data_ptr(), *act, dz.ptr, None, 0, 1, db.ptr, rows, c,
                                             p, seed, _st()))
    return dz.f32().view(rows, c), db.f32()


def _apply_dropped(y, i, use_resid, use_mask):
    """an element is dropped iff the output is resid * rowmask bit for bit (without a residual: f(z) * 0 = +-0, compared as a value)"""
    if not use_resid:
        return y == 0
    base = i.resid * i.rm[:, None] if use_mask else i.resid
    return _bits(y).view(y.shape) == _bits(base).view(y.shape)


@pytest.mark.parametrize("case", D.act_cases(), ids=D.act_case_id)
def test_act_apply_and_grad_dropout_vs_host_mask(lib, case):
    from efficient_tts_amd import lib as L
    name, params, rows, c, p, seed = case
    act = L.actfn(name, params)
    i, keep, dev = D.act_inputs(rows, c), D.act_keep(case), _dev()
    z, up, resid, rm = i.z.to(dev), i.up.to(dev), i.resid.to(dev), i.rm.to(dev)
    cid = D.act_case_id(case)
    for use_mask in (False, True):
        live = _rows(i.rm != 0, c) if use_mask else torch.ones(rows, c, dtype=torch.bool)
        for use_resid in (False, True):
            tag = f"{cid} resid={int(use_resid)} mask={int(use_mask)}"
            ref = D.act_reference(case, use_resid, use_mask)
            y = _act_apply(lib, act, z, resid if use_resid else None, rm if use_mask else None, rows, c, p, seed)
            _same_set(_apply_dropped(y, i, use_resid, use_mask), keep == 0, live, f"efts_act_apply {tag}")
            assert bool((y[~live] == 0).all())
            _check("efts_act_apply.drop", tag, y, *ref["y"])
        dz, db = _act_grad(lib, act, up, z, rm if use_mask else None, i.db0, rows, c, p, seed)
        tag = f"{cid} mask={int(use_mask)}"
        _same_set(dz == 0, keep == 0, live, f"efts_act_grad {tag}")                   # exactly 0 on the dropped set, non-zero elsewhere on live rows
        assert bool((dz[~live] == 0).all())
        _check("efts_act_grad.drop.dz", tag, dz, *ref["dz"])
        _check("efts_act_grad.drop.dbias", tag, db, *ref["dbias"])


# ---------------------------------------------------------------------------------------------------------------------
# the pairs the engine uses: the exact zeros of the backward are the forward's dropped set (apart from dead rows)
# ---------------------------------------------------------------------------------------------------------------------
def _gemm_forward_for_pair(lib, sign):
    d = D.GEMM_PAIR_CASE
    c, r = d.case, D.gemm_reference(d)
    assert (c.m + 127) // 128 == 2 and c.n // 128 == 2 and d.sign
    ops = _device_operands(c, _dev())
    f, _, s = _gemm_run(lib, c, ops, G.AUTO, (d.p, d.seed), sign)
    a, _, _ = _gemm_run(lib, d.plain, ops, G.AUTO)
    return d, r, f, s, _gemm_dropped(d, r, f, a, d.seed, f"{d.name} forward")


def _act_bwd_dropout(lib, d, r, mode, y, x):
    c, dev = d.case, _dev()
    g = T._away((c.m, c.n), torch.Generator().manual_seed(c.m * c.n + mode))
    gd, yd, xd, rmd = g.to(dev), y.contiguous().to(dev), None if x is None else x.contiguous().to(dev), r.mask.contiguous().to(dev)
    dz = Out(c.m * c.n * 4)
    _call("efts_act_bwd_dropout", lib.efts_act_bwd_dropout(gd.data_ptr(), yd.data_ptr(), None if xd is None else xd.data_ptr(), rmd.data_ptr(), c.slope, mode,
                                                           dz.ptr, None, 0, 1, None, c.m, c.n, d.p, d.seed, _st()))
    return g, dz.f32().view(c.m, c.n)


@pytest.mark.parametrize("mode", [1, 4])
def test_pair_gemm_and_act_bwd_dropout(lib, mode):
    """mode 1: the sign from y - x of the forward's own output and residual; mode 4: from the forward launch's own sign words"""
    d, r, f, s, dropped = _gemm_forward_for_pair(lib, sign=mode == 4)
    live = _rows(r.mask != 0, d.case.n)
    g, dz = _act_bwd_dropout(lib, d, r, mode, f if mode == 1 else s, r.resid if mode == 1 else None)
    _same_set(dz == 0, dropped, live, f"efts_act_bwd_dropout mode {mode} after {d.name}")
    assert bool((dz[~live] == 0).all())
    if mode == 1:                                                                     # (and every value: the host transcription, bit for bit)
        want = T.act_bwd_ref(g, f, r.resid.contiguous(), r.mask, d.case.slope, 1, (d.p, d.seed)).dz
        assert torch.equal(_bits(dz), _bits(want))


def test_pair_act_apply_and_act_grad(lib):
    from efficient_tts_amd import lib as L
    case = next(k for k in D.act_cases() if (k[2], k[3]) == D.ACT_PAIR_SHAPE and k[0] == "SiLU")
    name, params, rows, c, p, seed = case
    act = L.actfn(name, params)
    i, dev = D.act_inputs(rows, c), _dev()
    z, up, resid, rm = i.z.to(dev), i.up.to(dev), i.resid.to(dev), i.rm.to(dev)
    live = _rows(i.rm != 0, c)
    y = _act_apply(lib, act, z, resid, rm, rows, c, p, seed)
    dropped = _apply_dropped(y, i, True, True) & live
    assert bool(dropped.any()) and bool((~dropped & live).any())
    dz, _ = _act_grad(lib, act, up, z, rm, i.db0, rows, c, p, seed)
    _same_set(dz == 0, dropped, live, "efts_act_grad after efts_act_apply")
    assert bool((dz[~live] == 0).all())


def test_pair_layernorm_rows_and_layernorm_bwd(lib):
    """One row of dy at a time into zeroed dgamma / dbeta: one addend per column, so dbeta is dy[row] * mask[row] * rowmask[row] exactly, and its
    zeros are the dropped set of that row of the forward launch, which ran with the same (seed, seed_add)"""
    case = D.LN_PAIR_CASE
    rows, c, p, seed, add = case
    assert rows > 8 and add is not None
    i, t = _ln_device(rows, c)
    word = _word(add)
    y = Out(rows * c * 4)
    _ln_rows(lib, t, rows, c, p, seed, word, y=y)
    fwd = y.f32().view(rows, c)
    keep = D.ln_keep(case)
    for row in range(rows):
        dy = torch.zeros(rows, c)
        dy[row] = i.dy[row]
        dyd = dy.to(_dev())
        dg, db, dz = Out(c * 4, torch.zeros(c)), Out(c * 4, torch.zeros(c)), Out(rows * c * 4)
        _call("efts_layernorm_bwd", lib.efts_layernorm_bwd(t["x"].data_ptr(), t["gamma"].data_ptr(), t["beta"].data_ptr(), D.LN_EPS, dyd.data_ptr(), None, None,
                                                           t["rm"].data_ptr(), dz.ptr, None, 0, 1, dg.ptr, db.ptr, None, None, None, rows, c, p, seed,
                                                           word.data_ptr(), _st()))
        got = db.f32()
        if float(i.rm[row]) == 0:
            assert bool((got == 0).all()) and bool((fwd[row] == 0).all())
            continue
        assert torch.equal(got == 0, fwd[row] == 0), f"row {row}: the backward's mask is not the forward's"
        assert torch.equal(got, i.dy[row] * keep[row])
        dz.bytes()
