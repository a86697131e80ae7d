"""GPU: efts_gemm per tiling against float64 of its own operands, and the forward packers against the host encoders.

The contraction (test_gemm_case, one id per case of gemm_reference.CASES).  The operand planes are encoded on the HOST (gemm_reference) and
copied in, so the pack kernels are no part of it, and the reference is computed from the decoded planes -- the exact numbers the kernel
multiplies -- so operand rounding is no part of the error: a bf16 launch is held to the bound of an fp32 sum, not to 2e-2.  Every output
lies inside a buffer pre-filled with a canary byte (0x7f: 3.39e38 as fp32) and is compared bit for bit outside rows [0, m) x columns [0, n).
Per case, every explicit tiling and AUTO runs:
  * a tiling gemm_reference.accepts allows: kernel_check._check (max(8 * e32, 2e-6) of max |ref|) and, per element, the a-priori bound
    n_terms * 2^-24 * sum |a||b| + one ulp per epilogue step; the plane bytes = the host encoding of the kernel's own fp32 result (of its
    LeakyReLU with plane_act), byte for byte; a plane written alone is decoded and checked like the fp32 result, plus its resolution;
  * GENERIC, WIDE, NARROW, RESIDENT and AUTO agree bit for bit (the small-M tiling sums in another order: float64 only);
  * a tiling `accepts` rejects raises ValueError and writes nothing.
BOUND_ONLY names the cases held to the a-priori bound alone (see there).

The packers (section 2): efts_pack_rows and efts_pack_weight byte for byte against the encoders; the weight-norm fold against float64.
"""
import ctypes as C
import hashlib
import json
import os

import pytest
import torch

import gemm_reference as R
from kernel_check import _call, _check, _dev, _rel, _st, load_lib, unpack_plane

pytestmark = pytest.mark.gpu

# Cases whose error against float64 exceeds max(8 * e32, 2e-6) although every tiling meets the a-priori bound on every element and the ring
# tilings agree bit for bit: a finding about the statistical bound (the MFMA accumulates in another order and precision than the CPU's
# float32 matmul), not about a kernel.  They assert the a-priori bound alone; their RATIO lines are still printed.
BOUND_ONLY = frozenset()

CANARY32 = int.from_bytes(bytes([R.CANARY] * 4), "little")


@pytest.fixture(scope="module")
def lib():
    return load_lib()


class _Outputs:
    """canary-filled outputs of one launch: fp32 [batch2][batch][8 + m + 8][ldo] (behind out_off floats), planes [batch][8 + m + 8][ldob]"""

    def __init__(self, c, dev):
        self.c = c
        g = R.OUT_GUARD
        self.rows = c.m + 2 * g
        nb = c.batch2 * c.batch
        self.f = torch.full((c.out_off + nb * self.rows * c.ldo_,), CANARY32, dtype=torch.int32, device=dev) if c.has_f32 else None
        self.p = torch.full((c.batch, self.rows, c.ldob), R.CANARY, dtype=torch.uint8, device=dev) if c.has_plane else None
        self.l = torch.full((c.batch, self.rows, c.ldob), R.CANARY, dtype=torch.uint8, device=dev) if c.lo else None

    def f_ptr(self):
        return self.f.data_ptr() + 4 * (self.c.out_off + R.OUT_GUARD * self.c.ldo_)

    def plane_ptr(self, t):
        return t.data_ptr() + R.OUT_GUARD * self.c.ldob

    def collect(self):
        """(fp32 [batch2][batch][m][n] or None, plane bytes [batch][m][ldob] or None, lo plane bytes or None), after asserting that every
        canary outside them is intact: rows outside [0, m), fp32 columns n .. ldo - 1, plane bytes past the row's padding, every batch item"""
        c, g = self.c, R.OUT_GUARD
        f = p = lo = None
        if self.f is not None:
            raw = self.f.cpu()
            assert bool((raw[:c.out_off] == CANARY32).all())
            v = raw[c.out_off:].view(c.batch2, c.batch, self.rows, c.ldo_)
            f = v[:, :, g:g + c.m, :c.n].clone().view(torch.float32)
            rest = v.clone()
            rest[:, :, g:g + c.m, :c.n] = CANARY32
            assert bool((rest == CANARY32).all()), f"{c.name}: fp32 canary overwritten outside rows [0, m) x columns [0, n)"
        rb = R.row_bytes(c.n, c.osplit) if c.has_plane else 0
        out = []
        for t in (self.p, self.l):
            if t is None:
                out.append(None)
                continue
            raw = t.cpu()
            rest = raw.clone()
            rest[:, g:g + c.m, :rb] = R.CANARY
            assert bool((rest == R.CANARY).all()), f"{c.name}: plane canary overwritten outside rows [0, m) or past the row's padding"
            out.append(raw[:, g:g + c.m].clone())
        p, lo = out
        return f, p, lo

    def untouched(self):
        return all(bool((t.cpu() == (CANARY32 if t.dtype == torch.int32 else R.CANARY)).all()) for t in (self.f, self.p, self.l) if t is not None)


def _device_operands(c, dev):
    op = R.operands(c)
    return dict(a=op.a.to(dev), b=op.b.to(dev), bias=op.bias.to(dev), resid=op.resid[:, :, :max(c.ldr, 1)].contiguous().to(dev),
                mask=op.mask.to(dev))


def _launch(lib, c, d, o, tiling, extra=None):
    from efficient_tts_amd import lib as L
    g = L.GemmArgs()
    ra = R.A_GUARD_LO + c.m + R.A_GUARD_HI
    g.a, g.lda = d["a"].data_ptr() + R.A_GUARD_LO * c.lda, c.lda
    g.b, g.ldb, g.b_tap_stride = d["b"].data_ptr(), c.ldb, c.n * c.ldb
    if c.batch > 1:
        g.a_batch_stride, g.b_batch_stride = ra * c.lda, (c.taps * c.n + 1) * c.ldb
    if c.batch2 > 1:
        g.batch2 = c.batch2
        g.a_batch2_stride, g.b_batch2_stride = c.batch * ra * c.lda, c.batch * (c.taps * c.n + 1) * c.ldb
        g.out_batch2_stride = c.batch * o.rows * c.ldo_
    g.split, g.taps, g.m, g.n, g.nchunk, g.batch = c.split, c.taps, c.m, c.n, c.nchunk, c.batch
    g.alpha, g.act, g.slope, g.dilation = c.alpha, c.act, c.slope, c.dil
    g.bias = d["bias"].data_ptr() if c.bias else None
    if c.resid:
        g.resid, g.ldr, g.resid_batch_stride = d["resid"].data_ptr(), c.ldr, (c.m + 2) * c.ldr
    if c.mask:
        g.rowmask, g.rowmask_batch_stride = d["mask"].data_ptr(), c.m + 3
    if c.has_f32:
        g.out_f32, g.ldo, g.out_batch_stride = o.f_ptr(), c.ldo_, o.rows * c.ldo_
    if c.has_plane:
        g.out_bf16, g.ldob, g.outb_batch_stride, g.out_split = o.plane_ptr(o.p), c.ldob, o.rows * c.ldob, c.osplit
        g.plane_act, g.plane_slope = int(c.plane_act), c.plane_slope
    if c.lo:
        g.out_bf16_lo = o.plane_ptr(o.l)
    g.tiling = tiling
    if extra is not None:
        extra(g)
    _call("efts_gemm", lib.efts_gemm(C.byref(g), _st()))


def _stat(kernel, name, got, ref64, ref32, extra, bound_only):
    """kernel_check._check -- or, for a BOUND_ONLY case, its RATIO line alone"""
    if not bound_only:
        _check(kernel, name, got, ref64, ref32, extra=extra)
        return
    e32, err = _rel(ref32.double(), ref64), _rel(got.double(), ref64)
    print(f"RATIO {kernel} {name} err={err:.3e} e32={e32:.3e} ratio={err / e32 if e32 > 0 else float('inf'):.2f} (a-priori bound only)")


def _plane_values(p, c):
    """plane bytes [batch][m][ldob] -> fp32 [1][batch][m][n]"""
    return unpack_plane(p.reshape(c.batch * c.m, c.ldob), c.batch, c.m, c.m, R.kp_of(c.n, c.osplit), c.osplit)[None, :, :, :c.n]


def _check_plane_bytes(c, p, values, what):
    """the bytes of elements < n equal the host encoding of `values` [batch][m][n]; the row's padding holds zero or the canary"""
    elem = R.element_bytes(c.n, c.osplit, c.ldob)
    rb = R.row_bytes(c.n, c.osplit)
    want = R.encode_rows(values.reshape(c.batch * c.m, c.n), c.osplit, c.ldob).view(c.batch, c.m, c.ldob)
    assert torch.equal(p[:, :, elem], want[:, :, elem]), f"{c.name}: {what} is not the host encoding of the kernel's own fp32 result"
    padding = p[:, :, :rb][:, :, ~elem[:rb]].reshape(-1).view(torch.int16)
    assert bool(((padding == 0) | (padding == 0x7F7F)).all()), f"{c.name}: {what}: padding columns hold neither zero nor the canary"


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_gemm_case(lib, case):
    c = case
    dev = _dev()
    d = _device_operands(c, dev)
    ref64, ref32, bound = R.reference(c)
    pref64, pref32, pbound = R.reference(c, True) if c.has_plane else (None, None, None)
    scale = float(ref64.abs().max())
    extra = R.TANH_ABS / scale if c.act == R.ACT_TANH else 0.0
    bound_only = c.name in BOUND_ONLY
    got = {}
    for tiling in R.EXPLICIT + (R.AUTO,):
        o = _Outputs(c, dev)
        tag = f"efts_gemm[{R.TILING_NAME[tiling]}]"
        if not R.accepts(c, tiling):
            with pytest.raises(ValueError):              # an explicit tiling the shape does not allow is an error, never a fallback
                _launch(lib, c, d, o, tiling)
            torch.cuda.synchronize()
            assert o.untouched(), f"{c.name}: the refused {tag} wrote to an output"
            continue
        _launch(lib, c, d, o, tiling)
        torch.cuda.synchronize()
        f, p, lo = o.collect()
        got[tiling] = (f, p, lo)
        if f is not None:
            _stat(tag, c.name, f, ref64, ref32, extra, bound_only)
            assert bool(((f.double() - ref64).abs() <= bound).all()), f"{c.name} {tag}: an element misses the a-priori bound"
        if p is not None and f is not None:              # the plane is the host encoding of the kernel's own fp32 result
            v = f[0]
            if c.plane_act:
                v = torch.where(v > 0, v, v * torch.tensor(c.plane_slope, dtype=torch.float32))
            _check_plane_bytes(c, p, v, "the plane")
            if lo is not None:                           # the bf16 remainder out - bf16(out), as a format-1 plane
                _check_plane_bytes(c, lo, v - v.bfloat16().float(), "the remainder plane")
        elif p is not None:                              # plane alone: decode it
            pv = _plane_values(p, c)
            res = R.storage_resolution(c.osplit)
            _stat(tag + ".plane", c.name, pv, pref64, pref32, extra + res, bound_only)
            assert bool(((pv.double() - pref64).abs() <= pbound + res * pref64.abs()).all()), f"{c.name} {tag}: a plane element misses the a-priori bound"
            padding = p[:, :, :R.row_bytes(c.n, c.osplit)][:, :, ~R.element_bytes(c.n, c.osplit, c.ldob)[:R.row_bytes(c.n, c.osplit)]]
            assert bool(((padding == 0) | (padding == R.CANARY)).all())
    assert all(t in got for t in c.tilings) and R.AUTO in got
    ring = [t for t in R.RING + (R.AUTO,) if t in got]
    for t in ring[1:]:                                   # the header's promise: the ring kernels and AUTO are bit-identical
        for x, y, what in zip(got[ring[0]], got[t], ("fp32 stream", "plane bytes", "remainder plane bytes")):
            assert (x is None and y is None) or torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                                            y.view(torch.int32) if y.dtype == torch.float32 else y), \
                f"{c.name}: {what} of {R.TILING_NAME[t]} differ from {R.TILING_NAME[ring[0]]}"


# ------------------------------------------------------------------------------------------------------------ 1b. the recorded bits
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_digests.json")


def _sha(*buffers):
    h = hashlib.sha256()
    for t in buffers:
        h.update(b"-" if t is None else t.cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:32]


def _extras(dev):
    """launches of the epilogue features that no case of gemm_reference.CASES carries (sign words + dropout, soft index, squared-error
    parts): (case, tilings, make), make() -> (canary-filled side outputs, hook that points the launch's arguments at them)"""
    G, W, A = R.GENERIC, R.WIDE, R.AUTO
    out = []
    for sp in (1, 2):
        c = R.Case(name=f"x-sign-drop-split{sp}", tilings=(G, W), split=sp, taps=5, m=362, n=128, K=R.chunk_k(sp), bias=True, act=R.ACT_LEAKY,
                   resid=True, mask=True, out="both")

        def make(c=c):
            sign = torch.full((c.m + 2 * R.OUT_GUARD, c.n // 8), R.CANARY, dtype=torch.uint8, device=dev)

            def hook(g):
                g.sign_mask, g.drop_p, g.drop_seed = sign.data_ptr() + R.OUT_GUARD * (c.n // 8), 0.25, 1234
            return [sign], hook
        out.append((c, (G, W, A), make))
    c = R.Case(name="x-soft-index", tilings=(G,), m=130, n=96, K=64, batch=2, alpha=0.125)

    def make(c=c):
        sidx = torch.full((c.batch * c.m + 8,), CANARY32, dtype=torch.int32, device=dev)
        kl, ql = (torch.tensor(v, dtype=torch.int32, device=dev) for v in ([96, 57], [130, 77]))

        def hook(g):
            g.soft_index, g.key_len, g.query_len = sidx.data_ptr(), kl.data_ptr(), ql.data_ptr()
        return [sidx], hook
    out.append((c, (G, A), make))
    c = R.Case(name="x-sqerr", tilings=(G,), m=130, n=96, K=64, batch=2, bias=True, mask=True)

    def make(c=c):
        target = torch.randn(c.batch, c.m, c.n, generator=torch.Generator().manual_seed(7)).to(dev)
        part = torch.full((c.batch * 2 * 4 + 4,), CANARY32, dtype=torch.int32, device=dev)       # [batch][2 tiles][4 waves]

        def hook(g):
            g.sqerr_target, g.ld_target, g.target_batch_stride, g.sqerr_part = target.data_ptr(), c.n, c.m * c.n, part.data_ptr()
        return [part], hook
    out.append((c, (G, A), make))
    return out


def gemm_digests(lib):
    """{"<case>/<tiling>": sha256 of the raw output buffers of that launch, canary rows and padding included}: every case of
    gemm_reference.CASES and of _extras on every tiling that accepts it and on AUTO"""
    dev = _dev()
    out = {}

    def run(c, tilings, make=lambda: ([], None)):
        d = _device_operands(c, dev)
        for tiling in tilings:
            if not R.accepts(c, tiling):
                continue
            o = _Outputs(c, dev)
            side, hook = make()
            _launch(lib, c, d, o, tiling, hook)
            torch.cuda.synchronize()
            out[f"{c.name}/{R.TILING_NAME[tiling]}"] = _sha(o.f, o.p, o.l, *side)

    for c in R.CASES:
        run(c, R.EXPLICIT + (R.AUTO,))
    for c, tilings, make in _extras(dev):
        run(c, tilings, make)
    return out


def test_gemm_bits_equal_the_recorded_launches(lib):
    """Every launch writes, bit for bit, what the commit named in tests/golden/gemm_digests.json wrote (tests/record_gemm_digests.py, run
    against a library built from that commit, records the file): a change of the kernels that is meant to keep their results keeps these."""
    with open(DIGESTS) as f:
        want = json.load(f)["digests"]
    got = gemm_digests(lib)
    assert sorted(got) == sorted(want), "the (case, tiling) launches differ from the recorded set"
    bad = sorted(k for k in got if got[k] != want[k])
    assert not bad, f"{len(bad)} of {len(got)} launches differ from the recorded bits: {bad[:12]}"


# ------------------------------------------------------------------------------------------------------------ 2. the forward packers
@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("B,T,c", [(2, 37, 80), (1, 130, 512), (3, 5, 24)])
def test_pack_rows_bytes_equal_the_host_encoder(lib, split, B, T, c):
    """device plane bytes = host encoder's, byte for byte, zero gap rows and zero K padding included; nothing outside the rows or past the
    K padding is written; the fp32 side output is the input (zero in the gap rows)"""
    dev = _dev()
    x = torch.randn(B, T, c, generator=torch.Generator().manual_seed(B * 1000 + T * 10 + split))
    Tp, g = T + 2, 3
    rows = B * Tp
    rb = R.row_bytes(c, split)
    ld = rb + 16
    xs = torch.zeros(B, Tp, c)
    xs[:, :T] = x
    want = torch.full((rows + 2 * g, ld), R.CANARY, dtype=torch.uint8)
    want[g:g + rows] = R.encode_rows(xs.view(rows, c), split, ld, fill=R.CANARY)
    pl = torch.full((rows + 2 * g, ld), R.CANARY, dtype=torch.uint8, device=dev)
    f = torch.full(((rows + 2 * g) * c,), CANARY32, dtype=torch.int32, device=dev)
    xd = x.to(dev)
    _call("efts_pack_rows", lib.efts_pack_rows(xd.data_ptr(), f.data_ptr() + 4 * g * c, pl.data_ptr() + g * ld, ld, B, T, Tp, c,
                                               R.kp_of(c, split), split, _st()))
    torch.cuda.synchronize()
    assert torch.equal(pl.cpu(), want)
    fw = torch.full((rows + 2 * g, c), CANARY32, dtype=torch.int32)
    fw[g:g + rows] = xs.view(rows, c).view(torch.int32)
    assert torch.equal(f.cpu().view(rows + 2 * g, c), fw)


@pytest.mark.parametrize("split", [1, 2, 3])
@pytest.mark.parametrize("taps", [1, 5])
@pytest.mark.parametrize("cout,cin", [(80, 512), (512, 80), (24, 130)])
def test_pack_weight_bytes_and_weight_norm(lib, split, taps, cout, cin):
    """g = None: plane bytes = host encoder's.  With a weight-norm gain: the decoded plane and w_f32_out against float64 g * v / ||v||"""
    dev = _dev()
    gen = torch.Generator().manual_seed(cout * 7 + cin + taps * 100 + split)
    w = torch.randn(cout, cin, taps, generator=gen) / (cin * taps) ** 0.5
    gain = torch.rand(cout, generator=gen) + 0.5
    ld = R.row_bytes(cin, split) + 16
    wd = w.to(dev)

    def pack(g, wout):
        pl = torch.full((taps * cout + 1, ld), R.CANARY, dtype=torch.uint8, device=dev)
        _call("efts_pack_weight", lib.efts_pack_weight(wd.data_ptr(), None if g is None else g.data_ptr(), None if wout is None else wout.data_ptr(),
                                                       pl.data_ptr(), ld, cout, cin, taps, split, _st()))
        torch.cuda.synchronize()
        raw = pl.cpu()
        assert bool((raw[taps * cout:] == R.CANARY).all())
        return raw[:taps * cout]

    assert torch.equal(pack(None, None), R.encode_weight(w, split, ld, fill=R.CANARY).view(taps * cout, ld))
    wout = torch.full((cout * cin * taps + 4,), CANARY32, dtype=torch.int32, device=dev)
    raw = pack(gain.to(dev), wout)
    assert bool((raw[:, R.row_bytes(cin, split):] == R.CANARY).all())
    norm = lambda v, dt: gain.to(dt)[:, None, None] * v.to(dt) / v.to(dt).pow(2).sum((1, 2), keepdim=True).sqrt()
    ref64, ref32 = norm(w, torch.float64), norm(w, torch.float32)
    dec = R.decode_weight(raw.view(taps, cout, ld), cin, split)
    assert float(dec[:, :, cin:].abs().max() if dec.shape[2] > cin else 0.0) == 0.0
    name = f"{cout}x{cin}x{taps}-split{split}"
    _check("efts_pack_weight.plane", name, dec[:, :, :cin].permute(1, 2, 0), ref64, ref32, extra=R.storage_resolution(split))
    wo = wout.cpu()
    assert bool((wo[cout * cin * taps:] == CANARY32).all())
    _check("efts_pack_weight.w_f32_out", name, wo[:cout * cin * taps].view(torch.float32).view(cout, cin, taps), ref64, ref32)
