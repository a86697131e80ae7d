"""GPU (-m gpu): efts_resconv5 -- one residual k5 convolution layer on hi/lo planes, ResConv1d.forward of the reference
(nntts/layers/efts_modules.py:48-51) -- against efts_gemm (bit-exact: same per-element summation order) and against an
fp64 restatement of the layer; every tile height, multi-tile schedules, ragged row counts, both operand formats and all
input / output stream formats."""
import pytest
import torch

pytestmark = pytest.mark.gpu
C = 512


@pytest.fixture(autouse=True, params=["8-wave", "one-wave-per-SIMD"])
def rc_kernel(request):
    """every case of this file runs on both kernels of efts_resconv5 (include/efts_abi.h efts_resconv5_args.kernel): the 8-wave ping-pong
    kernel (the default) and the one-wave-per-SIMD kernel with the generated main loop (csrc/efts_resconv4.h), which takes over where it
    applies (bf16 planes, 5 taps) -- same tiles, plans and, bit for bit, the same results"""
    from efficient_tts_amd import ops as P
    prev, P.RC_KERNEL = P.RC_KERNEL, (0 if request.param == "8-wave" else 2)
    yield request.param
    P.RC_KERNEL = prev


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def bf16_split(x):
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


class Case:
    """x (exactly representable as hi + lo), weights, bias, gap mask of a B x T row space, and the efts_gemm result.
    width: channels of the layer (n = cout; a multiple of 256).  cin: input channels where they differ from the width (K != n): the
    fp32 residual stream `xf` is then an independent [rows, width] stream, since the operand planes do not hold n columns"""

    def __init__(self, B, T, split, seed=0, width=512, cin=None):
        from efficient_tts_amd import lib as L, ops as P
        L.load(); L.require_device()
        self.L, self.P, self.split = L, P, split
        C = self.C = width
        K = self.K = width if cin is None else cin
        dev = _dev()
        torch.manual_seed(seed + 1000 * B + T)
        self.rs = rs = P.Rows(B, T)
        x = torch.randn(B, T, K, device=dev)
        hi, lo = bf16_split(x)
        x16 = hi.float() + lo.float()
        hi, lo = bf16_split(x16)                      # bf16(x16) may differ from bf16(x) at rounding ties
        self.x16 = x16
        self.a = P.Plane.for_rows(rs, K, split, dev)
        P.pack_rows(x16, None, self.a, rs)
        self.a_lo = None
        if split == 1:
            self.a_lo = P.Plane.for_rows(rs, K, 1, dev)
            P.pack_rows(lo.float().contiguous(), None, self.a_lo, rs)
        self.xf = P.F32Rows(rs, C, dev); self.xf.view().copy_(x16 if K == C else torch.randn(B, T, C, device=dev))
        self.w = (torch.randn(C, K, 5, device=dev) * 0.02).contiguous()
        self.pw = P.PackedWeight(C, K, 5, split, dev); self.pw.pack(self.w)
        self.bias = torch.randn(C, device=dev)
        lens = torch.randint(max(1, T // 2), T + 1, (B,), dtype=torch.int32, device=dev)
        self.mask = torch.zeros(rs.rows, device=dev)
        P.row_masks(lens, rs, None, self.mask)        # a LENGTH mask: rows past an item's length are zeroed too
        self.o_ref, self.p_ref = P.F32Rows(rs, C, dev), P.Plane.for_rows(rs, C, 2, dev)
        P.gemm(a=self.a, b_ptr=self.pw.ptr, ldb=self.pw.ld, b_tap_stride=self.pw.tap_stride, taps=5, m=rs.rows, n=C,
               act=L.ACT_LEAKY, slope=0.1, bias=self.bias, resid_ptr=self.xf.ptr, ldr=C, rowmask_ptr=self.mask.data_ptr(),
               out_f32_ptr=self.o_ref.ptr, ldo=C, out_plane=self.p_ref)
        torch.cuda.synchronize()

    def run(self, mode, plan=None):
        P, rs, dev, C = self.P, self.rs, _dev(), self.C
        o = P.F32Rows(rs, C, dev)
        if mode == "f32":          # fp32 residual in, fp32 + split-2 plane out
            y, yl = P.Plane.for_rows(rs, C, 2, dev), None
            P.resconv5(x=self.a, x_f32_ptr=self.xf.ptr, ldr=C, w=self.pw, m=rs.rows, n=C, bias=self.bias,
                       rowmask_ptr=self.mask.data_ptr(), y_f32_ptr=o.ptr, ldo=C, y=y, plan=plan)
        else:                      # planes in, planes of the same format out (+ fp32 for the comparison)
            y = P.Plane.for_rows(rs, C, self.split, dev)
            yl = P.Plane.for_rows(rs, C, 1, dev) if self.split == 1 else None
            P.resconv5(x=self.a, x_lo=self.a_lo, w=self.pw, m=rs.rows, n=C, bias=self.bias, rowmask_ptr=self.mask.data_ptr(),
                       y_f32_ptr=o.ptr, ldo=C, y=y, y_lo=yl, plan=plan)
        torch.cuda.synchronize()
        return o, y, yl

    def check(self, mode, plan=None):
        o, y, yl = self.run(mode, plan)
        C = self.C
        assert torch.equal(o.buf, self.o_ref.buf), f"fp32 differs: {(o.buf - self.o_ref.buf).abs().max().item():.3e}"
        if mode == "f32" or self.split == 2:
            assert torch.equal(y.buf, self.p_ref.buf)
        else:
            rh, rl = bf16_split(self.o_ref.buf)
            n = self.rs.alloc
            assert torch.equal(y.buf.view(torch.bfloat16).view(n, -1)[:, :C], rh)
            assert torch.equal(yl.buf.view(torch.bfloat16).view(n, -1)[:, :C], rl)


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("B,T", [(3, 37), (5, 300), (1, 1), (2, 801)])
@pytest.mark.parametrize("mode", ["f32", "planes"])
def test_resconv5_equals_gemm_automatic_schedule(split, B, T, mode):
    Case(B, T, split).check(mode)


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("classes", [[[2]], [[3]], [[4]], [[5]], [[6]], [[7]], [[8]], [[4], [2]], [[6, 2]], [[7, 6], [6, 7]], [[2, 3, 4, 5]],
                                     [[8, 3, 7]], [[8], [6], [4], [2]], [[5], [3], [7]]])
def test_resconv5_every_tile_height_and_multi_tile_schedules(split, classes):
    """explicit plans: every tile height in half units (odd ones split 4+3, 3+2, 2+1 blocks over the two wave rows), tiles of
    different heights in one workgroup (window buffers / ring slots carried across tiles, the next tile's first operands
    requested before the epilogue), 1 .. 4 classes"""
    c = Case(5, 300, split, seed=7)
    plan = c.P.make_plan(c.rs.rows, classes)
    c.check("planes", plan)
    c.check("f32", plan)


def _fp64_layer_error(c):
    """worst |efts_resconv5 - fp64| of one case, planes in / planes out"""
    o, _, _ = c.run("planes")
    rs = c.rs
    x = c.x16.double()                                                       # [B, T, C]
    hi, lo = bf16_split(c.w)
    w = (hi.double() + lo.double())                                          # bf16x3 operands: 16 mantissa bits of w
    conv = torch.nn.functional.conv1d(x.transpose(1, 2), w, c.bias.double(), padding=2).transpose(1, 2)
    y = x + torch.nn.functional.leaky_relu(conv, 0.1)
    y = y * c.mask.view(rs.B, rs.Tp)[:, :rs.T, None].double()
    got = o.view().double()
    return (got - y).abs().max().item()


def test_resconv5_vs_fp64_layer():
    """the layer itself against an fp64 restatement: y = (x + LeakyReLU(conv1d_k5(x_hi) + b)) * mask per item"""
    err = _fp64_layer_error(Case(3, 70, 2, seed=3))
    assert err <= 2e-4, err                                                  # dropped lo*lo term + fp32 accumulation of 2560 products


def test_resconv5_full_size_equals_gemm():
    """BASELINE config 2 row space (64 x 802 rows), both operand formats, the automatic two-class schedule"""
    for split in (1, 2):
        Case(64, 800, split, seed=11).check("planes")


def test_gemm_writes_the_remainder_plane():
    """efts_gemm(out_bf16_lo): hi + lo planes of a split-1 output rebuild the fp32 result to 16 mantissa bits"""
    from efficient_tts_amd import lib as L, ops as P
    c = Case(2, 50, 1, seed=5)
    dev = _dev()
    rs = c.rs
    o, y, yl = P.F32Rows(rs, C, dev), P.Plane.for_rows(rs, C, 1, dev), P.Plane.for_rows(rs, C, 1, dev)
    P.gemm(a=c.a, b_ptr=c.pw.ptr, ldb=c.pw.ld, b_tap_stride=c.pw.tap_stride, taps=5, m=rs.rows, n=C, act=L.ACT_LEAKY, slope=0.1,
           bias=c.bias, resid_ptr=c.xf.ptr, ldr=C, rowmask_ptr=c.mask.data_ptr(), out_f32_ptr=o.ptr, ldo=C, out_plane=y, out_plane_lo=yl)
    torch.cuda.synchronize()
    rh, rl = bf16_split(o.buf)
    assert torch.equal(y.buf.view(torch.bfloat16).view(rs.alloc, -1)[:, :C], rh)
    assert torch.equal(yl.buf.view(torch.bfloat16).view(rs.alloc, -1)[:, :C], rl)


@pytest.mark.parametrize("split", [1, 2])
def test_resconv5_race_screen(split):
    """The ping-pong loop orders its LDS-DMA writes and fragment reads by counted waits and barriers alone; a misplaced one shows
    up as a rare wrong tile, not as a steady failure.  120 launches at the full size (30 240 tiles, 1.2 M (chunk, tap) steps per
    workgroup row), back to back and beside a second stream that keeps the fabric busy with copies, every result compared bit
    for bit with efts_gemm's; then the same under an odd-height multi-tile plan."""
    c = Case(64, 800, split, seed=21)
    P, rs, dev = c.P, c.rs, _dev()
    y = P.Plane.for_rows(rs, C, split, dev)
    yl = P.Plane.for_rows(rs, C, 1, dev) if split == 1 else None
    o = P.F32Rows(rs, C, dev)
    side = torch.cuda.Stream(device=dev)
    junk_a, junk_b = torch.empty(64 << 20, dtype=torch.uint8, device=dev), torch.empty(64 << 20, dtype=torch.uint8, device=dev)
    bad = 0
    for plan in (None, P.make_plan(rs.rows, [[5, 3, 5], [3, 7, 3]])):
        for it in range(60):
            if it % 3 == 0:
                with torch.cuda.stream(side):
                    junk_b.copy_(junk_a)                      # 128 MB of unrelated traffic beside the launch
            o.buf.zero_(); y.buf.zero_()
            P.resconv5(x=c.a, x_lo=c.a_lo, w=c.pw, m=rs.rows, n=C, bias=c.bias, rowmask_ptr=c.mask.data_ptr(), y_f32_ptr=o.ptr, ldo=C,
                       y=y, y_lo=yl, plan=plan)
            bad += int(not torch.equal(o.buf, c.o_ref.buf))
            if split == 2:
                bad += int(not torch.equal(y.buf, c.p_ref.buf))
        torch.cuda.synchronize()
    assert bad == 0, f"{bad} of 120 launches differ from efts_gemm"


def _multi_two_layers(split, shapes, classes, width=512):
    """two Cases of `width` channels in one efts_resconv5_multi launch (the first planes -> planes, the second with the fp32 residual
    stream), each compared with its own efts_gemm launch bit for bit"""
    ca, cb = Case(*shapes[0], split, seed=3, width=width), Case(*shapes[1], split, seed=11, width=width)
    C = width
    P, dev = ca.P, _dev()
    outs, layers = [], []
    for c, mode in ((ca, "planes"), (cb, "f32")):
        o = P.F32Rows(c.rs, C, dev)
        if mode == "f32":
            y, yl = P.Plane.for_rows(c.rs, C, 2, dev), None
            kw = dict(x=c.a, x_f32_ptr=c.xf.ptr, ldr=C, w=c.pw, m=c.rs.rows, n=C, bias=c.bias, rowmask_ptr=c.mask.data_ptr(),
                      y_f32_ptr=o.ptr, ldo=C, y=y)
        else:
            y = P.Plane.for_rows(c.rs, C, split, dev)
            yl = P.Plane.for_rows(c.rs, C, 1, dev) if split == 1 else None
            kw = dict(x=c.a, x_lo=c.a_lo, w=c.pw, m=c.rs.rows, n=C, bias=c.bias, rowmask_ptr=c.mask.data_ptr(), y_f32_ptr=o.ptr, ldo=C,
                      y=y, y_lo=yl)
        layers.append(kw)
        outs.append((c, mode, o, y, yl))
    if classes is not None:
        layers[0]["plan"] = P.make_plan(ca.rs.rows + cb.rs.rows, classes)
    P.resconv5_multi(layers)
    torch.cuda.synchronize()
    for c, mode, o, y, yl in outs:
        assert torch.equal(o.buf, c.o_ref.buf), f"fp32 differs: {(o.buf - c.o_ref.buf).abs().max().item():.3e}"
        if mode == "f32" or split == 2:
            assert torch.equal(y.buf, c.p_ref.buf)
        else:
            rh, rl = bf16_split(c.o_ref.buf)
            n = c.rs.alloc
            assert torch.equal(y.buf.view(torch.bfloat16).view(n, -1)[:, :C], rh)
            assert torch.equal(yl.buf.view(torch.bfloat16).view(n, -1)[:, :C], rl)


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("shapes", [((5, 300), (3, 37)), ((2, 801), (2, 130)), ((3, 37), (5, 300)), ((1, 1), (1, 1)), ((16, 800), (16, 128))])
@pytest.mark.parametrize("classes", [None, [[7, 6], [6, 7]], [[3], [2]], [[8, 2, 5]]])
def test_resconv5_multi_two_layers_in_one_launch(split, shapes, classes):
    """efts_resconv5_multi: two independent layers (own operands, weights, bias, mask, outputs; different row counts) laid end to
    end in ONE persistent launch == each layer through efts_gemm, bit for bit -- for the automatic schedule and explicit ones whose
    tiles get cut at the layer boundary (tile heights change there, the operand streams carried across tiles switch layers)"""
    _multi_two_layers(split, shapes, classes)


class Case3(Case):
    """a k3 layer on the same operands: weights [C][C][3], reference = efts_gemm taps 3 (residual layer, or Conv1d + ReLU without
    the residual term and without a mask: the duration predictor's layer, nntts/layers/duration_predictor.py:57)"""

    def __init__(self, B, T, split, seed=0, plain=False, width=512, cin=None):
        super().__init__(B, T, split, seed, width, cin)
        L, P, rs, dev, C, K = self.L, self.P, self.rs, _dev(), self.C, self.K
        self.plain = plain
        self.w = (torch.randn(C, K, 3, device=dev) * 0.03).contiguous()
        self.pw = P.PackedWeight(C, K, 3, split, dev); self.pw.pack(self.w)
        self.o_ref, self.p_ref = P.F32Rows(rs, C, dev), P.Plane.for_rows(rs, C, 2, dev)
        if plain:
            P.gemm(a=self.a, b_ptr=self.pw.ptr, ldb=self.pw.ld, b_tap_stride=self.pw.tap_stride, taps=3, m=rs.rows, n=C, act=L.ACT_RELU,
                   bias=self.bias, out_f32_ptr=self.o_ref.ptr, ldo=C, out_plane=self.p_ref, tiling=L.TILING_GENERIC)
        else:
            P.gemm(a=self.a, b_ptr=self.pw.ptr, ldb=self.pw.ld, b_tap_stride=self.pw.tap_stride, taps=3, m=rs.rows, n=C, act=L.ACT_LEAKY,
                   slope=0.1, bias=self.bias, resid_ptr=self.xf.ptr, ldr=C, rowmask_ptr=self.mask.data_ptr(), out_f32_ptr=self.o_ref.ptr, ldo=C,
                   out_plane=self.p_ref, tiling=L.TILING_GENERIC)
        torch.cuda.synchronize()

    def kwargs(self, o, y):
        C = self.C
        if self.plain:
            return dict(x=self.a, x_lo=self.a_lo, w=self.pw, m=self.rs.rows, n=C, bias=self.bias, slope=0.0, y_f32_ptr=o.ptr, ldo=C, y=y,
                        taps=3, no_residual=True)
        return dict(x=self.a, x_lo=self.a_lo, w=self.pw, m=self.rs.rows, n=C, bias=self.bias, rowmask_ptr=self.mask.data_ptr(),
                    y_f32_ptr=o.ptr, ldo=C, y=y, taps=3)


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("B,T", [(3, 37), (5, 300), (2, 801), (1, 1)])
@pytest.mark.parametrize("plain", [False, True])
def test_resconv5_k3_layers_equal_gemm(split, B, T, plain):
    """efts_resconv5_args.taps = 3 (a k_size = 3 ResConv1d layer; with no_residual and slope 0 the duration predictor's Conv1d + ReLU)
    == efts_gemm taps 3 on the same operands, bit for bit"""
    c = Case3(B, T, split, seed=5, plain=plain)
    P, dev = c.P, _dev()
    o, y = P.F32Rows(c.rs, C, dev), P.Plane.for_rows(c.rs, C, 2, dev)
    P.resconv5(**c.kwargs(o, y))
    torch.cuda.synchronize()
    live = slice(c.L.GUARD_LO, c.L.GUARD_LO + c.rs.rows)
    assert torch.equal(o.buf[live], c.o_ref.buf[live]), f"fp32 differs: {(o.buf - c.o_ref.buf).abs().max().item():.3e}"
    assert torch.equal(y.buf[live].view(torch.bfloat16), c.p_ref.buf[live].view(torch.bfloat16))


@pytest.mark.parametrize("split", [1, 2])
def test_resconv5_multi_k5_layer_with_a_k3_rider(split):
    """a decoder-like k5 residual layer and the duration predictor's k3 Conv1d + ReLU (no residual, no mask, fp32 output) in one
    grouped launch: each equals its own efts_gemm launch bit for bit"""
    ca, cb = Case(16, 800, split, seed=3), Case3(16, 128, split, seed=11, plain=True)
    P, dev = ca.P, _dev()
    oa, ya = P.F32Rows(ca.rs, C, dev), P.Plane.for_rows(ca.rs, C, 2, dev)
    ob, yb = P.F32Rows(cb.rs, C, dev), P.Plane.for_rows(cb.rs, C, 2, dev)
    ka = dict(x=ca.a, x_lo=ca.a_lo, w=ca.pw, m=ca.rs.rows, n=C, bias=ca.bias, rowmask_ptr=ca.mask.data_ptr(), y_f32_ptr=oa.ptr, ldo=C, y=ya)
    P.resconv5_multi([ka, cb.kwargs(ob, yb)])
    torch.cuda.synchronize()
    assert torch.equal(oa.buf, ca.o_ref.buf)
    live = slice(cb.L.GUARD_LO, cb.L.GUARD_LO + cb.rs.rows)
    assert torch.equal(ob.buf[live], cb.o_ref.buf[live])
    assert torch.equal(yb.buf[live].view(torch.bfloat16), cb.p_ref.buf[live].view(torch.bfloat16))


# =====================================================================================================================
# Off the 512-channel width.  What runs where:
#   width   column tiles (ntn = n / 256)   K chunks, bf16 / bf16x3   tile-to-tile window parity (c.wpar += nchunk)
#   256     1                              4 / 8                     never flips
#   512     2 (everything above)           8 / 16                    never flips
#   768     3 (85 slots of 256 CUs + 1)    12 / 24                   never flips
#   1024    4                              16 / 32                   never flips
#   256 <- cin 64 / 192 / 320              1, 3, 5 / 2, 6, 10        flips with every tile in bf16 (odd), never in bf16x3
# kernel = 2 (the "one-wave-per-SIMD" half of the autouse fixture) runs the generated main loop for bf16 planes with 5 taps and at least
# two K chunks; every bf16x3 case, every 3-tap case and cin = 64 in bf16 (one chunk) run on the 8-wave kernel under both fixture values.
# =====================================================================================================================
WIDTHS = [256, 768, 1024]
SMALL_SHAPES = [(3, 37), (5, 300), (1, 1)]
PLANS = [None, [[2, 3, 2]], [[7, 6], [6, 7]], [[8, 3, 7]]]


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("B,T", SMALL_SHAPES)
@pytest.mark.parametrize("width", WIDTHS)
def test_resconv5_other_widths_equal_gemm(width, B, T, split):
    """square layers of 256 / 768 / 1024 channels (1 / 3 / 4 column tiles; grid = groups * ntn) == efts_gemm bit for bit: both stream
    modes, the automatic schedule and explicit plans with two and three tiles per group (117, 1510 and 3 rows: fewer groups than
    classes at the short ones).  The chunk count is even at every square width, so the window parity never flips here."""
    c = Case(B, T, split, seed=13, width=width)
    for classes in PLANS:
        plan = None if classes is None else c.P.make_plan(c.rs.rows, classes)
        for mode in ("f32", "planes"):
            c.check(mode, plan)
    print(f"width {width} split {split} {B}x{T}: {len(PLANS) * 2} launches bit-equal to efts_gemm")


@pytest.mark.parametrize("width", WIDTHS)
def test_resconv5_other_widths_vs_fp64_layer(width):
    """test_resconv5_vs_fp64_layer at the other widths.  Its 2e-4 stands for the dropped lo*lo term and the fp32 accumulation of
    5 * 512 = 2560 products; both grow with the number of products, so the bound here is 2e-4 * (5 * width / 2560)."""
    err = _fp64_layer_error(Case(3, 70, 2, seed=3, width=width))
    bound = 2e-4 * (5 * width / 2560)
    print(f"width {width}: worst |efts_resconv5 - fp64| {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("width", [256, 768])
@pytest.mark.parametrize("shapes", [((5, 300), (3, 37)), ((3, 37), (5, 300)), ((1, 1), (2, 130))])
@pytest.mark.parametrize("classes", [None, [[7, 6], [6, 7]], [[8, 2, 5]]])
def test_resconv5_multi_other_widths(split, width, shapes, classes):
    """efts_resconv5_multi with two layers of 256 (one column tile) and of 768 channels (three), different row counts, the automatic
    schedule and explicit plans whose tiles are cut at the layer boundary: each layer == its own efts_gemm launch, bit for bit"""
    _multi_two_layers(split, shapes, classes, width=width)
    print(f"width {width} split {split} {shapes}: both layers bit-equal to efts_gemm")


def _kn_reference(c, pw, taps, residual):
    """efts_gemm on the generic tiling for a K != n case: (fp32 rows, split-2 plane)"""
    L, P, rs, C = c.L, c.P, c.rs, c.C
    o, p = P.F32Rows(rs, C, _dev()), P.Plane.for_rows(rs, C, 2, _dev())
    kw = dict(resid_ptr=c.xf.ptr, ldr=C) if residual else {}
    P.gemm(a=c.a, b_ptr=pw.ptr, ldb=pw.ld, b_tap_stride=pw.tap_stride, taps=taps, m=rs.rows, n=C, act=L.ACT_LEAKY, slope=0.1, bias=c.bias,
           rowmask_ptr=c.mask.data_ptr(), out_f32_ptr=o.ptr, ldo=C, out_plane=p, tiling=L.TILING_GENERIC, **kw)
    torch.cuda.synchronize()
    return o, p


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("taps", [5, 3])
@pytest.mark.parametrize("B,T", SMALL_SHAPES)
@pytest.mark.parametrize("cin", [64, 192, 320])
def test_resconv5_k_differs_from_n(cin, B, T, taps, split):
    """n = 256 from cin = 64 / 192 / 320 inputs: 1 / 3 / 5 K chunks in bf16, 2 / 6 / 10 in bf16x3.  With one chunk there are fewer
    K steps than ring stages and the wrapping prefetch runs on the first step of the first tile; with an odd count every tile hands
    the other window buffer to the next one (and takes its second staging buffer from it), which the explicit plans with three tiles
    per group exercise.  The residual comes from an fp32 stream of n columns (the planes hold only cin: see
    test_resconv5_refuses_a_plane_residual_narrower_than_n), or is left out (no_residual).  == efts_gemm on the generic tiling, bit
    for bit, fp32 rows and the split-2 output plane.
    Under kernel = 2 only (split 1, taps 5, cin 192 / 320) run the generated main loop; cin = 64 in bf16 (nchunk = 1 < 2), every
    bf16x3 case and every 3-tap case fall back to the 8-wave kernel, so the two fixture values run the same code there."""
    c = (Case if taps == 5 else Case3)(B, T, split, seed=17, width=256, cin=cin)
    P, L, rs, dev, n = c.P, c.L, c.rs, _dev(), 256
    assert c.a.nchunk == (cin + (63 if split == 1 else 31)) // (64 if split == 1 else 32)
    live = slice(L.GUARD_LO, L.GUARD_LO + rs.rows)
    for residual in (True, False):
        o_ref, p_ref = _kn_reference(c, c.pw, taps, residual)
        for classes in (None, [[2, 3, 2]], [[8, 3, 7]], [[5, 3, 5], [3, 7, 3]]):
            plan = None if classes is None else P.make_plan(rs.rows, classes)
            o, y = P.F32Rows(rs, n, dev), P.Plane.for_rows(rs, n, 2, dev)
            kw = dict(x_f32_ptr=c.xf.ptr, ldr=n) if residual else dict(no_residual=True)
            P.resconv5(x=c.a, w=c.pw, m=rs.rows, n=n, bias=c.bias, rowmask_ptr=c.mask.data_ptr(), y_f32_ptr=o.ptr, ldo=n, y=y, taps=taps,
                       plan=plan, **kw)
            torch.cuda.synchronize()
            assert torch.equal(o.buf[live], o_ref.buf[live]), (residual, classes, f"{(o.buf - o_ref.buf).abs().max().item():.3e}")
            assert torch.equal(y.buf[live].view(torch.bfloat16), p_ref.buf[live].view(torch.bfloat16)), (residual, classes)
    print(f"cin {cin} -> 256, nchunk {c.a.nchunk}, taps {taps}, split {split}, {B}x{T}: 8 launches bit-equal to efts_gemm (generic tiling)")


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("multi", [False, True])
def test_resconv5_refuses_a_plane_residual_narrower_than_n(split, multi):
    """The epilogue addresses residual columns 0 .. n - 1 of the stream that carries the residual (vx / r_a / r_al in
    csrc/efts_resconv_tile.h).  Planes of nchunk * 64 (bf16) or nchunk * 32 (bf16x3) < n columns do not hold them -- the loads would
    return the row's padding or the next row's values -- so the combination is refused with EFTS_ESHAPE before any launch: the error
    names the cause and canary-filled outputs are untouched.  The same planes with x_f32 or no_residual are accepted
    (test_resconv5_k_differs_from_n)."""
    c = Case(3, 37, split, seed=19, width=256, cin=192)
    P, L, rs, dev = c.P, c.L, c.rs, _dev()
    lib = L.load()
    o = P.F32Rows(rs, 256, dev); o.buf.fill_(7.0)
    y = P.Plane.for_rows(rs, 256, split, dev); y.buf.fill_(0xAB)
    yl = None
    if split == 1:
        yl = P.Plane.for_rows(rs, 256, 1, dev); yl.buf.fill_(0xAB)
    g = (L.ResConv5Args * 1)()
    P._resconv5_fill(g[0], x=c.a, x_lo=c.a_lo, w=c.pw, m=rs.rows, n=256, bias=c.bias, rowmask_ptr=c.mask.data_ptr(), y_f32_ptr=o.ptr, ldo=256,
                     y=y, y_lo=yl)
    rc = lib.efts_resconv5_multi(g, 1, P._stream()) if multi else lib.efts_resconv5(g, P._stream())
    torch.cuda.synchronize()
    msg = lib.efts_last_error()
    assert rc == -2, rc                                                        # EFTS_ESHAPE
    assert b"residual" in msg and b"fewer than n = 256" in msg and (b"nchunk * 64 = 192" if split == 1 else b"nchunk * 32 = 192") in msg, msg
    assert bool((o.buf == 7.0).all()) and bool((y.buf == 0xAB).all()) and (yl is None or bool((yl.buf == 0xAB).all()))
    with pytest.raises(ValueError, match="residual from the planes"):
        P.resconv5(x=c.a, x_lo=c.a_lo, w=c.pw, m=rs.rows, n=256, bias=c.bias, y_f32_ptr=o.ptr, ldo=256)
    print(f"split {split}: refused with EFTS_ESHAPE, outputs untouched: {msg.decode()}")
