"""GPU (-m gpu): the HiFi-GAN generator step by step, off the V1 configuration, against tests/vocoder_reference.py.

`HiFiGANGenerator.forward(..., keep={})` (eager launches, `graphs = False`) clones what every step wrote.  Each step is then checked
ALONE: the plain reference of that step runs in float64 and in float32 on the DEVICE'S OWN kept input (upcast), and the device's output
of the step is compared with it, so that a mistake can neither hide behind an earlier stage nor be blamed on one.  Items are taken out
of the shared row space one by one and given to the reference without padding.

    step          input (kept)                    output (kept)                 contraction launches
    conv_pre      the mel                         "pre" plane of leaky(x)       1
    up{i}         "pre" / "s{i-1}" plane          "up{i}" fp32 (u / 2 offset)   1   (tap / column permutation of `_pack`, row offset)
    x{i}          "up{i}"                         "x{i}" plane of leaky * mask  0   (efts_act_bwd mode 3)
    r{i}.{j}.{d}  "up{i}" / "r{i}.{j}.{d-1}"      "r{i}.{j}.{d}" fp32           2   (convs1 + convs2, residual, mask)
    s{i}          the last "r{i}.{j}.*" of each j "s{i}" plane of leaky(mean)   0   (efts_mean_act_rows; slope 0.01 at the last stage)
    out           "s{last}" plane                 "out" fp32                    1   (n = 1, ldo = 1, tanh epilogue)

Bounds.  precision "fp32" (exact operands): `kernel_check._check` unchanged, max(8 * e32, 2e-6) with 8 * e32 <= 2e-4 asserted; a value
read from a format-3 plane is exact, nothing is added.  "bf16x3" / "bf16": the single-launch figures of test_gemm_conv_vs_fp64, 2e-5 and
2e-2 of max |ref|, times the contraction launches of the step, plus the resolution of the plane the value was decoded from (2^-16 /
2^-8); the two steps without a contraction are held to `_check`'s bound plus that resolution.  The operand a launch consumes is decoded
from its plane as the kernel reads it (hi + lo), so the rounding of an earlier step's output is not charged to the step after it.
Asserted with ==: rows past an item's length, the rows between items, the guard rows in front of and behind every row space, and the
plane padding columns c .. roundup(c, chunk) - 1, in every kept plane, every residual fp32 stream and the output.
Whole generator, fp32 mode: against the float64 `forward` with `_check(chain=True)`.

Configurations (tests/vocoder_reference.py:CASES; lengths in mel frames):
    narrow     64 -> 32, 16 channels, rates (4, 2), residual kernels (3, 7) with dilations (1, 3) and (1, 3, 5), lengths 9 / 1 / 14:
               16 channels are less than one operand chunk, a stride-4 transposed convolution, a mean of two, both ping-pong parities
    v2ish      32 -> 16, 8 channels, rates (2, 2), one residual kernel 11 with dilations (1, 5), 20 mels, lengths 6 / 11: a mean of one,
               a mel plane narrower than a chunk, a first rate of 2 (13 gap frames)
    gap        64 -> 32, 16, rates (4, 4), the V1 residual blocks, lengths 12 / 12 / 5 at T = 12: with 4 gap frames item 0's tail would
               sit 16 rows in front of item 1 and the k = 11, d = 5 halo of 25 rows would read it; also `torch.equal` to the items alone
    resident   64 -> 32, 16, 8, rates (4, 4, 2), one item of 60 frames: 2144 rows of 8 channels reach resident32_kernel by the AUTO rule
    v1-small   the shipped V1 configuration, lengths 5 / 3: the 512 / 256 / 128-channel tilings and the stride-8 transposed convolution

and `efts_mean_act_rows` alone against float64: 1 x 4, 5 x 8, 257 x 32, 4097 x 512 and 8200 x 512 (past 4096 blocks of 256 quads: the
grid-stride loop), one to three inputs, ld = c and ld > c, fp32 output and / or a plane of each format, prefilled with 7.0 / 0xAB.

Measured on one MI355X (worst over all configurations and steps of a kind; fp32: err / e32 where 8 * e32 is the bound, and the worst
error where the 2e-6 floor is; bf16x3 / bf16: worst error and its bound):

    step       checks  fp32: worst err / e32                     fp32: worst under the floor   bf16x3: worst err (bound)               bf16: worst err (bound)
    conv_pre        5  2.02  (gap: 9.3e-07 / 4.6e-07)            -                             6.8e-06 (3.5e-05)  v2ish                3.8e-03 (2.4e-02)  gap
    up             13  3.29  (v1-small up1: 1.1e-06 / 3.3e-07)   4.5e-07  (gap up0)            7.0e-06 (2.0e-05)  resident up2         2.3e-03 (2.0e-02)  resident up2
    x_plane        13  -                                         5.6e-09  (v1-small x3)        6.8e-06 (1.7e-05)  v1-small x0          3.4e-03 (3.9e-03)  v1-small x0
    res_pair       95  1.97  (v1-small r0.2.0: 1.2e-06 / 6.3e-07) 8.3e-07  (v1-small r1.2.1)    5.2e-06 (4.0e-05)  resident r2.0.0      2.3e-03 (4.0e-02)  resident r2.0.1
    mean_act       13  -                                         1.1e-07  (gap s1)             5.9e-06 (1.7e-05)  resident s1          3.1e-03 (3.9e-03)  resident s1
    conv_post       5  1.56  (v1-small: 4.9e-07 / 3.1e-07)       2.9e-07  (resident)           5.7e-06 (2.0e-05)  gap                  2.6e-03 (2.0e-02)  v1-small
    generator       5  1.44  (gap: 8.8e-07 / 6.1e-07)            -
    efts_mean_act_rows alone (45 fp32 / plane3 checks, 30 plane2, 15 plane1): fp32 and plane3 1.1e-07 (1 x 4, three inputs: equal to e32);
    plane2 5.9e-06 of 1.7e-05; plane1 2.9e-03 of 3.9e-03 (4097 x 512, one input)

Every fp32 ratio is below FACTOR = 8.  No bf16x3 or bf16 error of a contraction step is within a factor of two of its bound (the closest:
`up` in bf16x3, 0.35 of it).  The two steps without a contraction, x_plane and mean_act, and the plane1 row of the kernel alone, are the rounding
of the plane format and nothing else: a bf16 plane rounds to nearest, 2^-9 of the largest value at the worst against a resolution of 2^-8, so
their bf16 figures sit at 0.75 to 0.87 of the bound by construction (bf16x3: 0.34 to 0.40); that bound is the format's resolution as the
other files use it and was not widened.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import vocoder_reference as VR
from kernel_check import FLOOR, _call, _check, _dev, _rel, _st, load_lib, unpack_plane

pytestmark = pytest.mark.gpu

SPLIT = {"bf16": 1, "bf16x3": 2, "fp32": 3}
LAUNCH = {"bf16x3": 2e-5, "bf16": 2e-2}                   # one efts_gemm launch, of max |ref| (test_gemm_conv_vs_fp64)
RESOLUTION = {"fp32": 0.0, "bf16x3": 2.0 ** -16, "bf16": 2.0 ** -8}
PRECISIONS = ["fp32", "bf16x3", "bf16"]


@pytest.fixture(scope="module")
def lib():
    return load_lib()


@functools.lru_cache(maxsize=None)
def _case(name):
    cs = VR.CASES[name]
    P = VR.fill(cs["cfg"], cs["seed"])
    mel = VR.mel_input(cs["cfg"], len(cs["lengths"]), cs["T"], cs["seed"])
    return cs, P, mel, VR.Reference(cs["cfg"], P, torch.float64), VR.Reference(cs["cfg"], P, torch.float32)


@functools.lru_cache(maxsize=None)
def _whole(name):
    cs, P, mel, R64, R32 = _case(name)
    return R64.forward(mel, cs["lengths"])["out"], R32.forward(mel, cs["lengths"])["out"]


def _model(name, precision, graphs=False):
    from efficient_tts_amd.vocoder import HiFiGANGenerator
    cs, P, _, _, _ = _case(name)
    m = HiFiGANGenerator(cs["cfg"], precision=precision)
    m.load_state_dict(P)
    m = m.to(_dev()).eval()
    m.graphs = graphs
    return m


def _decode(buf, split):
    """a kept operand plane uint8 [alloc][ld] -> float32 [alloc][every column of its chunks]"""
    alloc, ld = buf.shape
    kp = ld // 128 * (64 if split == 1 else 32)
    return unpack_plane(buf, 1, alloc, alloc, kp, split)[0]


def _items(full, c, rate, pitch, lens, guard, zeros=True):
    """the items of a row space [alloc][>= c] as [1, c, len * rate] each; with `zeros`, everything that is not a live row and column of
    an item -- guard rows, the rows between items and past a length, padding columns -- must be exactly 0"""
    full = full.cpu()
    live = torch.zeros(full.shape[0], dtype=torch.bool)
    items = []
    for b, n in enumerate(lens):
        lo = guard + b * pitch * rate
        live[lo:lo + n * rate] = True
        items.append(full[lo:lo + n * rate, :c].t().contiguous()[None].float())
    if zeros:
        assert bool((full[~live] == 0).all()), "rows outside the items must be exactly 0"
        assert bool((full[:, c:] == 0).all()), "padding columns must be exactly 0"
    return items


def _step_check(prec, kind, case, got, ref64, ref32, launches, from_plane):
    got, ref64, ref32 = torch.cat(got, 2), torch.cat(ref64, 2), torch.cat(ref32, 2)
    res = RESOLUTION[prec] if from_plane else 0.0
    if prec == "fp32" or launches == 0:
        _check(kind, f"{case} {prec}", got, ref64, ref32, extra=res)
        return
    assert bool(torch.isfinite(got).all())
    err, bound = _rel(got.double(), ref64), launches * LAUNCH[prec] + res
    print(f"RATIO {kind} {case} {prec} err={err:.3e} bound={bound:.3e} ratio={err / bound:.2f}")
    assert err <= bound, f"{kind} {case} {prec}: error {err:.3e} vs float64, bound {bound:.3e}"


def _both(R64, R32, fn, *xs):
    return fn(R64, *xs), fn(R32, *xs)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(VR.CASES))
def test_every_step_alone_vs_fp64(lib, name, precision):
    from efficient_tts_amd.vocoder import _GUARD
    cs, P, mel, R64, R32 = _case(name)
    cfg, lens, T = cs["cfg"], cs["lengths"], cs["T"]
    sp = SPLIT[precision]
    m = _model(name, precision)
    keep = {}
    audio = m(mel.to(_dev()), torch.tensor(lens), keep=keep)
    torch.cuda.synchronize()
    keep = {k: v.cpu() if torch.is_tensor(v) else v for k, v in keep.items()}
    pitch, rates = keep["pitch"], R64.rates
    assert pitch == T + m.gap_frames
    nk = len(R64.res_kernels)

    def plane(key, c, rate):
        return _items(_decode(keep[key], sp), c, rate, pitch, lens, _GUARD)

    def check(kind, key, got, refs, launches, from_plane):
        _step_check(precision, kind, f"{name}:{key}", got, [r[0] for r in refs], [r[1] for r in refs], launches, from_plane)

    # conv_pre -> the plane of leaky(x)
    c = int(cfg["upsample_initial_channel"])
    cur = plane("pre", c, 1)
    check("conv_pre", "pre", cur, [_both(R64, R32, lambda R, x: F.leaky_relu(R.conv_pre(x), VR.LRELU_SLOPE), mel[b:b + 1, :, :n])
                                   for b, n in enumerate(lens)], 1, True)
    rate = 1
    for i, u in enumerate(rates):
        rate *= u
        c = VR.channels(cfg, i)
        last = i == len(rates) - 1
        # the transposed convolution, fed with the device's own plane of leaky(x)
        up = _items(keep[f"up{i}"], c, rate, pitch, lens, 0, zeros=False)
        check("up", f"up{i}", up, [_both(R64, R32, lambda R, x: R.up(i, x, activated=True), x) for x in cur], 1, False)
        # masked LeakyReLU plane of it
        check("x_plane", f"x{i}", plane(f"x{i}", c, rate), [_both(R64, R32, lambda R, x: F.leaky_relu(x.to(R.dtype), VR.LRELU_SLOPE), x) for x in up],
              0, True)
        finals = []
        for j in range(nk):
            r = up
            for d_i in range(len(R64.res_dilations[j])):
                key = f"r{i}.{j}.{d_i}"
                nxt = _items(keep[key], c, rate, pitch, lens, _GUARD)
                check("res_pair", key, nxt, [_both(R64, R32, lambda R, x: R.res_pair(R.block(i, j), d_i, x), x) for x in r], 2, False)
                r = nxt
            finals.append(r)
        slope = VR.POST_SLOPE if last else VR.LRELU_SLOPE
        cur = plane(f"s{i}", c, rate)
        check("mean_act", f"s{i}", cur, [_both(R64, R32, lambda R, *xs: F.leaky_relu(R.mean(list(xs)), slope), *[f[b] for f in finals])
                                         for b in range(len(lens))], 0, True)
    out = _items(keep["out"], 1, rate, pitch, lens, 0)
    check("conv_post", "out", out, [_both(R64, R32, lambda R, x: R.conv_post(x, activated=True), x) for x in cur], 1, False)
    # what forward() returns is that buffer, item by item, silent past every length
    audio = audio.cpu()
    assert audio.shape == (len(lens), 1, T * rate)
    for b, n in enumerate(lens):
        assert torch.equal(audio[b, :, :n * rate], out[b][0]) and bool((audio[b, :, n * rate:] == 0).all())
    if precision == "fp32":
        w64, w32 = _whole(name)
        _check("generator", f"{name} fp32", audio, w64, w32, chain=True)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_gap_batch_equals_items_alone(precision):
    """`gap`: rates (4, 4) under the V1 residual blocks.  Item 0 fills all T = 12 frames, so the zero rows in front of item 1 at the first
    upsampled stage are gap_frames * 4: with the 4 frames V1 needs they would be 16, fewer than the 25-row halo of the k = 11, d = 5
    convolution, and item 1 would read item 0's tail.  The property of test_ragged_batch_equals_single_utterances, with the launches
    captured as forward() does by default."""
    cs, P, mel, _, _ = _case("gap")
    lens, T = cs["lengths"], cs["T"]
    m = _model("gap", precision, graphs=True)
    y = m(mel.to(_dev()), torch.tensor(lens))
    assert y.shape == (len(lens), 1, T * 16)
    for b, n in enumerate(lens):
        alone = m(mel[b:b + 1, :, :n].contiguous().to(_dev()))
        assert torch.equal(y[b, :, :n * 16], alone[0]), (precision, b)
        assert bool((y[b, :, n * 16:] == 0).all())


# =====================================================================================================================
# efts_mean_act_rows alone
# =====================================================================================================================
def _touched(rows_alloc, ldp, rows, c, split):
    """bytes of a plane [rows_alloc][ldp] that a writer of `rows` x `c` values touches"""
    t = torch.zeros(rows_alloc, ldp, dtype=torch.bool)
    if split == 1:
        t[:rows, :2 * c] = True
        return t
    for q in range((c + 31) // 32):
        n = min(32, c - 32 * q)
        if split == 3:
            t[:rows, 128 * q:128 * q + 4 * n] = True
        else:
            t[:rows, 128 * q:128 * q + 2 * n] = True
            t[:rows, 128 * q + 64:128 * q + 64 + 2 * n] = True
    return t


@pytest.mark.parametrize("rows,c", [(1, 4), (5, 8), (257, 32), (4097, 512), (8200, 512)])
def test_mean_act_rows_vs_fp64(lib, rows, c):
    """efts_mean_act_rows: m = (a + b + c3) * scale as fp32 and / or the operand plane of leaky(m).  One quad of columns per thread,
    256 per block, at most 4096 blocks: one thread, 10 quads, 2056 quads, 524 416 quads in 2049 blocks, and 1 049 600 quads, which is past
    4096 blocks, so the grid-stride loop turns twice for some threads."""
    dev = _dev()
    g = torch.Generator().manual_seed(rows * 1000 + c)
    slope = 0.1
    for nin in (1, 2, 3):
        ld = c if nin == 2 else c + 8
        src = [torch.randn(rows, ld, generator=g) for _ in range(nin)]
        d = [s.to(dev) for s in src] + [None] * (3 - nin)
        scale = float(torch.tensor(1.0 / nin, dtype=torch.float32))                   # the float the kernel is given
        s64, s32 = src[0][:, :c].double(), src[0][:, :c].clone()
        for s in src[1:]:
            s64, s32 = s64 + s[:, :c].double(), s32 + s[:, :c]
        m64, m32 = s64 * scale, s32 * torch.tensor(scale, dtype=torch.float32)
        p64, p32 = F.leaky_relu(m64, slope), F.leaky_relu(m32, slope)
        first = None
        for with_out, split in ((True, None), (False, 1), (False, 2), (False, 3), (True, 2)):
            ldo = c + 4
            out = torch.full((rows + 2, ldo), 7.0, device=dev) if with_out else None
            nchunk = 0 if split is None else (c + (64 if split == 1 else 32) - 1) // (64 if split == 1 else 32)
            ldp = nchunk * 128 + (128 if rows == 5 else 0)
            pl = torch.full((rows + 2, ldp), 0xAB, dtype=torch.uint8, device=dev) if split else None
            _call("efts_mean_act_rows", lib.efts_mean_act_rows(d[0].data_ptr(), None if d[1] is None else d[1].data_ptr(),
                                                               None if d[2] is None else d[2].data_ptr(), ld, scale, slope,
                                                               None if out is None else out.data_ptr(), ldo if with_out else 0,
                                                               None if pl is None else pl.data_ptr(), ldp, split or 1, rows, c, _st()))
            torch.cuda.synchronize()
            case = f"{rows}x{c} inputs={nin} ld={ld} out={with_out} plane={split}"
            if out is not None:
                out = out.cpu()
                _check("efts_mean_act_rows.fp32", case, out[:rows, :c], m64, m32)
                assert bool((out[rows:] == 7.0).all()) and bool((out[:, c:] == 7.0).all())            # untouched
                if first is None:
                    first = out[:rows, :c].clone()
                else:
                    assert torch.equal(out[:rows, :c].contiguous().view(torch.int32), first.view(torch.int32))   # a plane next to it changes no bit
            if pl is not None:
                raw = pl.cpu()
                t = _touched(rows + 2, ldp, rows, c, split)
                assert bool((raw[~t] == 0xAB).all())                                                  # rows past the end, padding columns, bytes past the chunks
                clean = torch.where(t, raw, torch.zeros_like(raw))[:, :nchunk * 128].contiguous()
                got = unpack_plane(clean, 1, rows + 2, rows, nchunk * (64 if split == 1 else 32), split)[0][:, :c]
                _check(f"efts_mean_act_rows.plane{split}", case, got, p64, p32, extra={1: 2.0 ** -8, 2: 2.0 ** -16, 3: 0.0}[split])
                if split == 3 and first is not None:                                                  # format 3 holds leaky of the very fp32 mean
                    want = torch.where(first > 0, first, first * torch.tensor(slope, dtype=torch.float32))
                    assert float((got - want).abs().max()) <= FLOOR * float(want.abs().max())
