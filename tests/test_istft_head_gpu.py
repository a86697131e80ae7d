"""GPU (-m gpu): the iSTFTNet head -- `efts_istft_head` (csrc/efts_istft_head.hip) alone and through `HiFiGANGenerator` -- against
tests/istft_reference.py.

The kernel alone: z ~ 1.5 * randn in a ragged row space of B = 6 items, N + 2 columns, N = 16 and 8, two batches per N that hold the
lengths 0, 4, 5, FR - 1, FR, FR + 1 and 3 FR + 1 (FR = 1024 / h, the frames of hops a workgroup owns) in mixed order at a pitch of
3 FR + 8 rows.  Every sample against `head()` in float64; the yardstick is the same z through torch.exp / sin / torch.istft in fp32 on
the CPU, also against float64; the bound is 4 x the yardstick's worst error (the convention of the STFT-family kernels: a different but
equally long fp32 summation order plus the device's exp / sin / cos).  Samples at t >= h L are exactly 0; an item alone, the batch with
garbage behind every item's frames and a captured call give the bits of the batch.

Through the generator (eager launches, `keep`): cases "c4c4i" and "rb2-n8" of tests/istft_reference.py.  `z` against the float64
reference fed the device's own decoded `s` plane, held to the one-launch bound of tests/test_vocoder_stages_gpu.py in each precision
(constants imported), frame 0 of every item (the only frame that sees the reflected row) on its own; the audio from the device's own z
to the head bound; the batch equal to the items alone, bit for bit; silence past every length.  End to end in fp32: the V1 generator's
fp32 end-to-end error (configuration, weights and mel of tests/test_vocoder.py, against the float64 reference) is measured on the same
visit and the iSTFT cases are allowed that error times max_t sum_j |d out[t] / d z[j]| of the float64 reference on the case.

EFTS_WRITE_PROFILES=1 merges the figures into profiles/istft_head_error.json.  Measured on one MI355X: see that file.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import istft_reference as IR
import vocoder_reference as VR
from kernel_check import _call, _check, _dev, _rel, _st, load_lib
from test_vocoder_stages_gpu import LAUNCH, PRECISIONS, RESOLUTION, SPLIT, _decode, _items

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = 1024                                     # EFTS_ISTFT_RUN


def _record(key, value):
    """how profiles/istft_head_error.json is produced: EFTS_WRITE_PROFILES=1 merges this test's figures into it"""
    if not os.environ.get("EFTS_WRITE_PROFILES"):
        return
    path = os.path.join(ROOT, "profiles", "istft_head_error.json")
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[key] = value
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _tables(N):
    ang = 2.0 * np.pi * torch.arange(N, dtype=torch.float64) / N
    return IR.window(N, torch.float32).to(_dev()), torch.stack([torch.cos(ang), torch.sin(ang)], 1).float().contiguous().to(_dev())


def _head(lib, z, lens, pitch, N, h, out_len, ld, tables, li=None, audio=None):
    from efficient_tts_amd import lib as L
    B = len(lens)
    audio = torch.full((B, ld), 7.0, device=_dev()) if audio is None else audio
    li = torch.tensor(lens, dtype=torch.int32, device=_dev()) if li is None else li
    a = L.IstftHeadArgs()
    a.mode, a.B, a.pitch, a.z, a.z_rows, a.lengths, a.len_mul = L.ISTFT_SYNTH, B, pitch, z.data_ptr(), z.shape[0], li.data_ptr(), 1
    a.window, a.twiddle, a.n_fft, a.hop, a.audio, a.ld_audio, a.out_len = tables[0].data_ptr(), tables[1].data_ptr(), N, h, audio.data_ptr(), ld, out_len
    _call("efts_istft_head", lib.efts_istft_head(ctypes.byref(a), _st()))
    return audio


def _yardstick(zf, N, h):
    """z [L + 1, N + 2] float32 through torch.exp / sin / torch.istft in fp32 on the CPU"""
    K = N // 2 + 1
    spec = torch.exp(zf[:, :K]) * torch.exp(1j * torch.sin(zf[:, K:]))
    return torch.istft(spec.t()[None], N, h, N, window=torch.hann_window(N), center=True)[0]


@functools.lru_cache(maxsize=None)
def _alone_case(N, batch):
    h = N // 4
    FR = RUN // h
    lens = ([FR + 1, 0, 4, 3 * FR + 1, 5, FR - 1], [FR, 5, 0, 3 * FR + 1, FR - 1, 4])[batch]
    pitch = 3 * FR + 8
    z = 1.5 * torch.randn(len(lens) * pitch, N + 2, generator=torch.Generator().manual_seed(100 * N + batch))
    ref, yard = [], 0.0
    for b, L in enumerate(lens):
        zf = z[b * pitch:b * pitch + L + 1]
        ref.append(IR.head(zf.double(), N, h))
        if L:
            yard = max(yard, float((_yardstick(zf, N, h).double() - ref[-1]).abs().max()))
    return lens, pitch, z, ref, yard


@pytest.mark.parametrize("batch", [0, 1])
@pytest.mark.parametrize("N", [16, 8])
def test_kernel_alone_vs_fp64(lib, N, batch):
    h = N // 4
    lens, pitch, z, ref, yard = _alone_case(N, batch)
    out_len = (h * max(lens) + 3) // 4 * 4 + 4
    ld = out_len + 8
    tables = _tables(N)
    zd = z.to(_dev())
    got_d = _head(lib, zd, lens, pitch, N, h, out_len, ld, tables)
    got = got_d.cpu()
    assert bool((got[:, out_len:] == 7.0).all())                                   # nothing behind out_len is written
    worst = 0.0
    for b, L in enumerate(lens):
        assert bool((got[b, h * L:out_len] == 0).all()), f"item {b}: samples past h L must be exactly 0"
        if L:
            assert bool(torch.isfinite(got[b, :h * L]).all())
            worst = max(worst, float((got[b, :h * L].double() - ref[b]).abs().max()))
    bound = 4.0 * yard
    print(f"N {N} batch {batch}: max |device - float64| {worst:.3e}; yardstick (fp32 torch.istft on the CPU) {yard:.3e}; bound 4 x = {bound:.3e}")
    _record(f"kernel_alone_n{N}_batch{batch}", {"lengths": lens, "device_max_abs_error": worst, "yardstick_fp32_torch_istft_cpu_max_abs_error": yard,
                                               "bound_4x": bound, "largest_value": max(float(r.abs().max()) for r in ref if r.numel())})
    assert 0.0 < yard < 1e-4                                                        # the yardstick itself is an fp32 rounding error
    assert worst <= bound
    # each item alone equals the item in the batch
    for b, L in enumerate(lens):
        one = _head(lib, zd[b * pitch:(b + 1) * pitch].contiguous(), [L], pitch, N, h, out_len, ld, tables).cpu()
        assert torch.equal(one[0].view(torch.int32), got[b].view(torch.int32)), f"item {b} alone differs from the item in the batch"
    # garbage in the rows of z past every item's frames changes no bit
    dirty = z.clone()
    for b, L in enumerate(lens):
        lo = b * pitch + (L + 1 if L else 0)
        dirty[lo:(b + 1) * pitch] = torch.tensor([float("nan"), 1e30, -1e30, 80.0, float("inf")]).repeat(N)[:N + 2]
    got2 = _head(lib, dirty.to(_dev()), lens, pitch, N, h, out_len, ld, tables).cpu()
    assert torch.equal(got2.view(torch.int32), got.view(torch.int32))
    # a captured call replays the eager bits
    li, cap = torch.tensor(lens, dtype=torch.int32, device=_dev()), torch.full((len(lens), ld), 7.0, device=_dev())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _head(lib, zd, lens, pitch, N, h, out_len, ld, tables, li=li, audio=cap)
    cap[:, :out_len] = 3.0
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap.cpu().view(torch.int32), got.view(torch.int32))


def test_argument_errors(lib):
    """bad arguments are refused before any launch"""
    from efficient_tts_amd import lib as L
    N, h = 16, 4
    tables = _tables(N)
    z = torch.zeros(64, N + 2, device=_dev())
    audio = torch.zeros(1, 64, device=_dev())
    li = torch.tensor([8], dtype=torch.int32, device=_dev())

    def call(**kw):
        a = L.IstftHeadArgs()
        a.mode, a.B, a.pitch, a.z, a.z_rows, a.lengths, a.len_mul = L.ISTFT_SYNTH, 1, 64, z.data_ptr(), 64, li.data_ptr(), 1
        a.window, a.twiddle, a.n_fft, a.hop, a.audio, a.ld_audio, a.out_len = tables[0].data_ptr(), tables[1].data_ptr(), N, h, audio.data_ptr(), 64, 64
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.efts_istft_head(ctypes.byref(a), _st())

    assert call() == 0
    assert call(n_fft=64, hop=16) == -1 and call(n_fft=12, hop=3) == -1 and call(hop=8) == -1 and call(mode=2) == -1 and call(reserved=1) == -1
    assert call(z=z.data_ptr() + 8) == -3 and call(audio=audio.data_ptr() + 4) == -3 and call(ld_audio=66) == -3
    assert call(pitch=63) == -2 and call(out_len=62) == -2 and call(B=0) == -2 and call(ld_audio=32) == -2
    assert call(mode=L.ISTFT_REFLECT, plane=None) == -1 and call(mode=L.ISTFT_REFLECT, plane=z.data_ptr() + 72, ld_plane=72) == -3
    torch.cuda.synchronize()


# =====================================================================================================================
# through the generator
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def _case(name):
    cs = IR.ISTFT_CASES[name]
    P = IR.fill(cs["cfg"], cs["seed"])
    mel = IR.mel_input(cs["cfg"], len(cs["lengths"]), cs["T"], cs["seed"])
    return cs, P, mel, IR.reference(cs["cfg"], P, torch.float64), IR.reference(cs["cfg"], P, torch.float32)


def _model(name, precision, graphs=False):
    from efficient_tts_amd.vocoder import HiFiGANGenerator
    cs, P, _, _, _ = _case(name)
    m = HiFiGANGenerator(cs["cfg"], precision=precision)
    m.load_state_dict(P)
    m = m.to(_dev()).eval()
    m.graphs = graphs
    return m


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(IR.ISTFT_CASES))
def test_head_through_the_generator(name, precision):
    from efficient_tts_amd.vocoder import _GUARD
    cs, P, mel, R64, R32 = _case(name)
    cfg, lens, T = cs["cfg"], cs["lengths"], cs["T"]
    N, h = IR.istft_params(cfg)
    rate = R64.hop                                                                  # rows per mel frame at the last stage
    c = VR.channels(cfg, len(cfg["upsample_rates"]) - 1)
    m = _model(name, precision)
    assert m.hop == rate * h
    keep = {}
    audio = m(mel.to(_dev()), torch.tensor(lens), keep=keep).cpu()
    pitch = keep["pitch"] * rate
    assert audio.shape == (len(lens), 1, T * rate * h) and torch.equal(audio, keep["out"].cpu())
    s_items = _items(_decode(keep[f"s{len(cfg['upsample_rates']) - 1}"].cpu(), SPLIT[precision]), c, rate, keep["pitch"], lens, _GUARD)
    z_all = keep["z"].cpu()
    worst_head, yard = 0.0, 0.0
    for b, n in enumerate(lens):
        L = n * rate
        z_dev = z_all[b * pitch:b * pitch + L + 1]                                  # [L + 1, N + 2]
        z64, z32 = R64.conv_post_z(s_items[b], activated=True)[0].t(), R32.conv_post_z(s_items[b], activated=True)[0].t()
        for what, sl in (("z", slice(None)), ("z frame 0", slice(0, 1))):
            if precision == "fp32":
                _check(f"conv_post {what}", f"{name} item {b}", z_dev[sl], z64[sl], z32[sl])
            else:
                err, bound = float((z_dev[sl].double() - z64[sl]).abs().max()) / float(z64.abs().max()), LAUNCH[precision]
                print(f"RATIO conv_post {what} {name} item {b} {precision} err={err:.3e} bound={bound:.3e}")
                assert err <= bound, f"{what} {name} item {b} {precision}: error {err:.3e} of max |z| vs float64, bound {bound:.3e}"
        # rows of z behind the item's frames are masked
        assert bool((z_all[b * pitch + L + 1:(b + 1) * pitch] == 0).all())
        # the audio from the device's own z
        ref = IR.head(z_dev.double(), N, h)
        worst_head = max(worst_head, float((audio[b, 0, :L * h].double() - ref).abs().max()))
        yard = max(yard, float((_yardstick(z_dev, N, h).double() - ref).abs().max()))
        assert bool((audio[b, 0, L * h:] == 0).all())
        alone = m(mel[b:b + 1, :, :n].contiguous().to(_dev())).cpu()
        assert torch.equal(alone[0, 0].view(torch.int32), audio[b, 0, :L * h].view(torch.int32)), (name, precision, b)
    print(f"{name} {precision}: audio from the device's own z, max |device - float64| {worst_head:.3e}; yardstick {yard:.3e}; bound 4 x = {4 * yard:.3e}")
    _record(f"generator_head_{name}_{precision}", {"device_max_abs_error": worst_head, "yardstick_fp32_torch_istft_cpu_max_abs_error": yard, "bound_4x": 4 * yard})
    assert worst_head <= 4.0 * yard


@functools.lru_cache(maxsize=None)
def _v1_fp32_error():
    """max |V1 generator in fp32 precision - float64 reference|: configuration, weights and mel of tests/test_vocoder.py"""
    from efficient_tts_amd.vocoder import HiFiGANGenerator
    from oracle import hifigan_oracle as HO
    from test_vocoder import CFG, GOLD
    P = HO.fill_params()
    mel = torch.from_numpy(np.load(GOLD)["mel_a"])
    m = HiFiGANGenerator(CFG, precision="fp32")
    m.load_state_dict(P)
    m = m.to(_dev()).eval()
    ref = VR.forward(P, mel, None, CFG, torch.float64)["out"]
    return float((m(mel.to(_dev())).cpu().double() - ref).abs().max())


def _gain(z64, N, h):
    """max_t sum_j |d out[t] / d z[j]| of the float64 head at z64 [L + 1, N + 2]"""
    J = torch.autograd.functional.jacobian(lambda z: IR.head(z, N, h), z64)
    return float(J.abs().flatten(1).sum(1).max())


@pytest.mark.parametrize("name", list(IR.ISTFT_CASES))
def test_end_to_end_fp32_vs_fp64(name):
    cs, P, mel, R64, _ = _case(name)
    lens, T = cs["lengths"], cs["T"]
    N, h = IR.istft_params(cs["cfg"])
    e_v1 = _v1_fp32_error()
    st = R64.forward(mel, lens)
    gain = 0.0
    for b, n in enumerate(lens):
        x = R64._forward_dense(mel[b:b + 1, :, :n])[f"mean{len(cs['cfg']['upsample_rates']) - 1}"]
        gain = max(gain, _gain(R64.conv_post_z(x)[0].t().contiguous(), N, h))
    audio = _model(name, "fp32")(mel.to(_dev()), torch.tensor(lens)).cpu()
    err, bound = float((audio.double() - st["out"]).abs().max()), e_v1 * gain
    print(f"{name}: end to end fp32 max |device - float64| {err:.3e}; V1 fp32 end-to-end error {e_v1:.3e} x max |d out / d z| {gain:.3e} = {bound:.3e}")
    _record(f"end_to_end_fp32_{name}", {"device_max_abs_error": err, "v1_fp32_end_to_end_max_abs_error": e_v1, "max_abs_row_sum_dout_dz": gain, "bound": bound})
    assert bool(torch.isfinite(audio).all()) and err <= bound


@pytest.mark.parametrize("precision", PRECISIONS)
def test_captured_forward_equals_eager(precision):
    """forward() captures its launches by default: the replay gives the eager bits, for the batch and with other lengths on the same graph"""
    cs, P, mel, _, _ = _case("c4c4i")
    eager, graphed = _model("c4c4i", precision), _model("c4c4i", precision, graphs=True)
    for lens in (cs["lengths"], [3, 1, 12]):
        a = eager(mel.to(_dev()), torch.tensor(lens))
        for _ in range(3):
            b = graphed(mel.to(_dev()), torch.tensor(lens))
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
