"""CPU: the float64 reference of the iSTFTNet head (tests/istft_reference.py) against torch.istft and against a from-scratch restatement of
the published generator, what the constructor refuses, the untouched HiFi-GAN generator, and the ABI of efts_istft_head.  No device."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import istft_reference as IR
import vocoder_reference as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("L", [4, 5, 64, 1000])
@pytest.mark.parametrize("N", [8, 16, 32])
def test_head_equals_torch_istft(N, L):
    h, K = N // 4, N // 2 + 1
    z = 1.5 * torch.randn(L + 1, N + 2, dtype=torch.float64, generator=torch.Generator().manual_seed(N * 10000 + L))
    spec = torch.exp(z[:, :K]) * torch.exp(1j * torch.sin(z[:, K:]))
    want = torch.istft(spec.t()[None], N, h, N, window=torch.hann_window(N, dtype=torch.float64), center=True)[0]
    got = IR.head(z, N, h)
    assert got.shape == want.shape == (h * L,)
    assert float((got - want).abs().max()) <= 1e-12
    assert IR.head(z[:1], N, h).numel() == 0                       # L = 0: no samples


def _published(cfg, P, mel):
    """the published iSTFTNet generator restated from the paper: the HiFi-GAN trunk, leaky_relu, ReflectionPad1d((1, 0)), conv_post to
    N + 2 channels, spec = exp(x[:, :K]), phase = sin(x[:, K:]), torch.istft of spec * exp(1j * phase) with the Hann window"""
    N, h = IR.istft_params(cfg)
    K = N // 2 + 1
    w, b = {}, {}
    for name, v in P.items():
        if name.endswith(".weight_v"):
            pre = name[:-len(".weight_v")]
            v64, g64 = v.double(), P[pre + ".weight_g"].double()
            w[pre] = g64 * v64 / v64.flatten(1).norm(dim=1).view(-1, 1, 1)
        elif name.endswith(".bias"):
            b[name[:-len(".bias")]] = v.double()
    x = F.conv1d(mel.double(), w["conv_pre"], b["conv_pre"], padding=3)
    nk, n = len(cfg["resblock_kernel_sizes"]), 0
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        x = F.conv_transpose1d(F.leaky_relu(x, 0.1), w[f"ups.{i}"], b[f"ups.{i}"], stride=u, padding=(k - u) // 2)
        xs = None
        for kk, ds in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]):
            r = x
            if str(cfg["resblock"]) == "1":
                for d_i, d in enumerate(ds):
                    t = F.conv1d(F.leaky_relu(r, 0.1), w[f"resblocks.{n}.convs1.{d_i}"], b[f"resblocks.{n}.convs1.{d_i}"], padding=(kk * d - d) // 2, dilation=d)
                    t = F.conv1d(F.leaky_relu(t, 0.1), w[f"resblocks.{n}.convs2.{d_i}"], b[f"resblocks.{n}.convs2.{d_i}"], padding=(kk - 1) // 2)
                    r = t + r
            else:
                for d_i, d in enumerate(ds[:2]):
                    r = F.conv1d(F.leaky_relu(r, 0.1), w[f"resblocks.{n}.convs.{d_i}"], b[f"resblocks.{n}.convs.{d_i}"], padding=(kk * d - d) // 2, dilation=d) + r
            xs = r if xs is None else xs + r
            n += 1
        x = xs / nk
    x = nn.ReflectionPad1d((1, 0))(F.leaky_relu(x))
    x = F.conv1d(x, w["conv_post"], b["conv_post"], padding=3)
    spec, phase = torch.exp(x[:, :K]), torch.sin(x[:, K:])
    return torch.istft(spec * torch.exp(1j * phase), N, h, N, window=torch.hann_window(N, dtype=torch.float64), center=True)[:, None]


@pytest.mark.parametrize("name", list(IR.ISTFT_CASES))
def test_reference_forward_equals_the_published_generator(name):
    cs = IR.ISTFT_CASES[name]
    cfg, lens, T = cs["cfg"], cs["lengths"], cs["T"]
    P = IR.fill(cfg, cs["seed"])
    mel = IR.mel_input(cfg, len(lens), T, cs["seed"])
    N, h = IR.istft_params(cfg)
    out = IR.forward(P, mel, lens, cfg)["out"]
    hop = IR.reference(cfg, P).hop * h
    assert out.shape == (len(lens), 1, T * hop)
    for b, n in enumerate(lens):
        want = _published(cfg, P, mel[b:b + 1, :, :n])
        assert want.shape == (1, 1, n * hop)
        assert float((out[b:b + 1, :, :n * hop] - want).abs().max()) <= 1e-10
        assert bool((out[b, :, n * hop:] == 0).all())


BASE = IR.ISTFT_CASES["c4c4i"]["cfg"]
REFUSED = {
    "n_fft 64": (dict(gen_istft_n_fft=64, gen_istft_hop_size=16), "efts_istft_head takes 8, 16, 32"),
    "n_fft 12": (dict(gen_istft_n_fft=12, gen_istft_hop_size=3), "efts_istft_head takes 8, 16, 32"),
    "hop 8 under 16": (dict(gen_istft_n_fft=16, gen_istft_hop_size=8), "hop = n_fft / 4 = 4"),
    "hop 2 under 16": (dict(gen_istft_n_fft=16, gen_istft_hop_size=2), "hop = n_fft / 4 = 4"),
    "n_fft without hop": (dict(gen_istft_n_fft=16, gen_istft_hop_size=None), "hop = n_fft / 4 = 4"),
    "hop without n_fft": (dict(gen_istft_n_fft=None, gen_istft_hop_size=4), "gen_istft_hop_size without gen_istft_n_fft"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_constructor_refusals(case):
    from efficient_tts_amd.vocoder import HiFiGANGenerator
    extra, why = REFUSED[case]
    cfg = {k: v for k, v in {**BASE, **extra}.items() if v is not None}
    with pytest.raises(NotImplementedError) as ei:
        HiFiGANGenerator(cfg)
    assert why in str(ei.value)


@pytest.mark.parametrize("name", list(IR.ISTFT_CASES))
def test_generator_with_the_key(name):
    """conv_post has N + 2 channels under weight norm, hop = prod(rates) * h, the HiFi-GAN key set and nothing else in the state dict;
    no CPU path"""
    from efficient_tts_amd.vocoder import HiFiGANGenerator
    cfg = IR.ISTFT_CASES[name]["cfg"]
    N, h = IR.istft_params(cfg)
    m = HiFiGANGenerator(cfg)
    shapes = IR.param_shapes(cfg)
    sd = m.state_dict()
    assert list(sd.keys()) == list(shapes.keys()) and all(tuple(sd[k].shape) == tuple(shapes[k]) for k in shapes)
    assert tuple(sd["conv_post.weight_v"].shape)[0] == N + 2
    rate = 1
    for u in cfg["upsample_rates"]:
        rate *= u
    assert m.hop == rate * h
    m.load_state_dict(IR.fill(cfg, 1))
    m.remove_weight_norm()
    assert "conv_post.weight" in m.state_dict() and not any("window" in k or "twiddle" in k for k in m.state_dict())
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, int(cfg["num_mels"]), 4))
    c8c8i = dict(VR.V1, upsample_rates=[8, 8], upsample_kernel_sizes=[16, 16], gen_istft_n_fft=16, gen_istft_hop_size=4)
    assert HiFiGANGenerator(c8c8i).hop == 256


@pytest.mark.parametrize("name", ["gap", "v1-small"])
def test_generator_without_the_key_is_the_generator_of_before(name):
    from efficient_tts_amd.vocoder import HiFiGANGenerator, _TanhHead
    cfg = VR.CASES[name]["cfg"]
    m = HiFiGANGenerator(cfg)
    shapes = VR.param_shapes(cfg)
    sd = m.state_dict()
    assert list(sd.keys()) == list(shapes.keys()) and all(tuple(sd[k].shape) == tuple(shapes[k]) for k in shapes)
    rate = 1
    for u in cfg["upsample_rates"]:
        rate *= u
    assert m.hop == rate and isinstance(m._head, _TanhHead) and m._head.tag == ()          # the graph tag is the tag of before


def test_abi_of_the_head():
    """the header declares efts_istft_head, the library exports it, the revision is 602, the argument block is the ctypes mirror, and bad
    arguments are refused before any launch"""
    import subprocess
    import tempfile
    from efficient_tts_amd import build as B
    from efficient_tts_amd import lib as L
    B.build(verbose=False)
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "efts_abi.h")).read()
    assert re.search(r"int efts_istft_head\(const efts_istft_head_args\* a, void\* stream\);", hdr)
    assert "efts_istft_head" in L.exported_symbols() and hasattr(lib, "efts_istft_head")
    assert int(re.search(r"#define EFTS_ABI_VERSION (\d+)", hdr).group(1)) == 602 == L.ABI_VERSION == lib.efts_version()
    assert int(re.search(r"#define EFTS_ISTFT_RUN (\d+)", hdr).group(1)) == L.ISTFT_RUN
    assert (int(re.search(r"#define EFTS_ISTFT_SYNTH (\d+)", hdr).group(1)), int(re.search(r"#define EFTS_ISTFT_REFLECT (\d+)", hdr).group(1))) == (L.ISTFT_SYNTH, L.ISTFT_REFLECT)
    fields = [f for f, _ in L.IstftHeadArgs._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "efts_abi.h"\nint main(){\nprintf(" %zu", sizeof(efts_istft_head_args));' +
           "".join(f'printf(" %zu", offsetof(efts_istft_head_args, {f}));' for f in fields) + "return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got == [ctypes.sizeof(L.IstftHeadArgs)] + [getattr(L.IstftHeadArgs, f).offset for f in fields]

    assert lib.efts_istft_head(None, None) == -1 and b"null args" in lib.efts_last_error()
    buf = (ctypes.c_float * 1024)()
    base = (ctypes.addressof(buf) + 15) & ~15

    def call(**kw):
        a = L.IstftHeadArgs()
        a.mode, a.B, a.pitch, a.z, a.z_rows, a.lengths, a.len_mul = L.ISTFT_SYNTH, 1, 16, base, 16, base, 1
        a.window, a.twiddle, a.n_fft, a.hop, a.audio, a.ld_audio, a.out_len = base, base, 16, 4, base, 64, 64
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.efts_istft_head(ctypes.byref(a), None), lib.efts_last_error()

    for kw, rc, word in ((dict(n_fft=64, hop=16), -1, b"n_fft must be 8, 16 or 32"), (dict(n_fft=4, hop=1), -1, b"n_fft"), (dict(hop=8), -1, b"hop must be n_fft / 4"),
                         (dict(mode=2), -1, b"mode"), (dict(reserved=1), -1, b"reserved"), (dict(z=None), -1, b"null operand"),
                         (dict(z=base + 8), -3, b"16-byte aligned"), (dict(audio=base + 4), -3, b"16-byte aligned"), (dict(ld_audio=66), -3, b"16-byte aligned"),
                         (dict(pitch=15), -2, b"pitch"), (dict(out_len=62), -2, b"out_len"), (dict(B=0), -2, b"items"), (dict(ld_audio=32), -2, b"ld_audio"),
                         (dict(mode=L.ISTFT_REFLECT), -1, b"null plane"), (dict(mode=L.ISTFT_REFLECT, plane=base + 8, ld_plane=128), -3, b"16-byte aligned"),
                         (dict(mode=L.ISTFT_REFLECT, plane=base, ld_plane=72), -3, b"16-byte aligned")):
        got_rc, msg = call(**kw)
        assert got_rc == rc and word in msg, (kw, got_rc, msg)


def test_inference_refuses_a_generator_off_the_frame_grid(tmp_path):
    """bin/inference.build_vocoder (shared by bin/score and bin/vocoder_score): a generator that does not make 256 samples per frame is refused
    with a reason; checked on the host up to the point where the weights would go to the device"""
    import json
    from types import SimpleNamespace
    from efficient_tts_amd.bin import inference as I
    cfg = dict(IR.ISTFT_CASES["c4c4i"]["cfg"])
    (tmp_path / "c.json").write_text(json.dumps(cfg))
    torch.save({"generator": IR.fill(cfg, 3)}, tmp_path / "g.pt")
    args = SimpleNamespace(vocoder="hifigan", vocoder_config=str(tmp_path / "c.json"), vocoder_checkpoint=str(tmp_path / "g.pt"), precision="bf16x3", gl_iters=2)
    with pytest.raises(ValueError) as ei:
        I.build_vocoder(args, torch.device("cpu"))
    assert "64 samples per mel frame" in str(ei.value)
