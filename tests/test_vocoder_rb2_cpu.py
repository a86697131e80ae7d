"""CPU: the `resblock: "2"` side of HiFiGANGenerator that needs no device  --  the reference's state-dict layout, the float64 restatement
(tests/vocoder_rb2_reference.py) against the golden output of the reference Generator (tests/golden/hifigan_rb2_small.npz, written by
tools/gen_golden_hifigan_rb2.py), what the constructor refuses and why, and the argument block of efts_resblock2."""
import os

import numpy as np
import pytest
import torch

import vocoder_rb2_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "hifigan_rb2_small.npz")

# state_dict of nntts.vocoders.hifigan_model.Generator for RR.GOLDEN (c0 = 64, rates (4, 2), residual kernels (3, 7)), in registration order
GOLDEN_KEYS = {
    "conv_pre.bias": (64,), "conv_pre.weight_g": (64, 1, 1), "conv_pre.weight_v": (64, 80, 7),
    "ups.0.bias": (32,), "ups.0.weight_g": (64, 1, 1), "ups.0.weight_v": (64, 32, 8),
    "ups.1.bias": (16,), "ups.1.weight_g": (32, 1, 1), "ups.1.weight_v": (32, 16, 4),
    "resblocks.0.convs.0.bias": (32,), "resblocks.0.convs.0.weight_g": (32, 1, 1), "resblocks.0.convs.0.weight_v": (32, 32, 3),
    "resblocks.0.convs.1.bias": (32,), "resblocks.0.convs.1.weight_g": (32, 1, 1), "resblocks.0.convs.1.weight_v": (32, 32, 3),
    "resblocks.1.convs.0.bias": (32,), "resblocks.1.convs.0.weight_g": (32, 1, 1), "resblocks.1.convs.0.weight_v": (32, 32, 7),
    "resblocks.1.convs.1.bias": (32,), "resblocks.1.convs.1.weight_g": (32, 1, 1), "resblocks.1.convs.1.weight_v": (32, 32, 7),
    "resblocks.2.convs.0.bias": (16,), "resblocks.2.convs.0.weight_g": (16, 1, 1), "resblocks.2.convs.0.weight_v": (16, 16, 3),
    "resblocks.2.convs.1.bias": (16,), "resblocks.2.convs.1.weight_g": (16, 1, 1), "resblocks.2.convs.1.weight_v": (16, 16, 3),
    "resblocks.3.convs.0.bias": (16,), "resblocks.3.convs.0.weight_g": (16, 1, 1), "resblocks.3.convs.0.weight_v": (16, 16, 7),
    "resblocks.3.convs.1.bias": (16,), "resblocks.3.convs.1.weight_g": (16, 1, 1), "resblocks.3.convs.1.weight_v": (16, 16, 7),
    "conv_post.bias": (1,), "conv_post.weight_g": (1, 1, 1), "conv_post.weight_v": (1, 16, 7),
}


def test_v3_configuration_constructs():
    """the published light configuration: ResBlock2, k = 7 with d = 12 (a 72-row window span) in its third block"""
    from efficient_tts_amd.vocoder import HiFiGANGenerator
    m = HiFiGANGenerator(RR.V3)
    assert m.resblock == "2" and m.fused_resblock2 is False          # the measured default (profiles/vocoder_rb2_timing.json)
    assert m.gap_frames == 5                                  # the largest single halo, (7 - 1) / 2 * 12 = 36 rows, in frames of 8 rows
    assert [type(rb).__name__ for rb in m.resblocks] == ["_ResBlock2"] * 9
    assert [(rb.convs[0].in_channels, rb.kernel_size, rb.dilation) for rb in m.resblocks] == [
        (c, k, d) for c in (128, 64, 32) for k, d in ((3, (1, 2)), (5, (2, 6)), (7, (3, 12)))]
    assert [c.padding for c in m.resblocks[2].convs] == [(9,), (36,)]
    sd = m.state_dict()
    assert list(sd.keys()) == list(RR.param_shapes(RR.V3).keys())
    assert all(tuple(v.shape) == RR.param_shapes(RR.V3)[k] for k, v in sd.items())
    # which launches run a block: every V3 block fits the fused launch; with the flag off only the k = 7, d = 12 block stays fused
    geo = [(c, k, d) for c in (128, 64, 32) for k, d in ((3, (1, 2)), (5, (2, 6)), (7, (3, 12)))]
    assert [m._rb2_fused(*g) for g in geo] == [False, False, True] * 3
    m.fused_resblock2 = True
    assert all(m._rb2_fused(*g) for g in geo)


def test_state_dict_is_the_references_for_resblock2():
    from efficient_tts_amd.vocoder import HiFiGANGenerator
    m = HiFiGANGenerator(RR.GOLDEN)
    sd = m.state_dict()
    assert list(sd.keys()) == list(GOLDEN_KEYS.keys()) == list(RR.param_shapes(RR.GOLDEN).keys())
    for k, v in sd.items():
        assert tuple(v.shape) == GOLDEN_KEYS[k] == RR.param_shapes(RR.GOLDEN)[k], k
    g = np.load(GOLD)
    assert sorted(g.files) == sorted(list(GOLDEN_KEYS) + ["mel", "audio"])
    m.load_state_dict({k: torch.from_numpy(g[k]) for k in GOLDEN_KEYS})          # the reference's state dict loads unchanged (strict)
    m.remove_weight_norm()
    assert "resblocks.3.convs.1.weight" in m.state_dict() and "resblocks.3.convs.1.weight_g" not in m.state_dict()
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 80, 4))                                                 # no CPU path


def test_float64_restatement_matches_the_reference_golden():
    """the golden audio is the REFERENCE Generator's float32 output; the float64 restatement agrees with it to float32 rounding of a
    chain of this depth, and the float32 restatement agrees with the float64 one alike -- so the golden lies within the float32
    restatement's own distance (times the factor of kernel_check) of float64"""
    g = np.load(GOLD)
    P = {k: torch.from_numpy(g[k]) for k in GOLDEN_KEYS}
    for k, v in RR.fill(RR.GOLDEN, RR.GOLDEN_SEED).items():
        assert torch.equal(v, P[k]), k                                            # the fixture's weights are the seeded fill
    mel = torch.from_numpy(g["mel"])
    assert torch.equal(mel, RR.mel_input(RR.GOLDEN, 1, RR.GOLDEN_T, RR.GOLDEN_SEED))
    y64 = RR.forward(P, mel, None, RR.GOLDEN, torch.float64)["out"]
    y32 = RR.forward(P, mel, None, RR.GOLDEN, torch.float32)["out"]
    gold = torch.from_numpy(g["audio"]).double()
    assert gold.shape == y64.shape == (1, 1, RR.GOLDEN_T * 8)
    e_gold, e32 = float((gold - y64).abs().max()), float((y32.double() - y64).abs().max())
    print(f"golden vs float64 {e_gold:.3e}; float32 restatement vs float64 {e32:.3e}; max |y| {float(y64.abs().max()):.3f}")
    assert e_gold <= max(8 * e32, 2e-6 * float(y64.abs().max()))


def test_lengths_run_the_items_alone():
    cs = RR.CASES["narrow"]
    P, mel = RR.fill(cs["cfg"], cs["seed"]), RR.mel_input(cs["cfg"], 3, cs["T"], cs["seed"])
    out = RR.forward(P, mel, cs["lengths"], cs["cfg"])
    one = RR.forward(P, mel[1:2, :, :1], None, cs["cfg"])
    assert torch.equal(out["out"][1, :, :8], one["out"][0]) and bool((out["out"][1, :, 8:] == 0).all())
    assert set(one) == {"pre", "up0", "up1", "r0.0", "r0.1", "r1.0", "r1.1", "mean0", "mean1", "out"}


_BASE = dict(resblock="2", upsample_rates=[4, 4], upsample_kernel_sizes=[8, 8], upsample_initial_channel=64,
             resblock_kernel_sizes=[3, 7], resblock_dilation_sizes=[[1, 2], [3, 12]], num_mels=80)
REFUSED = {
    "three dilations": (dict(resblock_dilation_sizes=[[1, 2], [1, 3, 5]]), "exactly dilation[0] and dilation[1]"),
    "one dilation": (dict(resblock_dilation_sizes=[[1], [3, 12]]), "exactly dilation[0] and dilation[1]"),
    "more than 128 channels with a span above 64": (dict(upsample_initial_channel=512), "efts_resblock2 takes c <= 128"),
    "halo sum above 64 with a span above 64": (dict(resblock_kernel_sizes=[3, 9], resblock_dilation_sizes=[[1, 2], [4, 13]]),
                                               "(k - 1) / 2 * (d0 + d1) <= 64"),
    "dilation 0": (dict(resblock_dilation_sizes=[[1, 0], [3, 12]]), "d >= 1"),
    "residual kernel 13": (dict(resblock_kernel_sizes=[3, 13]), "kernel size 13"),
    "resblock 3": (dict(resblock="3"), "ResBlock1 ('1') and ResBlock2 ('2')"),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_constructor_refuses_with_the_reason(what):
    from efficient_tts_amd.vocoder import HiFiGANGenerator
    change, reason = REFUSED[what]
    with pytest.raises(NotImplementedError) as e:
        HiFiGANGenerator(dict(_BASE, **change))
    assert reason in str(e.value), (what, str(e.value))


def test_constructor_accepts_what_one_of_the_two_paths_can_run():
    from efficient_tts_amd.vocoder import HiFiGANGenerator, _refusal
    HiFiGANGenerator(_BASE)
    for cs in RR.CASES.values():
        HiFiGANGenerator(cs["cfg"])
    # more than 128 channels is fine while two efts_gemm launches can run every block (spans up to 64 rows) ...
    m = HiFiGANGenerator(dict(_BASE, upsample_initial_channel=512, resblock_dilation_sizes=[[1, 2], [3, 10]]))
    m.fused_resblock2 = True
    assert not m._rb2_fused(256, 7, (3, 10)) and m._rb2_fused(128, 7, (3, 10))
    # ... and a halo sum above 64 likewise: k = 11, d = (6, 6) has spans of 60 rows and a halo sum of 60; k = 11, d = (6, 7) is beyond both
    assert _refusal((4, 4), (8, 8), (11,), ((6, 6),), 64, 80, "2") is None
    assert "(k - 1) / 2 * (d0 + d1) <= 64" in _refusal((4, 4), (8, 8), (11,), ((6, 7),), 64, 80, "2")
    # the limit case sits exactly on the halo limit
    assert HiFiGANGenerator(RR.CASES["limit"]["cfg"]).gap_frames == 12


def test_each_block_kind_owns_its_packed_names_and_its_refusals():
    """what depends on the kind lives in the block classes: the packed names in launch order (`packed`) are the lists the generator
    used to write out itself, and `_refusal` says about a block exactly what the block's class says (`refusal`)"""
    import vocoder_reference as VR
    from efficient_tts_amd.vocoder import HiFiGANGenerator, _refusal, _ResBlock1, _ResBlock2

    def names(m):
        return [name for n, rb in enumerate(m.resblocks) for name, _ in rb.packed(n)]
    v1, v3 = HiFiGANGenerator(VR.V1), HiFiGANGenerator(RR.V3)
    assert names(v1)[:18] == ["rb0.c1.0", "rb0.c2.0", "rb0.c1.1", "rb0.c2.1", "rb0.c1.2", "rb0.c2.2",
                              "rb1.c1.0", "rb1.c2.0", "rb1.c1.1", "rb1.c2.1", "rb1.c1.2", "rb1.c2.2",
                              "rb2.c1.0", "rb2.c2.0", "rb2.c1.1", "rb2.c2.1", "rb2.c1.2", "rb2.c2.2"]          # the first stage
    assert len(names(v1)) == len(set(names(v1))) == 72 and names(v1)[-1] == "rb11.c2.2"                        # 4 stages x 3 blocks x 3 pairs
    assert names(v3)[:6] == ["rb0.c.0", "rb0.c.1", "rb1.c.0", "rb1.c.1", "rb2.c.0", "rb2.c.1"]                 # the first stage
    assert len(names(v3)) == len(set(names(v3))) == 18 and names(v3)[-1] == "rb8.c.1"                          # 3 stages x 3 blocks x 2 turns
    rb = v1.resblocks[4]
    assert [id(m) for _, m in rb.packed(4)] == [id(m) for d in range(3) for m in (rb.convs1[d], rb.convs2[d])]
    assert [id(m) for _, m in v3.resblocks[5].packed(5)] == [id(m) for m in v3.resblocks[5].convs]

    def through_the_class(cfg, cls):
        c_max = cfg["upsample_initial_channel"] // 2
        return next((w for w in (cls.refusal(k, tuple(ds), c_max) for k, ds in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]))
                     if w is not None), None)

    def whole(cfg):
        return _refusal(tuple(cfg["upsample_rates"]), tuple(cfg["upsample_kernel_sizes"]), tuple(cfg["resblock_kernel_sizes"]),
                        tuple(tuple(d) for d in cfg["resblock_dilation_sizes"]), cfg["upsample_initial_channel"], cfg["num_mels"], cfg["resblock"])
    for what, (change, reason) in REFUSED.items():
        cfg = dict(_BASE, **change)
        assert reason in whole(cfg), what
        if what not in ("residual kernel 13", "resblock 3"):           # (those two are refused before a block class is asked)
            assert reason in through_the_class(cfg, _ResBlock2) and through_the_class(cfg, _ResBlock2) == whole(cfg), what
    for cfg in [_BASE] + [cs["cfg"] for cs in RR.CASES.values()]:
        assert whole(cfg) is None and through_the_class(cfg, _ResBlock2) is None
    for cfg in [VR.V1] + [cs["cfg"] for cs in VR.CASES.values()]:
        assert whole(cfg) is None and through_the_class(cfg, _ResBlock1) is None
    assert _ResBlock2.refusal(11, (6, 6), 32) is None and "(k - 1) / 2 * (d0 + d1) <= 64" in _ResBlock2.refusal(11, (6, 7), 32)
    assert "(k - 1) * d <= 64 rows" in _ResBlock1.refusal(11, (1, 7), 256) and "d >= 1" in _ResBlock1.refusal(3, (1, 0), 256)
    assert _ResBlock1.refusal(7, (3, 12), 256) == whole(dict(VR.V1, resblock_kernel_sizes=[7], resblock_dilation_sizes=[[3, 12]]))


def test_resblock2_args_layout_and_argument_errors():
    """sizeof / offsets of efts_resblock2_args as compiled by gcc == the ctypes mirror, and the entry refuses bad arguments before any launch"""
    import ctypes
    import subprocess
    import tempfile
    from efficient_tts_amd import build as B
    from efficient_tts_amd import lib as L
    fields = [f for f, _ in L.ResBlock2Args._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "efts_abi.h"\nint main(){\nprintf(" %zu", sizeof(efts_resblock2_args));' +
           "".join(f'printf(" %zu", offsetof(efts_resblock2_args, {f}));' for f in fields) + "return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got == [ctypes.sizeof(L.ResBlock2Args)] + [getattr(L.ResBlock2Args, f).offset for f in fields]
    B.build(verbose=False)
    lib = L.load()
    assert lib.efts_resblock2(None, None) == -1 and b"null args" in lib.efts_last_error()
    g = L.ResBlock2Args()
    g.x = g.p0 = g.w0 = g.w1 = g.out = 4096
    g.split, g.m, g.c, g.k, g.d0, g.d1, g.ldx, g.ldo, g.ldp, g.ldw, g.w_tap_stride = 2, 100, 32, 7, 3, 12, 32, 32, 128, 128, 32 * 128

    def rc(**kw):
        h = L.ResBlock2Args.from_buffer_copy(g)
        for k, v in kw.items():
            setattr(h, k, v)
        return lib.efts_resblock2(ctypes.byref(h), None), lib.efts_last_error()
    assert rc(reserved=1)[0] == -1 and rc(d0=65)[0] == -2 and b"1 .. 64" in rc(d0=65)[1]
    assert rc(split=4)[0] == -1 and rc(k=4)[0] == -1 and rc(k=13)[0] == -1 and rc(x=None)[0] == -1
    assert rc(m=0)[0] == -2 and rc(c=132, ldx=132, ldo=132, ldp=640, ldw=640, w_tap_stride=132 * 640)[0] == -2 and rc(c=30)[0] == -2
    assert rc(d0=0)[0] == -2 and rc(ldp=64)[0] == -2 and rc(ldx=28)[0] == -2
    code, msg = rc(d1=19)                                       # 3 * (3 + 19) = 66 rows
    assert code == -2 and b"must not exceed 64" in msg
    assert rc(out=4100)[0] == -3 and rc(ldo=34)[0] == -3 and rc(ldp=136)[0] == -3
