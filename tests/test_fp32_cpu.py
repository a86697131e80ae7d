"""CPU: precision="fp32" (operand format 3) -- construction, routing, and the refusals that need no device: every entry point without
an fp32 form rejects format 3 before any launch, and training refuses an fp32 model."""
import pytest

from efficient_tts_amd import build as B
from efficient_tts_amd import lib as L

HIFIGAN_V1 = dict(resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
                  resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], num_mels=80)


@pytest.fixture(scope="module")
def lib():
    B.build(verbose=False)
    return L.load()


@pytest.fixture(scope="module")
def model():
    from efficient_tts_amd import EfficientTTSCNN
    return EfficientTTSCNN(num_symbols=76, precision="fp32")


def test_format3_is_named_in_the_abi():
    assert (L.SPLIT_BF16, L.SPLIT_BF16X3, L.SPLIT_FP32) == (1, 2, 3)
    assert L.ABI_VERSION == 602


def test_fp32_models_construct_with_generic_routing(model):
    from efficient_tts_amd.model import FP32_GENERIC_OPTIONS
    from efficient_tts_amd.vocoder import HiFiGANGenerator
    assert model.precision == "fp32" and model.split == 3 and model.align_split == 3
    for name in FP32_GENERIC_OPTIONS:
        assert getattr(model, name) is False, name
    gen = HiFiGANGenerator(HIFIGAN_V1, precision="fp32")
    assert gen.split == 3


@pytest.mark.parametrize("name", ["resconv", "fuse_prenet", "fuse_expand", "embed_conv", "small_m"])
def test_fused_options_refuse_fp32(model, name):
    with pytest.raises(ValueError, match=name):
        setattr(model, name, True)
    setattr(model, name, False)                      # (turning it off is allowed)
    assert getattr(model, name) is False


def test_other_precisions_keep_their_fused_defaults():
    from efficient_tts_amd import EfficientTTSCNN
    m = EfficientTTSCNN(num_symbols=76, precision="bf16x3")
    assert m.resconv and m.fuse_prenet and m.fuse_expand and m.embed_conv and m.small_m and m.align_split == 2
    m.resconv = False
    m.resconv = True


def test_unknown_precision_is_refused():
    from efficient_tts_amd import EfficientTTSCNN
    from efficient_tts_amd.vocoder import HiFiGANGenerator
    with pytest.raises(ValueError):
        EfficientTTSCNN(num_symbols=76, precision="fp16")
    with pytest.raises(ValueError):
        HiFiGANGenerator(HIFIGAN_V1, precision="fp16")


def _gemm_args(split, tiling):
    g = L.GemmArgs()
    g.a, g.b, g.lda, g.ldb = 4096, 8192, 128, 128           # never dereferenced: the refusals come before any launch
    g.split, g.taps, g.m, g.n, g.nchunk, g.batch = split, 5, 256, 128, 1, 1
    g.out_f32, g.ldo = 16384, 128
    g.tiling = tiling
    return g


@pytest.mark.parametrize("tiling", [L.TILING_WIDE, L.TILING_NARROW, L.TILING_RESIDENT, L.TILING_SMALLM])
def test_gemm_format3_refuses_the_other_tilings(lib, tiling):
    assert lib.efts_gemm(_gemm_args(3, tiling), None) == -1          # EFTS_EINVAL, no fallback
    assert b"split 3" in lib.efts_last_error()


def test_gemm_unknown_format_still_refused(lib):
    for split in (0, 4):
        assert lib.efts_gemm(_gemm_args(split, L.TILING_AUTO), None) == -1
        assert b"split" in lib.efts_last_error()
    g = _gemm_args(3, L.TILING_AUTO)
    g.out_bf16, g.ldob, g.out_split = 32768, 128, 4
    assert lib.efts_gemm(g, None) == -1 and b"out_split" in lib.efts_last_error()
    g.out_split = 2                                              # a format-3 contraction writes fp32 planes only
    assert lib.efts_gemm(g, None) == -1 and b"out_split" in lib.efts_last_error()


def test_resconv5_refuses_format3(lib):
    for multi in (False, True):
        r = L.ResConv5Args()
        r.x, r.ldx, r.w, r.ldw, r.w_tap_stride = 4096, 128, 8192, 128, 256 * 128
        r.split, r.m, r.n, r.nchunk, r.slope = 3, 256, 256, 1, 0.1
        r.y_f32, r.ldo = 16384, 256
        rc = lib.efts_resconv5_multi((L.ResConv5Args * 1)(r), 1, None) if multi else lib.efts_resconv5(r, None)
        assert rc == -1
        assert b"split" in lib.efts_last_error()


def test_fused_and_training_entry_points_refuse_format3(lib):
    f = L.FrameLinearArgs()
    f.x, f.w, f.split, f.B, f.n, f.y_f32 = 4096, 8192, 3, 1, 128, 16384
    assert lib.efts_frame_linear(f, None) == -1 and b"split" in lib.efts_last_error()
    e = L.ExpandArgs()
    e.e, e.v, e.B, e.T1, e.T1p, e.T2, e.T2p, e.n, e.y, e.y_split = 4096, 8192, 1, 8, 10, 16, 18, 128, 16384, 3
    assert lib.efts_expand(e, None) == -1 and b"split" in lib.efts_last_error()
    assert lib.efts_embed_conv(4096, None, 8192, 16384, None, 0.1, 32768, 65536, 128, 1, 4, 6, 128, 76, 5, 3, None) == -1
    assert b"split" in lib.efts_last_error()
    # efts_resconv5 with the residual taken from planes that hold fewer than n columns (nchunk * 64 in bf16, nchunk * 32 in bf16x3): EFTS_ESHAPE,
    # while the same shape with an fp32 residual stream or without the residual term passes the checks (tests/test_resconv_gpu.py runs those)
    for split, nchunk in ((1, 3), (2, 6), (1, 1), (2, 7)):
        r = L.ResConv5Args()
        r.x, r.ldx, r.w, r.ldw, r.w_tap_stride = 4096, nchunk * 128, 8192, nchunk * 128, 256 * nchunk * 128
        r.split, r.m, r.n, r.nchunk, r.slope = split, 256, 256, nchunk, 0.1
        r.y_f32, r.ldo = 16384, 256
        for rc in (lib.efts_resconv5(r, None), lib.efts_resconv5_multi((L.ResConv5Args * 1)(r), 1, None)):
            assert rc == -2 and b"residual from the planes" in lib.efts_last_error() and b"fewer than n = 256" in lib.efts_last_error()
    assert lib.efts_pack_weight_t(4096, 8192, 2048, 512, 512, 5, 3, None) == -1 and b"split" in lib.efts_last_error()
    assert lib.efts_pack_weights_grouped(4096, 1, None, 2048, 2048, 512, 512, 5, 3, 1, None) == -1 and b"split" in lib.efts_last_error()
    assert lib.efts_pack_t(4096, 512, 8192, 256, 0, 3, 64, 512, -2, 5, 64, None) == -1 and b"split" in lib.efts_last_error()
    assert lib.efts_act_grad(4096, 8192, None, 1, 0.1, 0.0, None, 16384, 128, 3, None, 8, 32, 0.0, 0, None) == -1
    assert b"split" in lib.efts_last_error()
    for fn in ("efts_reconst_alpha", "efts_pack_vt"):
        args = ((4096, None, None, 0.01, None, 8192, 128, 1, 8, 8, 10, 1, None) if fn == "efts_reconst_alpha"
                else (4096, 128, 8192, 128, 1, 8, 10, 128, 1, None))
        assert getattr(lib, fn)(*args) == -1 and b"split" in lib.efts_last_error()      # (format 1 has no form there either)


def test_training_refuses_an_fp32_model(model):
    from efficient_tts_amd.optim import EftsAdam
    from efficient_tts_amd.train import TrainEngine
    from efficient_tts_amd.trainer import EfficientTTSTrainer
    with pytest.raises(NotImplementedError, match="bf16x3"):
        TrainEngine(model)
    with pytest.raises(NotImplementedError, match="bf16x3"):
        EftsAdam(model)
    with pytest.raises(NotImplementedError, match="bf16x3"):
        EfficientTTSTrainer(1, 1, None, None, model, None, None, {"outdir": "unused"})


def test_inference_cli_accepts_fp32():
    from efficient_tts_amd.bin.inference import get_parser
    a = get_parser().parse_args(["--checkpoint", "c.pkl", "--test_fid_scp", "t.scp", "--outdir", "o", "--precision", "fp32"])
    assert a.precision == "fp32"
