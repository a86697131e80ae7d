"""GPU (-m gpu): the training-side and fused forward kernels off the 512-channel width.  Every test here is the body of an existing
512-channel test with the width as an argument (the helpers live beside those tests), so references, metrics and bounds are theirs:

    kernel                                      widths here                        what changes with the width
    efts_resconv5 dgrad + activation backward   256, 768                           1 / 3 column tiles (512: 2): grid = groups * ntn, the bias-part
                                                                                   table has groups * tiles * 2 rows of n floats; 4 / 12 K chunks in
                                                                                   bf16 and 8 / 24 in bf16x3 (all even: the window parity never flips);
                                                                                   the fused launch never runs on the kernel = 2 main loop
    efts_wgrad_tn_grouped / _reduce_grouped     256x256, 768x768, 128x64, 384x192  1 .. 6 row tiles of 128 outputs, 1 .. 12 column steps of 64 inputs
    efts_frame_linear                           n 128 / 256 / 768, cin 8 .. 128    1 / 2 / 6 column tiles of 128, one or two K chunks
    efts_expand, efts_pack_vt                   256, 768                           2 / 6 column tiles of 128; B * C rows of the transposed value plane

Each test prints its worst error beside its bound, or states bit equality."""
import pytest
import torch

from test_align_gpu import expand_vs_fp64_and_the_unfused_chain
from test_gpu_parity import frame_linear_equals_pack_rows_plus_gemm
from test_gpu_train import dgrad_act_launch, grouped_wgrad_against_float64

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("shape", [(3, 333), (5, 300)])
@pytest.mark.parametrize("width", [256, 768])
def test_dgrad_launch_with_the_fused_activation_backward_other_widths(width, shape, split):
    """test_dgrad_launch_with_the_fused_activation_backward at 256 and 768 channels, against efts_gemm (G') and efts_act_bwd mode 5 |
    EFTS_ACT_BWD_BIAS_PARTS (dZ plane, column sums): G' and the dZ plane bit for bit, the sum of the bias-part rows within the 512-channel
    test's 1e-4 relative + 2e-3 (the two sum the same values over different row blocks).  The table starts from a non-zero pattern and is
    followed by a canary row: every one of its efts_resconv5_bias_rows(m, n) rows is written (rows of tiles the schedule does not have
    with zeros) and nothing behind them; one row fewer is refused."""
    dgrad_act_launch(split, shape, C=width, via_gemm=True)


# (split, B, T, count, wgs, taps): taps 1 / 3 / 5, both plane formats, count 1 and 3, the automatic workgroup count (0) and a cap that
# cuts the tiles unevenly, rows that are no multiple of the step
WGRAD_CASES = ((1, 3, 333, 3, 0, 5), (2, 2, 130, 1, 0, 3), (1, 2, 90, 1, 7, 1), (2, 3, 200, 3, 24, 5), (1, 1, 7, 3, 40, 3), (2, 2, 64, 1, 7, 1))


@pytest.mark.parametrize("cout,cin", [(256, 256), (768, 768), (128, 64), (384, 192)])
def test_grouped_wgrad_other_widths_against_float64(cout, cin):
    """test_grouped_wgrad_alone_against_float64 for [cout][cin][taps] weights other than 512 x 512, down to one 128 x 64 tile per tap: weight
    norm, bias sums, float64 reference and bound as there (1e-5 / 3e-5 of the largest gradient + 1e-6: the bound follows the row count,
    which is the contraction length, not the width); every case is launched twice and must give the same bits."""
    grouped_wgrad_against_float64(WGRAD_CASES, cout=cout, cin=cin, report=True)


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("max_workgroups", [0, 3])
@pytest.mark.parametrize("cin", [8, 24, 80, 128])
@pytest.mark.parametrize("n", [128, 256, 768])
def test_frame_linear_other_widths_equal_pack_rows_plus_gemm(n, cin, max_workgroups, split):
    """test_frame_linear_equals_pack_rows_plus_gemm with n = 128 / 256 / 768 outputs (512 there) on a ragged-free 3 x 129-frame row space:
    bit for bit, without a workgroup cap and with three workgroups walking all the tiles"""
    frame_linear_equals_pack_rows_plus_gemm(split, (3, 129, cin), C=n, max_workgroups=max_workgroups)
    print(f"frame_linear n {n} cin {cin} split {split} max_workgroups {max_workgroups}: bit-equal to efts_pack_rows + efts_gemm")


@pytest.mark.parametrize("fmt", ["split2", "split1", "f32"])
@pytest.mark.parametrize("B,T1,T2", [(3, 9, 33), (2, 130, 211)])
@pytest.mark.parametrize("width", [256, 768])
def test_expand_other_widths_vs_fp64_and_the_unfused_chain(width, B, T1, T2, fmt):
    """test_expand_vs_fp64_and_the_unfused_chain (tests/test_align_gpu.py holds the float64 restatement of efts_expand, `_expand_ref64`; the
    alignment references of tests/fwd_cases.py stop at reconstruct_alignment) at 256 and 768 channels, T1 = 9 (one partial K chunk) and 130
    (five chunks, the last partial): the fused launch within 2e-5 of the output range (+ 2^-16 for the hi/lo formats) of float64 and of
    the efts_reconst_alpha + efts_pack_vt + efts_gemm chain, which runs efts_pack_vt on B * width rows"""
    expand_vs_fp64_and_the_unfused_chain(B, T1, T2, True, fmt, C=width, report=True)
