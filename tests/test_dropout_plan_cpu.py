"""The mask family of train-mode Dropout (efficient_tts_amd/dropout.py): pure arithmetic, no device.  The expected seeds were worked out
from the formulas as they stood before the plan existed (model._dropout_base / _dropout_seeds, TrainEngine._begin_step,
GraphedStep._refresh), not from the code under test."""
import pytest

from efficient_tts_amd import dropout as D

M = 0xFFFFFFFF
KS = (10, 24, 32, 40)            # text-encoder layer 0, mel-encoder layer 4, decoder layer 2, the prenet


def _plan(seed, rank, step, conv_p=0.1, ptr=None):
    return D.DropoutPlan(conv_p, 0.1, D.rank_base(seed, rank), step, ptr)


def _dur_seeds(p):
    return [p.dur(i)[1] for i in (0, 1)]


def test_launch_indices():
    assert D.LAUNCH == dict(te=10, me=20, dec=30, prenet=40, other=50)


@pytest.mark.parametrize("seed, rank, step, base, conv, dur", [
    (0x5EED, 0, 7, 0x5EED, (3631668289, 3631779155, 3631842507, 3631905859), [24315, 24316]),
    (0x5EED, 3, 7, 3668364288, (3626713444, 3626824310, 3626887662, 3626951014), [3668364302, 3668364303]),
    (0xFFFFFFF0, 0, 9, 0xFFFFFFF0, (None, None, None, 488029916), [2, 3]),                       # the sums wrap at 2^32
])
def test_seeds_of_a_step(seed, rank, step, base, conv, dur):
    p = _plan(seed, rank, step)
    assert D.rank_base(seed, rank) == p.base == base
    for k, want in zip(KS, conv):
        if want is not None:
            assert p.conv(k) == (0.1, want)
    assert _dur_seeds(p) == dur
    assert [p.dur(i) for i in (0, 1, 2, 3)] == [(0.1, (dur[0] + d) & M, None) for d in (0, 1, 3, 4)]     # beyond two layers: seed1 + i
    assert p.conv_active


@pytest.mark.parametrize("step", [1, 9, 2 ** 31 + 5])
@pytest.mark.parametrize("seed, rank", [(0x5EED, 0), (0x5EED, 3), (0xFFFFFFF0, 0)])
def test_captured_seeds_plus_the_step_word_are_the_eager_seeds(seed, rank, step):
    """A captured step passes seeds without the step's share and the address of a device word that holds it.  efts_layernorm_rows /
    _dot (csrc/efts_ops.hip, layernorm kernel) and efts_layernorm_bwd (csrc/efts_train.hip) take `hash_u32(drop_seed + *seed_add)`
    with both operands `unsigned`: a plain 32-bit unsigned add, which wraps modulo 2^32 (and the word is stored as 32 bits)."""
    eager, cap = _plan(seed, rank, step), _plan(seed, rank, step, ptr=0x1000)
    for i in (0, 1):
        p_, s_, ptr = cap.dur(i)
        assert (p_, ptr) == (0.1, 0x1000) and eager.dur(i)[2] is None
        assert (s_ + D.DropoutPlan.step_word(step)) % 2 ** 32 == eager.dur(i)[1]
        assert s_ == (D.rank_base(seed, rank) + i) & M                       # constant from step to step: the graph's launches keep it
    assert D.DropoutPlan.step_word(step) == 2 * step
    assert cap.conv(40) == eager.conv(40)                                    # by value in both forms


def test_without_conv_dropout():
    p, q = _plan(0x5EED, 0, 7, conv_p=0.0), _plan(0x5EED, 0, 7)
    assert all(p.conv(k) == (0.0, 0) for k in KS) and not p.conv_active
    assert _dur_seeds(p) == _dur_seeds(q) == [24315, 24316] and p.dur(0)[0] == 0.1
    assert D.NONE.conv(40) == (0.0, 0) and not D.NONE.conv_active and D.NONE.dur(0) == D.NONE.dur(1) == (0.0, 0, None)


def test_probes_do_not_move_the_sequence_and_steps_do():
    from efficient_tts_amd import EfficientTTSCNN
    m = EfficientTTSCNN(num_symbols=76, use_masking=True)                    # dropout_rate 0.1, train() mode, never forwarded
    assert (m.dropout_calls, m.dropout_seed) == (0, 0x5EED)
    m.dropout_calls = 5
    assert [m.probe_dropout().calls for _ in range(2)] == [6, 7] and m.dropout_calls == 5
    m.dropout_calls = 6                                                      # a real step has moved the sequence: the probes start over
    probe = m.probe_dropout()
    assert probe.calls == 7 and m.dropout_calls == 6
    step = m.step_dropout()
    assert step.calls == 7 and m.dropout_calls == 7 and step == probe       # a probe draws the masks of the step that comes next
    assert step == D.DropoutPlan(0.1, 0.1, 0x5EED, 7) and step.step_word_ptr is None
    assert m.step_dropout(0x2000) == D.DropoutPlan(0.1, 0.1, 0x5EED, 8, 0x2000) and m.dropout_calls == 8
    m.eval()                                                                 # the engine still counts the step; nothing is dropped
    assert m.step_dropout() == D.DropoutPlan(0.0, 0.0, 0x5EED, 9)
