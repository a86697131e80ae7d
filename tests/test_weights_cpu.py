"""WeightPlanes (efficient_tts_amd/weights.py), the owner of the packed weight planes, on the CPU: a stub library records the grouped
repack launches (`efts_pack_weights_grouped`) instead of running them, so the lifecycle -- when a repack happens, when it counts as
done, what a failure leaves behind -- and the launches themselves are checked without a GPU."""
import ctypes as C
import gc
import weakref

import pytest
import torch

from efficient_tts_amd import lib as L, ops as O
from efficient_tts_amd.model import EfficientTTSCNN
from efficient_tts_amd.train import TrainEngine

CONFIGS = {
    "a": dict(num_symbols=12, n_channels=256, symbol_embedding_dim=256, n_text_encoder_layer=2, n_mel_encoder_layer=1,
              n_decoder_layer=2, dropout_rate=0.0),
    # 7 taps: the text / mel stacks take the row pack kernels, which read a folded fp32 copy; query fc, shared key / value, bf16
    "b": dict(num_symbols=12, n_channels=256, symbol_embedding_dim=256, n_text_encoder_layer=1, n_mel_encoder_layer=2,
              n_decoder_layer=1, k_size=7, use_mel_query_fc=True, share_text_encoder_key_value=True, precision="bf16",
              dropout_rate=0.0),
}

# The launches the model enqueued before WeightPlanes existed (EfficientTTSCNN._weights, recorded with the same stub): per launch
# (phase, items, ld, ld_t, cout, cin, taps, split, with_t, item rows), a row named by its columns (weight parameter, weight-norm gain,
# folded fp32 copy, forward plane, dgrad plane).  "eager": the first eval repack; "phased": the training engine's repack after it.
EXPECTED = {
    "a": {
        "eager": [
            (None, 5, 1024, 0, 256, 256, 5, 2, 0, (
                ("text_encoder.layers.0.conv.0.weight_v", "text_encoder.layers.0.conv.0.weight_g", None, "text_encoder.0", None),
                ("text_encoder.layers.1.conv.0.weight_v", "text_encoder.layers.1.conv.0.weight_g", None, "text_encoder.1", None),
                ("mel_encoder.layers.0.conv.0.weight_v", "mel_encoder.layers.0.conv.0.weight_g", None, "mel_encoder.0", None),
                ("decoder.layers.0.conv.0.weight_v", "decoder.layers.0.conv.0.weight_g", None, "decoder.0", None),
                ("decoder.layers.1.conv.0.weight_v", "decoder.layers.1.conv.0.weight_g", None, "decoder.1", None),
            )),
            (None, 2, 1024, 0, 256, 256, 3, 2, 0, (
                ("duration_predictor.conv.0.0.weight", None, None, "dur.0", None),
                ("duration_predictor.conv.1.0.weight", None, None, "dur.1", None),
            )),
            (None, 2, 1024, 0, 256, 256, 1, 2, 0, (
                ("text_encoder_key.weight", None, None, "key", None),
                ("text_encoder_value.weight", None, None, "value", None),
            )),
            (None, 1, 384, 0, 256, 80, 1, 2, 0, (
                ("mel_prenet.0.weight", None, None, "prenet", None),
            )),
            (None, 1, 1024, 0, 80, 256, 1, 2, 0, (
                ("mel_output_layer.weight", None, None, "head", None),
            )),
        ],
        "phased": [
            ("me", 3, 1024, 1024, 256, 256, 5, 2, 1, (
                ("mel_encoder.layers.0.conv.0.weight_v", "mel_encoder.layers.0.conv.0.weight_g", None, "mel_encoder.0", "mel_encoder.0"),
                ("decoder.layers.0.conv.0.weight_v", "decoder.layers.0.conv.0.weight_g", None, "decoder.0", "decoder.0"),
                ("decoder.layers.1.conv.0.weight_v", "decoder.layers.1.conv.0.weight_g", None, "decoder.1", "decoder.1"),
            )),
            ("me", 1, 384, 0, 256, 80, 1, 2, 0, (
                ("mel_prenet.0.weight", None, None, "prenet", None),
            )),
            ("me", 1, 1024, 384, 80, 256, 1, 2, 1, (
                ("mel_output_layer.weight", None, None, "head", "head"),
            )),
            ("te", 2, 1024, 1024, 256, 256, 5, 2, 1, (
                ("text_encoder.layers.0.conv.0.weight_v", "text_encoder.layers.0.conv.0.weight_g", None, "text_encoder.0", "text_encoder.0"),
                ("text_encoder.layers.1.conv.0.weight_v", "text_encoder.layers.1.conv.0.weight_g", None, "text_encoder.1", "text_encoder.1"),
            )),
            ("te", 2, 1024, 1024, 256, 256, 3, 2, 1, (
                ("duration_predictor.conv.0.0.weight", None, None, "dur.0", "dur.0"),
                ("duration_predictor.conv.1.0.weight", None, None, "dur.1", "dur.1"),
            )),
            ("te", 2, 1024, 1024, 256, 256, 1, 2, 1, (
                ("text_encoder_key.weight", None, None, "key", "key"),
                ("text_encoder_value.weight", None, None, "value", "value"),
            )),
        ],
    },
    "b": {
        "eager": [
            (None, 4, 512, 0, 256, 256, 7, 1, 0, (
                ("text_encoder.layers.0.conv.0.weight_v", "text_encoder.layers.0.conv.0.weight_g", None, "text_encoder.0", None),
                ("mel_encoder.layers.0.conv.0.weight_v", "mel_encoder.layers.0.conv.0.weight_g", None, "mel_encoder.0", None),
                ("mel_encoder.layers.1.conv.0.weight_v", "mel_encoder.layers.1.conv.0.weight_g", None, "mel_encoder.1", None),
                ("decoder.layers.0.conv.0.weight_v", "decoder.layers.0.conv.0.weight_g", None, "decoder.0", None),
            )),
            (None, 2, 512, 0, 256, 256, 3, 1, 0, (
                ("duration_predictor.conv.0.0.weight", None, None, "dur.0", None),
                ("duration_predictor.conv.1.0.weight", None, None, "dur.1", None),
            )),
            (None, 2, 512, 0, 256, 256, 1, 1, 0, (
                ("text_encoder_key.weight", None, None, "key", None),
                ("mel_query_fc.weight", None, None, "qfc", None),
            )),
            (None, 1, 256, 0, 256, 80, 1, 1, 0, (
                ("mel_prenet.0.weight", None, None, "prenet", None),
            )),
            (None, 1, 512, 0, 80, 256, 1, 1, 0, (
                ("mel_output_layer.weight", None, None, "head", None),
            )),
        ],
        "phased": [
            ("me", 3, 512, 512, 256, 256, 7, 1, 1, (
                ("mel_encoder.layers.0.conv.0.weight_v", "mel_encoder.layers.0.conv.0.weight_g", "mel_encoder.0", "mel_encoder.0", "mel_encoder.0"),
                ("mel_encoder.layers.1.conv.0.weight_v", "mel_encoder.layers.1.conv.0.weight_g", "mel_encoder.1", "mel_encoder.1", "mel_encoder.1"),
                ("decoder.layers.0.conv.0.weight_v", "decoder.layers.0.conv.0.weight_g", "decoder.0", "decoder.0", "decoder.0"),
            )),
            ("me", 1, 256, 0, 256, 80, 1, 1, 0, (
                ("mel_prenet.0.weight", None, None, "prenet", None),
            )),
            ("me", 1, 512, 256, 80, 256, 1, 1, 1, (
                ("mel_output_layer.weight", None, None, "head", "head"),
            )),
            ("me", 1, 512, 512, 256, 256, 1, 1, 1, (
                ("mel_query_fc.weight", None, None, "qfc", "qfc"),
            )),
            ("te", 1, 512, 512, 256, 256, 7, 1, 1, (
                ("text_encoder.layers.0.conv.0.weight_v", "text_encoder.layers.0.conv.0.weight_g", "text_encoder.0", "text_encoder.0", "text_encoder.0"),
            )),
            ("te", 2, 512, 512, 256, 256, 3, 1, 1, (
                ("duration_predictor.conv.0.0.weight", None, None, "dur.0", "dur.0"),
                ("duration_predictor.conv.1.0.weight", None, None, "dur.1", "dur.1"),
            )),
            ("te", 1, 512, 512, 256, 256, 1, 1, 1, (
                ("text_encoder_key.weight", None, None, "key", "key"),
            )),
        ],
    },
}


class _StubLib:
    def __init__(self):
        self.calls, self.phase, self.rc = [], None, 0

    def efts_pack_weights_grouped(self, table, n, scale, ld, ld_t, cout, cin, taps, split, with_t, stream):
        rows = list((C.c_int64 * (5 * n)).from_address(table))
        self.calls.append((self.phase, n, ld, ld_t, cout, cin, taps, split, with_t, [tuple(rows[5 * i:5 * i + 5]) for i in range(n)]))
        return self.rc

    def efts_last_error(self):
        return b"stub failure"


@pytest.fixture
def stub(monkeypatch):
    lib = _StubLib()
    monkeypatch.setattr(L, "load", lambda: lib)
    monkeypatch.setattr(O, "_stream", lambda: 0)
    return lib


def _model(cfg="a"):
    torch.manual_seed(0)
    m = EfficientTTSCNN(**CONFIGS[cfg])
    return m, TrainEngine(m)


def _issue(m, stub, *phases):
    for ph in phases:
        stub.phase = ph
        m.planes.issue(ph)
    stub.phase = None


def _train_repack(m, eng, stub):
    eng._prepare_weights()
    _issue(m, stub, "me", "te")


def _named(m, eng, calls):
    prm = {p.data_ptr(): n for n, p in m.named_parameters()}
    cols = (prm, prm, {t.data_ptr(): n for n, t in eng.folded.items()}, {w.ptr: n for n, w in m.planes.packed.items()},
            {w.ptr: n for n, w in eng.wt.items()})
    return [c[:9] + (tuple(tuple(None if a == 0 else col[a] for a, col in zip(r, cols)) for r in c[9]),) for c in calls]


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_repack_launches_are_the_recorded_ones(stub, cfg):
    m, eng = _model(cfg)
    m.planes.get(m)
    eager = list(stub.calls)
    stub.calls.clear()
    _train_repack(m, eng, stub)
    assert _named(m, eng, eager) == EXPECTED[cfg]["eager"]
    assert _named(m, eng, stub.calls) == EXPECTED[cfg]["phased"]


def test_a_phased_repack_counts_only_once_its_last_phase_is_issued(stub):
    m, eng = _model()
    gen = m.planes.gen
    eng._prepare_weights()
    assert stub.calls == [] and m.planes.gen == gen                # scheduled: nothing launched yet
    _issue(m, stub, "me")
    assert m.planes.gen == gen and {c[0] for c in stub.calls} == {"me"}
    with pytest.raises(RuntimeError):
        m.planes.get(m)                                            # ("te" is still pending)
    _issue(m, stub, "te")
    assert m.planes.gen == gen + 1
    stub.calls.clear()
    m.planes.get(m)
    _train_repack(m, eng, stub)
    assert stub.calls == [] and m.planes.gen == gen + 1            # current: neither path repacks


@pytest.mark.parametrize("then", ["get", "schedule"])
def test_a_failure_between_schedule_and_the_last_issue_leaves_the_planes_stale(stub, then):
    m, eng = _model()
    _train_repack(m, eng, stub)
    gen = m.planes.gen
    m.planes.invalidate()
    eng._prepare_weights()
    stub.rc = 1
    with pytest.raises(L.EftsError):
        _issue(m, stub, "me")
    stub.rc = 0
    assert m.planes.gen == gen
    stub.calls.clear()
    if then == "get":
        m.planes.get(m)
    else:
        _train_repack(m, eng, stub)
    assert stub.calls and m.planes.gen == gen + 1                  # repacked


def test_a_second_schedule_and_an_unknown_phase_raise(stub):
    m, eng = _model()
    eng._prepare_weights()
    with pytest.raises(RuntimeError):
        eng._prepare_weights()
    _issue(m, stub, "me", "te")                                    # the first schedule is intact
    m.planes.invalidate()
    eng._prepare_weights()
    with pytest.raises(ValueError):
        m.planes.issue("mel")
    stub.calls.clear()
    m.planes.get(m)                                                # (the abandoned repack left the planes stale)
    assert stub.calls


def test_invalidate_forces_a_repack(stub):
    m, eng = _model()
    m.planes.get(m)
    n = len(stub.calls)
    m.planes.get(m)
    assert len(stub.calls) == n
    m.planes.invalidate()
    m.planes.get(m)
    assert len(stub.calls) == 2 * n
    _train_repack(m, eng, stub)
    stub.calls.clear()
    m.planes.invalidate()
    _train_repack(m, eng, stub)
    assert {c[0] for c in stub.calls} == {"me", "te"}


def test_the_training_repack_follows_an_eager_one(stub):
    """parameters unchanged, but the eval repack did not write the training engine's folded and dgrad copies: the next training
    repack must"""
    m, eng = _model("b")
    m.planes.get(m)
    stub.calls.clear()
    _train_repack(m, eng, stub)
    assert len(stub.calls) == len(EXPECTED["b"]["phased"])
    stub.calls.clear()
    m.planes.get(m)                                                # (the training repack wrote the forward planes too)
    _train_repack(m, eng, stub)
    assert stub.calls == []


def test_the_tag_changes_with_the_planes_and_the_parameter_storages(stub):
    m, eng = _model()
    m.planes.get(m)
    tag = m.planes.tag()
    m.planes.invalidate()
    assert m.planes.tag() == tag                                   # (a captured step invalidates after every replay)
    _train_repack(m, eng, stub)
    with torch.no_grad():
        m.mel_output_layer.weight.add_(1.0)                        # in place: same storage
    stub.calls.clear()
    m.planes.get(m)
    assert stub.calls and m.planes.tag() == tag
    head = m.mel_output_layer.weight
    head.data = head.data.clone()                                  # new storage
    assert m.planes.tag() == tag                                   # (not before the repack)
    m.planes.get(m)
    tag2 = m.planes.tag()
    assert tag2 != tag
    m.planes.packed.pop("head")                                    # the plane is re-created by the next repack
    m.planes.invalidate()
    m.planes.get(m)
    assert m.planes.tag() != tag2


def test_a_model_is_freed_without_the_cyclic_collector(stub):
    """the planes hold no reference to their model: a model left to the cyclic garbage collector is freed at whatever allocation
    triggers a collection, which may fall inside another model's graph capture"""
    m, eng = _model()
    _train_repack(m, eng, stub)
    m.planes.get(m)
    ref = weakref.ref(m)
    gc.collect()
    gc.disable()
    try:
        del m, eng
        assert ref() is None
    finally:
        gc.enable()


@pytest.mark.parametrize("k", [1, 2, 3])
def test_the_engine_refuses_a_duration_predictor_it_cannot_train(k):
    """the training step is written out for two duration-predictor layers: another depth is refused when the engine is built, by name,
    instead of an IndexError deep in the step (one layer) or a third layer that silently gets a zero gradient"""
    torch.manual_seed(0)
    m = EfficientTTSCNN(**CONFIGS["a"], n_duration_layer=k)
    if k == 2:
        assert TrainEngine(m).last is None
    else:
        with pytest.raises(NotImplementedError, match="n_duration_layer"):
            TrainEngine(m)
