"""GPU (-m gpu): every buffer a HiFi-GAN forward writes holds, bit for bit, what the commit named in tests/golden/vocoder_digests.json wrote.

The host driver of efficient_tts_amd/vocoder.py only issues launches; a change of the driver that is meant to keep the launches -- splitting it
into stages, moving a block kind's launches into its class -- keeps these bits, and equal bits are the proof, not a tolerance.  An entry is one
eager forward (`graphs = False`) with `keep={}`: the sha256 of every kept buffer (whole, guard rows included) and of the returned audio, and
the value of "pitch".  Entries: every case of vocoder_reference.CASES (ResBlock1) and every case of vocoder_rb2_reference.CASES (ResBlock2)
with `fused_resblock2` True and False, each in the three precisions: 39 forward passes at the stage tests' own shapes.
The same recorded bits must come out with `branch_streams = False` (the chains of a stage in a row on one stream), and a hipGraph replay
returns the audio of the eager run.

Re-recording.  After a DELIBERATE change of a kernel's results, record again from the changed commit once its stage tests pass
(`python tests/record_vocoder_digests.py <commit>`).  For a change that must not alter a bit, the file is recorded at the PARENT commit, in a
checkout of the parent with its own library built, never from the changed code: tests/record_vocoder_digests.py uses nothing but
`HiFiGANGenerator(cfg, precision)`, `load_state_dict`, `graphs`, `fused_resblock2` and `forward(mel, lengths, keep={})`.
"""
import hashlib
import json
import os

import pytest
import torch

import vocoder_rb2_reference as RR
import vocoder_reference as VR

pytestmark = pytest.mark.gpu

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocoder_digests.json")
PRECISIONS = ("fp32", "bf16x3", "bf16")
# (entry name, reference module, case, precision, fused_resblock2 or None)
ENTRIES = [(f"rb1/{name}/{p}", VR, name, p, None) for name in VR.CASES for p in PRECISIONS] + \
          [(f"rb2/{name}/{p}/{'fused' if fused else 'composed'}", RR, name, p, fused)
           for name in RR.CASES for p in PRECISIONS for fused in (True, False)]


def _sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def _model(ref, name, precision, fused, graphs=False):
    from efficient_tts_amd.vocoder import HiFiGANGenerator
    cs = ref.CASES[name]
    m = HiFiGANGenerator(cs["cfg"], precision=precision)
    m.load_state_dict(ref.fill(cs["cfg"], cs["seed"]))
    m = m.to(torch.device("cuda:0")).eval()
    m.graphs = graphs
    if fused is not None:
        m.fused_resblock2 = fused
    return m


def _inputs(ref, name):
    cs = ref.CASES[name]
    mel = ref.mel_input(cs["cfg"], len(cs["lengths"]), cs["T"], cs["seed"])
    return mel.to(torch.device("cuda:0")), torch.tensor(cs["lengths"])


def entry_digest(ref, name, precision, fused, branch_streams=True):
    """{"pitch": rows per item, "audio": sha256, "<kept key>": sha256 ...} of one eager forward"""
    m = _model(ref, name, precision, fused)
    m.branch_streams = branch_streams
    keep = {}
    audio = m(*_inputs(ref, name), keep=keep)
    torch.cuda.synchronize()
    out = {"pitch": int(keep.pop("pitch")), "audio": _sha(audio)}
    for k in sorted(keep):
        out[k] = _sha(keep[k])
    return out


def vocoder_digests():
    return {e[0]: entry_digest(*e[1:]) for e in ENTRIES}


@pytest.fixture(scope="module")
def recorded():
    with open(DIGESTS) as f:
        return json.load(f)["digests"]


def _differences(got, want):
    return sorted(f"{name}:{k}" for name in got for k in set(got[name]) | set(want[name]) if got[name].get(k) != want[name].get(k))


def test_every_kept_buffer_equals_the_recorded_bits(recorded):
    got = vocoder_digests()
    assert sorted(got) == sorted(recorded) == sorted(e[0] for e in ENTRIES), "the entries differ from the recorded set"
    bad = _differences(got, recorded)
    assert not bad, f"{len(bad)} buffers differ from the recorded bits: {bad}"


@pytest.mark.parametrize("family,name", [("rb1", "gap"), ("rb2", "v3-small")])
def test_chains_in_a_row_give_the_recorded_bits(recorded, family, name):
    """`branch_streams = False`: the same launches on one stream, the same bits in every buffer"""
    got = {e[0]: entry_digest(*e[1:], branch_streams=False) for e in ENTRIES if e[0].startswith(f"{family}/{name}/")}
    assert len(got) == (3 if family == "rb1" else 6)
    bad = _differences(got, recorded)
    assert not bad, f"{len(bad)} buffers differ with the chains in a row: {bad}"


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("ref,name", [(VR, "gap"), (RR, "v3-small")], ids=["gap", "v3-small"])
def test_graph_replay_equals_eager(ref, name, precision):
    """the graph cache runs the first two calls of a shape eagerly and then decides by the host's share of the time: the policy is pinned
    to "graph" and the capture asserted, as test_vocoder_rb2_gpu.py::test_batch_equals_items_alone_and_graph_replay_equals_eager does"""
    x, l = _inputs(ref, name)
    eager = _model(ref, name, precision, None)(x, l).clone()
    m = _model(ref, name, precision, None, graphs=True)
    cache = m._graph_cache
    cache.EAGER_MAX_HOST_SHARE = -1.0
    ys = [m(x, l).clone() for _ in range(4)]                # eager, eager (timed), capture + replay, replay
    assert cache.captures == 1 and cache.entries[("voc", x.shape[0], x.shape[2])].graph is not None
    for y in ys:
        assert torch.equal(y, eager), (name, precision)
