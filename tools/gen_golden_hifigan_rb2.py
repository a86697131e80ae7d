"""Writes tests/golden/hifigan_rb2_small.npz from the REFERENCE generator (imported from /root/reference, run in the build container
only): the reference Generator with a small `resblock: "2"` configuration (tests/vocoder_rb2_reference.py:GOLDEN), the name-keyed
parameter fill of that module, one mel input.  Arrays only: every parameter under its state-dict name, "mel" and "audio"."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")
import vocoder_rb2_reference as RR                           # noqa: E402
from nntts.vocoders.hifigan_model import Generator          # noqa: E402
from nntts.vocoders.env import AttrDict                     # noqa: E402

if __name__ == "__main__":
    cfg = dict(RR.GOLDEN)
    gen = Generator(AttrDict(cfg)).eval()
    P = RR.fill(cfg, RR.GOLDEN_SEED)
    sd = gen.state_dict()
    assert list(sd.keys()) == list(P.keys()), "param_shapes() must list the reference's keys in order"
    for k in sd:
        assert tuple(sd[k].shape) == tuple(P[k].shape), (k, sd[k].shape, P[k].shape)
    gen.load_state_dict(P)
    mel = RR.mel_input(cfg, 1, RR.GOLDEN_T, RR.GOLDEN_SEED)
    with torch.no_grad():
        y = gen(mel)
        y64 = RR.forward(P, mel, None, cfg, torch.float64)["out"]
    print(tuple(y.shape), "ref max", float(y.abs().max()), "restatement (float64) vs reference (float32)", float((y.double() - y64).abs().max()))
    out = {k: v.numpy() for k, v in P.items()}
    out["mel"], out["audio"] = mel.numpy(), y.numpy()
    path = os.path.join(ROOT, "tests", "golden", "hifigan_rb2_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
