#!/usr/bin/env python3
"""How far the fp32 reference fixtures of the widths other than 512 (tests/golden/variant_c256 / c768 / c1024.npz) are from the exact
value, and what the tests may therefore ask of them (CPU only):

    python tools/width_error.py            # rewrites profiles/width_error.json

Per width: the oracle (oracle/efts_oracle.py) evaluated in FLOAT64 on the fixture's inputs against the fixture -- the error of the
fp32 reference itself, machine independent to ~1e-12 -- and, for comparison, the same oracle evaluated in float32 on this host against
the fixture and against the float64 value.  With the name-keyed random fill the wide models have losses of 348 (c768) and 2560 (c1024)
and |mel| up to 51 / 146, and their fp32 gradients carry rounding noise of up to 2.6e-3 of a tensor's largest entry (c768,
decoder.layers.0.conv.0.bias: one entry; 6e-4 broadly in the mel encoder).  A float32 evaluation lands within 1e-4 of the fixture only
where it happens to round like the host that made the fixture: seen 7.7e-5 (c768) and 1.2e-5 (c1024) on one host, 4.1e-3 (c1024) on
another.  So tests/test_oracle_golden.py holds the oracle to these fixtures in float64, with the gradient bound
max(2e-4, 4 x the reference error recorded here) -- the rule of tests/test_stoi_gpu.py -- and the forward bounds of its TOL unchanged.
`device` holds what one MI355X run of tests/test_gpu_variants.py printed for the same fixtures (bf16x3), beside the bounds it met."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import efts_oracle as O  # noqa: E402

WIDTHS = dict(c256=256, c768=768, c1024=1024)
FORWARD = ("loss", "mel_loss", "dur_loss", "imv", "e", "dur_pred", "log_delta_e", "mel_pred", "reconst_alpha")
# printed by tests/test_gpu_variants.py on one MI355X (default routing): max-abs mel error and its bound max(1e-3, 2.5e-5 max|mel|);
# worst gradient entry relative to its tensor's max and the number of entries above 1e-2 (bounds: 6e-2, at most two)
DEVICE = dict(c256=dict(mel=2.09e-5, mel_bound=1.00e-3, grad_worst=1.04e-2, grad_above_1e2=1),
              c768=dict(mel=5.95e-4, mel_bound=1.27e-3, grad_worst=2.62e-4, grad_above_1e2=0),
              c1024=dict(mel=1.74e-3, mel_bound=3.65e-3, grad_worst=1.17e-2, grad_above_1e2=1))


def evaluate(g, hp, dtype):
    """(forward outputs, {name: gradient samples at the fixture's stride}, inference mel) of the oracle in `dtype`"""
    P = {k: v.to(dtype).requires_grad_(True) for k, v in O.fill_params(hp).items()}
    o = O.forward(P, torch.from_numpy(g["text"]), torch.from_numpy(g["text_lengths"]), torch.from_numpy(g["speech"]).to(dtype),
                  torch.from_numpy(g["speech_lengths"]), hp)
    o["loss"].backward()
    grads = {}
    for k, p in P.items():
        flat = p.grad.reshape(-1).double().numpy()
        grads[k] = flat[:: int(g["grad_stride:" + k])] if "grad_stride:" + k in g.files else flat
    with torch.no_grad():
        inf = O.inference({k: v.detach() for k, v in P.items()}, torch.from_numpy(g["inf_text"]), hp)["mel_pred"]
    return {k: o[k].detach().double() for k in FORWARD}, grads, inf.double()


def grad_distance(a, b, g):
    """worst |a - b| relative to the fixture tensor's largest entry, over all tensors but the analytically zero key bias"""
    worst, where = 0.0, ""
    for k in a:
        if k == "text_encoder_key.bias":
            continue
        d = float(np.abs(a[k] - b[k]).max()) / max(float(np.abs(g["grad:" + k]).max()), 1e-3)
        if d > worst:
            worst, where = d, k
    return worst, where


def main():
    torch.set_num_threads(8)
    out = {}
    for name, C in WIDTHS.items():
        g = np.load(os.path.join(ROOT, "tests", "golden", f"variant_{name}.npz"))
        hp = dict(O.DEFAULT_HP, n_channels=C)
        fix = {k[5:]: g[k].astype(np.float64) for k in g.files if k.startswith("grad:")}
        f64, g64, i64 = evaluate(g, hp, torch.float64)
        f32, g32, i32 = evaluate(g, hp, torch.float32)
        ref_fwd = {k: float((f64[k] - torch.from_numpy(np.asarray(g[k])).double()).abs().max()) for k in FORWARD}
        ref_grad, where = grad_distance(g64, fix, g)
        r = dict(loss=float(g["loss"]), mel_max=float(np.abs(g["mel_pred"]).max()),
                 reference_vs_float64=dict(forward=ref_fwd, grad_worst_rel=ref_grad, grad_worst_tensor=where,
                                           inference_mel=float((i64 - torch.from_numpy(g["inf_mel_pred"]).double()).abs().max())),
                 float32_oracle_on_this_host=dict(grad_vs_fixture=grad_distance(g32, fix, g)[0], grad_vs_float64=grad_distance(g32, g64, g)[0],
                                                  mel_vs_fixture=float((f32["mel_pred"] - torch.from_numpy(g["mel_pred"]).double()).abs().max())),
                 bounds=dict(cpu_float64_grad=max(2e-4, 4.0 * ref_grad), cpu_float64_grad_rule="max(2e-4, 4 x reference_vs_float64.grad_worst_rel)",
                             device_mel=max(1e-3, 2.5e-5 * float(np.abs(g["mel_pred"]).max())), device_grad="1e-2 of the tensor's max, at most two entries above it, none above 6e-2"),
                 device=DEVICE[name])
        out[name] = r
        print(name, json.dumps(r["reference_vs_float64"]), json.dumps(r["float32_oracle_on_this_host"]), r["bounds"]["cpu_float64_grad"])
    with open(os.path.join(ROOT, "profiles", "width_error.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
