"""TEST INFRASTRUCTURE.  Generates tests/golden/reference_pins.npz, the fixture tests/test_oracle_vs_reference.py pins the
restatement (oracle/torch_oracle.py) against, by running the *reference itself* (imported read-only through
oracle/ref_import.py):

    python oracle/gen_golden_pins.py

  sd_<case>_keys / _shapes     state_dict key order and shapes of the reference SlotModel, per SD_CASES entry
  xslot_<case>_<param>         the reference SlotAttention's (randomly initialised) parameters, per XSLOT_CASES entry
  xslot_<case>_logits / _loss  its forward on xslot_inputs(case)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import torch_oracle as O  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "reference_pins.npz")

SD_CASES = [("resnet18", 10, 1, 1, True), ("resnest26d", 10, 1, 3, False), ("resnest50d", 100, 3, 3, False)]   # arch, C, spc, L, mnist
XSLOT_CASES = [(10, 1, 49, 3, 1, 2), (6, 3, 81, 1, -1, 1)]                                                  # C, spc, N, L, ls, power


def case_id(case):
    return "_".join(str(v) for v in case)


def xslot_inputs(case):
    """(x + pe, x): post-ReLU tokens [3, N, 64] and a position encoding, drawn from numpy.random.default_rng(5)."""
    N = case[2]
    rng = np.random.default_rng(5)
    x = torch.from_numpy(np.maximum(rng.standard_normal((3, N, 64)), 0).astype(np.float32))
    pe = torch.from_numpy(rng.standard_normal((1, N, 64)).astype(np.float32))
    return x + pe, x


def main():
    from oracle import ref_import as R
    if not R.reference_available():
        raise SystemExit("the reference tree is not at %s (SCOUTER_REFERENCE_ROOT)" % R.REFERENCE_ROOT)
    torch.manual_seed(0)
    out = {}
    for case in SD_CASES:
        arch, C, spc, L, mnist = case
        args = R.make_args(model=arch, num_classes=C, slots_per_class=spc, channel=O.ARCHS[arch]["channel"],
                           to_k_layer=L, dataset="MNIST" if mnist else "ImageNet")
        sd = R.build_reference_slot_model(args).state_dict()
        out["sd_%s_keys" % case_id(case)] = np.array(list(sd.keys()))
        out["sd_%s_shapes" % case_id(case)] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    for case in XSLOT_CASES:
        C, spc, N, L, ls, power = case
        m = R.build_reference_slot_attention(C, spc, 64, loss_status=ls, power=power, to_k_layer=L)
        for k, v in m.state_dict().items():
            out["xslot_%s_%s" % (case_id(case), k)] = v.detach().numpy()
        x_pe, x = xslot_inputs(case)
        with torch.no_grad():
            logits, loss = m(x_pe, x)
        out["xslot_%s_logits" % case_id(case)] = logits.numpy()
        out["xslot_%s_loss" % case_id(case)] = np.array(float(loss))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
