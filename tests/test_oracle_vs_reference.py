"""Pin of the restatement against the reference itself, through the fixture oracle/gen_golden_pins.py recorded from it
(tests/golden/reference_pins.npz): state_dict layout of the reference SlotModel and the reference SlotAttention forward.
Runs anywhere (no reference, no GPU needed)."""
import os

import numpy as np
import pytest
import torch

from oracle import torch_oracle as O
from oracle.gen_golden_pins import SD_CASES, XSLOT_CASES, case_id, xslot_inputs

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_pins.npz"), allow_pickle=False)


@pytest.mark.parametrize("arch,C,spc,L,mnist", SD_CASES)
def test_state_dict_spec_equals_reference(arch, C, spc, L, mnist):
    cid = case_id((arch, C, spc, L, mnist))
    keys = [str(k) for k in GOLD["sd_%s_keys" % cid]]
    shapes = [tuple(int(s) for s in str(v).split(",") if s) for v in GOLD["sd_%s_shapes" % cid]]
    spec = O.state_dict_spec(arch, C, spc, L, in_chans=1 if mnist else 3, mnist_stem=mnist)
    assert keys == list(spec.keys())
    assert all(shape == tuple(spec[k]) for k, shape in zip(keys, shapes))


@pytest.mark.parametrize("C,spc,N,L,ls,power", XSLOT_CASES)
def test_xslot_restatement_equals_reference_module(C, spc, N, L, ls, power):
    cid = case_id((C, spc, N, L, ls, power))
    pre = "xslot_%s_" % cid
    P = {"slot." + k[len(pre):]: torch.from_numpy(GOLD[k]) for k in GOLD.files
         if k.startswith(pre) and k[len(pre):] not in ("logits", "loss")}
    x_pe, x = xslot_inputs((C, spc, N, L, ls, power))
    with torch.no_grad():
        logits, loss = O.xslot_forward(P, x_pe, x, C, spc, ls, power)
    np.testing.assert_allclose(logits.numpy(), GOLD[pre + "logits"], atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(float(loss), float(GOLD[pre + "loss"]), atol=1e-7, rtol=1e-6)
