#!/usr/bin/env python3
"""Record the precision-16 outputs that tests/test_inference_bf16.py pins bit for bit (tests/golden/precision16_parent_bits.npz).
   python tools/gen_golden_precision16.py sim|gpu [out.npz]
Run it on the commit whose bits are to be kept: `sim` runs tests/precision_checks.precision16_cases on that commit's wave-simulator
build, `gpu` on its libesmi.so (or the library ESMI_LIB names) on the device.  The tier's arrays are merged into the file, the other
tier's are kept."""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

tier = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "precision16_parent_bits.npz")
from tests import precision_checks as V
if tier == "sim":
    from tests.simlib import use_sim
    with use_sim():
        got = V.precision16_cases("cpu")
else:
    got = V.precision16_cases("cuda:0")
arrays = dict(np.load(out)) if os.path.exists(out) else {}
arrays = {k: v for k, v in arrays.items() if not k.startswith(tier + "_")}
arrays.update({f"{tier}_{k}": v for k, v in got.items()})
np.savez_compressed(out, **arrays)
print({k: v.shape for k, v in arrays.items()})
