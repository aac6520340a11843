"""Record tests/golden/glue_parent_bits.npz: the exact outputs of the depthwise 3x3 + SiLU, stem and depth-to-space kernels in the f32 class and the
fp16-storage class, as the library in use computes them.  Run ONCE on an MI355X against a build of the commit BEFORE csrc/glue_core.h merged the
per-class copies of these kernels (XP_LIB_PATH selects that build); tests/test_gpu_glue_classes.py::test_bits_are_those_before_the_merge then holds
every later build to those bits.  Not to be re-run to make a failing test pass: a difference is a change of results.

    XP_LIB_PATH=<parent build>/libxpoint_hip.so python tools/make_golden_glue.py [out.npz]

The cases, the synth names of their inputs and the calls are those of the test module (compute_bits), so generator and test cannot drift apart; the
file holds outputs only (np.savez, uncompressed, < 200 KB)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_gpu_glue_classes as G  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else G.GOLDEN
    from xpoint_amd import _lib
    arrays = {}
    for op in ("dwconv", "stem", "d2s"):
        arrays.update(G.compute_bits(op))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "wb") as fh:
        np.savez(fh, **arrays)
    size = os.path.getsize(out)
    assert size <= 200 * 1024, size
    print(f"{out}: {len(arrays)} arrays, {size} bytes, from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
