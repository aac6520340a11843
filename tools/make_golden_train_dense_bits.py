"""Record tests/golden/train_dense_parent_bits.json: the digests of every dense training operator's results at the shapes of
tests/test_gpu_train_dense_bits.py, of one whole step of VSSEncoder and of XPointNet, and the profiler's launch tallies, as the code in use computes
them.  Run ONCE on an MI355X at the commit BEFORE csrc/train_dense.hip was split; the test then holds every later commit to
those bits and launches.  Not to be re-run to make a failing test pass: a difference is a change of results.

    python tools/make_golden_train_dense_bits.py [out.json]

The cases and the calls are those of the test module (compute_bits, launch_tally), so generator and test cannot drift apart.  Every case runs twice;
if any digest or tally differs between the two runs nothing is written."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_gpu_train_dense_bits as G  # noqa: E402


def record():
    out = {c: G.compute_bits(c) for c in G.CASES}
    out["launches"] = {c: G.launch_tally(c) for c in G.TALLIED}
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else G.GOLDEN
    first, second = record(), record()
    unstable = [(c, k) for c in first for k in first[c] if first[c][k] != second[c].get(k)]
    if unstable or first.keys() != second.keys():
        print(f"NOT written: {len(unstable)} entries differ between two runs: {unstable}")
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(first, fh, indent=1, sort_keys=True)
        fh.write("\n")
    n = sum(len(v) for c, v in first.items() if c != "launches")
    print(f"{path}: {len(G.CASES)} cases, {n} digests, {len(G.TALLIED)} launch tallies, {os.path.getsize(path)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
