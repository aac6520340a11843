"""Record tests/golden/ss2d_seq_parent_bits.json: the sha256 of every image's output of the sequential SS2D core (f32 rows, P32 image, fp16 with f32 copies)
at the shapes of tests/test_gpu_ss2d_seq_bits.py, as the library in use computes them.  Run ONCE on an MI355X at the commit BEFORE the sequential kernels were
refit to two waves per SIMD; the test then holds every later commit to those bits.  Not to be re-run to make a failing test pass: a
difference is a change of results.

    python tools/make_golden_ss2d_seq_bits.py [out.json]

The shapes, inputs and calls are the test module's (compute, run_child), so generator and test cannot drift apart.  One child process per XP_SS2D_SEQ_NW
(0 = automatic, 1, 2, 4); the file holds ONE digest per (shape, output, image), so nothing is written unless every batch and every NW gave the same digest for
the same image, every output was finite and every canary intact."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_gpu_ss2d_seq_bits as G  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else G.GOLDEN
    sha, findings = {}, []
    for nw in G.NWS:
        for key, g in sorted(G.run_child(nw).items()):
            shape, kind, _ = key.split("/")
            if not (g["finite"] and g["intact"]):
                findings.append(f"NW {nw} {key}: finite {g['finite']}, canary intact {g['intact']}")
            have = sha.setdefault(f"{shape}/{kind}", [])
            n = min(len(have), len(g["sha"]))
            if have[:n] != g["sha"][:n]:
                findings.append(f"NW {nw} {key}: digests differ from another batch / NW of the same images")
            if len(g["sha"]) > len(have):
                sha[f"{shape}/{kind}"] = g["sha"]
    if findings:
        print("NOT written:\n" + "\n".join(findings))
        return 1
    import torch
    from xpoint_amd import build
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(dict(sha=sha, source_hash=build.source_hash(), compute_units=torch.cuda.get_device_properties(0).multi_processor_count), fh, indent=1,
                  sort_keys=True)
        fh.write("\n")
    print(f"{path}: {len(sha)} (shape, output) entries, {sum(len(v) for v in sha.values())} image digests, {os.path.getsize(path)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
