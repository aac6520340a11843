"""Record tests/golden/ss2d_chunked_parent_bits.json: the sha256 of every image's output of the chunked SS2D core (f32, f32 containers in the mixed-precision
class, fp16 storage) and of the first sequential kernel at the shapes of tests/test_gpu_ss2d_chunked_bits.py, as the library in use computes them.  Run ONCE on
an MI355X with the library of the commit BEFORE csrc/ss2d.hip was split by form (XP_LIB_PATH selects that build); the test then holds
every later commit to those bits.  Not to be re-run to make a failing test pass: a difference is a change of results.

    XP_LIB_PATH=<parent build>/libxpoint_hip.so python tools/make_golden_ss2d_chunked_bits.py [out.json [source hash of that build]]

The shapes, inputs and calls are the test module's (compute, run_child), so generator and test cannot drift apart.  The file holds ONE digest per (shape,
class, image), so nothing is written unless the batches 1 and 3 gave the same digest for the same image, every output was finite and every canary intact."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_gpu_ss2d_chunked_bits as G  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else G.GOLDEN
    sha, findings = {}, []
    got = dict(G.compute())
    got.update(G.run_child())
    if sorted(got) != sorted(G.want_keys() + G.want_keys(v1=True)):
        findings.append("the calls made are not the calls the test expects")
    for key, g in sorted(got.items()):
        group, shape, cls, _ = key.split("/")
        if not (g["finite"] and g["intact"]):
            findings.append(f"{key}: finite {g['finite']}, canary intact {g['intact']}")
        have = sha.setdefault(f"{group}/{shape}/{cls}", [])
        n = min(len(have), len(g["sha"]))
        if have[:n] != g["sha"][:n]:
            findings.append(f"{key}: digests differ from another batch of the same images")
        if len(g["sha"]) > len(have):
            sha[f"{group}/{shape}/{cls}"] = g["sha"]
    if findings:
        print("NOT written:\n" + "\n".join(findings))
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(dict(sha=sha, source_hash=sys.argv[2] if len(sys.argv) > 2 else ""), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{path}: {len(sha)} (shape, class) entries, {sum(len(v) for v in sha.values())} image digests, {os.path.getsize(path)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
