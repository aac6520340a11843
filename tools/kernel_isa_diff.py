"""Compare every kernel of two builds of the same sources, instruction for instruction, with the compiler's resource report beside it: the check behind
profiles/ss2d_split_resources.txt and profiles/train_dense_refactor_resources.txt.

Compile the files under comparison in two directories, one per tree, with the library's flags (xpoint_amd/build.py: FLAGS) plus
`-Rpass-analysis=kernel-resource-usage -save-temps`, keeping hipcc's stderr as <name>.log beside the saved *-gfx950.s:

    hipcc -x hip -c <tree>/xpoint_amd/csrc/ss2d_seq.hip -o ss2d_seq.o <FLAGS> -Rpass-analysis=kernel-resource-usage -save-temps 2> ss2d_seq.log
    python tools/kernel_isa_diff.py <parent dir> <new dir> [old=new ...]

One row per kernel: the new tree's VGPR / AGPR / scratch / LDS / occupancy, SGPR parent -> new, and "identical" when the two bodies are the same
instructions (symbol names, labels, comments and directives ignored), else both instruction counts; a row whose resources differ says so.  `old=new`
pairs rewrite substrings of the PARENT's mangled names before matching, for a type that moved between namespaces (the SS2D split:
NS_10SS2DParamsE=10SS2DParams)."""
import collections
import glob
import re
import subprocess
import sys

FIELDS = ("VGPRs", "AGPRs", "ScratchSize", "LDS", "Occupancy")


def remarks(paths):
    out, cur = {}, None
    for path in paths:
        for ln in open(path, errors="ignore"):
            m = re.search(r"Function Name: (\S+)", ln)
            if m:
                cur = m.group(1)
                out[cur] = {}
                continue
            m = re.search(r"remark: .*?:\s+(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
            if m and cur:
                out[cur][m.group(1).split(" ")[0]] = int(m.group(2))
    return out


def bodies(paths):
    out, cur = {}, None
    for path in paths:
        for ln in open(path, errors="ignore"):
            s = ln.strip()
            m = re.match(r"^(_Z\w+):", s)
            if m:
                cur = m.group(1)
                out[cur] = []
                continue
            if cur is None:
                continue
            if s.startswith(".Lfunc_end"):
                cur = None
                continue
            if not s or s.startswith(";") or s.startswith("."):         # comments, labels, directives
                continue
            s = re.sub(r";.*$", "", s).strip()
            out[cur].append(re.sub(r"_Z\w+", "SYM", re.sub(r"\.LBB\d+_\d+", "L", s)))
    return out


def demangle(name):
    # (binutils' c++filt does not know DF16_ = _Float16: demangle it as Dh = __fp16 and put the name back)
    d = subprocess.run(["c++filt", name.replace("DF16_", "Dh")], capture_output=True, text=True).stdout.strip().replace("__fp16", "_Float16")
    return re.sub(r"\(.*\)$", "", d.replace("(anonymous namespace)::", "").replace("void ", ""))


def main():
    parent, new = sys.argv[1], sys.argv[2]
    renames = [a.split("=", 1) for a in sys.argv[3:]]

    def canon(n):
        for old, to in renames:
            n = n.replace(old, to)
        return n
    rp = {canon(k): v for k, v in remarks(glob.glob(parent + "/*.log")).items()}
    bp = {canon(k): v for k, v in bodies(glob.glob(parent + "/*gfx950.s")).items()}
    rn, bn = remarks(glob.glob(new + "/*.log")), bodies(glob.glob(new + "/*gfx950.s"))
    print(f"{len(rp)} kernels in the parent, {len(rn)} in the new tree; only in parent: {sorted(set(rp) - set(rn))}; only in new: {sorted(set(rn) - set(rp))}")
    rows, fam = [], collections.Counter()
    for k in set(rp) & set(rn):
        a, b, name = rp[k], rn[k], demangle(k)
        fam[re.split(r"[<I]", name.replace("_ZN12_GLOBAL__N_1", ""), maxsplit=1)[0]] += 1
        same = k in bp and bp[k] == bn.get(k)
        row = f"{name} | {b['VGPRs']} | {b['AGPRs']} | {b['ScratchSize']} | {b['LDS']} | {b['Occupancy']} | {a['TotalSGPRs']} -> {b['TotalSGPRs']} | "
        row += "identical" if same else f"instructions {len(bp.get(k, []))} -> {len(bn.get(k, []))}"
        if any(a[f] != b[f] for f in FIELDS):
            row += f"   DIFFERS: parent {a}"
        rows.append(row)
    print(f"identical disassembly: {sum(r.endswith('identical') for r in rows)} of {len(rows)}; instances per kernel: {dict(sorted(fam.items()))}")
    print("kernel | VGPR | AGPR | scratch | LDS | occupancy | SGPR parent -> new | disassembly")
    print("\n".join(sorted(rows)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
