"""The forward's launch plan, recorded without a GPU.

csrc/model.cpp is a fixed launch sequence behind the C ABI.  A stand-alone host program (launch_plans/driver.cpp) links libxpoint_hip.so
and DEFINES every launching entry point itself (a stub translation unit generated from _lib._SIGNATURES), so model.cpp's calls land in the
stubs by ELF symbol interposition while the size queries and predicates stay the library's own.  Each stub prints its name and arguments
(pointers as offsets from fake base addresses that are never dereferenced); no HIP call is made.  The printed plan — which kernel, which
operands, which workspace region — is compared with the text under tests/launch_plans/: a change of model.cpp that is meant to leave the
behaviour alone leaves these files alone, and a fusion shows up as a readable diff.

`python tests/test_cpu_launch_plan.py --record` rewrites the expectations from the built library."""
import difflib
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from xpoint_amd import _lib  # noqa: E402

PLANS = os.path.join(ROOT, "tests", "launch_plans")
BIG = ["batch=16", "H=480", "W=640"]
X3 = ["engine=0"]

# name -> (entry point, driver arguments, environment, how the plan is stored); shapes 2 x 64 x 96, embed 96, depths 2,2,2,2 unless stated.
# Every plan is pinned byte for byte.  Its first part, the weight layout (xp_weights_numel, xp_param_count, every xp_param_info row), is the same for all
# scenarios of one model and stored once per model (layout_*.txt).  The rest — size queries, launches, return code, error text — is stored as
#   "text"   the full text (<name>.txt): the plan of each arithmetic class, shape and model, of the prepare functions, of the error paths;
#   a name   the unified diff (no context) against that scenario's text (<name>.diff): what a knob or an output selection changes, and nothing else.
SCENARIOS = {
    "h2": ("ex", [], {}, "text"),
    "x3": ("ex", X3, {}, "text"),
    "products3": ("ex", X3 + ["products=3"], {}, "x3"),
    "products1": ("ex", X3 + ["products=1"], {}, "x3"),
    "f32": ("ex", ["wsplit=0"], {}, "text"),
    "amp16": ("ex", ["amp=1"], {}, "text"),
    "f16": ("f16", [], {}, "text"),
    "h2_prob_only": ("ex", ["outs=5"], {}, "h2"),
    "h2_enc_only": ("ex", ["outs=4"], {}, "h2"),
    "h2_16x480x640": ("ex", BIG, {}, "text"),
    "f16_16x480x640": ("f16", BIG, {}, "text"),
    "h2_1x32x32": ("ex", ["batch=1", "H=32", "W=32"], {}, "text"),
    "h2_no_fused_mlp": ("ex", [], {"XP_NO_FUSED_MLP": "1"}, "h2"),
    "h2_fuse_maxc96": ("ex", [], {"XP_FUSE_MAXC": "96"}, "h2"),
    "h2_fused_x3": ("ex", [], {"XP_FUSED_X3": "1"}, "h2"),
    "f16_no_ln_proj": ("f16", [], {"XP_NO_LN_PROJ_F16": "1"}, "f16"),
    "f16_no_fused_mlp1": ("f16", [], {"XP_NO_FUSED_MLP_F16": "1"}, "f16"),
    "f16_no_fused_mlp2": ("f16", [], {"XP_NO_FUSED_MLP_F16": "2"}, "f16"),
    "h2_embed32_depths1111": ("ex", ["embed=32", "depths=1,1,1,1"], {}, "text"),
    "h2_depths2242": ("ex", ["depths=2,2,4,2"], {}, "text"),
    "prepare_split": ("prepare_split", [], {}, "text"),
    "prepare_f16": ("prepare_f16", [], {}, "text"),
    "err_workspace_one_byte_short": ("ex", ["ws_delta=-1"], {}, "text"),
    "err_h48": ("ex", ["H=48"], {}, "text"),
    "err_amp_without_wsplit": ("ex", ["amp=1", "wsplit=0"], {}, "text"),
}

# per-launch override masks (xp_set_dense_override), stored as hashes: every single bit, and a few combinations
MASKS = [1 << i for i in range(47)] + [(1 << 47) - 1, 0x3, 0x1C, 0x7 << 41, (1 << 44) | (1 << 46), 0x1F << 21, (1 << 3) | (1 << 9) | (1 << 40),
                                       ((1 << 47) - 1) & ~((1 << 23) - 1)]
# depths 2,2,4,2: blocks 7, 8 and 9 share the last block's bits (the clipped block index of build_layout), so the masks are what pins that rule
MASK_SHAPES = {"2x64x96": [], "16x480x640": BIG, "2x64x96_depths2242": ["depths=2,2,4,2"]}

_C_TYPES = {_lib.c_p: ("const void*", "%s"), _lib.c_i: ("int", "%d"), _lib.c_f: ("float", "%.9g"), _lib.c_l: ("long long", "%lld"),
            _lib.c_sz: ("size_t", "%zu")}
_NOT_STUBBED = re.compile(r"xp_ctx_|xp_param_info$|xp_forward_shapes$|xp_prepare_|xp_xpoint_forward")
# the three internal C++ entry points of csrc/xp_common.h (C++ linkage: stubbed by hand, same signatures)
_CXX_STUBS = r"""
int xp_depth_to_space_nhwc_st(const float* x, float* y, int batch, int H, int W, int C, int bs, float limit, int* status, void* stream) {
    if (!plan_silent) printf("xp_depth_to_space_nhwc_st %s %s %d %d %d %d %d %.9g %s %s\n", plan_ptr(x), plan_ptr(y), batch, H, W, C, bs, limit, plan_ptr(status), plan_ptr(stream));
    return 0;
}
int xp_softmax_shuffle_st(const float* logits, float* prob, int batch, int Hc, int Wc, int r, int ld, int mode, int* status, void* stream) {
    if (!plan_silent) printf("xp_softmax_shuffle_st %s %s %d %d %d %d %d %d %s %s\n", plan_ptr(logits), plan_ptr(prob), batch, Hc, Wc, r, ld, mode, plan_ptr(status), plan_ptr(stream));
    return 0;
}
int xp_l2norm_rows_st(const float* x, float* y, int64_t rows, int C, float eps, int* status, void* stream) {
    if (!plan_silent) printf("xp_l2norm_rows_st %s %s %lld %d %.9g %s %s\n", plan_ptr(x), plan_ptr(y), (long long)rows, C, eps, plan_ptr(status), plan_ptr(stream));
    return 0;
}
"""


def stubbed_entry_points():
    """Every C entry point model.cpp calls whose last argument is the stream, except the context / layout / prepare / forward functions."""
    src = open(os.path.join(ROOT, "xpoint_amd", "csrc", "model.cpp")).read()
    called = set(re.findall(r"\b(xp_[a-z0-9_]+)\s*\(", src))
    return sorted(n for n, a in _lib._SIGNATURES.items() if n in called and a and a[-1] is _lib.c_p and not _NOT_STUBBED.match(n))


def stub_source():
    out = ["#include <stdint.h>", "#include <stdio.h>", 'extern "C" int plan_silent;', 'extern "C" const char* plan_ptr(const void* p);', 'extern "C" {']
    for name in stubbed_entry_points():
        args = _lib._SIGNATURES[name]
        decl = ", ".join(f"{_C_TYPES[t][0]} a{i}" for i, t in enumerate(args))
        fmt = " ".join(_C_TYPES[t][1] for t in args)
        vals = ", ".join((f"plan_ptr(a{i})" if t is _lib.c_p else (f"(double)a{i}" if t is _lib.c_f else f"a{i}")) for i, t in enumerate(args))
        out.append(f'int {name}({decl}) {{ if (!plan_silent) printf("{name} {fmt}\\n", {vals}); return 0; }}')
    out.append("}")
    return "\n".join(out) + _CXX_STUBS


def build_driver(tmp, lib_path=None):
    """Compile driver + stubs with the host C++ compiler against the built library (rpath to its directory).  Returns the program's path."""
    lib_path = lib_path or _lib.LIB_PATH
    assert os.path.exists(lib_path), f"{lib_path} not built"
    libdir = os.path.join(str(tmp), "lib")
    os.makedirs(libdir, exist_ok=True)
    shutil.copy(lib_path, os.path.join(libdir, "libxpoint_hip.so"))      # under its link name, whatever the file is called
    stubs = os.path.join(str(tmp), "stubs.cpp")
    open(stubs, "w").write(stub_source())
    exe = os.path.join(str(tmp), "launch_plan_driver")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    cmd = [cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(PLANS, "driver.cpp"), stubs, "-o", exe,
           "-L", libdir, "-lxpoint_hip", "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined", "-rdynamic"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "driver build failed:\n" + r.stdout + r.stderr
    return exe


def run_driver(exe, entry, args, env=None):
    """One child process (the library reads its knobs once per process)."""
    e = {k: v for k, v in os.environ.items() if not k.startswith("XP_")}      # knobs: only the scenario's own
    e.update(env or {})
    r = subprocess.run([exe, entry] + list(args), capture_output=True, text=True, env=e, timeout=120)
    assert r.returncode == 0, f"driver {entry} {args} exited {r.returncode}:\n{r.stdout[-2000:]}{r.stderr[-2000:]}"
    return r.stdout


def mask_plans(exe, shape_args):
    """{mask (hex): sha256 of that mask's part of the plan} for every mask of MASKS at one shape (one process: the override is no knob)."""
    txt = run_driver(exe, "ex", shape_args + ["masks=" + ",".join(f"{m:x}" for m in MASKS)])
    parts = re.split(r"^== override ([0-9a-f]+)\n", txt, flags=re.M)
    out = {"header": hashlib.sha256(parts[0].encode()).hexdigest()}
    for m, body in zip(parts[1::2], parts[2::2]):
        out[m] = hashlib.sha256(body.encode()).hexdigest()
    assert len(out) == len(MASKS) + 1
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("launch_plan"))


def test_stubs_cover_the_launching_entry_points():
    names = stubbed_entry_points()
    assert {"xp_gemm_nt_h2", "xp_gemm_nt_x3", "xp_gemm_nt", "xp_gemm_nt_h2s", "xp_gemm_nt_f16", "xp_ss2d_core_fwd_ex", "xp_ss2d_core_fwd_f16", "xp_mlp_fused_h2",
            "xp_split_weights_x3", "xp_f32_to_f16", "xp_round_f16", "xp_layernorm_p32"} <= set(names)
    assert not [n for n in names if _NOT_STUBBED.match(n)]


def plan_of(exe, name):
    """(layout file name, layout lines, remaining lines) of one scenario's plan."""
    entry, args, env, _ = SCENARIOS[name]
    lines = run_driver(exe, entry, args, env).splitlines()
    n = next(i for i, l in enumerate(lines) if not l.startswith(("xp_weights_numel ", "xp_param_count ", "xp_param_info ")))
    model = {k: v for k, v in (a.split("=") for a in args if a.startswith(("embed=", "depths=")))}
    return f"layout_{model.get('embed', '96')}_{model.get('depths', '2,2,2,2').replace(',', '')}.txt", lines[:n], lines[n:]


def stored(fname):
    return open(os.path.join(PLANS, fname)).read().splitlines()


def delta(base, lines):
    return [l.rstrip("\n") for l in difflib.unified_diff(base, lines, "base", "plan", n=0, lineterm="")]


def assert_same_lines(what, got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{what}: first difference at line {i + 1}:\n  expected: {w}\n  got:      {g}"
    n = min(len(got), len(want))
    assert len(got) == len(want), (f"{what}: {len(got)} lines, expected {len(want)}; first difference at line {n + 1}: "
                                   f"{'unexpected ' + got[n] if len(got) > n else 'missing ' + want[n]}")


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_launch_plan(driver, name):
    how = SCENARIOS[name][3]
    layout, head, body = plan_of(driver, name)
    assert_same_lines(f"launch plan {name!r}, weight layout ({layout})", head, stored(layout))
    if how == "text":
        assert_same_lines(f"launch plan {name!r}", body, stored(name + ".txt"))
    else:
        assert SCENARIOS[how][3] == "text"
        assert_same_lines(f"launch plan {name!r}, as a diff against {how!r}", delta(stored(how + ".txt"), body), stored(name + ".diff"))
    assert body[-2].startswith("rc ") and (body[-2] == "rc 0") != name.startswith("err_")


@pytest.mark.parametrize("shape", sorted(MASK_SHAPES))
def test_override_mask_plans(driver, shape):
    want = json.load(open(os.path.join(PLANS, "hashes.json")))["override_masks"][shape]
    got = mask_plans(driver, MASK_SHAPES[shape])
    assert sorted(got) == sorted(want)
    for m in ["header"] + [f"{m:x}" for m in MASKS]:
        assert got[m] == want[m], f"launch plan under override mask 0x{m} at {shape} differs from the recorded one"


def test_dense_launch_count_matches_the_header():
    from xpoint_amd import models
    hdr = open(os.path.join(ROOT, "include", "xpoint_hip.h")).read()
    assert models.XPoint.N_DENSE_LAUNCHES == int(re.search(r"#define\s+XP_DENSE_LAUNCHES\s+(\d+)", hdr).group(1)) == 47


def record(lib_path=None):
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp, lib_path)
        plans = {name: plan_of(exe, name) for name in SCENARIOS}
        write = lambda fname, lines: open(os.path.join(PLANS, fname), "w").write("".join(l + "\n" for l in lines))      # noqa: E731
        hashes = {"override_masks": {s: mask_plans(exe, a) for s, a in MASK_SHAPES.items()}}
        for name, (layout, head, body) in plans.items():
            how = SCENARIOS[name][3]
            write(layout, head)
            if how == "text":
                write(name + ".txt", body)
            else:
                write(name + ".diff", delta(plans[how][2], body))
        json.dump(hashes, open(os.path.join(PLANS, "hashes.json"), "w"), indent=0, sort_keys=True)


if __name__ == "__main__":
    if "--record" in sys.argv:
        record()
