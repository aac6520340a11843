"""The chunked SS2D core (ss2d_pass1 / ss2d_pass2 / ss2d_pass3, csrc/ss2d_chunked.hip) and the first sequential kernel (ss2d_seq_scan + ss2d_seq_merge_ln,
csrc/ss2d_seq.hip) held to the bits of the commit BEFORE csrc/ss2d.hip was split by form: sha256 digests of every image's output,
recorded once from that commit's library by tools/make_golden_ss2d_chunked_bits.py into tests/golden/ss2d_chunked_parent_bits.json.  The dt_rank >= 16
sequential kernels are held the same way by test_gpu_ss2d_seq_bits.py.

Chunked form, forced with xp_ss2d_core_set_mode(0), at the six shapes of test_gpu_ss2d_chunk_edges.py (its docstring says which edge each reaches: partial
chunk, empty chunk slot, T = 16 and 32, the instance without bounds tests, the wave-per-pixel out_norm branch, the spilling dt_rank 48 instances), each in
the three classes: "f32" (xp_ss2d_core_fwd), "amp16" (the same entry point on f32 containers under xp_set_amp_mode(1)) and "f16" (xp_ss2d_core_fwd_f16
without f32 copies: fp16 storage).

First sequential kernel: ss2d_seq_scan<R> is taken in mode 1 when dt_rank < 16 and C % 64 == 0 ("seq1", f32 output), and at dt_rank >= 16 under
XP_SS2D_SEQ_V1=1 ("seq1v1"): the knob is read once per process, so those shapes run in ONE child process (`_child`), which prints one JSON line.

The core is batch-invariant (pinned elsewhere), so ONE digest per (shape, class, image) serves the batches 1 and 3: a batch of b images is checked image by
image against the first b digests.

Fault detection: the workspace is NaN-filled before every call and the output sits in a canary allocation; every output value must be finite and every padding
word intact."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ss2d_chunked_parent_bits.json")

CHUNKED_SHAPES = [(5, 7, 96, 6), (5, 14, 96, 6), (9, 13, 192, 12), (8, 16, 96, 6), (4, 8, 384, 24), (3, 5, 96, 48)]      # H, W, C, dt_rank
CLASSES = ("f32", "amp16", "f16")
# (C, H, W, dt_rank): a tile is 32 steps of a route
#   64, 4, 6, 4     one partial tile                                  64, 5, 7, 4     a full tile plus 3 steps
#   128, 8, 16, 8   exactly four full tiles                           192, 9, 13, 12  odd H for the column-major walk, ragged
SEQ1_SHAPES = [(64, 4, 6, 4), (64, 5, 7, 4), (128, 8, 16, 8), (192, 9, 13, 12)]
SEQ1_V1_SHAPES = [(384, 4, 6, 24), (768, 7, 9, 48)]                     # the same kernel at dt_rank >= 16: only under XP_SS2D_SEQ_V1=1
BATCHES = (1, 3)
PAY32, PAY16 = 0x7FA5C3E1, 0x7D5A       # NaN payloads no kernel produces (test_gpu_batch_invariance.py)


def _inputs(tag, B, H, W, C, R):
    """test_ss2d_core_vs_oracle's ranges from the hash generator (bit-reproducible): every image has its own values."""
    import torch
    from xpoint_amd import synth
    t = f"chunkbits/{tag}/{H}x{W}x{C}r{R}"
    g = lambda n, s, lo, hi: torch.from_numpy(synth.uniform(f"{t}/{n}", s, lo, hi)).cuda()
    return dict(u=g("u", (B, H, W, C), -0.3, 1.0), xdbl=g("xdbl", (B * H * W, 4 * (R + 2)), -0.9, 0.9), wdt=g("wdt", (4, R, C), -R ** -0.5, R ** -0.5),
                dtb=g("dtb", (4, C), -6.9, -2.25), A=-torch.exp(g("A", (4, C), -0.5, 0.5)), D=g("D", (4, C), 0.5, 1.5), lnw=g("lnw", (C,), 0.8, 1.2),
                lnb=g("lnb", (C,), -0.1, 0.1))


def _canary(rows, cols, dtype, pay):
    import torch
    full = torch.empty(((rows + 255) // 256 * 256 + 256, cols), dtype=dtype, device="cuda")
    bits = full.view(torch.int32 if dtype == torch.float32 else torch.int16)
    bits.fill_(pay)
    return full, bits


def run_case(L, inp, H, W, C, R, B, cls):
    """One call on the first B images in the form the caller has forced.  (per-image sha256 of the output bytes, every value finite, every padding word intact)."""
    import torch
    Li = H * W
    M = B * Li
    nbytes = L.load().xp_ss2d_core_workspace_bytes(B, H, W, C)
    ws = torch.full((nbytes // 4 + 16,), float("nan"), device="cuda")
    par = [L.ptr(inp[k]) for k in ("wdt", "dtb", "A", "D", "lnw", "lnb")]
    tail = (L.ptr(ws), ctypes.c_size_t(nbytes), B, H, W, C, R, 1, 1e-5, L.current_stream())
    u, xdbl = inp["u"][:B].contiguous(), inp["xdbl"][:M].contiguous()
    if cls == "f16":
        full, bits = _canary(M, C, torch.float16, PAY16)
        u16, x16 = u.half(), xdbl.half()
        L.call("xp_ss2d_core_fwd_f16", L.ptr(u16), L.ptr(x16), None, None, *par, ctypes.c_void_p(full.data_ptr()), *tail)
    elif cls == "amp16":                                                # the same half values in f32 containers
        full, bits = _canary(M, C, torch.float32, PAY32)
        u32, x32 = u.half().float(), xdbl.half().float()
        L.call("xp_set_amp_mode", 1)
        try:
            L.call("xp_ss2d_core_fwd", L.ptr(u32), L.ptr(x32), *par, ctypes.c_void_p(full.data_ptr()), *tail)
            torch.cuda.synchronize()
        finally:
            L.call("xp_set_amp_mode", 0)
    else:
        full, bits = _canary(M, C, torch.float32, PAY32)
        L.call("xp_ss2d_core_fwd", L.ptr(u), L.ptr(xdbl), *par, ctypes.c_void_p(full.data_ptr()), *tail)
    torch.cuda.synchronize()
    finite = bool(torch.isfinite(full[:M]).all())
    intact = bool((bits[M:] == (PAY32 if full.dtype == torch.float32 else PAY16)).all())
    host = full[:M].cpu().numpy()
    return [hashlib.sha256(host[i * Li:(i + 1) * Li].tobytes()).hexdigest() for i in range(B)], finite, intact


def _sweep(L, mode, group, shapes, classes, out):
    L.call("xp_ss2d_core_set_mode", mode)
    try:
        for (H, W, C, R) in shapes:
            inp = _inputs(group, max(BATCHES), H, W, C, R)
            for B in BATCHES:
                for cls in classes:
                    sha, finite, intact = run_case(L, inp, H, W, C, R, B, cls)
                    out[f"{group}/{H},{W},{C},{R}/{cls}/{B}"] = dict(sha=sha, finite=finite, intact=intact)
    finally:
        L.call("xp_ss2d_core_set_mode", -1)


def compute(v1=False):
    """{"group/H,W,C,R/class/batch": {"sha": [per image], "finite": bool, "intact": bool}}.  v1 False: the chunked form (mode 0) in its three classes and the
    first sequential kernel at dt_rank < 16 (mode 1); v1 True, in a process started with XP_SS2D_SEQ_V1=1: that kernel at dt_rank >= 16."""
    from xpoint_amd import _lib as L
    out = {}
    if v1:
        assert os.environ.get("XP_SS2D_SEQ_V1") == "1"
        _sweep(L, 1, "seq1v1", [(H, W, C, R) for (C, H, W, R) in SEQ1_V1_SHAPES], ("f32",), out)
    else:
        _sweep(L, 0, "chunked", CHUNKED_SHAPES, CLASSES, out)
        _sweep(L, 1, "seq1", [(H, W, C, R) for (C, H, W, R) in SEQ1_SHAPES], ("f32",), out)
    return out


def want_keys(v1=False):
    if v1:
        return [f"seq1v1/{H},{W},{C},{R}/f32/{B}" for (C, H, W, R) in SEQ1_V1_SHAPES for B in BATCHES]
    return ([f"chunked/{H},{W},{C},{R}/{cls}/{B}" for (H, W, C, R) in CHUNKED_SHAPES for B in BATCHES for cls in CLASSES] +
            [f"seq1/{H},{W},{C},{R}/f32/{B}" for (C, H, W, R) in SEQ1_SHAPES for B in BATCHES])


def _child():
    print("CHUNKBITS " + json.dumps(compute(v1=True)), flush=True)


def run_child():
    env = dict(os.environ, XP_SS2D_SEQ_V1="1")
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_ss2d_chunked_bits import _child; _child()"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("CHUNKBITS ")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0][len("CHUNKBITS "):])


def _check(got, want, what):
    gold = json.load(open(GOLDEN))["sha"]
    assert sorted(got) == sorted(want)
    bad = []
    for key in want:
        group, shape, cls, B = key.split("/")
        g, ref = got[key], gold[f"{group}/{shape}/{cls}"]
        assert len(ref) >= int(B), f"{key}: the golden file holds {len(ref)} images"
        if not g["finite"]:
            bad.append(f"{key}: a non-finite output value")
        if not g["intact"]:
            bad.append(f"{key}: a padding word of the output changed")
        diff = [i for i in range(int(B)) if g["sha"][i] != ref[i]]
        if diff:
            bad.append(f"{key}: images {diff} differ from the parent's bits")
    print(f"\nss2d {what} bits: {len(want)} calls, {sum(int(k.split('/')[3]) for k in want)} images against the parent's digests, {len(bad)} findings")
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_ss2d_chunked_and_first_seq_match_parent_bits(gpu_lib):
    _check(compute(), want_keys(), "chunked form + first sequential kernel")


@pytest.mark.gpu
def test_ss2d_first_seq_kernel_at_large_dt_rank_matches_parent_bits(gpu_lib):
    _check(run_child(), want_keys(v1=True), "first sequential kernel under XP_SS2D_SEQ_V1=1")
