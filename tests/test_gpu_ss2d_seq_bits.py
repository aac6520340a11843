"""The sequential SS2D core (ss2d_seq_scan2 / ss2d_seq_scan3 + ss2d_seq_merge_ln, csrc/ss2d_seq.hip) held to the bits of the commit BEFORE its kernels were refit
to two waves per SIMD: sha256 digests of every image's output, recorded once from that commit's library by
tools/make_golden_ss2d_seq_bits.py into tests/golden/ss2d_seq_parent_bits.json.

Three outputs per shape: xp_ss2d_core_fwd_ex in mode 1 as f32 rows ("f32") and as the P32 image ("p32"), and xp_ss2d_core_fwd_f16 given f32 copies ("f16").  The
core is batch-invariant and bit-identical for every NW (both pinned elsewhere), so ONE digest per (shape, output, image) serves every batch and every NW: a
batch of b images is checked image by image against the first b digests.  XP_SS2D_SEQ_NW is read once per process, so each NW runs in a child process
(`_child`), which prints one JSON line; NW 0 is the automatic choice and runs a batch in each of its regimes.

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
GOLDEN = os.path.join(ROOT, "tests", "golden", "ss2d_seq_parent_bits.json")

# (C, H, W) per image; dt_rank = C / 16.  A tile is 32 steps of a route, a workgroup has NW = 1 / 2 / 4 waves taking tiles in turn:
#   384, 4, 6    one partial tile: fewer tiles than waves          768, 4, 5    the same at dt_rank 48
#   768, 7, 9    two tiles, the second partial                      384, 8, 16   exactly four full tiles
#   384, 8, 20   five tiles: a wave's second tile meets its own deferred stores and the prefetch
#   384, 33, 29  odd H (the column-major routes' division), L % 32 != 0, 30 tiles
SHAPES = [(384, 4, 6), (768, 4, 5), (768, 7, 9), (384, 8, 16), (384, 8, 20), (384, 33, 29)]
OUTPUTS = ("f32", "p32", "f16")
NWS = ("0", "1", "2", "4")
PAY32, PAY16 = 0x7FA5C3E1, 0x7D5A       # NaN payloads no kernel produces (test_gpu_batch_invariance.py)
RESIDENT = 2                            # waves per SIMD the sequential kernels are built to fit (launch_ss2d_seq's rule; the compiler report in profiles/ss2d_seq_occupancy.txt)


def regime_batches(C, n_simd):
    """One batch per regime of launch_ss2d_seq's automatic choice: the largest NW in 4 / 2 / 1 with routes x NW <= RESIDENT x SIMDs, routes = 4 (C / 64) batch."""
    per = 4 * (C // 64)
    return {4: RESIDENT * n_simd // (4 * per), 2: RESIDENT * n_simd // (2 * per), 1: RESIDENT * n_simd // (2 * per) + 1}


def batches_for(C, nw, n_simd):
    """1 and 3 for every NW; the automatic choice also gets a batch in each of its regimes."""
    return sorted({1, 3} | (set(regime_batches(C, n_simd).values()) if nw == "0" else set()))


def max_batch(C, n_simd):
    return max(batches_for(C, "0", n_simd))


def _inputs(C, H, W, B):
    """test_ss2d_core_vs_oracle's ranges from the hash generator (bit-reproducible): every image has its own values."""
    import torch
    from xpoint_amd import synth
    R = C // 16
    t = f"seqbits/{C}x{H}x{W}"
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


def run_case(L, inp, C, H, W, B, kind):
    """One call on the first B images.  (per-image sha256 of the output bytes, every value finite, every padding word intact)."""
    import torch
    R, Li = C // 16, H * W
    M = B * Li
    nbytes = L.load().xp_ss2d_core_workspace_bytes(B, H, W, C)
    ws = torch.full((nbytes // 4 + 16,), float("nan"), device="cuda")
    par = [L.ptr(inp[k]) for k in ("wdt", "dtb", "A", "D", "lnw", "lnb")]
    tail = (L.ptr(ws), ctypes.c_size_t(nbytes), B, H, W, C, R, 1, 1e-5, L.current_stream())
    u, xdbl = inp["u"][:B].contiguous(), inp["xdbl"][:M].contiguous()
    if kind == "f16":
        full, bits = _canary(M, C, torch.float16, PAY16)
        u16, x16 = u.half(), xdbl.half()
        u32, x32 = u16.float(), x16.float()
        L.call("xp_ss2d_core_fwd_f16", L.ptr(u16), L.ptr(x16), L.ptr(u32), L.ptr(x32), *par, ctypes.c_void_p(full.data_ptr()), *tail)
    else:                                                               # the P32 image of a row has the row's size: C (hi, lo) fp16 pairs
        full, bits = _canary(M, C, torch.float32, PAY32)
        L.call("xp_ss2d_core_fwd_ex", L.ptr(u), L.ptr(xdbl), *par, ctypes.c_void_p(full.data_ptr()), 2 if kind == "p32" else 0, *tail)
    torch.cuda.synchronize()
    vals = full[:M].view(torch.float16) if kind == "p32" else full[:M]
    finite = bool(torch.isfinite(vals).all())
    intact = bool((bits[M:] == (PAY32 if full.dtype == torch.float32 else PAY16)).all())
    host = full[:M].cpu().numpy()
    return [hashlib.sha256(host[i * Li:(i + 1) * Li].tobytes()).hexdigest() for i in range(B)], finite, intact


def compute(nw):
    """{"C,H,W/kind/batch": {"sha": [per image], "finite": bool, "intact": bool}} with the sequential form forced (mode 1) in THIS process's XP_SS2D_SEQ_NW."""
    import torch
    from xpoint_amd import _lib as L
    n_simd = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    out = {}
    L.call("xp_ss2d_core_set_mode", 1)
    try:
        for (C, H, W) in SHAPES:
            inp = _inputs(C, H, W, max_batch(C, n_simd))
            for B in batches_for(C, nw, n_simd):
                for kind in OUTPUTS:
                    sha, finite, intact = run_case(L, inp, C, H, W, B, kind)
                    out[f"{C},{H},{W}/{kind}/{B}"] = dict(sha=sha, finite=finite, intact=intact)
    finally:
        L.call("xp_ss2d_core_set_mode", -1)
    return out


def _child():
    print("SEQBITS " + json.dumps(compute(os.environ.get("XP_SS2D_SEQ_NW", "0"))), flush=True)


def run_child(nw):
    env = dict(os.environ, XP_SS2D_SEQ_NW=nw)
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_ss2d_seq_bits import _child; _child()"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("SEQBITS ")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0][len("SEQBITS "):])


@pytest.mark.gpu
@pytest.mark.parametrize("nw", NWS)
def test_ss2d_seq_matches_parent_bits(gpu_lib, nw):
    import torch
    gold = json.load(open(GOLDEN))["sha"]
    n_simd = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    got = run_child(nw)
    want = [f"{C},{H},{W}/{kind}/{B}" for (C, H, W) in SHAPES for B in batches_for(C, nw, n_simd) for kind in OUTPUTS]
    assert sorted(got) == sorted(want)
    if nw == "0":                   # the automatic choice met each of its regimes
        for C in {s[0] for s in SHAPES}:
            per, b = 4 * (C // 64), regime_batches(C, n_simd)
            pick = lambda n: 4 if per * n * 4 <= RESIDENT * n_simd else (2 if per * n * 2 <= RESIDENT * n_simd else 1)
            assert b[4] >= 1 and all(pick(n) == k for k, n in b.items()), (C, b)
    bad = []
    for key in want:
        shape, kind, B = key.split("/")
        g, ref = got[key], gold[f"{shape}/{kind}"]
        assert len(ref) >= int(B), f"{key}: the golden file holds {len(ref)} images (recorded on a smaller device?)"
        if not g["finite"]:
            bad.append(f"{key}: a non-finite output value")
        if not g["intact"]:
            bad.append(f"{key}: a padding word of the output changed")
        diff = [i for i in range(int(B)) if g["sha"][i] != ref[i]]
        if diff:
            bad.append(f"{key}: images {diff[:8]}{' ...' if len(diff) > 8 else ''} differ from the parent's bits")
    print(f"\nss2d_seq bits, XP_SS2D_SEQ_NW={nw}: {len(want)} calls, {sum(int(k.split('/')[2]) for k in want)} images against the parent's digests, {len(bad)} findings")
    assert not bad, "\n".join(bad)
