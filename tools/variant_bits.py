"""Forced kernel variants (the XP_* tuning knobs) against the default dispatch.  The library reads each knob once per process, so every setting
runs in a child process of its own; the child writes its outputs and a canary verdict as .npy files into a directory, and the caller
(tests/test_gpu_batch_invariance.py) holds them to fp64 and to the default run's bits.

    python tools/variant_bits.py child OUTDIR GROUP      (GROUP: x3 | ring | f16 | mlp | scan | all)
    python tools/variant_bits.py OUTDIR                  (every setting, one child at a time; prints a summary)"""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

# (group, env) — the default run (group "all") first
VARIANTS = ([("all", {})] + [("x3", {"XP_X3_TILE": str(t)}) for t in range(5)] + [("ring", {"XP_RING_TILE": str(t)}) for t in range(3)]
            + [("f16", {"XP_F16_TILE": str(t), "XP_F16_BK": str(bk)}) for bk in (32, 64) for t in range(6)]
            + [("mlp", {"XP_MLP_NW8": "1"})] + [("scan", {k: "1"}) for k in ("XP_SCAN_V1", "XP_SCAN_V2", "XP_SCAN_OLD_GEN")])
M = 2411                                            # ragged: no tile divides it
X3_LAYERS = [(768, 192), (1536, 384), (3072, 768)]  # model (N, K), EMBED_DIM 96
RING_LAYERS = [(768, 768), (1536, 384)]
F16_LAYERS = [(768, 192), (1536, 384), (768, 3072)]
MLP_LAYERS = [(96, 384), (64, 256), (32, 128)]      # the widths XP_MLP_NW8 applies to
SCAN_CASES = [(1, 384, 4096, 1, 4), (2, 384, 768, 1, 4), (2, 384, 1024, 16, 4)]      # batch, dim, seqlen, d_state, groups: both sides of kScanV2MinLen
_TILES = ["128x32", "128x64", "128x96", "64x128", "128x128"]
_F16_TILES = ["128x32", "128x64", "128x96", "128x128", "128x192", "256x128"]
_RING_TILES = ["256x256", "256x128", "128x128"]


def expected_tags(env):
    """Profiling tags a child under this knob setting must have launched: proof that the forced variant ran."""
    if "XP_X3_TILE" in env:
        return {"gemm_x3_mfma_" + _TILES[int(env["XP_X3_TILE"])]}
    if "XP_RING_TILE" in env:
        return {"gemm_ring_h2s_" + _RING_TILES[int(env["XP_RING_TILE"])]}
    if "XP_F16_TILE" in env:
        t = int(env["XP_F16_TILE"])
        if env["XP_F16_BK"] == "32":          # the 32-deep slab has no 128 x 192 / 256 x 128 instance: 128 x 128
            return {"gemm_f16_mfma_" + _F16_TILES[min(t, 3)] + "_k32"}
        return {"gemm_f16_mfma_" + _F16_TILES[t]}
    if "XP_MLP_NW8" in env:
        return {f"proj_mlp_fused_x3_c{c}_nw8" for c, _ in MLP_LAYERS}
    if "XP_SCAN_V1" in env:
        return {"selective_scan_fwd_n1", "selective_scan_fwd_gen"}
    if "XP_SCAN_V2" in env:
        return {"selective_scan_fwd_n1v2", "selective_scan_fwd_gen"}
    if "XP_SCAN_OLD_GEN" in env:
        return {"selective_scan_fwd_old"}
    return set()
PAY32, PAY8 = 0x7FA5C3E1, 0xA5


def variant_name(env):
    return "default" if not env else "_".join(f"{k}={v}" for k, v in sorted(env.items()))


def _child(outdir, group):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from xpoint_amd import _lib as L
    st = L.current_stream()
    g = torch.Generator(device="cuda")
    g.manual_seed(99)
    canaries = []

    def seed(name):              # every case draws its own inputs, whichever groups the child runs
        g.manual_seed(sum(ord(c) * 131 ** i for i, c in enumerate(name)) % (1 << 31))

    def rand(shape, lo=-1.0, hi=1.0):
        return torch.rand(shape, generator=g, device="cuda", dtype=torch.float64).mul_(hi - lo).add_(lo).float()

    def buf(rows, cols, dtype=torch.float32, ld=None, init=None):
        ld = ld or cols
        full = torch.empty(((rows + 255) // 256 * 256 + 256, ld), dtype=dtype, device="cuda")
        pay = PAY32 if dtype == torch.float32 else 0x7D5A
        full.view(torch.int32 if dtype == torch.float32 else torch.int16).fill_(pay)
        if init is not None:
            full[:rows, :cols].copy_(init)
        keep = torch.ones(full.shape, dtype=torch.bool, device="cuda")
        keep[:rows, :cols] = False
        canaries.append((full, keep, pay))
        return full

    def bytebuf(nbytes, rows):
        full = torch.full((nbytes + ((rows + 255) // 256 * 256 + 256 - rows) * max(16, -(-nbytes // rows)),), PAY8, dtype=torch.uint8, device="cuda")
        canaries.append((full, None, nbytes))
        return full

    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    out = {}
    L.call("xp_prof_reset")
    L.call("xp_prof_enable", 1)

    def save(name, t, inputs=()):
        out[name] = t
        if group == "all":
            for i, x in enumerate(inputs):
                out[f"{name}.in{i}"] = x

    def split(kind, W, N, K):
        P = bytebuf(getattr(L.load(), f"xp_split_weights_{kind}_bytes")(N, K), N)
        L.call(f"xp_split_weights_{kind}", vp(W), vp(P), N, K, st)
        return P

    if group in ("x3", "all"):
        for (N, K) in X3_LAYERS:
            seed(f"x3_{N}_{K}")
            A0, W0, b = rand((M, K)), rand((N, K)) / K ** 0.5, rand((N,), -0.5, 0.5)
            A, W = buf(M, K, init=A0), buf(N, K, init=W0)
            C = buf(M, N, ld=N + 8)
            L.call("xp_gemm_nt_x3", vp(A), vp(split("x3", W, N, K)), vp(C), L.ptr(b), None, None, None, M, N, K, K, N + 8, N, 0, st)
            save(f"x3_{N}_{K}", C[:M, :N], (A0, W0, b))
    if group in ("ring", "all"):
        for (N, K) in RING_LAYERS:
            seed(f"ring_{N}_{K}")
            A0, W0, b = rand((M, K)), rand((N, K)) / K ** 0.5, rand((N,), -0.5, 0.5)
            A, W = buf(M, K, init=A0), buf(N, K, init=W0)
            Ap = buf(M, K)
            L.call("xp_split_activations_h2", vp(A), vp(Ap), M, K, K, st)
            C = buf(M, N, ld=N + 8)
            L.call("xp_gemm_nt_h2s", vp(Ap), vp(split("h2", W, N, K)), vp(C), 0, L.ptr(b), None, None, None, M, N, K, N + 8, N, 0, st)
            save(f"ring_{N}_{K}", C[:M, :N], (A0, W0, b))
    if group in ("f16", "all"):
        for (N, K) in F16_LAYERS:
            seed(f"f16_{N}_{K}")
            A0, W0, b = rand((M, K)).half(), (rand((N, K)) / K ** 0.5).half(), rand((N,), -0.5, 0.5)
            A, W = buf(M, K, torch.float16, init=A0), buf(N, K, torch.float16, init=W0)
            C = buf(M, N, torch.float16, ld=N + 8)
            L.call("xp_gemm_nt_f16", vp(A), vp(W), vp(C), 0, L.ptr(b), None, None, None, M, N, K, K, N + 8, N, 0, st)
            save(f"f16_{N}_{K}", C[:M, :N], (A0, W0, b))
    if group in ("mlp", "all"):
        for (Cc, H4) in MLP_LAYERS:
            seed(f"mlp_{Cc}_{H4}")
            X0, T0 = rand((M, Cc), -2.0, 2.0), rand((M, Cc))
            lw, lb = rand((Cc,), 0.5, 1.5), rand((Cc,), -0.5, 0.5)
            W1, W2, W0 = rand((H4, Cc), -0.2, 0.2), rand((Cc, H4), -0.1, 0.1), rand((Cc, Cc), -0.2, 0.2)
            b1, b2 = rand((H4,), -0.5, 0.5), rand((Cc,), -0.5, 0.5)
            X, T = buf(M, Cc, init=X0), buf(M, Cc, init=T0)
            P1, P2, P0 = split("x3", buf(H4, Cc, init=W1), H4, Cc), split("x3", buf(Cc, H4, init=W2), Cc, H4), split("x3", buf(Cc, Cc, init=W0), Cc, Cc)
            pack = bytebuf(L.load().xp_mlp_fused_x3_pack_bytes(Cc, H4, 1), 2 * H4 + Cc)
            L.call("xp_mlp_fused_x3_pack", vp(P1), vp(P2), vp(P0), vp(pack), Cc, H4, st)
            L.call("xp_mlp_fused_x3", vp(X), vp(T), L.ptr(lw), L.ptr(lb), vp(pack), L.ptr(b1), L.ptr(b2), M, Cc, H4, 1e-5, st)
            save(f"mlp_{Cc}_{H4}", X[:M], (X0, T0, lw, lb, W1, b1, W2, b2, W0))
    if group in ("scan", "all"):
        for (B, D, Ls, N, G) in SCAN_CASES:
            seed(f"scan_{B}_{D}_{Ls}_{N}_{G}")
            u0, d0 = rand((B * D, Ls)), rand((B * D, Ls), -3.0, 1.0)
            A0 = rand((D, N), -1.0, -0.05)
            B0, C0 = rand((B * G * N, Ls)), rand((B * G * N, Ls))
            D0, bias0 = rand((D,)), rand((D,), -0.5, 0.5)
            u, d, Bm, Cm = buf(B * D, Ls, init=u0), buf(B * D, Ls, init=d0), buf(B * G * N, Ls, init=B0), buf(B * G * N, Ls, init=C0)
            o = buf(B * D, Ls)
            L.call("xp_selective_scan_fwd", vp(u), vp(d), L.ptr(A0), vp(Bm), vp(Cm), L.ptr(D0), L.ptr(bias0), vp(o), None, B, D, D, Ls, N, G, 1, st)
            save(f"scan_{B}_{D}_{Ls}_{N}_{G}", o[:B * D], (u0, d0, A0, B0, C0, D0, bias0))
    torch.cuda.synchronize()
    lib = L.load()
    name = ctypes.create_string_buffer(64)
    ms, cnt, fl, by = ctypes.c_double(), ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
    tags = []
    for i in range(lib.xp_prof_count()):
        lib.xp_prof_get(i, name, 64, ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(by))
        tags.append(name.value.decode())
    L.call("xp_prof_enable", 0)
    ok = True
    for full, keep, pay in canaries:
        if keep is None:
            ok &= bool((full[pay:] == PAY8).all())
        else:
            ok &= bool((full.view(torch.int32 if full.dtype == torch.float32 else torch.int16)[keep] == pay).all())
    os.makedirs(outdir, exist_ok=True)
    for k, t in out.items():
        np.save(os.path.join(outdir, k + ".npy"), t.cpu().numpy())
    np.save(os.path.join(outdir, "canaries_intact.npy"), np.array(ok))
    with open(os.path.join(outdir, "tags.txt"), "w") as f:
        f.write("\n".join(tags))
    print("CHILD_OK", len(out), "outputs, canaries intact:", ok)


def run(outdir, timeout=300):
    """One child per setting, one at a time; {variant name: (group, env, directory)}.  A child that fails raises with its stderr: nothing retries."""
    res = {}
    for group, env in VARIANTS:
        name = variant_name(env)
        d = os.path.join(outdir, name)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", d, group], env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=timeout, cwd=ROOT)
        if r.returncode != 0 or "CHILD_OK" not in r.stdout:
            raise RuntimeError(f"variant {name} failed (exit {r.returncode}):\n{r.stderr[-3000:]}")
        res[name] = (group, env, d)
    return res


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        _child(sys.argv[2], sys.argv[3])
    else:
        for name, (group, env, d) in run(sys.argv[1] if len(sys.argv) > 1 else "variant_bits_out").items():
            print(f"{name:40s} {group:5s} {d}")
