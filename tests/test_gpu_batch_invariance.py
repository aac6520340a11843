"""Batch invariance of every dense entry point, kernel by kernel.

A kernel may pick its tile, workgroup shape or launch split from the row count M only if the choice never changes a bit.  For each such rule
these tests take a layer of the model (its (N, K) or (C, hidden) from the gemm / conv / fused-tail call sites of csrc/model.cpp, EMBED_DIM 96
and 32), pick M and M' on opposite sides of the rule's threshold, run the layer on M' rows and on the first M of those rows, and require the
shared rows to be bit-identical.  The profiling tags (xp_prof_*) prove that the two calls really ran different variants — a rule that moves
fails the test instead of leaving it testing nothing — and both sides are held to the precision class's fp64 bar.

Every buffer a call touches (inputs, outputs, residuals, weight packs) sits in a canary allocation: the rows are padded to the next multiple
of 256 plus 256 more, outputs with an ldc take ldc = N + 8, and every padding word holds one fixed NaN payload that must survive the call.
Each straddle prints one line: entry point, class, layer, M and M', the tag on each side, whether the bits agree, and err / bound."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_h2 import _f16_ref, _ulp16

pytestmark = pytest.mark.gpu

PAY32 = 0x7FA5C3E1          # a NaN payload no kernel produces (f32)
PAY16 = 0x7D5A              # the same for fp16 containers
PAY8 = 0xA5                 # weight-pack bytes

# (N, K) of every model GEMM with N >= 512: fc1 of stages 1 - 3, in_proj / out_proj and fc2 of stage 3 (EMBED_DIM 96); fc1 of stages 2 - 3 (EMBED_DIM 32)
GEMM_LAYERS = [(768, 192), (1536, 384), (768, 768), (3072, 768), (768, 3072), (512, 128), (1024, 256)]
# convolutions with Co >= 512: the stage-2 downsample (EMBED_DIM 96, 30 x 40 -> 15 x 20) and the head conv at 60 x 80 (EMBED_DIM 96 and 32)
CONV_LAYERS = [(30, 40, 384, 768, 2, 0), (60, 80, 48, 512, 1, 1), (60, 80, 16, 512, 1, 1)]
# (C, hidden) of the fused block tails (stages 0 - 1 of EMBED_DIM 96, stages 0 - 2 of EMBED_DIM 32)
MLP_LAYERS = [(96, 384), (192, 768), (32, 128), (64, 256), (128, 512)]


def _lib():
    from xpoint_amd import _lib as L
    return L


def _pad_rows(r):
    return (r + 255) // 256 * 256 + 256


class Canary:
    """A (rows, cols) tensor inside a (pad_rows(rows), ld) allocation whose every other word holds the NaN payload."""

    def __init__(self, rows, cols, dtype=torch.float32, ld=None, init=None):
        ld = ld or cols
        self.full = torch.empty((_pad_rows(rows), ld), dtype=dtype, device="cuda")
        self.pay = PAY32 if dtype == torch.float32 else PAY16
        self.bits().fill_(self.pay)
        self.keep = torch.ones(self.full.shape, dtype=torch.bool, device="cuda")
        self.keep[:rows, :cols] = False
        self.t = self.full[:rows, :cols]
        if init is not None:
            self.t.copy_(init)

    def bits(self):
        return self.full.view(torch.int32 if self.full.dtype == torch.float32 else torch.int16)

    def ptr(self):
        return ctypes.c_void_p(self.full.data_ptr())

    def intact(self):
        return bool((self.bits()[self.keep] == self.pay).all())


class ByteCanary:
    """nbytes of weight pack followed by the padding of 256 + round-up rows of `row_bytes` each, filled with PAY8."""

    def __init__(self, nbytes, rows):
        row_bytes = max(16, -(-nbytes // rows))
        self.n = nbytes
        self.full = torch.full((nbytes + (_pad_rows(rows) - rows) * row_bytes,), PAY8, dtype=torch.uint8, device="cuda")

    def ptr(self):
        return ctypes.c_void_p(self.full.data_ptr())

    def intact(self):
        return bool((self.full[self.n:] == PAY8).all())


def _rand(g, shape, lo=-1.0, hi=1.0):
    return torch.rand(shape, generator=g, device="cuda", dtype=torch.float64).mul_(hi - lo).add_(lo).float()


def _tags(fn):
    """Run fn with kernel profiling on; {tag: launches}."""
    L = _lib()
    lib = L.load()
    torch.cuda.synchronize()
    L.call("xp_prof_reset")
    L.call("xp_prof_enable", 1)
    try:
        fn()
        torch.cuda.synchronize()
        out = {}
        name = ctypes.create_string_buffer(64)
        ms, cnt, fl, by = ctypes.c_double(), ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        for i in range(lib.xp_prof_count()):
            lib.xp_prof_get(i, name, 64, ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(by))
            out[name.value.decode()] = cnt.value
    finally:
        L.call("xp_prof_enable", 0)
        L.call("xp_prof_reset")
    return out


def _shape_tag_probe():
    """Child of test_shape_tags_and_roofline_numerators (XP_PROF_SHAPES is read once per process): one launch per dense launcher with profiling on;
    prints {tag: [launches, flops, bytes]} as one JSON line."""
    import json
    L = _lib()
    lib = L.load()
    st = L.current_stream()
    g = torch.Generator(device="cuda")
    g.manual_seed(99)

    def packs(W0, N, K):
        out = []
        for kind in ("x3", "h2"):
            buf = torch.empty(getattr(lib, f"xp_split_weights_{kind}_bytes")(N, K), dtype=torch.uint8, device="cuda")
            L.call(f"xp_split_weights_{kind}", L.ptr(W0), ctypes.c_void_p(buf.data_ptr()), N, K, st)
            out.append(ctypes.c_void_p(buf.data_ptr()))
            keep.append(buf)
        return out

    keep = []
    vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    # (a) plain GEMM with a residual and GELU
    M, N, K = 130, 40, 32
    A, W, R, C = _rand(g, (M, K)), _rand(g, (N, K)), _rand(g, (M, N)), torch.empty((M, N), device="cuda")
    Wx3, Wh2 = packs(W, N, K)
    Ah, Wh, Rh, Ch = A.half(), W.half(), R.half(), torch.empty((M, N), dtype=torch.float16, device="cuda")
    # (b) strided 3 x 3 convolution: Ho 3, Wo 5, M 15, K 72
    Hi, Wi, Ci, Co = 6, 10, 8, 40
    X, Wc, Y = _rand(g, (Hi * Wi, Ci)), _rand(g, (Co, 9 * Ci)), torch.empty((15, Co), device="cuda")
    Wcx3, Wch2 = packs(Wc, Co, 9 * Ci)
    Xh, Wch, Yh = X.half(), Wc.half(), torch.empty((15, Co), dtype=torch.float16, device="cuda")
    # (c) the ping-pong kernel, (d) the ring engine on a P32 image
    Ac, Wcc, Cc = _rand(g, (130, 768)), _rand(g, (384, 768)), torch.empty((130, 384), device="cuda")
    _, Wcch2 = packs(Wcc, 384, 768)
    Ad, Wd, Cd = _rand(g, (130, 256)), _rand(g, (256, 256)), torch.empty((130, 256), device="cuda")
    _, Wdh2 = packs(Wd, 256, 256)
    Adp = torch.empty((130, 256), device="cuda")
    L.call("xp_split_activations_h2", L.ptr(Ad), L.ptr(Adp), 130, 256, 256, st)

    def run():
        L.call("xp_gemm_nt", L.ptr(A), L.ptr(W), L.ptr(C), None, None, None, L.ptr(R), M, N, K, K, N, N, 1, st)
        L.call("xp_conv3x3_nhwc", L.ptr(X), L.ptr(Wc), L.ptr(Y), None, None, None, 1, Hi, Wi, Ci, Co, 2, 0, 0, st)
        for products in (6, 3):
            _dense_products(products)
            L.call("xp_gemm_nt_x3", L.ptr(A), Wx3, L.ptr(C), None, None, None, L.ptr(R), M, N, K, K, N, N, 1, st)
            L.call("xp_conv3x3_nhwc_x3", L.ptr(X), Wcx3, L.ptr(Y), None, None, None, 1, Hi, Wi, Ci, Co, 2, 0, 0, st)
        _dense_products(6)
        L.call("xp_gemm_nt_h2", L.ptr(A), Wh2, L.ptr(C), None, None, None, L.ptr(R), M, N, K, K, N, N, 1, st)
        L.call("xp_conv3x3_nhwc_h2", L.ptr(X), Wch2, L.ptr(Y), None, None, None, 1, Hi, Wi, Ci, Co, 2, 0, 0, st)
        L.call("xp_gemm_nt_f16", vp(Ah), vp(Wh), vp(Ch), 0, None, None, None, vp(Rh), M, N, K, K, N, N, 1, st)
        L.call("xp_conv3x3_nhwc_f16", vp(Xh), vp(Wch), vp(Yh), 0, None, None, None, 1, Hi, Wi, Ci, Co, 2, 0, 0, st)
        L.call("xp_gemm_nt_h2", L.ptr(Ac), Wcch2, L.ptr(Cc), None, None, None, None, 130, 384, 768, 768, 384, 0, 0, st)
        L.call("xp_gemm_nt_h2s", L.ptr(Adp), Wdh2, L.ptr(Cd), 0, None, None, None, None, 130, 256, 256, 256, 0, 0, st)

    torch.cuda.synchronize()
    L.call("xp_prof_reset")
    L.call("xp_prof_enable", 1)
    try:
        run()
        torch.cuda.synchronize()
        out = {}
        name = ctypes.create_string_buffer(96)
        ms, cnt, fl, by = ctypes.c_double(), ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        for i in range(lib.xp_prof_count()):
            lib.xp_prof_get(i, name, 96, ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(by))
            out[name.value.decode()] = [cnt.value, fl.value, by.value]
    finally:
        L.call("xp_prof_enable", 0)
        L.call("xp_prof_reset")
    print("SHAPE_TAGS " + json.dumps(out, sort_keys=True))


# what _shape_tag_probe printed on the commit before the dense engines' host code moved into csrc/dense_host.h: the tags are strings and the numerators
# doubles formed from the same integer expressions, so equality is exact
SHAPE_TAGS = {
    "conv3x3_f16_mfma_128x64_M15_N40_K72": [1, 86400.0, 7920.0],
    "conv3x3_f32_mfma_128x64_M15_N40_K72": [1, 86400.0, 15840.0],
    "conv3x3_h2r_mfma_128x64_M15_N40_K72": [1, 86400.0, 15840.0],
    "conv3x3_x3_mfma_128x64_M15_N40_K72": [1, 86400.0, 21600.0],
    "conv3x3_x3_mfma_128x64_np3_M15_N40_K72": [1, 86400.0, 21600.0],
    "gemm_f16_mfma_128x64_k32_M130_N40_K32": [1, 332800.0, 31680.0],
    "gemm_f32_mfma_128x64_M130_N40_K32_gelu": [1, 332800.0, 63360.0],
    "gemm_h2_mfma_128x64_M130_N40_K32_gelu": [1, 332800.0, 63360.0],
    "gemm_h2p_mfma_128x128_M130_N384_K768": [1, 76677120.0, 1778688.0],
    "gemm_ring_h2s_128x128_M130_N256_K256": [1, 17039360.0, 528384.0],
    "gemm_x3_mfma_128x64_M130_N40_K32_gelu": [1, 332800.0, 65920.0],
    "gemm_x3_mfma_128x64_np3_M130_N40_K32_gelu": [1, 332800.0, 65920.0],
}


def test_shape_tags_and_roofline_numerators(gpu_lib):
    """Per-shape tags (XP_PROF_SHAPES=1) and the flops / bytes every dense launcher hands to the profiler, one case per launcher, against the recorded table."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_batch_invariance as t; t._shape_tag_probe()"], env=dict(os.environ, XP_PROF_SHAPES="1"),
                       capture_output=True, text=True, timeout=120, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("SHAPE_TAGS ")][-1]
    got = json.loads(line[len("SHAPE_TAGS "):])
    print(line)
    assert got == SHAPE_TAGS


def _report(entry, cls, layer, M, Mp, tm, tmp, equal, errs):
    e = " ".join(f"{err:.2e}/{bound:.2e}" for err, bound in errs)
    print(f"{entry:22s} {cls:4s} {str(layer):26s} M {M:6d} M' {Mp:6d}  {tm}  |  {tmp}  bits-equal {equal}  err/bound {e}")


def _dense_products(n):
    _lib().call("xp_set_dense_products", n)


def _planes(x, n):
    out, r = [], x
    for _ in range(n):
        q = r.to(torch.bfloat16).float()
        out.append(q)
        r = r - q
    return out


# the plane restatement of xp_set_dense_products 3 / 1 (test_gpu_kernels.py::test_dense_precision_classes_kernel_level): frac of the exact error allowed
TERMS = {6: None, 3: [(1, 0), (0, 1), (0, 0)], 1: [(0, 0)]}
FRAC = {3: 0.5, 1: 0.05}
# the fused tails re-truncate the LayerNorm output and the hidden activation to bf16 planes: over thousands of rows a value next to a rounding boundary
# falls the other way somewhere and moves its row by one bf16 step.  Such rows are held to the 3-product fraction ...
FRAC_FUSED = 0.5
FUSED_FLIP_ROWS = 0.02       # ... and the rows that miss the kernel-level bar FRAC[products] are that rare


def _fused_class_errors(out, emu, exact, products):
    """(max |out - restatement|, max |out - exact|, fraction of rows farther from the restatement than FRAC[products] x the exact error + 2e-5)."""
    d_emu = (out.double() - emu).abs().amax(1)
    e_exact = float((out.double() - exact).abs().max())
    return float(d_emu.max()), e_exact, float((d_emu > FRAC[products] * e_exact + 2e-5).double().mean())


def _mm(a, w, terms):
    if terms is None:
        return a.double() @ w.double().t()
    ap, wp = _planes(a.float(), 2), _planes(w.float(), 2)
    return sum(ap[i].double() @ wp[j].double().t() for i, j in terms)


# ------------------------------------------------------------------------------------------------------------------------- tile rules, restated
def _tile_by_n(N):
    """The N-only branches shared by gemm.hip / gemm_x3.hip / gemm_h2.hip dispatch: 128 x 32 / 64 / 96, or None (the M-dependent branch)."""
    if N <= 32:
        return "128x32"
    if N <= 64:
        return "128x64"
    if N <= 96 or (N % 96 == 0 and (N // 96) % 4 != 0):
        return "128x96"
    return None


def _f32_tile(M, N):          # csrc/gemm.hip dispatch(): 64 x 128 when M <= 8192 and N >= 512
    return _tile_by_n(N) or ("64x128" if M <= 8192 and N >= 512 else "128x128")


def _f32_threshold(N):
    return 8192


def _x3_tile(M, N):           # csrc/gemm_x3.hip dispatch(): 64 x 128 when M <= 8192, N >= 512 and fewer than 512 tiles of 128 x 128
    return _tile_by_n(N) or ("64x128" if M <= 8192 and N >= 512 and math.ceil(M / 128) * math.ceil(N / 128) < 512 else "128x128")


def _x3_threshold(N):
    return min(8192, 128 * (511 // math.ceil(N / 128)))


def _h2p_applies(N, K):       # csrc/gemm_h2p.hip xp_gemm_h2p_applies(): the ping-pong kernel takes K >= 768, K % 64 == 0, N >= 384 whatever M is
    return K % 64 == 0 and K >= 768 and N >= 384


def _h2_tag(M, N, K):         # csrc/gemm_h2.hip dispatch(): 64 x 128 when there are fewer than 128 tiles of 128 x 128
    t = _tile_by_n(N)
    if t is None:
        if _h2p_applies(N, K):
            return "gemm_h2p_mfma_128x128"
        t = "64x128" if math.ceil(M / 128) * math.ceil(N / 128) < 128 else "128x128"
    return "gemm_h2_mfma_" + t


def _h2_threshold(N):
    return 128 * (127 // math.ceil(N / 128))


def _ring_tile(M, N):         # csrc/gemm_ring.hip ring_dispatch(): the largest tile that still gives >= 192 workgroups
    tiles = lambda bm, bn: math.ceil(M / bm) * math.ceil(N / bn)
    return "256x256" if tiles(256, 256) >= 192 and N > 128 else "256x128" if tiles(256, 128) >= 192 else "128x128"


def _ring_thresholds(N):
    """The largest M of each smaller tile: M <= t1 -> 128 x 128, t1 < M <= t0 -> 256 x 128, above -> 256 x 256."""
    return [256 * (math.ceil(192 / math.ceil(N / 128)) - 1), 256 * (math.ceil(192 / math.ceil(N / 256)) - 1)]


def _f16_tag(N, K):           # csrc/gemm_f16.hip f16_dispatch(): tile and slab depth from the layer (N, K) only
    sel = 0 if N <= 32 else 1 if N <= 64 else 2 if (N <= 96 or (N % 96 == 0 and (N // 96) % 4 != 0)) else 3
    if K > 192:
        if 96 < N < 256 and N % 32 != 0:
            sel = 0
        if (N == 192 and K >= 512) or (N == 1536 and K <= 512):
            sel = 4
        elif N == 384 and K >= 1024:
            sel = 5
    tile = ["128x32", "128x64", "128x96", "128x128", "128x192", "256x128"][sel]
    return "gemm_f16_mfma_" + tile + ("_k32" if K <= 192 else "")


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------------------------------------ GEMM entries
def _straddle_ms(entry, N, K):
    """[(M, M')] pairs on opposite sides of each M threshold of the entry's tile rule, both ragged."""
    if entry == "f32":
        ts = [_f32_threshold(N)]
    elif entry == "x3":
        ts = [_x3_threshold(N)]
    elif entry == "h2":
        ts = [_h2_threshold(N)] if not _h2p_applies(N, K) else [2688]
    elif entry == "h2s":
        ts = _ring_thresholds(N)
    else:
        ts = [2400]               # no M rule: one pair's stage-2 rows against eight pairs'
    return [(t - 45, t + 77) if entry != "f16" else (t - 1, 8 * t + 11) for t in ts]


def _expect_tag(entry, M, N, K, products):
    if entry == "f32":
        return "gemm_f32_mfma_" + _f32_tile(M, N)
    if entry == "x3":
        return "gemm_x3_mfma_" + _x3_tile(M, N) + ("" if products == 6 else f"_np{products}")
    if entry == "h2":
        return _h2_tag(M, N, K)
    if entry == "h2s":
        return "gemm_ring_h2s_" + _ring_tile(M, N)
    return _f16_tag(N, K)


GEMM_CASES = [("f32", 6), ("x3", 6), ("x3", 3), ("x3", 1), ("h2", 6), ("h2s", 6), ("f16", 6)]


@pytest.mark.parametrize("entry,products", GEMM_CASES, ids=[f"{e}-p{p}" for e, p in GEMM_CASES])
def test_gemm_straddles_are_bit_identical(gpu_lib, entry, products):
    L = _lib()
    st = L.current_stream()
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    cls = {"f32": "f32", "x3": {6: "x3", 3: "x2", 1: "bf16"}[products], "h2": "h2", "h2s": "h2", "f16": "f16"}[entry]
    ran = 0
    _dense_products(products)
    try:
        for (N, K) in GEMM_LAYERS:
            if entry == "h2s" and not L.load().xp_gemm_nt_h2s_applies(N, K):
                continue
            act, with_res = (1, False) if N == 4 * K else (0, True)
            for (M, Mp) in _straddle_ms(entry, N, K):
                ran += 1
                _gemm_straddle(L, st, g, entry, products, cls, N, K, M, Mp, act, with_res)
    finally:
        _dense_products(6)
    assert ran >= 4


def _gemm_straddle(L, st, g, entry, products, cls, N, K, M, Mp, act, with_res):
    f16 = entry == "f16"
    dt = torch.float16 if f16 else torch.float32
    A0 = _rand(g, (Mp, K))
    W0 = _rand(g, (N, K)) / math.sqrt(K)
    bias = _rand(g, (N,), -0.5, 0.5)
    R0 = _rand(g, (Mp, N)) if with_res else None
    if f16:
        A0, W0, R0 = A0.half(), W0.half(), (R0.half() if with_res else None)
    A = Canary(Mp, K, dt, init=A0)
    Wc = Canary(N, K, dt, init=W0)
    R = Canary(Mp, N, dt, init=R0) if with_res else None
    bufs = [A, Wc] + ([R] if R else [])
    # weights in the entry's own form
    if entry == "x3":
        Wp = ByteCanary(L.load().xp_split_weights_x3_bytes(N, K), N)
        L.call("xp_split_weights_x3", Wc.ptr(), Wp.ptr(), N, K, st)
    elif entry in ("h2", "h2s"):
        Wp = ByteCanary(L.load().xp_split_weights_h2_bytes(N, K), N)
        L.call("xp_split_weights_h2", Wc.ptr(), Wp.ptr(), N, K, st)
    else:
        Wp = None
    if entry == "h2s":
        assert L.load().xp_p32_bytes(Mp, K) == Mp * K * 4
        Ap = Canary(Mp, K, torch.float32)                  # the P32 image: 4 bytes per element, rows in order
        L.call("xp_split_activations_h2", A.ptr(), Ap.ptr(), Mp, K, K, st)
        bufs.append(Ap)
    ldc = N + 8
    outs = {}
    tags = {}
    for m in (Mp, M):
        C = Canary(m, N, dt, ld=ldc)
        rp = R.ptr() if R else None
        if entry == "f32":
            fn = lambda: L.call("xp_gemm_nt", A.ptr(), Wc.ptr(), C.ptr(), L.ptr(bias), None, None, rp, m, N, K, K, ldc, N, act, st)
        elif entry == "x3":
            fn = lambda: L.call("xp_gemm_nt_x3", A.ptr(), Wp.ptr(), C.ptr(), L.ptr(bias), None, None, rp, m, N, K, K, ldc, N, act, st)
        elif entry == "h2":
            fn = lambda: L.call("xp_gemm_nt_h2", A.ptr(), Wp.ptr(), C.ptr(), L.ptr(bias), None, None, rp, m, N, K, K, ldc, N, act, st)
        elif entry == "h2s":
            fn = lambda: L.call("xp_gemm_nt_h2s", Ap.ptr(), Wp.ptr(), C.ptr(), 0, L.ptr(bias), None, None, rp, m, N, K, ldc, N, act, st)
        else:
            fn = lambda: L.call("xp_gemm_nt_f16", A.ptr(), Wc.ptr(), C.ptr(), 0, L.ptr(bias), None, None, rp, m, N, K, K, ldc, N, act, st)
        tags[m] = _tags(fn)
        assert tags[m] == {_expect_tag(entry, m, N, K, products): 1}, (entry, N, K, m, tags[m])
        assert C.intact(), f"{entry} {cls} ({N}, {K}) M = {m}: a padding word of C changed (ldc = {ldc})"
        outs[m] = C.t.clone()
    for b in bufs:
        assert b.intact(), f"{entry} {cls} ({N}, {K}): an input's padding changed"
    assert Wp is None or Wp.intact(), f"{entry} {cls} ({N}, {K}): the weight pack's padding changed"
    if entry != "f16" and not (entry == "h2" and _h2p_applies(N, K)):
        assert tags[M] != tags[Mp], f"{entry} ({N}, {K}): M = {M} and M' = {Mp} no longer straddle the tile rule"
    equal = torch.equal(outs[Mp][:M], outs[M])
    # fp64 bars, both sides
    errs = []
    if f16:
        ref, mag = _f16_ref(A0, W0, bias, None, None, R0, act)
        noise = 4e-6 * F.linear(A0.double().abs(), W0.double().abs())
        for m in (Mp, M):
            d = (outs[m].double() - ref[:m]).abs()
            ulps = float(((d - noise[:m]).clamp_min(0) / _ulp16(mag[:m])).max())
            errs.append((ulps, 2.01))
            assert ulps <= 2.01 and float((d == 0).double().mean()) > 0.97, (entry, N, K, m, ulps)
    else:
        def finish(acc):
            v = acc + bias.double()
            if act == 1:
                v = F.gelu(v)
            return v + R0.double() if with_res else v
        exact = finish(_mm(A0, W0, None))
        scale = max(1.0, float(exact.abs().max()))
        if entry == "x3" and products != 6:
            emu = finish(_mm(A0, W0, TERMS[products]))
            for m in (Mp, M):
                e_emu = float((outs[m].double() - emu[:m]).abs().max())
                e_exact = float((outs[m].double() - exact[:m]).abs().max())
                bound = 5e-6 * scale
                errs.append((e_emu, bound))
                # as test_dense_precision_classes_kernel_level: on the class's restatement, far closer to it than to the exact result, and the class differs
                assert e_emu <= bound and e_emu <= FRAC[products] * e_exact, (entry, products, N, K, m, e_emu, e_exact)
                assert products != 1 or e_exact > 1e-3, (entry, N, K, m, e_exact)
        else:
            if entry != "f32":
                C32 = torch.empty((Mp, N), device="cuda")
                L.call("xp_gemm_nt", L.ptr(A0), L.ptr(W0), L.ptr(C32), L.ptr(bias), None, None, L.ptr(R0), Mp, N, K, K, N, N, act, st)
            for m in (Mp, M):
                err = float((outs[m].double() - exact[:m]).abs().max())
                bound = 2e-5 * scale
                if entry != "f32":
                    bound = min(bound, 2.0 * float((C32[:m].double() - exact[:m]).abs().max()) + 1e-7)
                errs.append((err, bound))
                assert err <= bound, (entry, N, K, m, err, bound)
    _report(entry, cls, (N, K), M, Mp, next(iter(tags[M])), next(iter(tags[Mp])), equal, errs)
    assert equal, f"{entry} {cls} ({N}, {K}): rows 0..{M} differ between M = {M} and M' = {Mp}"


# ------------------------------------------------------------------------------------------------------------------------------ convolutions
CONV_CASES = [("f32", 6), ("x3", 6), ("x3", 3), ("x3", 1)]


@pytest.mark.parametrize("entry,products", CONV_CASES, ids=[f"{e}-p{p}" for e, p in CONV_CASES])
def test_conv_straddles_are_bit_identical(gpu_lib, entry, products):
    """The implicit-GEMM convolutions take their tile from M = batch * Ho * Wo: the straddle changes the batch."""
    L = _lib()
    st = L.current_stream()
    g = torch.Generator(device="cuda")
    g.manual_seed(4321)
    cls = {"f32": "f32", "x3": {6: "x3", 3: "x2", 1: "bf16"}[products]}[entry]
    _dense_products(products)
    try:
        for (Hi, Wi, Ci, Co, stride, reflect) in CONV_LAYERS:
            Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
            thr = _f32_threshold(Co) if entry == "f32" else _x3_threshold(Co)
            B = thr // (Ho * Wo)                          # the largest batch on the small-M side
            Bp = B + 1
            head = stride == 1
            act = 2 if head else 0
            x0 = _rand(g, (Bp * Hi * Wi, Ci))
            w0 = _rand(g, (Co, 9 * Ci)) / math.sqrt(9 * Ci)
            b = _rand(g, (Co,), -0.5, 0.5)
            sc, sh = (_rand(g, (Co,), 0.5, 1.5), _rand(g, (Co,), -0.5, 0.5)) if head else (None, None)
            X = Canary(Bp * Hi * Wi, Ci, init=x0)
            Wc = Canary(Co, 9 * Ci, init=w0)
            if entry == "x3":
                Wp = ByteCanary(L.load().xp_split_weights_x3_bytes(Co, 9 * Ci), Co)
                L.call("xp_split_weights_x3", Wc.ptr(), Wp.ptr(), Co, 9 * Ci, st)
            outs, tags = {}, {}
            for bb in (Bp, B):
                Y = Canary(bb * Ho * Wo, Co)
                if entry == "f32":
                    fn = lambda: L.call("xp_conv3x3_nhwc", X.ptr(), Wc.ptr(), Y.ptr(), L.ptr(b), L.ptr(sc), L.ptr(sh), bb, Hi, Wi, Ci, Co, stride, reflect, act, st)
                    tile = _f32_tile(bb * Ho * Wo, Co)
                else:
                    fn = lambda: L.call("xp_conv3x3_nhwc_x3", X.ptr(), Wp.ptr(), Y.ptr(), L.ptr(b), L.ptr(sc), L.ptr(sh), bb, Hi, Wi, Ci, Co, stride, reflect, act, st)
                    tile = _x3_tile(bb * Ho * Wo, Co)
                tags[bb] = _tags(fn)
                want = ("conv3x3_f32_mfma_" if entry == "f32" else "conv3x3_x3_mfma_") + tile + ("" if entry == "f32" or products == 6 else f"_np{products}")
                assert tags[bb] == {want: 1}, (entry, Co, bb, tags[bb])
                assert Y.intact(), f"{entry} conv Co = {Co}, batch {bb}: a padding word of the output changed"
                outs[bb] = Y.t.clone()
            assert X.intact() and Wc.intact() and (entry == "f32" or Wp.intact())
            assert tags[B] != tags[Bp], "the straddle no longer crosses the tile rule"
            equal = torch.equal(outs[Bp][:B * Ho * Wo], outs[B])

            def conv(xx, ww):
                xin = xx.double().view(Bp, Hi, Wi, Ci).permute(0, 3, 1, 2)
                if reflect:
                    xin = F.pad(xin, (1, 1, 1, 1), mode="reflect")
                wt = ww.double().view(Co, 3, 3, Ci).permute(0, 3, 1, 2)
                return F.conv2d(xin, wt, None, stride=stride, padding=0 if reflect else 1).permute(0, 2, 3, 1).reshape(Bp * Ho * Wo, Co)

            def finish(acc):
                v = acc + b.double()
                if act == 2:
                    v = v.clamp_min(0) * sc.double() + sh.double()
                return v

            exact = finish(conv(x0, w0))
            scale = max(1.0, float(exact.abs().max()))
            errs = []
            for bb in (Bp, B):
                m = bb * Ho * Wo
                err = float((outs[bb].double() - exact[:m]).abs().max())
                if entry == "x3" and products != 6:
                    xp_, wp_ = _planes(x0, 2), _planes(w0, 2)
                    emu = finish(sum(conv(xp_[i], wp_[j]) for i, j in TERMS[products]))
                    e_emu = float((outs[bb].double() - emu[:m]).abs().max())
                    bound = 5e-6 * scale
                    errs.append((e_emu, bound))
                    assert e_emu <= bound and e_emu <= FRAC[products] * err, (entry, products, Co, bb, e_emu, err)
                    assert products != 1 or err > 1e-3, (entry, Co, bb, err)
                else:
                    errs.append((err, 2e-5 * scale))
                    assert err <= 2e-5 * scale, (entry, Co, bb, err)
            _report("conv3x3 " + entry, cls, (Hi, Wi, Ci, Co, stride), B * Ho * Wo, Bp * Ho * Wo, next(iter(tags[B])), next(iter(tags[Bp])), equal, errs)
            assert equal, f"{entry} conv Co = {Co}: batch {B} differs from the first {B} images of batch {Bp}"
    finally:
        _dense_products(6)


# ------------------------------------------------------------------------------------------------------------------------------ fused block tails
def _mlp_straddles(engine, C):
    """The h2 instances at C = 192 (csrc/mlp_fused.hip launch_mlp_pre): 4-wave workgroups when M <= n_cu * 128, else 8-wave ones with the last round
    run as a second 4-wave launch when it is at most half full.  M on the small side, M' with a split tail: 1 launch against 2.  Everything else has
    no M rule: a ragged M against a larger ragged M'."""
    if engine == "h2" and C == 192:
        n = _n_cu()
        return [(n * 128 - 45, n * 256 + n * 64 + 77, 1, 2)]
    return [(2399, 4811, 1, 1)]


def _mlp_tag(kind, engine, C, products):
    if engine == "f16":
        return ("mlp_fused_f16_c" if kind == "mlp" else "ln_proj_f16_c") + str(C)
    tag = ("proj_mlp_fused_" if kind == "mlp" else "ln_proj_") + engine + "_c" + str(C)        # the x3 / h2 tails run with out_proj (T1)
    return tag + (f"_np{products}" if engine == "x3" and products != 6 else "")


MLP_CASES = [("mlp", "x3", 6), ("mlp", "x3", 3), ("mlp", "x3", 1), ("mlp", "h2", 6), ("mlp", "f16", 6),
             ("ln_proj", "x3", 6), ("ln_proj", "x3", 3), ("ln_proj", "x3", 1), ("ln_proj", "h2", 6), ("ln_proj", "f16", 6)]


@pytest.mark.parametrize("kind,engine,products", MLP_CASES, ids=[f"{k}-{e}-p{p}" for k, e, p in MLP_CASES])
def test_fused_tail_straddles_are_bit_identical(gpu_lib, kind, engine, products):
    L = _lib()
    st = L.current_stream()
    g = torch.Generator(device="cuda")
    g.manual_seed(777)
    cls = {"x3": {6: "x3", 3: "x2", 1: "bf16"}[products], "h2": "h2", "f16": "f16"}[engine]
    _dense_products(products)
    try:
        for (C, H4) in MLP_LAYERS:
            if engine == "f16" and not L.load().xp_mlp_fused_f16_supported(C, H4):
                continue
            for (M, Mp, n_m, n_mp) in _mlp_straddles(engine, C):
                if kind == "mlp":
                    _mlp_straddle(L, st, g, engine, products, cls, C, H4, M, Mp, n_m, n_mp)
                else:
                    _ln_proj_straddle(L, st, g, engine, products, cls, C, M, Mp, n_m, n_mp)
    finally:
        _dense_products(6)


def _split(L, st, entry, Wc, N, K):
    Wp = ByteCanary((L.load().xp_split_weights_x3_bytes if entry == "x3" else L.load().xp_split_weights_h2_bytes)(N, K), N)
    L.call("xp_split_weights_x3" if entry == "x3" else "xp_split_weights_h2", Wc.ptr(), Wp.ptr(), N, K, st)
    return Wp


def _check_launches(tags, want_tag, n):
    assert tags == {want_tag: n}, (tags, want_tag, n)


def _mlp_straddle(L, st, g, engine, products, cls, C, H4, M, Mp, n_m, n_mp):
    f16 = engine == "f16"
    dt = torch.float16 if f16 else torch.float32
    X0 = _rand(g, (Mp, C), -2.0, 2.0)
    T10 = _rand(g, (Mp, C))
    lw, lb = _rand(g, (C,), 0.5, 1.5), _rand(g, (C,), -0.5, 0.5)
    W10, W20, W00 = _rand(g, (H4, C), -0.2, 0.2), _rand(g, (C, H4), -0.1, 0.1), _rand(g, (C, C), -0.2, 0.2)
    b1, b2 = _rand(g, (H4,), -0.5, 0.5), _rand(g, (C,), -0.5, 0.5)
    if f16:
        X0, T10, W10, W20 = X0.half(), T10.half(), W10.half(), W20.half()     # f16: T1 is the block's normalised input `a`
    W1, W2 = Canary(H4, C, dt, init=W10), Canary(C, H4, dt, init=W20)
    T1 = Canary(Mp, C, dt, init=T10)
    bufs, packs = [W1, W2, T1], []
    if engine == "x3":
        W0 = Canary(C, C, init=W00)
        W1x, W2x, W0x = _split(L, st, "x3", W1, H4, C), _split(L, st, "x3", W2, C, H4), _split(L, st, "x3", W0, C, C)
        pack = ByteCanary(L.load().xp_mlp_fused_x3_pack_bytes(C, H4, 1), 2 * H4 + C)
        L.call("xp_mlp_fused_x3_pack", W1x.ptr(), W2x.ptr(), W0x.ptr(), pack.ptr(), C, H4, st)
        bufs.append(W0); packs += [W1x, W2x, W0x, pack]
    elif engine == "h2":
        W0 = Canary(C, C, init=W00)
        W1x, W2x, W0x = _split(L, st, "h2", W1, H4, C), _split(L, st, "h2", W2, C, H4), _split(L, st, "h2", W0, C, C)
        pack = ByteCanary(L.load().xp_mlp_fused_h2_pack_bytes(C, H4, 1), 2 * H4 + C)
        L.call("xp_mlp_fused_h2_pack", W1x.ptr(), W2x.ptr(), W0x.ptr(), pack.ptr(), C, H4, st)
        bufs.append(W0); packs += [W1x, W2x, W0x, pack]
    outs, tags = {}, {}
    for m, n in ((Mp, n_mp), (M, n_m)):
        X = Canary(m, C, dt, init=X0[:m])
        if engine == "x3":
            fn = lambda: L.call("xp_mlp_fused_x3", X.ptr(), T1.ptr(), L.ptr(lw), L.ptr(lb), pack.ptr(), L.ptr(b1), L.ptr(b2), m, C, H4, 1e-5, st)
        elif engine == "h2":
            fn = lambda: L.call("xp_mlp_fused_h2", X.ptr(), T1.ptr(), L.ptr(lw), L.ptr(lb), pack.ptr(), W1x.ptr(), W2x.ptr(), W0x.ptr(),
                                L.ptr(b1), L.ptr(b2), m, C, H4, 1e-5, st)
        else:
            fn = lambda: L.call("xp_mlp_fused_f16", T1.ptr(), X.ptr(), W1.ptr(), L.ptr(b1), W2.ptr(), L.ptr(b2), m, C, H4, st)
        tags[m] = _tags(fn)
        _check_launches(tags[m], _mlp_tag("mlp", engine, C, products), n)
        assert X.intact(), f"mlp {engine} C = {C}, M = {m}: a padding word of X changed"
        outs[m] = X.t.clone()
    assert all(b.intact() for b in bufs + packs), f"mlp {engine} C = {C}: an input's or a weight pack's padding changed"
    equal = torch.equal(outs[Mp][:M], outs[M])
    errs = []
    if f16:
        h = (F.gelu((F.linear(T10.double(), W10.double()) + b1.double()).float().half().double()).float().half().double())
        y = (F.linear(h, W20.double()) + b2.double()).float().half().double()
        ref = (y + X0.double()).float().half().double()
        mag = torch.maximum(ref.abs(), y.abs())
        noise = 4e-6 * F.linear(h.abs(), W20.double().abs())
        for m in (Mp, M):
            d = (outs[m].double() - ref[:m]).abs()
            u = float(((d - noise[:m]).clamp_min(0) / _ulp16(mag[:m])).max())
            # test_mlp_fused_f16's 2.01 ulps on all but the elements whose hidden value sits on an fp16 rounding boundary (the f32 order of fc1 decides it):
            # such a flip moves its element by at most one more ulp, and flips are rare
            ulp = ((d - noise[:m]).clamp_min(0) / _ulp16(mag[:m]))
            flips = float((ulp > 2.01).double().mean())
            errs.append((u, 3.01))
            assert u <= 3.01 and flips <= 1e-4 and float((d == 0).double().mean()) > 0.95, (C, m, u, flips)
    else:
        def chain(t):
            x1 = X0.double() + _mm(T10, W00, t)
            hh = F.layer_norm(x1.float(), (C,), lw, lb, 1e-5)
            hh = F.gelu((_mm(hh, W10, t) + b1.double()).float())
            return x1 + _mm(hh, W20, t) + b2.double()
        exact = chain(None)
        scale = max(1.0, float(exact.abs().max()))
        if engine == "x3" and products != 6:
            emu = chain(TERMS[products])
            for m in (Mp, M):
                e_emu, e_exact, flips = _fused_class_errors(outs[m], emu[:m], exact[:m], products)
                bound = FRAC_FUSED * e_exact + 2e-5
                errs.append((e_emu, bound))
                print(f"    rows off the class restatement's bar: {flips:.4f}")
                assert e_emu <= bound and flips <= FUSED_FLIP_ROWS, (engine, products, C, m, e_emu, e_exact, flips)
        else:
            # the exact-f32 launches the fused kernel replaces (out_proj + residual, LayerNorm, fc1 + GELU, fc2 + residual)
            Xr = X0.clone(); Tn = torch.empty_like(Xr); Hb = torch.empty((Mp, H4), device="cuda")
            L.call("xp_gemm_nt", L.ptr(T10), L.ptr(W00), L.ptr(Xr), None, None, None, L.ptr(Xr), Mp, C, C, C, C, C, 0, st)
            L.call("xp_layernorm", L.ptr(Xr), L.ptr(Tn), L.ptr(lw), L.ptr(lb), Mp, C, 1e-5, 0, st)
            L.call("xp_gemm_nt", L.ptr(Tn), L.ptr(W10), L.ptr(Hb), L.ptr(b1), None, None, None, Mp, H4, C, C, H4, 0, 1, st)
            L.call("xp_gemm_nt", L.ptr(Hb), L.ptr(W20), L.ptr(Xr), L.ptr(b2), None, None, L.ptr(Xr), Mp, C, H4, H4, C, C, 0, st)
            for m in (Mp, M):
                err = float((outs[m].double() - exact[:m]).abs().max())
                bound = min(2e-5 * scale, 2.0 * float((Xr[:m].double() - exact[:m]).abs().max()) + 1e-6)
                errs.append((err, bound))
                assert err <= bound, (engine, C, m, err, bound)
    if n_m != n_mp:
        assert tags[M] != tags[Mp], f"mlp {engine} C = {C}: M = {M} and M' = {Mp} no longer straddle the launch rules"
    _report("mlp_fused_" + engine, cls, (C, H4), M, Mp, tags[M], tags[Mp], equal, errs)
    assert equal, f"mlp {engine} C = {C}: rows 0..{M} differ between M = {M} and M' = {Mp}"


def _ln_proj_straddle(L, st, g, engine, products, cls, C, M, Mp, n_m, n_mp):
    """LayerNorm + in_proj (N = C, the model's call) in one launch."""
    f16 = engine == "f16"
    dt = torch.float16 if f16 else torch.float32
    N = C
    X0 = _rand(g, (Mp, C), -2.0, 2.0)
    lw, lb = _rand(g, (C,), 0.5, 1.5), _rand(g, (C,), -0.5, 0.5)
    W00 = _rand(g, (N, C), -0.3, 0.3)
    if f16:
        X0, W00 = X0.half(), W00.half()
    X = Canary(Mp, C, dt, init=X0)
    W0 = Canary(N, C, dt, init=W00)
    packs = []
    if engine != "f16":
        W0x = _split(L, st, engine, W0, N, C)
        nb = (L.load().xp_ln_proj_x3_pack_bytes if engine == "x3" else L.load().xp_ln_proj_h2_pack_bytes)(C, N)
        assert nb > 0
        pack = ByteCanary(nb, N)
        L.call(f"xp_ln_proj_{engine}_pack", W0x.ptr(), pack.ptr(), C, N, st)
        packs = [W0x, pack]
    outs, tags = {}, {}
    for m, n in ((Mp, n_mp), (M, n_m)):
        Y = Canary(m, N, dt)
        if engine == "x3":
            fn = lambda: L.call("xp_ln_proj_x3", X.ptr(), L.ptr(lw), L.ptr(lb), pack.ptr(), Y.ptr(), m, C, N, 1e-5, st)
        elif engine == "h2":
            fn = lambda: L.call("xp_ln_proj_h2", X.ptr(), L.ptr(lw), L.ptr(lb), pack.ptr(), W0x.ptr(), Y.ptr(), m, C, N, 1e-5, st)
        else:
            fn = lambda: L.call("xp_ln_proj_f16", X.ptr(), L.ptr(lw), L.ptr(lb), ctypes.c_float(1e-5), W0.ptr(), Y.ptr(), m, C, st)
        tags[m] = _tags(fn)
        _check_launches(tags[m], _mlp_tag("ln_proj", engine, C, products), n)
        assert Y.intact(), f"ln_proj {engine} C = {C}, M = {m}: a padding word of the output changed"
        outs[m] = Y.t.clone()
    assert X.intact() and W0.intact() and all(p.intact() for p in packs), f"ln_proj {engine} C = {C}: an input's padding changed"
    equal = torch.equal(outs[Mp][:M], outs[M])
    errs = []
    ln = F.layer_norm(X0.double(), (C,), lw.double(), lb.double(), 1e-5)
    if f16:
        # a = r16(LN(x)) may fall one fp16 ulp either way of the kernel's (the order of the row sums): bound its effect by one ulp of every |a| |w| term
        a = ln.float().half().double()
        ref = F.linear(a, W00.double()).float().half().double()
        slack = F.linear(_ulp16(a), W00.double().abs())
        for m in (Mp, M):
            d = (outs[m].double() - ref[:m]).abs()
            u = float(((d - slack[:m]).clamp_min(0) / _ulp16(ref[:m])).max())
            errs.append((u, 2.01))
            assert u <= 2.01 and float((d == 0).double().mean()) > 0.9, (C, m, u)
    else:
        exact = _mm(ln.float(), W00, None)
        scale = max(1.0, float(exact.abs().max()))
        if engine == "x3" and products != 6:
            emu = _mm(ln.float(), W00, TERMS[products])
            for m in (Mp, M):
                e_emu, e_exact, flips = _fused_class_errors(outs[m], emu[:m], exact[:m], products)
                bound = FRAC_FUSED * e_exact + 2e-5
                errs.append((e_emu, bound))
                print(f"    rows off the class restatement's bar: {flips:.4f}")
                assert e_emu <= bound and flips <= FUSED_FLIP_ROWS, (engine, products, C, m, e_emu, e_exact, flips)
        else:
            Tn = torch.empty((Mp, C), device="cuda"); Y32 = torch.empty((Mp, N), device="cuda")
            L.call("xp_layernorm", L.ptr(X0), L.ptr(Tn), L.ptr(lw), L.ptr(lb), Mp, C, 1e-5, 0, st)
            L.call("xp_gemm_nt", L.ptr(Tn), L.ptr(W00), L.ptr(Y32), None, None, None, None, Mp, N, C, C, N, 0, 0, st)
            for m in (Mp, M):
                err = float((outs[m].double() - exact[:m]).abs().max())
                bound = min(2e-5 * scale, 2.0 * float((Y32[:m].double() - exact[:m]).abs().max()) + 1e-6)
                errs.append((err, bound))
                assert err <= bound, (engine, C, m, err, bound)
    _report("ln_proj_" + engine, cls, (C, N), M, Mp, tags[M], tags[Mp], equal, errs)
    assert equal, f"ln_proj {engine} C = {C}: rows 0..{M} differ between M = {M} and M' = {Mp}"


# ------------------------------------------------------------------------------------------------------------------------------ selective scan
SCAN_V2_MIN_LEN = 4096         # csrc/selective_scan.hip kScanV2MinLen: d_state 1 rows at least this long run the 8-item kernel, whatever batch * dim is


@pytest.mark.parametrize("seqlen", [1024, 4096])
def test_selective_scan_rows_do_not_depend_on_the_batch(gpu_lib, seqlen):
    """xp_selective_scan_fwd, d_state 1, dim 1536 (4 groups of 384 channels): batch 1 against the first sequence of batch 3.  The kernel used to pick
    its scan (8-item DPP / 4-item shuffle, different association) from batch * dim < 3072, so one sequence's output depended on the rest of the call."""
    L = _lib()
    st = L.current_stream()
    g = torch.Generator(device="cuda")
    g.manual_seed(seqlen)
    dim, G, N, Bp = 1536, 4, 1, 3
    u0 = _rand(g, (Bp * dim, seqlen))
    dl0 = _rand(g, (Bp * dim, seqlen), -3.0, 1.0)
    A0 = _rand(g, (dim, N), -1.0, -0.05)
    B0, C0 = _rand(g, (Bp * G * N, seqlen)), _rand(g, (Bp * G * N, seqlen))
    D0, bias0 = _rand(g, (dim,)), _rand(g, (dim,), -0.5, 0.5)
    u, dl, Bm, Cm = (Canary(t.shape[0], seqlen, init=t) for t in (u0, dl0, B0, C0))
    outs, tags = {}, {}
    for b in (Bp, 1):
        out = Canary(b * dim, seqlen)
        fn = lambda: L.call("xp_selective_scan_fwd", u.ptr(), dl.ptr(), L.ptr(A0), Bm.ptr(), Cm.ptr(), L.ptr(D0), L.ptr(bias0), out.ptr(), None,
                            b, dim, dim, seqlen, N, G, 1, st)
        tags[b] = _tags(fn)
        assert tags[b] == {"selective_scan_fwd_n1v2" if seqlen >= SCAN_V2_MIN_LEN else "selective_scan_fwd_n1": 1}, tags[b]
        assert out.intact(), f"scan batch {b}: a padding word of out changed"
        outs[b] = out.t.clone()
    assert all(t.intact() for t in (u, dl, Bm, Cm))
    equal = torch.equal(outs[Bp][:dim], outs[1])
    # fp64 recurrence: delta = softplus(delta + bias) (torch threshold 20), h_t = exp(delta A) h_{t-1} + delta B_t u_t, y_t = C_t h_t + D u_t
    rows = Bp * dim
    grp = (torch.arange(rows, device="cuda") // dim) * G + (torch.arange(rows, device="cuda") % dim) // (dim // G)
    d = dl0.double() + bias0.double().repeat(Bp)[:, None]
    d = torch.where(d <= 20.0, F.softplus(d), d)
    a = torch.exp(d * A0.double()[:, 0].repeat(Bp)[:, None])
    bu = d * B0.double()[grp] * u0.double()
    h = torch.zeros(rows, dtype=torch.float64, device="cuda")
    ys = torch.empty((rows, seqlen), dtype=torch.float64, device="cuda")
    for t in range(seqlen):
        h = a[:, t] * h + bu[:, t]
        ys[:, t] = h
    ref = ys * C0.double()[grp] + D0.double().repeat(Bp)[:, None] * u0.double()
    errs = []
    for b in (Bp, 1):
        r = ref[:b * dim]
        err = float((outs[b].double() - r).abs().max())
        bound = 1e-5 * float(r.abs().max())
        errs.append((err, bound))
        assert err <= bound, (seqlen, b, err, bound)
    _report("selective_scan_fwd", "f32", (dim, seqlen, N), dim, Bp * dim, tags[1], tags[Bp], equal, errs)
    assert equal, f"scan: the first sequence of batch {Bp} differs from the same sequence alone"


# ------------------------------------------------------------------------------------------------------------------------------ forced variants
def _scan_ref(u0, d0, A0, B0, C0, D0, bias0, G):
    """fp64 selective scan (softplus threshold 20), rows (B * D, L), B / C (B * G * N, L)."""
    rows, Ls = u0.shape
    D, N = A0.shape
    r = torch.arange(rows, device="cuda")
    grp = (r // D) * G + (r % D) // (D // G)
    d = d0.double() + bias0.double().repeat(rows // D)[:, None]
    d = torch.where(d <= 20.0, F.softplus(d), d)
    A = A0.double().repeat(rows // D, 1)                                  # (rows, N)
    Bv = B0.double().view(-1, N, Ls)[grp]                                 # (rows, N, L)
    Cv = C0.double().view(-1, N, Ls)[grp]
    h = torch.zeros((rows, N), dtype=torch.float64, device="cuda")
    y = torch.empty((rows, Ls), dtype=torch.float64, device="cuda")
    for t in range(Ls):
        h = torch.exp(d[:, t:t + 1] * A) * h + (d[:, t:t + 1] * u0[:, t:t + 1].double()) * Bv[:, :, t]
        y[:, t] = (h * Cv[:, :, t]).sum(1)
    return y + D0.double().repeat(rows // D)[:, None] * u0.double()


def test_forced_variants_against_fp64_and_default_bits(gpu_lib, tmp_path):
    """Every tuning knob of the dense and scan kernels (XP_X3_TILE, XP_RING_TILE, XP_F16_TILE x XP_F16_BK, XP_MLP_NW8, XP_SCAN_V1 / V2 / OLD_GEN) in a
    child process of its own (tools/variant_bits.py), model layers at a ragged M with canary padding: each variant holds its class's fp64 bar and
    leaves the padding alone; where the code claims bit-identity (every x3 tile, every ring tile, every f16 tile at one slab depth, 8-wave against
    4-wave MLP workgroups) the bits equal the default run's."""
    import importlib.util
    import os
    import numpy as np
    spec = importlib.util.spec_from_file_location("variant_bits", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "variant_bits.py"))
    vb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vb)
    runs = vb.run(str(tmp_path))
    load = lambda d, k: torch.from_numpy(np.load(os.path.join(d, k + ".npy"))).cuda()
    dflt = runs["default"][2]
    L = _lib()
    st = L.current_stream()
    f16_by_bk = {}
    failures = []

    def check(ok, what):
        if not ok:
            failures.append(what)
    for name, (group, env, d) in runs.items():
        check(bool(np.load(os.path.join(d, "canaries_intact.npy"))), f"{name}: a canary word changed")
        ran = set(open(os.path.join(d, "tags.txt")).read().split())
        check(vb.expected_tags(env) <= ran, f"{name}: the forced variant did not run ({sorted(vb.expected_tags(env))} not all in {sorted(ran)})")
        keys = sorted(f[:-4] for f in os.listdir(d) if f.endswith(".npy") and ".in" not in f and f != "canaries_intact.npy")
        assert keys, name
        for k in keys:
            got = load(d, k)
            ins = [load(dflt, f"{k}.in{i}") for i in range(9) if os.path.exists(os.path.join(dflt, f"{k}.in{i}.npy"))]
            same = torch.equal(got, load(dflt, k))
            kind = k.split("_")[0]
            if kind in ("x3", "ring"):
                A0, W0, b = ins
                ref = A0.double() @ W0.double().t() + b.double()
                C32 = torch.empty(ref.shape, device="cuda")
                L.call("xp_gemm_nt", L.ptr(A0), L.ptr(W0), L.ptr(C32), L.ptr(b), None, None, None, A0.shape[0], W0.shape[0], W0.shape[1], W0.shape[1],
                       W0.shape[0], 0, 0, st)
                err = float((got.double() - ref).abs().max())
                bound = min(2e-5 * max(1.0, float(ref.abs().max())), 2.0 * float((C32.double() - ref).abs().max()) + 1e-7)
                check(err <= bound, (name, k, err, bound))
                check(same, f"{name}: {k} differs from the default tile's bits")
            elif kind == "f16":
                A0, W0, b = ins
                ref, mag = _f16_ref(A0, W0, b, None, None, None, 0)
                dd = (got.double() - ref).abs()
                noise = 4e-6 * F.linear(A0.double().abs(), W0.double().abs())
                err, bound = float(((dd - noise).clamp_min(0) / _ulp16(mag)).max()), 2.01
                check(err <= bound and float((dd == 0).double().mean()) > 0.97, (name, k, err))
                if group == "f16":
                    f16_by_bk.setdefault((env["XP_F16_BK"], k), []).append((name, got))
            elif kind == "mlp":
                X0, T0, lw, lb, W1, b1, W2, b2, W0 = ins
                x1 = X0.double() + T0.double() @ W0.double().t()
                hh = F.gelu(F.layer_norm(x1, (x1.shape[1],), lw.double(), lb.double(), 1e-5) @ W1.double().t() + b1.double())
                ref = x1 + hh @ W2.double().t() + b2.double()
                err, bound = float((got.double() - ref).abs().max()), 2e-5 * max(1.0, float(ref.abs().max()))
                check(err <= bound, (name, k, err))
                check(same, f"{name}: {k} differs from the 4-wave workgroups' bits")
            else:
                u0, d0, A0, B0, C0, D0, bias0 = ins
                ref = _scan_ref(u0, d0, A0, B0, C0, D0, bias0, int(k.split("_")[-1]))
                err, bound = float((got.double() - ref).abs().max()), 1e-5 * float(ref.abs().max())
                check(err <= bound, (name, k, err, bound))
            print(f"variant {name:32s} {k:18s} err/bound {err:.2e}/{bound:.2e}  bits equal to default {same}")
    for (bk, k), outs in f16_by_bk.items():              # f16: every tile at one slab depth walks K in the same order
        for name, got in outs[1:]:
            check(torch.equal(got, outs[0][1]), f"{name}: {k} differs from {outs[0][0]} at BK = {bk}")
    assert not failures, "\n".join(map(str, failures))
