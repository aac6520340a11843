"""The row-stationary implicit-GEMM 3x3 convolution (xp_conv3x3_nhwc_h2: gemm_h2r_kernel<TN, 1>) against the library's own plain GEMM on an
explicit im2col matrix (xp_gemm_nt_h2: the tile engine), BIT for bit.

Both engines walk K in 32-wide slabs, two k-steps per slab, three products per k-step in the order a1 b0, a0 b1, a0 b0, every accumulator on its own;
the convolution's K order is (kh, kw, ci) and a padded tap contributes exact zeros.  So the convolution must produce the very bits of the GEMM on
the im2col rows, whatever the kernel does about the tap geometry (worked out once per tap and lane, padded taps read as zeros through a bounded
buffer resource).

Which kernel a case runs is asserted from the profiling tag of its launch, because the dispatch is not what the shape suggests: a layer wider than 96
columns (other than 192) with fewer than 128 tiles of 128 x 128 runs the TILE engine's 64 x 128 convolution (conv3x3_h2_mfma_64x128), not the
row-stationary kernel.  The issue's three small wide shapes (Co = 264, 512, 768 at M = 30, 4, 12) are of that kind: they stay, as coverage of that
path, and each has a LARGE twin — same Ci, Co, stride and padding, one or two images big enough for 128 tiles — that runs gemm_h2r_kernel<4, 1>
(conv3x3_h2r_mfma_128x128: the instance of downsample 1, downsample 2 and the head trunk).  What the cases exercise: rows past M, row tiles that
cross an image boundary, partial column tiles and a remainder tile, a half slab past K and the padded even slab, outputs whose every pixel has padded
taps, every tap reflected, reflected and zero-padded borders of a large image, odd sizes, Ci % 16 != 0 (the general path), long K with N = 768.  The
output buffer is pre-filled with NaN so that a missed store shows.

Two shapes have a recorded reference.  For K >= 768, K % 64 == 0 and N >= 384 xp_gemm_nt_h2 runs the ping-pong kernel (gemm_h2p.hip), which sums the
even and the odd slabs apart: another order, and on the commit before this file 8471 of the 9216 values of the small 384 -> 768 case differed from it in
bits (largest difference 1.3e-5).  Ci = 384, Co = 768 is therefore compared, bit for bit, with the convolution's output recorded from that commit:
  * small (tile engine on both commits): tests/golden/conv_h2r_geometry_3x3x5x384_768.npy, three images; a smaller batch is its leading images;
  * large (gemm_h2r_kernel<4, 1> on both commits, asserted by tag when it was recorded): tests/golden/conv_h2r_geometry_2x75x73x384_768.npz holds
    every 32nd output row and the SHA-256 of all 2812 x 768 values (the whole output is 8.6 MB).
The same long K against an independent reference is the Ci = 368 twin (K = 3312, K % 64 != 0: the GEMM stays on the tile engine)."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from xpoint_amd import synth

pytestmark = pytest.mark.gpu

RS32, RS64, RS96, RS128, TILE64 = ("conv3x3_h2r_mfma_128x32", "conv3x3_h2r_mfma_128x64", "conv3x3_h2r_mfma_128x96", "conv3x3_h2r_mfma_128x128",
                                     "conv3x3_h2_mfma_64x128")
#        B, H, W, Ci, Co, stride, reflect, tag of the kernel that must run
SMALL = [(2, 5, 7, 48, 40, 1, 1, RS64),          # M = 70: rows past M, the tile crosses the image boundary; partial column tile; K = 432 = 13.5 slabs
         (1, 9, 11, 16, 264, 2, 0, TILE64),      # odd sizes; M = 30: the tile engine
         (3, 4, 4, 96, 192, 2, 0, RS96),         # 2 x 2 outputs per image: every output pixel has padded taps
         (1, 6, 6, 8, 32, 1, 0, RS32),           # Ci % 16 != 0: the general path
         (1, 2, 2, 48, 512, 1, 1, TILE64),       # every tap reflected; M = 4: the tile engine
         (2, 3, 5, 384, 768, 2, 0, TILE64)]      # long K, N = 768; M = 12: the tile engine
# the large twins: cdiv(M, 128) * cdiv(Co, 128) >= 128, so the row-stationary 128 x 128 instance runs
LARGE = [(1, 147, 149, 16, 264, 2, 0, RS128),    # odd sizes, M = 74 * 75 = 5550 (rows past M); column tiles 128 + 128 + a remainder of 8; K = 144
         (1, 63, 65, 48, 512, 1, 1, RS128),      # the head trunk's layer: reflected borders, M = 4095 (one row past M), K = 432 = 13.5 slabs
         (2, 75, 73, 384, 768, 2, 0, RS128),     # downsample 2's layer: long K = 3456, N = 768, M = 2 * 38 * 37 = 2812, the tile crosses the image boundary
         (2, 75, 73, 368, 768, 2, 0, RS128)]     # the same with K = 3312: the GEMM reference is the tile engine
CASES = SMALL + LARGE
EPILOGUE_CASES = [SMALL[0], LARGE[0], LARGE[1], SMALL[4]]      # scale / shift with ReLU (the head's epilogue), and the amp16 class
BATCH_CASES = [SMALL[0], SMALL[2], LARGE[1], SMALL[5]]

_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = {(3, 5, 384, 768, 2, 0): os.path.join(_GOLD, "conv_h2r_geometry_3x3x5x384_768.npy")}            # whole outputs of three images
GOLDEN_DIGEST = {(75, 73, 384, 768, 2, 0): os.path.join(_GOLD, "conv_h2r_geometry_2x75x73x384_768.npz")}  # rows[::32] + SHA-256, two images
DIGEST_STEP = 32


def _lib():
    from xpoint_amd import _lib as L
    return L


def _u(name, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(synth.uniform(name, shape, lo, hi))


def _split_h2(L, Wd):
    N, K = Wd.shape
    buf = torch.empty(L.load().xp_split_weights_h2_bytes(N, K), dtype=torch.uint8, device="cuda")
    L.call("xp_split_weights_h2", L.ptr(Wd), ctypes.c_void_p(buf.data_ptr()), N, K, L.current_stream())
    return buf


def _im2col(x, stride, reflect):
    """(B, H, W, Ci) NHWC on the device -> (B Ho Wo, 9 Ci) rows in (kh, kw, ci) order.  Copies only: every value is the input's bits or +0."""
    B, H, W, Ci = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect" if reflect else "constant")
    taps = [xp[:, :, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride].permute(0, 2, 3, 1)
            for kh in range(3) for kw in range(3)]
    return torch.stack(taps, dim=3).reshape(B * Ho * Wo, 9 * Ci).contiguous(), Ho, Wo


_inputs = {}


def _operands(Ci, Co, B, H, W):
    """The first B of three input images, split weights, bias, scale, shift of a shape: made once, shared, never written."""
    key = (Ci, Co, H, W)
    if key not in _inputs:
        L = _lib()
        x = _u(f"gx{Ci}_{H}_{W}", (3, H, W, Ci), -2.0, 2.0).cuda()
        w = _u(f"gw{Ci}_{Co}", (Co, 9 * Ci), -0.1, 0.1)
        w[Co // 2] *= 1e-3                                       # rows of different magnitude: the per-row weight scales matter
        _inputs[key] = (x, _split_h2(L, w.cuda()), _u(f"gb{Co}", (Co,)).cuda(), _u(f"gs{Co}", (Co,), 0.5, 1.5).cuda(),
                        _u(f"gt{Co}", (Co,), -0.5, 0.5).cuda())
    x, *rest = _inputs[key]
    return (x[:B].contiguous(), *rest)


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


def _conv(x, Wx, bias, scale, shift, Co, stride, reflect, act, tag):
    """The convolution into a NaN-filled buffer; `tag` is the kernel that must have run it (a silent fall-back to another engine fails here)."""
    L = _lib()
    B, H, W, Ci = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.full((B, Ho, Wo, Co), float("nan"), device="cuda")
    ran = _tags(lambda: L.call("xp_conv3x3_nhwc_h2", L.ptr(x), ctypes.c_void_p(Wx.data_ptr()), L.ptr(y), L.ptr(bias), L.ptr(scale), L.ptr(shift), B, H, W,
                               Ci, Co, stride, reflect, act, L.current_stream()))
    assert ran == {tag: 1}, f"conv {B}x{H}x{W}x{Ci} -> {Co}: expected one launch of {tag}, the profiler saw {ran}"
    return y


def _gemm_on_im2col(x, Wx, bias, scale, shift, Co, stride, reflect, act):
    L = _lib()
    A, Ho, Wo = _im2col(x, stride, reflect)
    M, K = A.shape
    C = torch.full((M, Co), float("nan"), device="cuda")
    L.call("xp_gemm_nt_h2", L.ptr(A), ctypes.c_void_p(Wx.data_ptr()), L.ptr(C), L.ptr(bias), L.ptr(scale), L.ptr(shift), None, M, Co, K, K, Co, Co, act,
           L.current_stream())
    return C.view(x.shape[0], Ho, Wo, Co)


def _reference(x, Wx, bias, Co, stride, reflect):
    """The plain (no activation, no affine) result the convolution must reproduce: the recorded one where the GEMM is not the tile engine."""
    B, H, W, Ci = x.shape
    path = GOLDEN.get((H, W, Ci, Co, stride, reflect))
    if path is None:
        return _gemm_on_im2col(x, Wx, bias, None, None, Co, stride, reflect, 0)
    return torch.from_numpy(np.load(path)[:B]).cuda()


def _assert_equals_recorded_digest(got, path, what):
    g = np.load(path)
    a = got.cpu().numpy()
    assert np.isfinite(a).all(), f"{what}: non-finite output"
    rows = np.ascontiguousarray(a.reshape(-1, a.shape[-1])[::DIGEST_STEP])
    diff = rows.view(np.int32) != g["rows"].view(np.int32)
    assert not diff.any(), (f"{what}: {int(diff.sum())} of {rows.size} recorded values differ in bits; first at (row / {DIGEST_STEP}, co) = "
                            f"{[int(v) for v in np.argwhere(diff)[0]]}; largest |difference| {float(np.abs(rows.astype(np.float64) - g['rows']).max()):.3e}")
    sha = hashlib.sha256(a.tobytes()).hexdigest()
    assert sha == str(g["sha256"]), f"{what}: the recorded rows agree but the SHA-256 of the whole output does not ({sha} vs {g['sha256']})"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same_bits(got, ref, what):
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output (a store was missed, or a padded tap was not zero)"
    diff = _bits(got) != _bits(ref)
    n = int(diff.sum())
    if n:
        idx = [int(v) for v in diff.nonzero()[0]]
        worst = float((got.double() - ref.double()).abs().max())
        raise AssertionError(f"{what}: {n} of {got.numel()} values differ in bits; first at (b, oh, ow, co) = {idx}: conv {float(got[tuple(idx)])!r} "
                             f"vs GEMM on im2col {float(ref[tuple(idx)])!r}; largest |difference| {worst:.3e}")


@pytest.mark.parametrize("B,H,W,Ci,Co,stride,reflect,tag", CASES)
def test_conv_h2r_equals_gemm_on_im2col(gpu_lib, B, H, W, Ci, Co, stride, reflect, tag):
    x, Wx, bias, _, _ = _operands(Ci, Co, B, H, W)
    got = _conv(x, Wx, bias, None, None, Co, stride, reflect, 0, tag)
    what = f"conv {B}x{H}x{W}x{Ci} -> {Co}, stride {stride}, {'reflect' if reflect else 'zero'}"
    digest = GOLDEN_DIGEST.get((H, W, Ci, Co, stride, reflect))
    if digest is not None:
        _assert_equals_recorded_digest(got, digest, what)
    else:
        _assert_same_bits(got, _reference(x, Wx, bias, Co, stride, reflect), what)


@pytest.mark.parametrize("amp", [0, 1])
@pytest.mark.parametrize("B,H,W,Ci,Co,stride,reflect,tag", EPILOGUE_CASES)
def test_conv_h2r_head_epilogue_and_amp16(gpu_lib, B, H, W, Ci, Co, stride, reflect, tag, amp):
    """ReLU then scale / shift (act 2: the head trunk's epilogue), in the f32 class and in the amp16 f32-container class (fp16 rounding after the bias
    add and after the affine: p.r16, the general form of the epilogue)."""
    L = _lib()
    x, Wx, bias, scale, shift = _operands(Ci, Co, B, H, W)
    L.call("xp_set_amp_mode", amp)
    try:
        got = _conv(x, Wx, bias, scale, shift, Co, stride, reflect, 2, tag)
        ref = _gemm_on_im2col(x, Wx, bias, scale, shift, Co, stride, reflect, 2)
        plain = _conv(x, Wx, bias, None, None, Co, stride, reflect, 0, tag)
    finally:
        L.call("xp_set_amp_mode", 0)
    _assert_same_bits(got, ref, f"conv {B}x{H}x{W}x{Ci} -> {Co} with ReLU + affine, amp {amp}")
    if amp:      # the class did round: every value is an fp16 number
        assert torch.equal(got, got.half().float()) and torch.equal(plain, plain.half().float())


@pytest.mark.parametrize("H,W,Ci,Co,stride,reflect,tag", [c[1:] for c in BATCH_CASES])
def test_conv_h2r_batch_invariance_and_determinism(gpu_lib, H, W, Ci, Co, stride, reflect, tag):
    """Image 0 of a B = 3 run equals the B = 1 run bit for bit (the row tiles fall differently on the images), and two runs are bit-equal.  The same
    kernel runs at both batch sizes (the cases are chosen so: the wide layer has 128 tiles at one image already)."""
    x, Wx, bias, _, _ = _operands(Ci, Co, 3, H, W)
    y3 = _conv(x, Wx, bias, None, None, Co, stride, reflect, 0, tag)
    y3b = _conv(x, Wx, bias, None, None, Co, stride, reflect, 0, tag)
    y1 = _conv(_operands(Ci, Co, 1, H, W)[0], Wx, bias, None, None, Co, stride, reflect, 0, tag)
    _assert_same_bits(y3b, y3, "second run of the same launch")
    _assert_same_bits(y3[:1], y1, "image 0 of the batch of 3 vs the batch of 1")
    _assert_same_bits(y3, _reference(x, Wx, bias, Co, stride, reflect), "batch of 3 vs the reference")
