"""Micro-benchmark of xp_conv3x3_nhwc_h2 on the five 3x3 convolutions of the 480x640 model at 16 images: us per launch (HIP events, 20 launches)
and the CRC-32 of each output.  CB_ONLY=0,2 selects; XP_LIB_PATH runs another build of the library (the CRCs of two builds must be equal);
XP_H2_TILE forces a column tile (A/B)."""
import ctypes
import os
import sys
import zlib

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from xpoint_amd import _lib as L  # noqa: E402

B = int(os.environ.get("CB_BATCH", "16"))
convs = [  # name, H, W, Ci, Co, stride, reflect, act, affine
    ("patch-embed 2", 240, 320, 48, 96, 2, 0, 0, False),
    ("downsample 0", 120, 160, 96, 192, 2, 0, 0, False),
    ("downsample 1", 60, 80, 192, 384, 2, 0, 0, False),
    ("downsample 2", 30, 40, 384, 768, 2, 0, 0, False),
    ("head trunk", 60, 80, 48, 512, 1, 1, 2, True),
]
if os.environ.get("CB_ONLY"):
    convs = [convs[int(i)] for i in os.environ["CB_ONLY"].split(",")]
st = L.current_stream()
for name, H, W, Ci, Co, stride, reflect, act, affine in convs:
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, H, W, Ci, device="cuda", generator=g)
    w = torch.randn(Co, 9 * Ci, device="cuda", generator=g) * 0.05
    b = torch.randn(Co, device="cuda", generator=g)
    sc = torch.rand(Co, device="cuda", generator=g) + 0.5 if affine else None
    sh = torch.randn(Co, device="cuda", generator=g) if affine else None
    Wx = torch.empty(L.load().xp_split_weights_h2_bytes(Co, 9 * Ci), dtype=torch.uint8, device="cuda")
    L.call("xp_split_weights_h2", L.ptr(w), ctypes.c_void_p(Wx.data_ptr()), Co, 9 * Ci, st)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.full((B, Ho, Wo, Co), float("nan"), device="cuda")

    def run():
        L.call("xp_conv3x3_nhwc_h2", L.ptr(x), ctypes.c_void_p(Wx.data_ptr()), L.ptr(y), L.ptr(b), L.ptr(sc), L.ptr(sh), B, H, W, Ci, Co, stride, reflect,
               act, st)

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 20
    e0.record()
    for _ in range(n):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    M, K = B * Ho * Wo, 9 * Ci
    crc = zlib.crc32(y.cpu().numpy().tobytes())
    print(f"{name:14s} M{M:7d} N{Co:4d} K{K:5d}: {ms * 1e3:8.1f} us  {2.0 * M * Co * K / ms / 1e9:6.1f} TF/s f32-eq  crc {crc:08x}", flush=True)
