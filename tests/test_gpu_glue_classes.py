"""The glue operations that exist in every precision class — depthwise 3x3 + SiLU, the stem (conv + LayerNorm + GELU) and depth-to-space — have ONE
device body each (csrc/glue_core.h), instantiated by csrc/elementwise.hip (f32 containers; with xp_set_amp_mode(1) the "amp16" class) and
csrc/elementwise_f16.hip (fp16 storage, "amp16f").  Two claims, both without a tolerance:

(a) amp16 and amp16f apply the same roundings at the same points: on fp16-exact inputs the f32-container entry under amp mode 1
    and the fp16-storage entry give the same values bit for bit.
(b) the f32 class (amp mode 0) and the fp16-storage class give the bits they gave before the bodies were merged: tests/golden/glue_parent_bits.npz,
    recorded by tools/make_golden_glue.py from a build of the commit before the merge.  The inputs are regenerated from synth names, not stored.

Every output sits in a canary allocation (test_gpu_batch_invariance.Canary) whose padding must survive the call, and the profiling tag of each
f32-class case proves which entry ran."""
import math
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_batch_invariance import Canary, _tags
from tests.test_gpu_h2 import _r16
from xpoint_amd import synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glue_parent_bits.npz")


def _lib():
    from xpoint_amd import _lib as L
    return L


def _u(name, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(synth.uniform("glue/" + name, shape, lo, hi)).cuda()


def _amp16(L, fn):
    """fn under xp_set_amp_mode(1), restored whatever happens."""
    L.call("xp_set_amp_mode", 1)
    try:
        fn()
    finally:
        L.call("xp_set_amp_mode", 0)


# --------------------------------------------------------------------------------------------------------------------- one call per entry
def _dw_f32(L, x, w9c, B, H, W, C, amp=False):
    """xp_dwconv3x3_silu on x (B, H, W, C) f32; the profiler must have seen exactly that entry."""
    M = B * H * W
    X, Y = Canary(M, C, init=x.reshape(M, C)), Canary(M, C)
    call = lambda: L.call("xp_dwconv3x3_silu", X.ptr(), L.ptr(w9c), Y.ptr(), B, H, W, C, L.current_stream())
    tags = _tags((lambda: _amp16(L, call)) if amp else call)
    assert tags == {"dwconv3x3_silu": 1}, tags
    assert X.intact() and Y.intact(), ("dwconv f32", amp, B, H, W, C)
    return Y.t.clone()


def _dw_f16(L, x16, w9c, B, H, W, C, copy):
    """xp_dwconv3x3_silu_f16; (half output, f32 copy or None)."""
    M = B * H * W
    X, Y, Y32 = Canary(M, C, torch.float16, init=x16.reshape(M, C)), Canary(M, C, torch.float16), Canary(M, C)
    L.call("xp_dwconv3x3_silu_f16", X.ptr(), L.ptr(w9c), Y.ptr(), Y32.ptr() if copy else None, B, H, W, C, L.current_stream())
    assert X.intact() and Y.intact() and Y32.intact(), ("dwconv f16", copy, B, H, W, C)
    if not copy:
        assert bool((Y32.bits() == Y32.pay).all()), "the f32 copy was written although none was asked for"
    return Y.t.clone(), (Y32.t.clone() if copy else None)


def _stem_params(CO, exact16):
    w, b = _u(f"stw/{CO}", (CO, 3, 3, 3), -0.4, 0.4), _u(f"stb/{CO}", (CO,), -0.2, 0.2)
    lnw, lnb = _u(f"stlnw/{CO}", (CO,), 0.8, 1.2), _u(f"stlnb/{CO}", (CO,), -0.2, 0.2)
    if exact16:
        w, b, lnw, lnb = (_r16(t).float() for t in (w, b, lnw, lnb))
    w9co = w.sum(dim=1).permute(1, 2, 0).reshape(9, CO).contiguous()          # the three identical input channels' weights folded, as the model packs them
    return w9co, b, lnw, lnb


def _stem(L, cls, img, par, B, H, W, CO, amp=False):
    """xp_stem_conv_ln_gelu (cls "f32"; amp: under amp mode 1) or xp_stem_conv_ln_gelu_f16 (cls "f16")."""
    rows = B * ((H + 1) // 2) * ((W + 1) // 2)
    Y = Canary(rows, CO, torch.float32 if cls == "f32" else torch.float16)
    entry = "xp_stem_conv_ln_gelu" if cls == "f32" else "xp_stem_conv_ln_gelu_f16"
    call = lambda: L.call(entry, L.ptr(img), *(L.ptr(t) for t in par), Y.ptr(), B, H, W, CO, 1e-5, L.current_stream())
    tags = _tags((lambda: _amp16(L, call)) if amp else call)
    assert tags == {entry[3:]: 1}, tags
    assert Y.intact(), ("stem", cls, amp, B, H, W, CO)
    return Y.t.clone()


def _d2s_f32(L, x, B, H, W, C):
    Cq = C // 16
    X, Y = Canary(B * H * W, C, init=x.reshape(-1, C)), Canary(B * H * W * 16, Cq)
    tags = _tags(lambda: L.call("xp_depth_to_space_nhwc", X.ptr(), Y.ptr(), B, H, W, C, 4, L.current_stream()))
    assert tags == {"depth_to_space": 1}, tags
    assert X.intact() and Y.intact(), ("depth_to_space f32", B, H, W, C)
    return Y.t.clone()


def _d2s_f16(L, x16, B, H, W, C):
    """xp_depth_to_space_nhwc_f16 with a zeroed status word; (f32 output, half output, status)."""
    Cq = C // 16
    X = Canary(B * H * W, C, torch.float16, init=x16.reshape(-1, C))
    Y32, Y16 = Canary(B * H * W * 16, Cq), Canary(B * H * W * 16, Cq, torch.float16)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.call("xp_depth_to_space_nhwc_f16", X.ptr(), Y32.ptr(), Y16.ptr(), B, H, W, C, 4, L.ptr(status), L.current_stream())
    torch.cuda.synchronize()
    assert X.intact() and Y32.intact() and Y16.intact(), ("depth_to_space f16", B, H, W, C)
    return Y32.t.clone(), Y16.t.clone(), int(status)


# ------------------------------------------------------------------------------------------------------------- (a) amp16 == amp16f, bit for bit
DW_AB_C, DW_AB_HW, DW_AB_B = (4, 96, 192), ((1, 1), (1, 9), (5, 7), (15, 20)), 3


def test_dwconv_amp16_equals_amp16f(gpu_lib):
    """1 x 1 and single-row images, ragged H / W against the 4 x 4 pixel block, grids shorter than the 8 XCDs and grids that are no multiple of 8 (the
    XCD band remap); the f32 copy of the fp16-storage entry equals both."""
    L = _lib()
    B, grids = DW_AB_B, []
    for C in DW_AB_C:
        w9c = _r16(_u(f"dww/{C}", (9, C), -0.5, 0.5)).float()
        for H, W in DW_AB_HW:
            x16 = _u(f"dwx/{C}/{H}x{W}", (B, H, W, C), -1.5, 1.5).half()
            o32 = _dw_f32(L, x16.float(), w9c, B, H, W, C, amp=True)
            o16, _ = _dw_f16(L, x16, w9c, B, H, W, C, copy=False)
            o16c, copy = _dw_f16(L, x16, w9c, B, H, W, C, copy=True)
            same = torch.equal(o32, o16.float())
            print(f"dwconv C {C} {B}x{H}x{W}: amp16 == amp16f {same}")
            assert same, (C, H, W, int((o32 != o16.float()).sum()))
            assert torch.equal(o16c, o16) and torch.equal(copy, o32), (C, H, W)
            grids.append(math.ceil(B * math.ceil(H / 4) * math.ceil(W / 4) * (C // 4) / 256))
    assert any(g < 8 for g in grids) and any(g > 8 and g % 8 for g in grids), grids


@pytest.mark.parametrize("CO", [16, 48])
def test_stem_amp16_equals_amp16f(gpu_lib, CO):
    """Both instances at odd image sizes (Ho = ceil(H / 2)) and a partial last workgroup."""
    L = _lib()
    par = _stem_params(CO, exact16=True)
    for B, H, W in ((2, 33, 47), (1, 7, 5)):
        img = _r16(_u(f"stimg/{H}x{W}", (B, 1, H, W), 0.0, 1.0)).float()
        o32 = _stem(L, "f32", img, par, B, H, W, CO, amp=True)
        o16 = _stem(L, "f16", img, par, B, H, W, CO)
        same = torch.equal(o32, o16.float())
        print(f"stem CO {CO} {B}x{H}x{W}: amp16 == amp16f {same}")
        assert same, (CO, B, H, W, int((o32 != o16.float()).sum()))


def test_depth_to_space_f32_equals_f16(gpu_lib):
    L = _lib()
    for B, H, W, C in ((1, 3, 5, 64), (3, 7, 9, 128)):
        x16 = _u(f"d2s/{B}x{H}x{W}x{C}", (B, H, W, C), -4.0, 4.0).half()
        y32, y16, status = _d2s_f16(L, x16, B, H, W, C)
        assert torch.equal(_d2s_f32(L, x16.float(), B, H, W, C), y32) and torch.equal(y32, y16.float()) and status == 0, (B, H, W, C, status)


# ------------------------------------------------------------------------------------------------------------- (b) the bits before the merge
DW_BITS = [(C, H, W) for C in (4, 96) for H, W in ((1, 1), (1, 9), (5, 7))] + [(12, 9, 13)]
STEM_BITS = [(CO, H, W) for CO in (16, 48) for H, W in ((7, 5), (9, 37))]           # 9 x 37: 95 output pixels, two workgroups with a partial second one
D2S_BITS = (1, 3, 5, 64)


def compute_bits(op):
    """{name: numpy array} of one operation's cases in the f32 class (amp mode 0) and the fp16-storage class: what tools/make_golden_glue.py records
    and what test_bits_are_those_before_the_merge compares."""
    L = _lib()
    out = {}
    if op == "dwconv":
        B = 2
        for C, H, W in DW_BITS:
            w9c = _u(f"bits/dww/{C}", (9, C), -0.5, 0.5)
            x = _u(f"bits/dwx/{C}/{H}x{W}", (B, H, W, C), -1.5, 1.5)
            out[f"dwconv/f32/C{C}_{H}x{W}"] = _dw_f32(L, x, w9c, B, H, W, C)
            out[f"dwconv/f16/C{C}_{H}x{W}"] = _dw_f16(L, x.half(), w9c, B, H, W, C, copy=False)[0]
    elif op == "stem":
        for CO, H, W in STEM_BITS:
            par = _stem_params(CO, exact16=False)
            img = _u(f"bits/stimg/{H}x{W}", (1, 1, H, W), 0.0, 1.0)
            out[f"stem/f32/CO{CO}_{H}x{W}"] = _stem(L, "f32", img, par, 1, H, W, CO)
            out[f"stem/f16/CO{CO}_{H}x{W}"] = _stem(L, "f16", img, par, 1, H, W, CO)
    else:
        B, H, W, C = D2S_BITS
        x = _u("bits/d2s", (B, H, W, C), -4.0, 4.0)
        out["d2s/f32/out"] = _d2s_f32(L, x, B, H, W, C)
        x16 = x.half()
        nan, lim = x16.clone(), x16.clone()
        nan.view(-1)[-1] = float("nan")
        lim.view(-1)[7] = float("inf")                  # the half form's limit: a value EQUAL to it is out of range (|x| < limit fails)
        y32, y16, s_fin = _d2s_f16(L, x16, B, H, W, C)
        out["d2s/f16/out32"], out["d2s/f16/out16"] = y32, y16
        # the status word for a finite input, one NaN in the last element, one value equal to the limit.  (The f32 form's status word is reachable only
        # through xp_xpoint_forward_ex, a whole model: test_gpu_amp16f_kernels.py::test_depth_to_space_f16_permutation_and_status covers the shared ballot.)
        out["d2s/f16/status"] = torch.tensor([s_fin, _d2s_f16(L, nan, B, H, W, C)[2], _d2s_f16(L, lim, B, H, W, C)[2]], dtype=torch.int32)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("op", ["dwconv", "stem", "d2s"])
def test_bits_are_those_before_the_merge(gpu_lib, op):
    gold = np.load(GOLDEN)
    mine = compute_bits(op)
    assert sorted(mine) == sorted(k for k in gold.files if k.startswith(op + "/")), (sorted(mine), gold.files)
    for k, v in mine.items():
        g = gold[k]
        assert v.dtype == g.dtype and v.shape == g.shape, (k, v.dtype, g.dtype, v.shape, g.shape)
        bits = np.uint32 if v.dtype.itemsize == 4 else np.uint16
        n_diff = int((v.view(bits) != g.view(bits)).sum())
        print(f"{k}: {v.size} values, {n_diff} differ from the recorded bits")
        assert n_diff == 0, (k, n_diff)
    if op == "d2s":
        assert mine["d2s/f16/status"].tolist() == [0, 1, 1]
