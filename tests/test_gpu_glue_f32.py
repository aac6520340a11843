"""The f32 class's glue kernels (csrc/elementwise.hip, csrc/glue_core.h) through the C ABI against the float64 restatements of tests/glue_f64.py: every
dispatch instance of xp_layernorm and xp_layernorm_p32 at both ends of its C range and on both sides of a workgroup's row edge, the depthwise kernel's
workgroup renumbering at grids of 1, 7, 8, 9, 15 and 17, the stem's odd sizes and partial last workgroup, both depth-to-space kernels, every lane slot,
padding and partial wave of the detector softmax, the L2 clamp, the layout change, the max pool, the cost-volume mean and the 8-bit conversion.

Every output lies inside a larger allocation whose margins on both sides hold one NaN payload that must survive the call (Guard).  Bars: exact for data
movement; for arithmetic the bar each kernel already has in test_gpu_kernels.py / test_gpu_backbones.py, B_k max(1, max |ref|).  Inputs that lose bits by
construction (LayerNorm rows with a common offset, softmax cells shifted by +-80, L2 rows scaled by 1e3 / 1e-3, LayerNorm + GELU) get
max(that, 4 x the error of torch's own float32 operator on the same inputs against the same float64 reference), computed on the CPU: the yardstick is the
reference, never the kernel.  Each case prints one line with its worst error and its bar; DESIGN.md section 18 holds the largest ratios measured."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import glue_cases as gc, glue_f64 as g64
from tests.test_gpu_batch_invariance import PAY8, PAY32
from tests.test_gpu_ring import _p32_planes, _ref_split
from xpoint_amd import synth

pytestmark = pytest.mark.gpu

BARS = {"layernorm": 3e-6, "dwconv": 2e-6, "stem": 5e-6, "softmax": 1e-6, "l2norm": 1e-6, "costvolume": 2e-7}
MARGIN_BYTES = 16384        # payload on each side of a guarded buffer: more than a whole LayerNorm workgroup's rows (255 x 16, 127 x 32, ... 3 x 1024 floats)


def _lib():
    from xpoint_amd import _lib as L
    return L


def _u(name, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(synth.uniform("glue32/" + name, shape, lo, hi))


class Guard:
    """n elements (float32 or uint8) starting `off` elements past a 16-byte boundary, with MARGIN_BYTES of payload before and after."""

    def __init__(self, n, dtype=torch.float32, off=0, init=None):
        MARGIN = MARGIN_BYTES // (4 if dtype == torch.float32 else 1)
        self.full = torch.empty(MARGIN + off + n + MARGIN, dtype=dtype, device="cuda")
        self.pay = PAY32 if dtype == torch.float32 else PAY8
        self.bits().fill_(self.pay)
        self.lo, self.hi = MARGIN + off, MARGIN + off + n
        self.t = self.full[self.lo:self.hi]
        if init is not None:
            self.t.copy_(init.reshape(-1))

    def bits(self):
        return self.full.view(torch.int32) if self.full.dtype == torch.float32 else self.full

    def ptr(self):
        return ctypes.c_void_p(self.full.data_ptr() + self.lo * self.full.element_size())

    def intact(self):
        b = self.bits()
        return bool((b[:self.lo] == self.pay).all()) and bool((b[self.hi:] == self.pay).all())

    def untouched(self):
        return bool((self.bits() == self.pay).all())


class Worst:
    """the largest err / bar of a test function and the cases whose error is above the unwidened bar"""

    def __init__(self, kernel):
        self.kernel, self.ratio, self.at, self.widened = kernel, 0.0, "", []

    def check(self, what, got, ref, ref32=None):
        got = got.detach().cpu().double().reshape(ref.shape)
        assert bool(torch.isfinite(got).all()), (self.kernel, what)
        err = float((got - ref).abs().max())
        base = BARS[self.kernel] * max(1.0, float(ref.abs().max()))
        e32 = float((ref32.double().reshape(ref.shape) - ref).abs().max()) if ref32 is not None else 0.0
        bar = max(base, 4.0 * e32)
        note = ""
        if err > base:
            note = f"  ABOVE the unwidened bar {base:.2e}"
            self.widened.append((what, err, base, bar))
        print(f"{self.kernel} {what}: err {err:.2e}, bar {bar:.2e}" + (f" (torch f32 err {e32:.2e})" if ref32 is not None else "") + note)
        if err / bar > self.ratio:
            self.ratio, self.at = err / bar, what
        assert err <= bar, (self.kernel, what, err, bar, base, e32)

    def report(self):
        print(f"== {self.kernel}: largest err / bar {self.ratio:.3f} at {self.at}; cases above the unwidened bar: {len(self.widened)}")
        for what, err, base, bar in self.widened[:8]:
            print(f"==     {what}: err {err:.2e}, unwidened {base:.2e}, bar {bar:.2e}")


# ------------------------------------------------------------------------------------------------------------------------------ LayerNorm
def _ln_inputs(C, rows):
    """(-3, 3); one row in 7 with a common offset of ten times the spread (the two-pass variance), one row in 11 constant (variance 0: the output is b).
    The constant is a multiple of 1 / 64 below 64, a number of at most 12 bits: every partial sum of up to 1024 copies of it has at most 22 bits and is
    exact in float32 in any order, so the mean is the constant and the variance is 0 in the kernel's arithmetic as it is in the reference's.  For a
    constant whose row sum rounds, the mean is one rounding off, and 1 / sqrt(eps) = 316 multiplies that: DESIGN.md section 18."""
    i = torch.arange(rows)[:, None]
    x = _u(f"ln/x/{C}/{rows}", (rows, C), -3.0, 3.0)
    x = torch.where(i % 7 == 3, x + 60.0, x)
    const = (i % 11 == 5)[:, 0]
    return torch.where(const[:, None], ((x[:, :1] * 64.0).floor() / 64.0).expand(rows, C), x).contiguous(), const


def test_layernorm_every_instance_vs_fp64(gpu_lib):
    """xp_layernorm: the scalar kernel and the eight layernorm_vec_kernel instances at the lowest and highest C of each, rows 1 and R - 1, R, R + 1 for the
    instance's R rows per workgroup (rows past M are loaded from row 0 and must not be stored), gelu 0 and 1."""
    L = _lib()
    st, wc, seen = L.current_stream(), Worst("layernorm"), set()
    for C, aligned in gc.LN_CASES:
        inst, R = gc.ln_instance(C, aligned)
        seen.add(inst)
        w, b = _u(f"ln/w/{C}", (C,), 0.5, 1.5), _u(f"ln/b/{C}", (C,))
        wd, bd = w.cuda(), b.cuda()
        for rows in gc.ln_rows(R):
            x, const = _ln_inputs(C, rows)
            X = Guard(rows * C, off=0 if aligned else 1, init=x)
            assert (X.ptr().value % 16 == 0) == aligned
            r32 = F.layer_norm(x, (C,), w, b, 1e-5)
            for gelu in (0, 1):
                Y = Guard(rows * C)
                L.call("xp_layernorm", X.ptr(), Y.ptr(), L.ptr(wd), L.ptr(bd), rows, C, 1e-5, gelu, st)
                torch.cuda.synchronize()
                assert X.intact() and Y.intact(), (C, aligned, rows, gelu)
                assert torch.equal(X.t.cpu(), x.reshape(-1)), (C, aligned, rows, gelu)
                if not gelu:
                    assert torch.equal(Y.t.cpu().view(rows, C)[const], b.expand(int(const.sum()), C)), (C, aligned, rows, "a constant row is not exactly b")
                # the widened bar only where the input calls for it: an offset row (row 3 is the first) or the GELU
                wc.check(f"{inst} C {C} rows {rows} gelu {gelu}" + ("" if aligned else " x + 4 bytes"), Y.t, g64.layernorm(x, w, b, 1e-5, bool(gelu)),
                         (F.gelu(r32) if gelu else r32) if gelu or rows > 3 else None)
    wc.report()
    assert seen == set(gc.LN_INSTANCES) | {"scalar"}


def test_layernorm_empty_and_refusals(gpu_lib):
    """rows = 0 is OK and writes nothing; C = 0, C = 1025 and a null pointer are refused; in the mixed-precision mode the fused GELU and C % 4 != 0 are
    refused.  No refused call writes its output."""
    L = _lib()
    st = L.current_stream()
    w, b = torch.ones(1028, device="cuda"), torch.zeros(1028, device="cuda")
    X, Y = Guard(8 * 1028, init=torch.ones(8 * 1028)), Guard(8 * 1028)
    L.call("xp_layernorm", X.ptr(), Y.ptr(), L.ptr(w), L.ptr(b), 0, 96, 1e-5, 0, st)
    for C, xp, gelu in ((0, X.ptr(), 0), (1025, X.ptr(), 0), (96, None, 1)):
        with pytest.raises(L.XPointHipError):
            L.call("xp_layernorm", xp, Y.ptr(), L.ptr(w), L.ptr(b), 8, C, 1e-5, gelu, st)
    L.call("xp_set_amp_mode", 1)
    try:
        for C, gelu in ((96, 1), (6, 0)):
            with pytest.raises(L.XPointHipError):
                L.call("xp_layernorm", X.ptr(), Y.ptr(), L.ptr(w), L.ptr(b), 8, C, 1e-5, gelu, st)
    finally:
        L.call("xp_set_amp_mode", 0)
    torch.cuda.synchronize()
    assert Y.untouched() and X.intact()


def test_layernorm_p32_every_instance_is_the_split_of_layernorm(gpu_lib):
    """xp_layernorm_p32 at each of its seven instances, around the workgroup's row edge: the two fp16 planes are the split of xp_layernorm's f32 output
    bit for bit, and nothing is written behind the xp_p32_bytes image."""
    L = _lib()
    st, seen = L.current_stream(), set()
    for C in gc.LNP_CS:
        inst, R = gc.lnp_instance(C)
        seen.add(inst)
        wd, bd = _u(f"ln/w/{C}", (C,), 0.5, 1.5).cuda(), _u(f"ln/b/{C}", (C,)).cuda()
        for rows in gc.ln_rows(R):
            X, Y = Guard(rows * C, init=_ln_inputs(C, rows)[0]), Guard(rows * C)
            nbytes = L.load().xp_p32_bytes(rows, C)
            assert nbytes == rows * C * 4
            P = Guard(nbytes, torch.uint8)
            L.call("xp_layernorm", X.ptr(), Y.ptr(), L.ptr(wd), L.ptr(bd), rows, C, 1e-5, 0, st)
            L.call("xp_layernorm_p32", X.ptr(), P.ptr(), L.ptr(wd), L.ptr(bd), rows, C, 1e-5, st)
            torch.cuda.synchronize()
            assert X.intact() and Y.intact() and P.intact(), (C, rows)
            hi, lo = _p32_planes(P.t.clone(), rows, C)
            h0, h1 = _ref_split(Y.t.cpu().view(rows, C))
            assert torch.equal(hi, h0.double()) and torch.equal(lo, h1.double()), (inst, C, rows)
        print(f"layernorm_p32 {inst} C {C} rows {gc.ln_rows(R)}: both planes bit-equal to the split of xp_layernorm")
    assert seen == set(gc.LN_INSTANCES) - {(4, 1, 4)}


def test_layernorm_p32_refusals(gpu_lib):
    L = _lib()
    st = L.current_stream()
    w, b = torch.ones(1056, device="cuda"), torch.zeros(1056, device="cuda")
    X, Xo, P = Guard(8 * 1056, init=torch.ones(8 * 1056)), Guard(8 * 1056, off=1, init=torch.ones(8 * 1056)), Guard(8 * 1056 * 4, torch.uint8)
    for C, xp in ((48, X.ptr()), (1056, X.ptr()), (96, Xo.ptr())):
        with pytest.raises(L.XPointHipError):
            L.call("xp_layernorm_p32", xp, P.ptr(), L.ptr(w), L.ptr(b), 8, C, 1e-5, st)
    L.call("xp_set_amp_mode", 1)
    try:
        with pytest.raises(L.XPointHipError):
            L.call("xp_layernorm_p32", X.ptr(), P.ptr(), L.ptr(w), L.ptr(b), 8, 96, 1e-5, st)
    finally:
        L.call("xp_set_amp_mode", 0)
    torch.cuda.synchronize()
    assert P.untouched()


# ------------------------------------------------------------------------------------------------------------------------------ depthwise, stem
def test_dwconv3x3_silu_small_images_and_every_grid(gpu_lib):
    """xp_dwconv3x3_silu: H and W below the 4 x 4 patch, C = 4, ragged sizes, and grids of 7, 8, 9, 15 and 17 workgroups (the XCD renumbering with
    nb < 8, nb % 8 == 0 and nb % 8 != 0)."""
    L = _lib()
    st, wc = L.current_stream(), Worst("dwconv")
    for B, H, W, C in gc.DW_CASES:
        x, w9c = _u(f"dw/x/{B}x{H}x{W}x{C}", (B, H, W, C)), _u(f"dw/w/{C}", (9, C))
        X, Y = Guard(x.numel(), init=x), Guard(x.numel())
        L.call("xp_dwconv3x3_silu", X.ptr(), L.ptr(w9c.cuda()), Y.ptr(), B, H, W, C, st)
        torch.cuda.synchronize()
        assert X.intact() and Y.intact(), (B, H, W, C)
        wc.check(f"{B}x{H}x{W}x{C} ({gc.dw_blocks(B, H, W, C)} workgroups)", Y.t, g64.dwconv3x3_silu(x, w9c))
    wc.report()
    Y = Guard(64)
    with pytest.raises(L.XPointHipError):
        L.call("xp_dwconv3x3_silu", X.ptr(), L.ptr(w9c.cuda()), Y.ptr(), 1, 2, 2, 6, st)
    torch.cuda.synchronize()
    assert Y.untouched()


def test_stem_conv_ln_gelu_odd_sizes_and_partial_workgroups(gpu_lib):
    """xp_stem_conv_ln_gelu, both instances: odd H and W (Ho = ceil(H / 2)), a lone partial workgroup, one workgroup + 8 pixels, three + 24."""
    L = _lib()
    st, wc = L.current_stream(), Worst("stem")
    for Co in gc.STEM_COS:
        w9co, bias = _u(f"stem/w/{Co}", (9, Co), -0.6, 0.6), _u(f"stem/b/{Co}", (Co,), -0.2, 0.2)
        lnw, lnb = _u(f"stem/lnw/{Co}", (Co,), 0.8, 1.2), _u(f"stem/lnb/{Co}", (Co,), -0.1, 0.1)
        dev = [t.cuda() for t in (w9co, bias, lnw, lnb)]
        for B, H, W in gc.STEM_CASES:
            img = _u(f"stem/img/{B}x{H}x{W}", (B, H, W), 0.0, 1.0)
            ref = g64.stem_conv_ln_gelu(img, w9co, bias, lnw, lnb, 1e-5)
            I, Y = Guard(img.numel(), init=img), Guard(ref.numel())
            L.call("xp_stem_conv_ln_gelu", I.ptr(), *[L.ptr(t) for t in dev], Y.ptr(), B, H, W, Co, 1e-5, st)
            torch.cuda.synchronize()
            assert I.intact() and Y.intact(), (Co, B, H, W)
            wc.check(f"Co {Co} {B}x{H}x{W} ({ref.numel() // Co} pixels)", Y.t, ref)
    wc.report()
    Y = Guard(64 * 32)
    with pytest.raises(L.XPointHipError):
        L.call("xp_stem_conv_ln_gelu", I.ptr(), *[L.ptr(t) for t in dev], Y.ptr(), 1, 2, 2, 32, 1e-5, st)
    torch.cuda.synchronize()
    assert Y.untouched()


# ------------------------------------------------------------------------------------------------------------------------------ data movement
def test_depth_to_space_both_kernels_exact(gpu_lib):
    """xp_depth_to_space_nhwc: the float4 kernel at bs 2, 3 and 4, the scalar kernel through Cq % 4 != 0 and through an input one float off its alignment."""
    L = _lib()
    st = L.current_stream()
    for B, H, W, C, bs, off in gc.D2S_CASES:
        x = _u(f"d2s/{B}x{H}x{W}x{C}/{bs}", (B, H, W, C))
        X, Y = Guard(x.numel(), off=off, init=x), Guard(x.numel())
        L.call("xp_depth_to_space_nhwc", X.ptr(), Y.ptr(), B, H, W, C, bs, st)
        torch.cuda.synchronize()
        assert X.intact() and Y.intact(), (B, H, W, C, bs, off)
        assert torch.equal(Y.t.cpu(), g64.depth_to_space(x, bs).reshape(-1)), (B, H, W, C, bs, off)
        print(f"depth_to_space {B}x{H}x{W}x{C} bs {bs} offset {off}: exact")
    Y = Guard(640)
    with pytest.raises(L.XPointHipError):
        L.call("xp_depth_to_space_nhwc", X.ptr(), Y.ptr(), 1, 2, 2, 40, 4, st)
    torch.cuda.synchronize()
    assert Y.untouched()


def test_nhwc_to_nchw_exact(gpu_lib):
    L = _lib()
    st = L.current_stream()
    for B, HW, C in gc.NCHW_CASES:
        x = _u(f"nchw/{B}x{HW}x{C}", (B, HW, C))
        X, Y = Guard(x.numel(), init=x), Guard(x.numel())
        L.call("xp_nhwc_to_nchw", X.ptr(), Y.ptr(), B, HW, C, st)
        torch.cuda.synchronize()
        assert X.intact() and Y.intact(), (B, HW, C)
        assert torch.equal(Y.t.cpu(), g64.nhwc_to_nchw(x).reshape(-1)), (B, HW, C)
        print(f"nhwc_to_nchw {B}x{HW}x{C}: exact")


def test_maxpool2_ties_infinities_and_odd_sizes_exact(gpu_lib):
    """xp_maxpool2_nhwc: values on 8 levels so that windows tie, a few +-inf; odd H and W drop the last row / column while the input keeps its full stride."""
    L = _lib()
    st = L.current_stream()
    for B, H, W, C in gc.POOL_CASES:
        x = (_u(f"pool/{B}x{H}x{W}x{C}", (B, H, W, C)) * 4.0).floor() / 4.0
        x.view(-1)[::13] = float("inf")
        x.view(-1)[5::17] = float("-inf")
        ref = F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()
        assert torch.equal(ref, g64.maxpool2(x))
        X, Y = Guard(x.numel(), init=x), Guard(ref.numel())
        L.call("xp_maxpool2_nhwc", X.ptr(), Y.ptr(), B, H, W, C, st)
        torch.cuda.synchronize()
        assert X.intact() and Y.intact(), (B, H, W, C)
        assert torch.equal(Y.t.cpu(), ref.reshape(-1)), (B, H, W, C)
        print(f"maxpool2 {B}x{H}x{W}x{C}: exact, {int(torch.isinf(ref).sum())} infinite outputs of {ref.numel()}")


@pytest.mark.parametrize("n", gc.U8_NS)
def test_u8_to_unit_f32_exact(gpu_lib, n):
    """xp_u8_to_unit_f32: every byte value in the vector part and in the scalar tail"""
    L = _lib()
    st = L.current_stream()
    for k0 in range(0, 256, n):
        src = ((torch.arange(n) + k0) % 256).to(torch.uint8)
        S, D = Guard(n, torch.uint8, init=src), Guard(n)
        L.call("xp_u8_to_unit_f32", S.ptr(), D.ptr(), n, st)
        torch.cuda.synchronize()
        assert S.intact() and D.intact(), (n, k0)
        assert torch.equal(D.t.cpu(), g64.u8_to_unit(src)), (n, k0)


# ------------------------------------------------------------------------------------------------------------------------------ detector and descriptor tails
def _smx_logits(kind, r, ld, B, Hc, Wc):
    nch, cells = r * r + 1, B * Hc * Wc
    lg = _u(f"smx/{kind}/{r}/{ld}/{B}x{Hc}x{Wc}", (cells, ld), -6.0, 6.0)
    cell = torch.arange(cells)
    if kind == "shifted":
        lg += torch.where(cell % 2 == 0, -80.0, 80.0)[:, None]
    if kind == "spike":
        lg[cell, (cell * 7 + 3) % nch] = 66.0           # at least 60 over every other logit; the dustbin and the second lane slot take their turns
    lg[:, nch:] = float("nan")
    return lg.view(B, Hc, Wc, ld)


def test_softmax_shuffle_every_slot_mode_and_partial_wave(gpu_lib):
    """xp_softmax_shuffle: r 1, 2, 8, 11 (one and two lane slots), ld = nch and nch + 7 with NaN in the padding columns, 1 - 17 cells (a last wave with 1 - 3
    of its 4 cells, a second workgroup), mode 0 plain / shifted by +-80 per cell / one logit 60 over the rest, and mode 1."""
    L = _lib()
    st, wc = L.current_stream(), Worst("softmax")
    for r in gc.SMX_RS:
        nch = r * r + 1
        for ld in (nch, nch + 7):
            for B, Hc, Wc in gc.SMX_CELLS:
                for kind in gc.SMX_KINDS:
                    mode = 1 if kind == "mode1" else 0
                    lg = _smx_logits(kind, r, ld, B, Hc, Wc)
                    ref = g64.softmax_shuffle(lg, r, mode)
                    r32 = None
                    if kind == "shifted":
                        p32 = F.softmax(lg[..., :nch], dim=-1)[..., :-1]
                        r32 = p32.reshape(B, Hc, Wc, r, r).permute(0, 1, 3, 2, 4).reshape(B, Hc * r, Wc * r)
                    X, P = Guard(lg.numel(), init=lg), Guard(ref.numel())
                    L.call("xp_softmax_shuffle", X.ptr(), P.ptr(), B, Hc, Wc, r, ld, mode, st)
                    torch.cuda.synchronize()
                    assert X.intact() and P.intact(), (r, ld, B, Hc, Wc, kind)
                    wc.check(f"r {r} ld {ld} {B}x{Hc}x{Wc} {kind}", P.t, ref, r32)
    wc.report()
    P = Guard(144 * 4)
    for r, ld in ((12, 145), (8, 64), (2, 4)):
        with pytest.raises(L.XPointHipError):
            L.call("xp_softmax_shuffle", X.ptr(), P.ptr(), 1, 1, 1, r, ld, 0, st)
    torch.cuda.synchronize()
    assert P.untouched()


def test_l2norm_rows_clamp_scales_and_ragged_widths(gpu_lib):
    """xp_l2norm_rows: C below, at and above whole waves, rows around the 4-row workgroup, rows scaled by 1, 1e-3 and 1e3, both forms (eps 1e-12 and the
    unclamped eps < 0).  With the clamp: a zero row gives zeros, a row of 1e-20 (norm below eps) gives x / eps."""
    L = _lib()
    st, wc = L.current_stream(), Worst("l2norm")
    for C in gc.L2_CS:
        for rows in gc.L2_ROWS:
            x = _u(f"l2/{C}/{rows}", (rows, C), -2.0, 2.0) * torch.tensor([1.0, 1e-3, 1e3])[torch.arange(rows) % 3][:, None]
            for eps in gc.L2_EPS:
                r32 = None
                if rows > 1:
                    r32 = F.normalize(x, p=2, dim=1, eps=1e-12) if eps >= 0 else x / x.norm(dim=1, keepdim=True)
                X, Y = Guard(rows * C, init=x), Guard(rows * C)
                L.call("xp_l2norm_rows", X.ptr(), Y.ptr(), rows, C, eps, st)
                torch.cuda.synchronize()
                assert X.intact() and Y.intact(), (C, rows, eps)
                wc.check(f"C {C} rows {rows} eps {eps:g}", Y.t, g64.l2norm_rows(x, eps), r32)
            for tiny_row in ([rows - 1] if rows > 1 else [None, 0]):
                xs = x.clone()
                xs[0] = 0.0
                if tiny_row is not None:
                    xs[tiny_row] = 1e-20
                X, Y = Guard(rows * C, init=xs), Guard(rows * C)
                L.call("xp_l2norm_rows", X.ptr(), Y.ptr(), rows, C, 1e-12, st)
                torch.cuda.synchronize()
                assert X.intact() and Y.intact(), (C, rows, tiny_row)
                got, ref = Y.t.cpu().view(rows, C), g64.l2norm_rows(xs, 1e-12)
                wc.check(f"C {C} rows {rows} zero row" + ("" if tiny_row is None else f", 1e-20 row {tiny_row}"), got, ref)
                if tiny_row is None or tiny_row != 0:
                    assert bool((got[0] == 0).all()), (C, rows, "the zero row")
                if tiny_row is not None:
                    # x / eps exactly, up to the two roundings of float32(1e-12) and of the quotient (2^-23 in all), far inside 1e-6 relative
                    rel = float(((got[tiny_row].double() - ref[tiny_row]).abs() / ref[tiny_row].abs()).max())
                    assert rel <= 1e-6 and abs(float(ref[tiny_row, 0]) / 1e-8 - 1.0) < 1e-6, (C, rows, rel)
    wc.report()


def test_costvolume_mean_small_and_largest_channel_counts(gpu_lib):
    """xp_costvolume_mean on unit rows: hw below the workgroup's 4 waves, C = 1, C not a multiple of 64, and C = 8192 (the bound: 32 KB of LDS)."""
    L = _lib()
    st, wc = L.current_stream(), Worst("costvolume")
    for B, hw, C in gc.CV_CASES:
        a, b = (F.normalize(_u(f"cv/{k}/{B}x{hw}x{C}", (B, hw, C)), dim=2) for k in "ab")
        A, Bq, V = Guard(a.numel(), init=a), Guard(b.numel(), init=b), Guard(B * hw)
        L.call("xp_costvolume_mean", A.ptr(), Bq.ptr(), V.ptr(), B, hw, C, st)
        torch.cuda.synchronize()
        assert A.intact() and Bq.intact() and V.intact(), (B, hw, C)
        wc.check(f"{B}x{hw}x{C}", V.t, g64.costvolume_mean(a, b).reshape(-1))
    wc.report()
    V = Guard(64)
    with pytest.raises(L.XPointHipError):
        L.call("xp_costvolume_mean", A.ptr(), Bq.ptr(), V.ptr(), 1, 1, 8193, st)
    torch.cuda.synchronize()
    assert V.untouched()
