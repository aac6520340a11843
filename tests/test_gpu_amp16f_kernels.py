"""The fp16-storage mixed-precision class ("amp16f") kernel by kernel against the float64 restatement of its recipe (tests/amp_recipe64.py):
the fused SS2D core in both of its forms and in every NW regime of the sequential one, the same recipe in f32 containers ("amp16": xp_set_amp_mode(1) +
xp_ss2d_core_fwd), the glue kernels of csrc/elementwise_f16.hip (stem, dwconv and depth-to-space: the shared bodies of csrc/glue_core.h) and the two conversions that are the recipe's rounding points.  The class's GEMM-type
kernels are pinned in test_gpu_h2.py.

Every output sits in a canary allocation (test_gpu_batch_invariance.Canary) whose padding must survive the call, and the profiling tags prove which form
of the SS2D core ran.  Each case prints one line: bit-equal fraction, near-tie fraction, worst fp16 ulp."""
import ctypes
import math

import pytest
import torch

from tests import amp_recipe64 as rc
from tests.test_gpu_batch_invariance import Canary, _tags
from tests.test_gpu_h2 import _r16, _ulp16
from xpoint_amd import synth

pytestmark = pytest.mark.gpu

SEQ_MAX_L = 8192            # csrc/ss2d.hip XP_SS2D_SEQ_DEFAULT_MAXL: the per-image L bound of the sequential form
KAPPA = 4e-7                # glue kernels: their f32 error bound in units of each rounding point's scale (about 7 f32 roundings of it)
# near-tie fractions at KAPPA with this data (one rounding point / two / three): the bars of assert_r16_exact_off_ties
TIES_LN, TIES_DW, TIES_STEM = 0.01, 0.02, 0.06


def _lib():
    from xpoint_amd import _lib as L
    return L


def _u(name, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(synth.uniform("amp16f/" + name, shape, lo, hi)).cuda()


def _stats(mine, ref):
    """test_gpu_model.py's check() numbers: the bit-equal fraction and the worst error in fp16 ulps of the reference, floored at its rms."""
    mine, ref = mine.double(), ref.double()
    rms = float(ref.pow(2).mean().sqrt())
    return float((mine == ref).double().mean()), float(((mine - ref).abs() / _ulp16(ref.abs().clamp_min(rms))).max())


# ------------------------------------------------------------------------------------------------------------------------------ SS2D core
def _takes_seq(H, W, C, R):
    """ss2d_takes_seq (csrc/ss2d.hip) for the fp16-storage class given f32 copies: C <= 768 and a multiple of 64, a dt_rank with whole 8-value fragment
    halves >= 16 (ss2d_seq_scan2_applies), planes inside the 32-bit buffer offsets, L <= 8192."""
    return C <= 768 and C % 64 == 0 and R in (16, 24, 48) and H * W * C < 2 ** 29 and H * W * 4 * (R + 2) < 2 ** 29 and H * W <= SEQ_MAX_L


def _core_inputs(tag, B, H, W, C, R, switches=False):
    """test_ss2d_core_vs_oracle's ranges; u and the x_proj weights rounded to fp16, xdbl = r16(u16 . r16(x_proj)^T).  switches: half the channels' dt bias
    around the softplus threshold (20), the other half around the series / logarithm switch of xp_softplus_decay_l2 (exp(dt) = 0.14, dt = -1.97)."""
    xw = _u(f"xp/{tag}", (4, R + 2, C), -C ** -0.5, C ** -0.5)
    dtw = _u(f"dtw/{tag}", (4, C, R), -R ** -0.5, R ** -0.5)
    if switches:
        h = C // 2
        dtb = torch.cat([_u(f"dtb20/{tag}", (4, h), 18.5, 21.5), _u(f"dtbsw/{tag}", (4, C - h), -2.7, -1.3)], 1)
    else:
        dtb = _u(f"dtb/{tag}", (4, C), -6.9, -2.25)
    u16 = _u(f"x/{tag}", (B, H, W, C), -0.3, 1.0).half()
    xw16 = xw[rc.ORDER].reshape(4 * (R + 2), C).half()
    return dict(u16=u16, xdbl16=rc.xdbl_amp64(u16.view(-1, C), xw16).half(), wdt=_r16(dtw)[rc.ORDER].permute(0, 2, 1).float().contiguous(),
                dtb=dtb[rc.ORDER].contiguous(), A=(-torch.exp(_u(f"al/{tag}", (4, C), -0.5, 0.5)))[rc.ORDER].contiguous(),
                D=_u(f"ds/{tag}", (4, C), 0.5, 1.5)[rc.ORDER].contiguous(), lnw=_u(f"onw/{tag}", (C,), 0.8, 1.2), lnb=_u(f"onb/{tag}", (C,), -0.1, 0.1))


def _core(L, inp, B, H, W, C, R, cls, copies=False):
    """One call of the core on the first B images of inp: cls "amp16f" (xp_ss2d_core_fwd_f16; copies: with f32 copies of u and xdbl) or "amp16"
    (xp_set_amp_mode(1) + xp_ss2d_core_fwd on the same half values in f32 containers).  (output, profiling tags)."""
    M = B * H * W
    u16, x16 = inp["u16"][:B].contiguous(), inp["xdbl16"][:M].contiguous()
    u32, x32 = u16.float(), x16.float()
    ws = torch.empty(L.load().xp_ss2d_core_workspace_bytes(B, H, W, C) // 4 + 16, device="cuda")
    par = [L.ptr(inp[k]) for k in ("wdt", "dtb", "A", "D", "lnw", "lnb")]
    tail = (L.ptr(ws), ws.numel() * 4, B, H, W, C, R, 1, 1e-5, L.current_stream())
    if cls == "amp16f":
        out = Canary(M, C, torch.float16)
        fn = lambda: L.call("xp_ss2d_core_fwd_f16", L.ptr(u16), L.ptr(x16), L.ptr(u32) if copies else None, L.ptr(x32) if copies else None, *par,
                            out.ptr(), *tail)
    else:
        out = Canary(M, C)

        def fn():
            L.call("xp_set_amp_mode", 1)
            try:
                L.call("xp_ss2d_core_fwd", L.ptr(u32), L.ptr(x32), *par, out.ptr(), *tail)
            finally:
                L.call("xp_set_amp_mode", 0)
    tags = _tags(fn)
    assert out.intact(), f"{cls} ({H}, {W}, {C}, {R}) B = {B}: a padding word of the output changed"
    return out.t.clone(), tags


def _form(tags):
    seq = "ss2d_seq_scan" in tags and "ss2d_seq_merge_ln" in tags
    chunked = all(k in tags for k in ("ss2d_pass1", "ss2d_pass2", "ss2d_pass3_row", "ss2d_pass3_col_ln"))
    assert seq != chunked, tags
    return "sequential" if seq else "chunked"


# (H, W, C, dt_rank) per image: stages 0 - 3 at 480 x 640, stage 2 of config C4 (1024 x 1024), the 64 x 96 model's deep stages (shorter than one 32-pixel
# tile), L % 32 != 0 with odd H, non-FULL chunks, and L above the sequential bound (chunked although copies are given)
CORE_SHAPES = [(120, 160, 96, 6), (60, 80, 192, 12), (30, 40, 384, 24), (15, 20, 768, 48), (64, 64, 384, 24), (4, 6, 384, 24), (2, 3, 768, 48),
               (33, 29, 384, 24), (15, 21, 192, 12), (96, 96, 384, 24)]
CORE_CASES = [s + (False,) for s in CORE_SHAPES] + [(30, 40, 384, 24, True), (60, 80, 192, 12, True)]


@pytest.mark.parametrize("H,W,C,R,switches", CORE_CASES, ids=[f"{h}x{w}xC{c}xR{r}" + ("-switches" if s else "") for h, w, c, r, s in CORE_CASES])
def test_ss2d_core_f16_vs_fp64(gpu_lib, H, W, C, R, switches):
    """(a) xp_ss2d_core_f16_wants_f32_copies is the rule of ss2d_takes_seq and the tags show that form ran; (b) the fast class without copies is bit-identical
    to xp_round_f16 of the f32-container class (same chunked instances, same out_norm code; only the exact half -> float loads differ); (c) the f32-container
    output against fp64; (d) the fp16 outputs of both forms against r16(fp64), and the sequential form against the chunked one."""
    L = _lib()
    B = 2
    inp = _core_inputs(f"{H}x{W}x{C}" + ("s" if switches else ""), B, H, W, C, R, switches)
    seq = _takes_seq(H, W, C, R)
    assert L.load().xp_ss2d_core_f16_wants_f32_copies(H, W, C, R) == int(seq)
    o16, t16 = _core(L, inp, B, H, W, C, R, "amp16f")
    oc, tc = _core(L, inp, B, H, W, C, R, "amp16f", copies=True)
    o32, t32 = _core(L, inp, B, H, W, C, R, "amp16")
    assert _form(t16) == "chunked" and _form(t32) == "chunked" and _form(tc) == ("sequential" if seq else "chunked"), (t16, tc, t32)
    r32 = torch.empty_like(o32)
    L.call("xp_round_f16", L.ptr(o32), L.ptr(r32), o32.numel(), L.current_stream())
    same_b = torch.equal(o16.float(), r32)
    on64, margin = rc.ss2d_core_amp64(inp["u16"], inp["xdbl16"], inp["wdt"], inp["dtb"], inp["A"], inp["D"], inp["lnw"], inp["lnb"], H, W)
    on64 = on64.reshape(-1, C)
    dt_ties = int((margin <= R * 2.0 ** -24).sum())
    rel = (o32.double() - on64).abs() / on64.abs().clamp_min(1.0)
    in_c, worst_c = float((rel <= 2e-5).double().mean()), float(rel.max())
    eq16, ulp16 = _stats(o16, rc.r16(on64))
    eqc, ulpc = _stats(oc, rc.r16(on64))
    eq_cc = float((oc == o16).double().mean())
    print(f"\nss2d_core ({H}, {W}, {C}, {R}){' switches' if switches else ''} B {B}: with copies {_form(tc)}; f16 == round(amp16) {same_b}; amp16 vs fp64 "
          f"{in_c:.5f} within 2e-5, worst {worst_c:.2e} ({dt_ties} dt near a tie); chunked f16 vs r16(fp64) bit-equal {eq16:.5f}, worst {ulp16:.2f} ulp; "
          f"with copies bit-equal {eqc:.5f}, worst {ulpc:.2f} ulp, {eq_cc:.5f} equal to the chunked result")
    assert same_b, "the fp16-storage core differs from xp_round_f16 of the f32-container core"
    assert in_c >= 0.999 and worst_c <= 2e-4, (in_c, worst_c)
    # bars just outside the MI355X measurement (bit-equal 0.99913 - 0.99955, worst 1.00 ulp; sequential vs chunked >= 0.99984 equal)
    assert eq16 >= 0.999 and ulp16 <= 1.01, (eq16, ulp16)
    if seq:
        assert eqc >= 0.999 and ulpc <= 1.01 and eq_cc >= 0.9995, (eqc, ulpc, eq_cc)
    else:
        assert torch.equal(oc, o16), "f32 copies changed the chunked form's result"


@pytest.mark.parametrize("H,W,C,R", [(30, 40, 384, 24), (33, 29, 384, 24), (15, 20, 768, 48)])
def test_ss2d_core_f16_sequential_nw_regimes_are_batch_invariant(gpu_lib, H, W, C, R):
    """launch_ss2d_seq runs NW = 4 / 2 / 1 waves per route, from routes = ceil(C / 64) 4 B against the chip's 4 x CU SIMDs: a batch in every regime (a change
    of the rule fails here instead of leaving the test on one side), every image's slice bit-identical to the image alone (B = 1)."""
    L = _lib()
    n_simd = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    per = math.ceil(C / 64) * 4
    nw = lambda b: 4 if per * b * 4 <= n_simd else (2 if per * b * 2 <= n_simd else 1)
    batches = {4: n_simd // (4 * per), 2: n_simd // (2 * per), 1: n_simd // (2 * per) + 1}
    assert batches[4] >= 2 and all(nw(b) == k for k, b in batches.items()), batches
    assert _takes_seq(H, W, C, R)
    Bn, Li = batches[1], H * W
    inp = _core_inputs(f"nw{H}x{W}x{C}", Bn, H, W, C, R)
    alone = []
    for i in range(Bn):
        one = dict(inp, u16=inp["u16"][i:i + 1], xdbl16=inp["xdbl16"][i * Li:(i + 1) * Li])
        o, t = _core(L, one, 1, H, W, C, R, "amp16f", copies=True)
        assert _form(t) == "sequential"
        alone.append(o)
    for k, b in batches.items():
        o, t = _core(L, inp, b, H, W, C, R, "amp16f", copies=True)
        assert _form(t) == "sequential"
        bad = [i for i in range(b) if not torch.equal(o[i * Li:(i + 1) * Li], alone[i])]
        print(f"ss2d_core_f16 ({H}, {W}, {C}, {R}) NW {k}: batch {b} ({per * b} routes, {n_simd} SIMDs); images differing from their B = 1 run: {bad}")
        assert not bad


# ------------------------------------------------------------------------------------------------------------------------------ glue kernels
@pytest.mark.parametrize("C", [8, 32, 64, 96, 192, 384, 768, 1024])      # every (lanes per row, vectors per lane) instance: 4/1 8/1 16/1 32/1 64/1 64/2
def test_layernorm_f16_vs_fp64(gpu_lib, C):
    """xp_layernorm_f16 at every instance and partial blocks of rows; one row in 7 with a common offset ten times its spread (the two-pass variance), one in
    11 constant (its output is exactly r16(bias))."""
    L = _lib()
    st = L.current_stream()
    w, b = _u(f"lnw/{C}", (C,), 0.5, 1.5), _u(f"lnb/{C}", (C,), -0.5, 0.5)
    for rows in (1, 63, 300, 4801):
        i = torch.arange(rows, device="cuda")[:, None]
        x = _u(f"lnx/{C}/{rows}", (rows, C), -2.0, 2.0)
        x = torch.where(i % 7 == 3, 2.0 * x + 24.0, x)
        const = (i % 11 == 5)[:, 0]
        x16 = torch.where(const[:, None], x[:, :1], x).half()
        X, Y = Canary(rows, C, torch.float16, init=x16), Canary(rows, C, torch.float16)
        L.call("xp_layernorm_f16", X.ptr(), Y.ptr(), L.ptr(w), L.ptr(b), rows, C, 1e-5, st)
        assert X.intact() and Y.intact(), (C, rows)
        assert torch.equal(Y.t[const], b.half().expand(int(const.sum()), C)), (C, rows)
        rc.assert_r16_exact_off_ties(f"layernorm_f16 C {C} rows {rows}", Y.t[~const], rc.layernorm_f16_64(x16[~const], w, b), KAPPA, TIES_LN)


def test_layernorm_f16_refusals(gpu_lib):
    L = _lib()
    w, b = torch.ones(1040, device="cuda"), torch.zeros(1040, device="cuda")
    X, Y = Canary(16, 1040, torch.float16, init=torch.ones(16, 1040, dtype=torch.float16)), Canary(16, 1040, torch.float16)
    for C, xp in ((12, X.ptr()), (1032, X.ptr()), (96, ctypes.c_void_p(X.full.data_ptr() + 2))):        # C % 8 != 0, C > 1024, x not 16-byte aligned
        with pytest.raises(L.XPointHipError):
            L.call("xp_layernorm_f16", xp, Y.ptr(), L.ptr(w), L.ptr(b), 16, C, 1e-5, L.current_stream())
    torch.cuda.synchronize()
    assert bool((Y.bits() == Y.pay).all()), "a refused call wrote its output"


def test_dwconv3x3_silu_f16_vs_fp64(gpu_lib):
    """xp_dwconv3x3_silu_f16: ragged H / W against the 4 x 4 pixel block, 1 x 1 and single-row images, batch 3; the half output without and with the f32 copy
    (which must hold the half values exactly); grids shorter than the 8 XCDs and grids not divisible by 8 (the kernel's XCD band remap)."""
    L = _lib()
    st = L.current_stream()
    B, grids = 3, []
    for C in (4, 12, 96, 192, 384, 768):
        w9c = _r16(_u(f"dww/{C}", (9, C), -0.5, 0.5)).float()
        for H, W in ((1, 1), (1, 9), (5, 7), (60, 80), (15, 20)):
            M = B * H * W
            x16 = _u(f"dwx/{C}/{H}x{W}", (B, H, W, C), -1.5, 1.5).half()
            X = Canary(M, C, torch.float16, init=x16.view(M, C))
            Y, Yc, Y32 = Canary(M, C, torch.float16), Canary(M, C, torch.float16), Canary(M, C)
            L.call("xp_dwconv3x3_silu_f16", X.ptr(), L.ptr(w9c), Y.ptr(), None, B, H, W, C, st)
            L.call("xp_dwconv3x3_silu_f16", X.ptr(), L.ptr(w9c), Yc.ptr(), Y32.ptr(), B, H, W, C, st)
            assert all(t.intact() for t in (X, Y, Yc, Y32)), (C, H, W)
            assert torch.equal(Yc.t, Y.t) and torch.equal(Y32.t, Y.t.float()), (C, H, W)
            rc.assert_r16_exact_off_ties(f"dwconv3x3_silu_f16 C {C} {B}x{H}x{W}", Y.t, rc.dwconv_silu_f16_64(x16, w9c), KAPPA, TIES_DW)
            grids.append(math.ceil(B * math.ceil(H / 4) * math.ceil(W / 4) * (C // 4) / 256))
    assert any(g > 8 and g % 8 for g in grids) and any(g < 8 for g in grids), grids


@pytest.mark.parametrize("CO", [16, 48])
def test_stem_conv_ln_gelu_f16_vs_fp64(gpu_lib, CO):
    """xp_stem_conv_ln_gelu_f16 (both instances) at odd image sizes (Ho = ceil(H / 2)) and a partial last workgroup; the three identical input channels'
    weights folded on the host as the model packs them."""
    L = _lib()
    st = L.current_stream()
    w, b = _u(f"stw/{CO}", (CO, 3, 3, 3), -0.4, 0.4), _u(f"stb/{CO}", (CO,), -0.2, 0.2)
    lnw, lnb = _u(f"stlnw/{CO}", (CO,), 0.8, 1.2), _u(f"stlnb/{CO}", (CO,), -0.2, 0.2)
    w9co = _r16(w).sum(dim=1).permute(1, 2, 0).reshape(9, CO).float().contiguous()
    b16 = _r16(b).float()
    for B, H, W in ((2, 33, 47), (2, 64, 97), (1, 7, 5)):
        img = _u(f"stimg/{H}x{W}", (B, 1, H, W), 0.0, 1.0)
        Y = Canary(B * ((H + 1) // 2) * ((W + 1) // 2), CO, torch.float16)
        L.call("xp_stem_conv_ln_gelu_f16", L.ptr(img), L.ptr(w9co), L.ptr(b16), L.ptr(lnw), L.ptr(lnb), Y.ptr(), B, H, W, CO, 1e-5, st)
        assert Y.intact(), (CO, H, W)
        rc.assert_r16_exact_off_ties(f"stem_conv_ln_gelu_f16 CO {CO} {B}x{H}x{W}", Y.t, rc.stem_f16_64(img, w, b, lnw, lnb, kappa=KAPPA), KAPPA, TIES_STEM)


def test_depth_to_space_f16_permutation_and_status(gpu_lib):
    """xp_depth_to_space_nhwc_f16: the oracle's permutation exactly, the f32 output = the half output; the status word untouched by finite input (+-65504
    included), XP_STATUS_ENC set by a single +inf, -inf or NaN anywhere (the last element lies in a partial last wave), bits already set kept."""
    L = _lib()
    st = L.current_stream()
    for B, H, W, C in ((2, 15, 20, 768), (1, 3, 5, 64), (3, 7, 9, 128)):
        n, Cq = B * H * W * C, C // 16
        x16 = _u(f"d2s/{B}x{H}x{W}x{C}", (B, H, W, C), -4.0, 4.0).half()
        x16.view(-1)[0], x16.view(-1)[-1] = 65504.0, -65504.0
        ref = rc.depth_to_space(x16.permute(0, 3, 1, 2).contiguous(), 4).permute(0, 2, 3, 1).reshape(-1, Cq)

        def run(xin, status):
            X = Canary(B * H * W, C, torch.float16, init=xin.view(-1, C))
            Y32, Y16 = Canary(n // Cq, Cq), Canary(n // Cq, Cq, torch.float16)
            L.call("xp_depth_to_space_nhwc_f16", X.ptr(), Y32.ptr(), Y16.ptr(), B, H, W, C, 4, L.ptr(status), st)
            torch.cuda.synchronize()
            assert X.intact() and Y32.intact() and Y16.intact(), (B, H, W, C)
            return Y32.t.clone(), Y16.t.clone()
        status = torch.full((1,), 6, dtype=torch.int32, device="cuda")      # XP_STATUS_PROB | XP_STATUS_DESC already set
        y32, y16 = run(x16, status)
        assert torch.equal(y16, ref) and torch.equal(y32, y16.float()), (B, H, W, C)
        assert int(status) == 6, int(status)
        for pos in (0, n // 2 + 1, n - 1):
            for v in (float("inf"), float("-inf"), float("nan")):
                xb = x16.clone()
                xb.view(-1)[pos] = v
                status = torch.full((1,), 6, dtype=torch.int32, device="cuda")
                run(xb, status)
                assert int(status) == 7, (B, H, W, C, pos, v, int(status))
        print(f"depth_to_space_f16 {B}x{H}x{W}x{C}: permutation exact, status word set by inf / -inf / NaN at 0, n/2 + 1, n - 1")


SPECIAL = [1.0 + 2 ** -11, 1.0 + 3 * 2 ** -11, -(1.0 + 2 ** -11), 2049.0, 2051.0, -2051.0,               # ties, both parities
           65519.99609375, -65519.99609375, 65520.0, -65520.0, 65504.0, 1e30,                            # the largest value that rounds to 65504, the smallest that overflows
           2.0 ** -24, 2.0 ** -25, -(2.0 ** -25), 3 * 2.0 ** -25, 1.5 * 2.0 ** -24, 2.0 ** -26, -(2.0 ** -26),  # subnormals; ties to 0 and to 2^-23; underflow to +-0
           2.0 ** -14 - 2.0 ** -25, 2.0 ** -15 + 2.0 ** -26, 0.0, -0.0, float("inf"), float("-inf"), float("nan"), 0.1, -3.14159]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025])
def test_f16_conversions_round_like_torch(gpu_lib, n):
    """xp_f32_to_f16 (the weight conversion) and xp_round_f16 (y.to(x.dtype) after the scan; also in place) bit for bit equal to torch's .half() (round to
    nearest even): ties, overflow to +-inf, subnormals and underflow with the sign of zero, NaN; the specials also in the scalar tail after the vector part."""
    L = _lib()
    st = L.current_stream()
    sp = torch.tensor(SPECIAL, dtype=torch.float32)
    e, m, s = (torch.from_numpy(synth.uniform(f"amp16f/cvt/{k}{n}", (n,), lo, hi)) for k, lo, hi in (("e", -27.0, 17.0), ("m", 1.0, 2.0), ("s", -1.0, 1.0)))
    rnd = (m * torch.exp2(e.floor()) * torch.sign(s)).float()
    vecs = [torch.cat([sp[i:i + n], rnd[:max(0, n - len(sp[i:i + n]))]]) for i in range(0, len(sp), n)] if n < len(sp) else [torch.cat([rnd[:n - len(sp)], sp])]
    for x in vecs:
        want, nan = x.half(), torch.isnan(x)
        X = Canary(1, n, init=x.view(1, n).cuda())
        Y16, Y32, Z = Canary(1, n, torch.float16), Canary(1, n), Canary(1, n, init=x.view(1, n).cuda())
        L.call("xp_f32_to_f16", X.ptr(), Y16.ptr(), n, st)
        L.call("xp_round_f16", X.ptr(), Y32.ptr(), n, st)
        L.call("xp_round_f16", Z.ptr(), Z.ptr(), n, st)
        torch.cuda.synchronize()
        assert all(t.intact() for t in (X, Y16, Y32, Z)), n
        g16, g32, gz = Y16.t.view(-1).cpu(), Y32.t.view(-1).cpu(), Z.t.view(-1).cpu()
        assert torch.equal(g16.view(torch.int16)[~nan], want.view(torch.int16)[~nan]) and bool(torch.isnan(g16[nan]).all()), (n, x, g16)
        for g in (g32, gz):
            assert torch.equal(g.view(torch.int32)[~nan], want.float().view(torch.int32)[~nan]) and bool(torch.isnan(g[nan]).all()), (n, x, g)
    print(f"f32 -> f16 conversions, n = {n}: {len(vecs)} vectors bit-equal to torch")
