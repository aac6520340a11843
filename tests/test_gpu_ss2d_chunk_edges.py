"""The chunked SS2D core's pass 3 at the smallest shapes where its once-per-chunk operand loads and its after-the-loop stores can go wrong
(csrc/ss2d_chunked.hip: a thread loads its chunk's T values of u, and the column pair the row pair's partial sums, in one batch before the forward route;
the row pair stores its T sums after the backward route).  All three instantiations of the template: f32 (xp_ss2d_core_fwd), the mixed-precision
recipe in f32 containers (xp_set_amp_mode(1) + xp_ss2d_core_fwd) and fp16 storage (xp_ss2d_core_fwd_f16).

    5 x 7,  C = 96,  R = 6    L = 35, T = 32, nc = 2 chunks in ONE workgroup of two chunk slots: the last chunk partial (3 of 32 pixels; offsets of
                              -1 in the operand batch), the general (bounds-tested) instance
    5 x 14, C = 96,  R = 6    L = 70, nc = 3 with two chunk slots per workgroup (nc % cpb != 0): the last workgroup holds a partial chunk (6 of 32
                              pixels) AND an empty slot — stage_chunk writes -1 for the whole slot, its threads skip the operand batch and the
                              deferred stores, out_norm skips its rows
    9 x 13, C = 192, R = 12   one chunk per workgroup, T = 16, L = 117 ragged
    8 x 16, C = 96,  R = 6    L = 128: every chunk and every workgroup complete — the instance without bounds tests (f32 and fp16 storage)
    4 x 8,  C = 384, R = 24   T = 16, the wave-per-pixel out_norm branch, one route's weights at a time
    3 x 5,  C = 96,  R = 48   T = 32 with the largest dt_rank: the instances that reach the register bound of a 768-thread workgroup and spill
                              (no model shape pairs them; the entry point accepts them); one chunk and an empty slot

Bounds.  f32: test_gpu_kernels.py::test_ss2d_core_vs_oracle's (max |out - oracle| < 2e-5 against oracle.xpoint_oracle.ss2d_core), same input ranges.
The two mixed-precision instantiations are held to their class's own reference, NOT to the oracle's f32 core: an fp16-rounded output cannot meet 2e-5
against it.  The reference is the float64 restatement of the recipe (tests/amp_recipe64.py, independent of the code under test), with the bars of
test_gpu_amp16f_kernels.py::test_ss2d_core_f16_vs_fp64: f32 containers within 2e-4 relative, fp16 storage within 1.01 fp16 ulp of r16(fp64) and
bit-identical to xp_round_f16 of the f32-container result.  That test also asserts two FRACTIONS (>= 0.999 of the outputs within 2e-5 / bit-equal) on
>= 10^5 outputs, i.e. a miss rate <= 1e-3.  On the n = 2 880 - 44 928 outputs here the same rate is asserted as a count: misses <= n 1e-3 +
4 sqrt(n 1e-3), the mean plus four standard deviations of a binomial at that rate (_max_misses), so that a sample of this size cannot fail by chance.

The workspace (carry entries and the row pair's partial sums `ya`) is filled with NaN before every call: the column pair reads exactly the `ya`
elements the row pair's deferred stores must have written, so a missed store shows as a non-finite output.

The input builders, the canary allocation and the tag reader are the private helpers of test_gpu_amp16f_kernels.py and
test_gpu_batch_invariance.py (this check is one file by design): a rename there has to be followed here."""
import functools
import math

import pytest
import torch

from oracle import xpoint_oracle as xo
from tests import amp_recipe64 as rc
from tests.test_gpu_amp16f_kernels import _core_inputs, _form, _stats
from tests.test_gpu_batch_invariance import Canary, _tags
from xpoint_amd import synth

pytestmark = pytest.mark.gpu

B = 2
SHAPES = [(5, 7, 96, 6), (5, 14, 96, 6), (9, 13, 192, 12), (8, 16, 96, 6), (4, 8, 384, 24), (3, 5, 96, 48)]      # H, W, C, dt_rank
IDS = [f"{h}x{w}xC{c}xR{r}" for h, w, c, r in SHAPES]
CHUNKED = {"ss2d_pass1", "ss2d_pass2", "ss2d_pass3_row", "ss2d_pass3_col_ln"}


def _max_misses(n):
    """Largest miss count of n outputs still consistent with a miss rate of 1e-3 (module docstring)."""
    return math.floor(n * 1e-3 + 4.0 * math.sqrt(n * 1e-3))


def _lib():
    from xpoint_amd import _lib as L
    return L


def _u(name, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(synth.uniform("ss2d_edges/" + name, shape, lo, hi))


def _nan_workspace(L, batch, H, W, C):
    nbytes = L.load().xp_ss2d_core_workspace_bytes(batch, H, W, C)
    return torch.full((nbytes // 4 + 16,), float("nan"), device="cuda"), nbytes


@functools.lru_cache(maxsize=None)
def _f32_case(H, W, C, R):
    """test_ss2d_core_vs_oracle's inputs (same ranges) in the kernels' layout, and the oracle's result (B, H, W, C): computed once per shape."""
    pre, order = "op.", rc.ORDER
    sd = {pre + "x_proj_weight": _u(f"xp{C}r{R}", (4, R + 2, C), -C ** -0.5, C ** -0.5),
          pre + "dt_projs_weight": _u(f"dtw{C}r{R}", (4, C, R), -R ** -0.5, R ** -0.5),
          pre + "dt_projs_bias": _u(f"dtb{C}", (4, C), -6.9, -2.25),
          pre + "A_logs": _u(f"al{C}", (4 * C, 1), -0.5, 0.5), pre + "Ds": _u(f"ds{C}", (4 * C,), 0.5, 1.5),
          pre + "out_norm.weight": _u(f"onw{C}", (C,), 0.8, 1.2), pre + "out_norm.bias": _u(f"onb{C}", (C,), -0.1, 0.1)}
    x = _u(f"x{C}x{H}x{W}", (B, C, H, W), -0.3, 1.0)
    ref = xo.ss2d_core(x, sd, pre)
    L = _lib()
    u = x.permute(0, 2, 3, 1).contiguous().cuda()
    xw = sd[pre + "x_proj_weight"][order].reshape(4 * (R + 2), C).contiguous().cuda()
    xdbl = torch.empty((B * H * W, 4 * (R + 2)), device="cuda")
    L.call("xp_gemm_nt", L.ptr(u), L.ptr(xw), L.ptr(xdbl), None, None, None, None, B * H * W, 4 * (R + 2), C, C, 4 * (R + 2), 0, 0, L.current_stream())
    torch.cuda.synchronize()
    par = [sd[pre + "dt_projs_weight"][order].permute(0, 2, 1).contiguous().cuda(), sd[pre + "dt_projs_bias"][order].contiguous().cuda(),
           (-torch.exp(sd[pre + "A_logs"].float())).view(4, C)[order].contiguous().cuda(), sd[pre + "Ds"].view(4, C)[order].contiguous().cuda(),
           sd[pre + "out_norm.weight"].cuda(), sd[pre + "out_norm.bias"].cuda()]
    return u, xdbl, par, ref


def _run_f32(H, W, C, R, batch=B):
    """xp_ss2d_core_fwd, chunked form, on the first `batch` images, NaN workspace, output in a canary allocation: (batch * H * W, C) f32."""
    L = _lib()
    u, xdbl, par, _ = _f32_case(H, W, C, R)
    ws, nbytes = _nan_workspace(L, batch, H, W, C)
    out = Canary(batch * H * W, C)

    def fn():
        L.call("xp_ss2d_core_set_mode", 0)
        try:
            L.call("xp_ss2d_core_fwd", L.ptr(u), L.ptr(xdbl), *[L.ptr(t) for t in par], out.ptr(), L.ptr(ws), nbytes, batch, H, W, C, R, 1, 1e-5,
                   L.current_stream())
            torch.cuda.synchronize()
        finally:
            L.call("xp_ss2d_core_set_mode", -1)
    tags = _tags(fn)
    assert CHUNKED <= set(tags), tags
    assert out.intact(), f"f32 ({H}, {W}, {C}, {R}) B = {batch}: a padding word of the output changed"
    return out.t.clone()


@functools.lru_cache(maxsize=None)
def _amp_case(H, W, C, R):
    """The mixed-precision classes' inputs (test_gpu_amp16f_kernels._core_inputs) and the float64 recipe's out_norm value (B * H * W, C): once per shape."""
    inp = _core_inputs(f"edges{H}x{W}x{C}r{R}", B, H, W, C, R)
    on64, _ = rc.ss2d_core_amp64(inp["u16"], inp["xdbl16"], inp["wdt"], inp["dtb"], inp["A"], inp["D"], inp["lnw"], inp["lnb"], H, W)
    return inp, on64.reshape(-1, C)


def _run_amp(cls, H, W, C, R, batch=B):
    """cls "amp16f": xp_ss2d_core_fwd_f16 without f32 copies (always the chunked form); "amp16": the same half values in f32 containers."""
    L = _lib()
    inp, _ = _amp_case(H, W, C, R)
    M = batch * H * W
    u16, x16 = inp["u16"][:batch].contiguous(), inp["xdbl16"][:M].contiguous()
    u32, x32 = u16.float(), x16.float()
    ws, nbytes = _nan_workspace(L, batch, H, W, C)
    par = [L.ptr(inp[k]) for k in ("wdt", "dtb", "A", "D", "lnw", "lnb")]
    tail = (L.ptr(ws), nbytes, batch, H, W, C, R, 1, 1e-5, L.current_stream())
    if cls == "amp16f":
        out = Canary(M, C, torch.float16)

        def fn():
            L.call("xp_ss2d_core_fwd_f16", L.ptr(u16), L.ptr(x16), None, None, *par, out.ptr(), *tail)
            torch.cuda.synchronize()
    else:
        out = Canary(M, C)

        def fn():
            L.call("xp_set_amp_mode", 1)
            try:
                L.call("xp_ss2d_core_fwd", L.ptr(u32), L.ptr(x32), *par, out.ptr(), *tail)
                torch.cuda.synchronize()
            finally:
                L.call("xp_set_amp_mode", 0)
    tags = _tags(fn)
    assert _form(tags) == "chunked", tags
    assert out.intact(), f"{cls} ({H}, {W}, {C}, {R}) B = {batch}: a padding word of the output changed"
    return out.t.clone()


@pytest.mark.parametrize("H,W,C,R", SHAPES, ids=IDS)
def test_chunk_edges_f32_vs_oracle(gpu_lib, H, W, C, R):
    out = _run_f32(H, W, C, R)
    ref = _f32_case(H, W, C, R)[3].reshape(-1, C)
    assert bool(torch.isfinite(out).all()), "non-finite output: the column pair read a workspace element that the row pair did not write"
    err = float((out.cpu() - ref).abs().max())
    print(f"\nss2d chunk edges f32 ({H}, {W}, {C}, {R}) B {B}: max |out - oracle| {err:.2e}")
    assert err < 2e-5, err


@pytest.mark.parametrize("H,W,C,R", SHAPES, ids=IDS)
def test_chunk_edges_mixed_precision_vs_fp64(gpu_lib, H, W, C, R):
    L = _lib()
    on64 = _amp_case(H, W, C, R)[1]
    o16, o32 = _run_amp("amp16f", H, W, C, R), _run_amp("amp16", H, W, C, R)
    assert bool(torch.isfinite(o16).all()) and bool(torch.isfinite(o32).all()), "non-finite output: a workspace element was read before it was written"
    r32 = torch.empty_like(o32)
    L.call("xp_round_f16", L.ptr(o32), L.ptr(r32), o32.numel(), L.current_stream())
    torch.cuda.synchronize()
    rel = (o32.double() - on64).abs() / on64.abs().clamp_min(1.0)
    in_c, worst_c = float((rel <= 2e-5).double().mean()), float(rel.max())
    eq16, ulp16 = _stats(o16, rc.r16(on64))
    print(f"\nss2d chunk edges ({H}, {W}, {C}, {R}) B {B}: f32 containers vs fp64 {in_c:.5f} within 2e-5, worst {worst_c:.2e}; fp16 storage vs r16(fp64) "
          f"bit-equal {eq16:.5f}, worst {ulp16:.2f} ulp")
    assert torch.equal(o16.float(), r32), "the fp16-storage core differs from xp_round_f16 of the f32-container core"
    assert worst_c <= 2e-4, worst_c
    assert ulp16 <= 1.01, ulp16
    n, k = on64.numel(), _max_misses(on64.numel())
    assert round((1.0 - in_c) * n) <= k and round((1.0 - eq16) * n) <= k, (n, k, in_c, eq16)


@pytest.mark.parametrize("H,W,C,R", SHAPES[:2], ids=IDS[:2])
def test_partial_chunk_cases_are_batch_invariant(gpu_lib, H, W, C, R):
    """5 x 7 (a partial last chunk; one full workgroup) and 5 x 14 (a partial last chunk and an empty chunk slot in the last workgroup) alone are
    bit-identical to image 0 of the batch of two, in every instantiation."""
    Li = H * W
    assert torch.equal(_run_f32(H, W, C, R, batch=1), _run_f32(H, W, C, R)[:Li])
    for cls in ("amp16f", "amp16"):
        assert torch.equal(_run_amp(cls, H, W, C, R, batch=1), _run_amp(cls, H, W, C, R)[:Li]), cls
