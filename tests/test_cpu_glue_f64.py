"""tests/glue_f64.py against torch's own float64 operators on ragged shapes (1e-12 for arithmetic, exact for data movement), and the case tables of
tests/test_gpu_glue_f32.py against the restated launch rules of tests/glue_cases.py: every xp_layernorm instance at both ends of its C range, every
xp_layernorm_p32 instance, the depthwise workgroup counts around the 8-XCD renumbering."""
import pytest
import torch
import torch.nn.functional as F

from oracle import xpoint_oracle as xo
from tests import glue_cases as gc, glue_f64 as g64

TOL = 1e-12


def _r(seed, shape, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo


def _close(got, ref):
    assert got.shape == ref.shape and got.dtype == torch.float64, (got.shape, ref.shape, got.dtype)
    err = float((got - ref).abs().max())
    assert err <= TOL * max(1.0, float(ref.abs().max())), err


@pytest.mark.parametrize("rows,C", [(5, 7), (3, 260)])
@pytest.mark.parametrize("gelu", [False, True])
def test_layernorm(rows, C, gelu):
    x, w, b = _r(1, (rows, C), -3, 3), _r(2, (C,), 0.5, 1.5), _r(3, (C,))
    x[1] += 60.0
    ref = F.layer_norm(x, (C,), w, b, 1e-5)
    _close(g64.layernorm(x, w, b, 1e-5, gelu), F.gelu(ref) if gelu else ref)
    const = g64.layernorm(torch.full((2, C), 1.75), w, b)
    assert torch.equal(const, b.expand(2, C)), "a constant row must give exactly the bias"


@pytest.mark.parametrize("B,H,W,C", [(2, 5, 9, 12), (1, 1, 7, 4)])
def test_dwconv3x3_silu(B, H, W, C):
    x, w9c = _r(4, (B, H, W, C)), _r(5, (9, C))
    ref = F.silu(F.conv2d(x.permute(0, 3, 1, 2), w9c.t().reshape(C, 1, 3, 3), None, padding=1, groups=C)).permute(0, 2, 3, 1)
    _close(g64.dwconv3x3_silu(x, w9c), ref)


@pytest.mark.parametrize("B,H,W,Co", [(2, 7, 9, 16), (1, 2, 5, 48), (1, 1, 1, 16)])
def test_stem_conv_ln_gelu(B, H, W, Co):
    img, w9co, bias = _r(6, (B, H, W), 0, 1), _r(7, (9, Co), -0.6, 0.6), _r(8, (Co,), -0.2, 0.2)
    lnw, lnb = _r(9, (Co,), 0.8, 1.2), _r(10, (Co,), -0.1, 0.1)
    conv = F.conv2d(img[:, None], w9co.t().reshape(Co, 1, 3, 3), bias, stride=2, padding=1).permute(0, 2, 3, 1)
    assert conv.shape[1:3] == ((H + 1) // 2, (W + 1) // 2)
    _close(g64.stem_conv_ln_gelu(img, w9co, bias, lnw, lnb, 1e-5), F.gelu(F.layer_norm(conv, (Co,), lnw, lnb, 1e-5)))


@pytest.mark.parametrize("B,H,W,C,bs", [(2, 3, 5, 32, 4), (1, 2, 3, 18, 3)])
def test_depth_to_space_is_the_oracles(B, H, W, C, bs):
    x = _r(11, (B, H, W, C))
    ref = xo.depth_to_space(x.permute(0, 3, 1, 2).contiguous(), bs).permute(0, 2, 3, 1)
    assert torch.equal(g64.depth_to_space(x, bs), ref)
    # and the formula itself, element by element
    Cq, y = C // (bs * bs), g64.depth_to_space(x, bs)
    for (n, h, w, i, j, c) in ((0, 1, 2, 0, 1, 0), (B - 1, H - 1, W - 1, bs - 1, bs - 2, Cq - 1)):
        assert y[n, bs * h + i, bs * w + j, c] == x[n, h, w, (bs * i + j) * Cq + c]


@pytest.mark.parametrize("B,Hc,Wc,r,pad", [(2, 3, 5, 8, 0), (1, 2, 3, 3, 6)])
def test_softmax_shuffle(B, Hc, Wc, r, pad):
    nch = r * r + 1
    lg = _r(12, (B, Hc, Wc, nch + pad), -6, 6)
    lg[..., nch:] = float("nan")
    lg[0, 0, 0, :nch] += 80.0
    ref = F.pixel_shuffle(F.softmax(lg[..., :nch].permute(0, 3, 1, 2), 1)[:, :-1], r)[:, 0]
    _close(g64.softmax_shuffle(lg, r, 0), ref)
    e = torch.exp(lg[..., :nch].permute(0, 3, 1, 2))
    _close(g64.softmax_shuffle(lg, r, 1), F.pixel_shuffle((e / (e.sum(1, keepdim=True) + 1e-5))[:, :-1], r)[:, 0])


@pytest.mark.parametrize("rows,C", [(5, 65), (3, 1)])
def test_l2norm_rows(rows, C):
    x = _r(13, (rows, C), -2, 2) * torch.tensor([1e-3, 1.0, 1e3, 1.0, 1.0])[:rows, None]
    _close(g64.l2norm_rows(x, 1e-12), F.normalize(x, p=2, dim=1, eps=1e-12))
    _close(g64.l2norm_rows(x, -1.0), x / x.norm(dim=1, keepdim=True))
    z = torch.zeros(2, C, dtype=torch.float64)
    z[1] = 1e-20
    got = g64.l2norm_rows(z, 1e-12)
    assert torch.equal(got[0], torch.zeros(C, dtype=torch.float64)) and torch.equal(got[1], z[1] / 1e-12)


@pytest.mark.parametrize("B,HW,C", [(2, 31, 33), (1, 5, 1)])
def test_nhwc_to_nchw(B, HW, C):
    x = _r(14, (B, HW, C))
    got = g64.nhwc_to_nchw(x)
    assert got.is_contiguous() and torch.equal(got, x.permute(0, 2, 1))


@pytest.mark.parametrize("B,H,W,C", [(2, 3, 5, 4), (1, 7, 2, 9)])
def test_maxpool2(B, H, W, C):
    x = (_r(15, (B, H, W, C)) * 4).floor() / 4
    x.view(-1)[::13] = float("inf")
    x.view(-1)[5::17] = float("-inf")
    assert torch.equal(g64.maxpool2(x), F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))


@pytest.mark.parametrize("B,hw,C", [(2, 3, 65), (1, 1, 1)])
def test_costvolume_mean(B, hw, C):
    a, b = F.normalize(_r(16, (B, hw, C)), dim=2), F.normalize(_r(17, (B, hw, C)), dim=2)
    ref = F.adaptive_avg_pool2d(torch.bmm(a, b.transpose(1, 2)).view(B, hw, hw, 1), 1).view(B, hw)
    _close(g64.costvolume_mean(a, b), ref)


def test_u8_to_unit_is_the_f32_division():
    k = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(g64.u8_to_unit(k), k.float() / 255.0)


# ------------------------------------------------------------------------------------------------------------------------------ launch rules and tables
def test_ln_instance_restates_the_ladder():
    assert gc.ln_instance(96) == ((32, 1, 4), 32) and gc.ln_instance(384) == ((64, 2, 1), 4) and gc.ln_instance(768) == ((64, 3, 1), 4)
    assert gc.ln_instance(16) == ((4, 1, 4), 256) and gc.ln_instance(1024) == ((64, 4, 1), 4)
    assert gc.ln_instance(96, aligned=False) == ("scalar", 4) and gc.ln_instance(63) == ("scalar", 4)
    for inst, (lo, hi) in gc.LN_RANGES.items():
        assert gc.ln_instance(lo)[0] == inst and gc.ln_instance(hi)[0] == inst
        assert lo == 4 or gc.ln_instance(lo - 4)[0] != inst
        assert hi == 1024 or gc.ln_instance(hi + 4)[0] != inst
        lpr, nv, rpg = inst
        assert gc.ln_instance(lo)[1] == 4 * (64 // lpr) * rpg and lpr * nv * 4 >= hi       # the lanes of a row hold all of it


def test_gpu_case_tables_reach_every_instance():
    seen = {}
    for C, aligned in gc.LN_CASES:
        seen.setdefault(gc.ln_instance(C, aligned)[0], []).append(C)
    assert set(seen) == set(gc.LN_INSTANCES) | {"scalar"}
    for inst in gc.LN_INSTANCES:
        assert sorted(seen[inst]) == list(gc.LN_RANGES[inst]), (inst, seen[inst])
    assert sorted(seen["scalar"]) == [1, 3, 63, 65, 96, 1022]
    for C, aligned in gc.LN_CASES:                                           # rows: 1 and both sides of a workgroup edge
        R = gc.ln_instance(C, aligned)[1]
        assert set(gc.ln_rows(R)) >= {1, R - 1, R, R + 1} - {0}
    assert {gc.lnp_instance(C)[0] for C in gc.LNP_CS} == set(gc.LN_INSTANCES) - {(4, 1, 4)}
    assert {32, 64, 128, 160, 256, 288, 512, 544, 800, 1024} <= set(gc.LNP_CS)
    assert {gc.dw_blocks(*s) for s in gc.DW_SMALL} == {1}
    assert all(gc.dw_blocks(*s) == nb and s[3] == 32 for nb, s in gc.DW_BLOCKS.items())
    assert {gc.dw_blocks(*s) for s in gc.DW_CASES} == {1, 7, 8, 9, 15, 17}
    assert gc.dw_blocks(1, 66, 62, 32) == 9
    # stem: output pixels against workgroups of 64
    assert [B * ((H + 1) // 2) * ((W + 1) // 2) for B, H, W in gc.STEM_CASES] == [1, 1, 6, 40, 72, 216]
    # depth-to-space: which cases take the scalar kernel (Cq % 4 != 0 or an unaligned buffer)
    scalar = [(C // (bs * bs), off) for (_, _, _, C, bs, off) in gc.D2S_CASES if (C // (bs * bs)) % 4 or off]
    assert scalar == [(1, 0), (2, 0), (48, 1), (2, 0)] and len(gc.D2S_CASES) == 8
    assert sorted(B * H * W for B, H, W in gc.SMX_CELLS) == [1, 3, 4, 5, 15, 16, 17]
