"""Case tables of tests/test_gpu_glue_f32.py and the two host-side restatements of launch rules that choose them, shared with
tests/test_cpu_glue_f64.py, which asserts on the CPU that the tables reach every dispatch instance.  Nothing here calls a kernel."""
import math


def ln_instance(C, aligned=True):
    """The kernel xp_layernorm launches for C channels (csrc/elementwise.hip, layernorm_impl: `const bool vec = (C % 4 == 0) && (... & 15) == 0` and the
    `C4 <=` ladder under it; XP_LN_LAUNCH gives RPG = 4 to NV == 1 and 1 otherwise): ("scalar" | (LPR, NV, RPG), rows per workgroup).  A workgroup is 4
    waves; a wave of the vector kernel holds 64 / LPR rows per pass and RPG passes, a wave of the scalar kernel one row.  aligned: x, y, w and b all on
    16-byte boundaries."""
    assert 1 <= C <= 1024
    if C % 4 or not aligned:
        return "scalar", 4
    C4 = C // 4
    for top, lpr, nv in ((4, 4, 1), (8, 8, 1), (16, 16, 1), (32, 32, 1), (64, 64, 1), (128, 64, 2), (192, 64, 3), (256, 64, 4)):
        if C4 <= top:
            rpg = 4 if nv == 1 else 1
            return (lpr, nv, rpg), 4 * (64 // lpr) * rpg


def lnp_instance(C):
    """The same for xp_layernorm_p32 (C a multiple of 32; its ladder starts at `C4 <= 8`, so C = 32 shares the 8-lane instance)."""
    assert C % 32 == 0 and 32 <= C <= 1024
    inst, rows = ln_instance(C)
    return ((8, 1, 4), 128) if inst == (4, 1, 4) else (inst, rows)


def dw_blocks(B, H, W, C):
    """Workgroups of xp_dwconv3x3_silu (csrc/elementwise.hip: `total = batch * ceil(H / DW_PH) * ceil(W / DW_PW) * (C / 4)`, grid xp_cdiv(total, 256)):
    a thread owns a 4 x 4 pixel patch of 4 channels."""
    assert C % 4 == 0
    return math.ceil(B * math.ceil(H / 4) * math.ceil(W / 4) * (C // 4) / 256)


LN_INSTANCES = [(4, 1, 4), (8, 1, 4), (16, 1, 4), (32, 1, 4), (64, 1, 4), (64, 2, 1), (64, 3, 1), (64, 4, 1)]
# instance -> (lowest C, highest C) of its range
LN_RANGES = {(4, 1, 4): (4, 16), (8, 1, 4): (20, 32), (16, 1, 4): (36, 64), (32, 1, 4): (68, 128), (64, 1, 4): (132, 256), (64, 2, 1): (260, 512),
             (64, 3, 1): (516, 768), (64, 4, 1): (772, 1024)}
# (C, aligned): both ends of every vector instance, then the scalar kernel (C % 4 != 0 below, between and above whole waves; C = 96 through a pointer
# that is one float off a 16-byte boundary)
LN_CASES = [(c, True) for lo_hi in LN_RANGES.values() for c in lo_hi] + [(1, True), (3, True), (63, True), (65, True), (1022, True), (96, False)]
LNP_CS = [32, 64, 96, 128, 160, 256, 288, 512, 544, 768, 800, 1024]


def ln_rows(rows_per_wg):
    """1 and the three row counts around a workgroup edge"""
    return sorted({1, rows_per_wg - 1, rows_per_wg, rows_per_wg + 1} - {0})


# (B, H, W, C): images below the 4 x 4 patch, C = 4, ragged sizes; then one C = 32 shape per workgroup count 7, 8, 9, 15, 17 (the kernel renumbers its
# workgroups over the 8 XCDs: q = nb >> 3, r = nb & 7)
DW_SMALL = [(1, 1, 1, 4), (1, 1, 7, 4), (1, 7, 1, 8), (2, 4, 4, 8), (1, 5, 9, 12), (3, 2, 3, 96)]
DW_BLOCKS = {7: (1, 53, 57, 32), 8: (1, 61, 58, 32), 9: (1, 66, 62, 32), 15: (1, 85, 83, 32), 17: (3, 45, 57, 32)}
DW_CASES = DW_SMALL + list(DW_BLOCKS.values())

# (B, H, W): 1, 1, 6, 40, 72 and 216 output pixels against workgroups of 64
STEM_CASES = [(1, 1, 1), (1, 2, 2), (1, 3, 5), (2, 7, 9), (1, 16, 18), (3, 15, 17)]
STEM_COS = [16, 48]

# (B, H, W, C, bs, x offset in floats); Cq = 2 and the offset buffer take the scalar kernel
D2S_CASES = [(1, 1, 1, 16, 4, 0), (2, 3, 5, 32, 4, 0), (1, 2, 3, 64, 4, 0), (2, 3, 5, 768, 4, 0), (1, 3, 2, 48, 2, 0), (1, 2, 2, 36, 3, 0),
             (2, 3, 5, 768, 4, 1), (1, 2, 3, 18, 3, 0)]

SMX_RS = [1, 2, 8, 11]
SMX_CELLS = [(1, 1, 1), (1, 1, 3), (1, 2, 2), (1, 1, 5), (1, 3, 5), (2, 2, 4), (1, 1, 17)]        # 1, 3, 4, 5, 15, 16, 17 cells; a wave takes 4
SMX_KINDS = ["plain", "shifted", "spike", "mode1"]

L2_CS = [1, 63, 64, 65, 256, 257]
L2_ROWS = [1, 3, 4, 5]
L2_EPS = [1e-12, -1.0]

NCHW_CASES = [(1, 1, 1), (2, 31, 33), (1, 32, 32), (3, 33, 31), (1, 65, 256), (2, 240, 48)]       # (B, HW, C) against 32 x 32 tiles
POOL_CASES = [(1, 2, 2, 1), (2, 3, 5, 4), (1, 4, 6, 65), (1, 7, 2, 256)]
CV_CASES = [(1, 1, 1), (2, 3, 65), (1, 5, 257), (1, 2, 8192)]                                     # (B, hw, C)
U8_NS = [1, 3, 4, 5, 1023, 1024, 1025]
