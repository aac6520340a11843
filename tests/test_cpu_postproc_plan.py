"""Which path of csrc/box_nms.hip a shape takes, pinned without a GPU.

`xp_box_nms_plan` answers with the launcher's own functions (make_nms_table, nms_two_launch_applies, nms_finish_plan), so these tests read the
library, not a copy of its rules.  tests/test_gpu_postproc_paths.py relies on every plan asserted here: a later change of a tile size, of the LDS
budget or of the form's conditions fails here, on the CPU, instead of silently moving a GPU test onto another path."""
import os

import numpy as np
import pytest

from tests import postproc_cases as pc
from xpoint_amd import _lib


@pytest.fixture(scope="module")
def lib():
    os.environ.pop("XP_NMS_SWEEP", None)          # the library reads it once, at the first plan: these are the plans of a plain process
    return _lib.load()


@pytest.mark.parametrize("shape,form,reach,bands", [((480, 640), 1, 6, 1), ((1000, 700), 1, 6, 2), ((1024, 1024), 1, 6, 3), ((2048, 640), 1, 6, 4)])
def test_model_sizes(lib, shape, form, reach, bands):
    got = pc.plan(lib, *shape, 8, 0.1)
    assert got[:3] == (form, reach, bands), got
    assert got[3] == -(-shape[0] // bands)


@pytest.mark.parametrize("size_iou,reach", pc.REACH_TABLE)
def test_reach_table(lib, size_iou, reach):
    size, iou = size_iou
    ovl, r = pc.overlap_table(size, iou)
    assert r == reach
    assert ovl[0, 0] and (reach == 15 or not ovl[reach + 1:, :].any())
    assert pc.plan(lib, 70, 100, size, iou)[1] == reach


@pytest.mark.parametrize("group", sorted(pc.GPU_SHAPES))
def test_shapes_of_the_gpu_tests(lib, group):
    for (H, W), size, iou, form, reach, bands in pc.GPU_SHAPES[group]:
        got = pc.plan(lib, H, W, size, iou)
        assert got[0] == form and got[1] == reach, ((H, W), size, iou, got)
        if form == pc.TWO_LAUNCH:
            assert got[2] == bands, ((H, W), size, iou, got)


def test_sweep_shapes_are_sweep_for_the_stated_reason(lib):
    assert pc.plan(lib, 200, 24, 8, 0.1)[0] == 0 and pc.plan(lib, 200, 32, 8, 0.1)[0] == 1           # W < 32
    assert -(-2080 // 32) == 65
    assert pc.plan(lib, 40, 2080, 8, 0.1)[0] == 0 and pc.plan(lib, 40, 2048, 8, 0.1)[0] == 1         # more than 64 mask words per row


def test_banded_shape_has_a_short_last_band(lib):
    for size, iou, reach in ((8, 0.1, 6), (16, 0.001, 15)):
        assert pc.plan(lib, 181, 2048, size, iou)[:4] == (1, reach, 2, 91)
    assert 2 * 91 - 181 == 1                                                                         # the last band is one row short


def test_list_overflow_inputs_outgrow_lds(lib):
    """The three images of the list-overflow GPU test leave more undecided candidates after round 1 than the finisher's LDS list holds, each on
    its own: a condition on the inputs (restated in numpy), not a measurement of the kernel."""
    form, reach, bands, brows, cap = pc.plan(lib, 96, 256, 8, 0.1)
    assert (form, reach, bands, brows, cap) == (1, 6, 1, 96, 19144)
    p = pc.case_a4()
    left = [pc.undecided_after_round1(p[b], 8, 0.1) for b in range(3)]
    print("candidates, round-1 keepers, undecided:", left, "list_cap", cap)
    assert [c for c, _, _ in left] == [96 * 256] * 3
    assert left[0][1] == 1 and left[1][1] == 1                       # ramp: the last pixel; constant: the first
    assert left[0][2] == left[1][2] == 24535
    assert all(u > cap for _, _, u in left), (left, cap)


def test_banded_inputs_outgrow_lds_too(lib):
    """Bands together with the workspace list: every band of the banded GPU cases leaves more undecided candidates than its LDS list holds.
    The constant images fill the short last band's workspace list to within two rows of the band's own pixels — more than the rows a band of
    full height leaves it in the image's slice, the case the list layout has to get right."""
    for size, iou in ((8, 0.1), (16, 0.001)):
        _, _, bands, brows, cap = pc.plan(lib, 181, 2048, size, iou)
        p = pc.case_a5()
        for b in range(2):
            left = pc.undecided_after_round1(p[b], size, iou, rows=brows)
            print("size", size, "image", b, "undecided per band", left, "list_cap", cap)
            assert len(left) == bands and min(left) > cap, (left, cap)
    _, _, bands, brows, cap = pc.plan(lib, 181, 2048, 8, 0.1)
    p = pc.case_a6()
    for b in range(2):
        left = pc.undecided_after_round1(p[b], 8, 0.1, rows=brows)
        assert left[0] > cap and left[1] == (181 - brows) * 2048 > (brows - 2) * 2048, left


def test_ridges_outrank_their_fields():
    """The ridge inputs: every field value is below every ridge value, so a ridge pixel is decided by ridge pixels alone (a chain through every
    tile / band border), and the fields still hold exact ties."""
    for p, sl in ((pc.case_a5(), np.s_[0, :, 300:304]), (pc.case_b1(), np.s_[0, :, 10:14]), (pc.case_b2(), np.s_[0, 18:22, :])):
        r = np.zeros(p.shape, bool)
        r[sl] = True
        assert p[sl].min() >= 0.5 and p[0][~r[0]].max() < 0.5
        vals, counts = np.unique(p[0][~r[0]], return_counts=True)
        assert counts.min() > 1 and len(vals) <= 256


# (batch, H, W, cap) -> xp_box_nms_workspace_bytes, xp_extract_keypoints_workspace_bytes(batch, H, W): recorded from the library as it was before
# box NMS and keypoint extraction moved into files of their own, never computed by the code under test
WORKSPACE_BYTES = [
    ((1, 1, 32, 1), 2080, 260),
    ((2, 65, 33, 1), 40272, 280),
    ((2, 200, 24, 1), 88128, 296),                   # the sweep form
    ((3, 96, 256, 24576), 1550176, 544),
    ((2, 181, 2048, 1), 6677056, 3152),
    ((16, 480, 640, 8192), 45833216, 19456),
]


def test_workspace_sizes_are_the_recorded_ones(lib):
    """The workspace layout has one definition (nms_core.h: nms_ws_layout); callers size their buffers with these two queries and tools/nms_bench.py
    reads the finisher's diagnostics from the END of the NMS workspace, so the totals may not move."""
    for shape, nms_bytes, kp_bytes in WORKSPACE_BYTES:
        assert lib.xp_box_nms_workspace_bytes(*shape) == nms_bytes, shape
        assert lib.xp_extract_keypoints_workspace_bytes(*shape[:3]) == kp_bytes, shape


def test_plan_refuses_what_the_launcher_refuses(lib):
    import ctypes
    out = (ctypes.c_int * 5)()
    for size in (0.0, 16.5, 7.25, -1.0):
        assert lib.xp_box_nms_plan(70, 100, size, 0.1, out) != 0
        assert b"size must be a positive multiple of 0.5" in lib.xp_last_error()
    assert lib.xp_box_nms_plan(0, 100, 8.0, 0.1, out) != 0


def test_plan_query_is_declared_bound_and_never_stubbed():
    """Declared in the header, bound in _lib, and the library's own in the launch-plan driver (like the size queries): it launches nothing."""
    from tests import test_cpu_launch_plan as lp
    assert "xp_box_nms_plan" in _lib.exported_symbols() and "xp_box_nms_plan" in _lib._SIGNATURES
    assert "xp_box_nms_plan" not in lp.stubbed_entry_points()
