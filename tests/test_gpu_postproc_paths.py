"""Every path of csrc/box_nms.hip and csrc/keypoints.hip against the oracle: both forms of box NMS (tile sweeps; local maxima + finisher, every reach, bands, the
undecided list in LDS and in the workspace, the stream-ordered modes), both paths of keypoint extraction and both of descriptor sampling.

Which path a shape takes is not assumed here: tests/test_cpu_postproc_plan.py pins it with `xp_box_nms_plan`, and the tests below assert the plan
again before they run.  NMS and keypoint results are compared EXACTLY (torch.equal with oracle.xpoint_oracle / torch.nonzero)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import xpoint_oracle as xo
from tests import postproc_cases as pc
from xpoint_amd import synth

pytestmark = pytest.mark.gpu

MIN_PROB = pc.MIN_PROB


def _L():
    from xpoint_amd import _lib as L
    return L


def _nms(p, size, iou, min_prob=MIN_PROB, mode=0, keep_top_k=0):
    """xp_box_nms called directly on p (B, H, W) float32 numpy / tensor.  mode 0: synchronous; mode > 0: stream-ordered with that many sweeps /
    finisher launches.  Returns (out on the CPU, left): left is None in synchronous mode, else xp_box_nms_check's answer."""
    L = _L()
    lib = L.load()
    pd = torch.as_tensor(p).cuda().contiguous()
    B, H, W = pd.shape
    cap = H * W if keep_top_k > 0 else 1
    out = torch.full_like(pd, float("nan"))                       # every pixel must be written
    ws = torch.empty(lib.xp_box_nms_workspace_bytes(B, H, W, cap), dtype=torch.uint8, device="cuda")
    conv = ctypes.c_int(0)
    L.check(lib.xp_box_nms(L.ptr(pd), L.ptr(out), L.ptr(ws), ws.numel(), B, H, W, float(size), float(min_prob), float(iou), int(keep_top_k), cap,
                           int(mode), ctypes.byref(conv) if mode == 0 else None, L.current_stream()), "xp_box_nms")
    left = None
    if mode > 0:
        c = ctypes.c_int(-1)
        L.check(lib.xp_box_nms_check(L.ptr(ws), B, H, W, ctypes.byref(c), L.current_stream()), "xp_box_nms_check")
        left = c.value
    else:
        assert conv.value == 1
    return out.cpu(), left


def _ref(p, size, iou, min_prob=MIN_PROB, keep_top_k=0):
    return xo.box_nms(torch.as_tensor(p).unsqueeze(1), size, min_prob, iou, keep_top_k)[:, 0]


def _assert_plan(gpu_lib, group):
    for (H, W), size, iou, form, reach, bands in pc.GPU_SHAPES[group]:
        got = pc.plan(gpu_lib, H, W, size, iou)
        assert got[:2] == (form, reach) and (form == pc.SWEEP or got[2] == bands), (group, (H, W), size, iou, got)


@pytest.fixture(scope="module")
def refs():
    """Oracle results, computed once per (case, size, iou) and shared; never modified."""
    cache = {}
    cases = {"a5": pc.case_a5, "a6": pc.case_a6, "b1": pc.case_b1, "b2": pc.case_b2, "a4": pc.case_a4}

    def get(case, size, iou):
        if case not in cache:
            cache[case] = {"p": cases[case]()}
        if (size, iou) not in cache[case]:
            cache[case][(size, iou)] = _ref(cache[case]["p"], size, iou)
        return cache[case]["p"], cache[case][(size, iou)]
    return get


# ------------------------------------------------------------------------------------------------ A. two-launch form
@pytest.mark.parametrize("shape", [(1, 32), (1, 33), (65, 33), (33, 64)])
def test_two_launch_edge_geometry(gpu_lib, shape):
    """One row; a last mask word holding one column; one row more than a tile (64) and than a round band (32): (65, 33) is two tiles and three
    round bands high with one column in the second mask word.  16-level field (ties), batch 2."""
    _assert_plan(gpu_lib, "A1")
    p = pc.field("a1/%dx%d" % shape, (2,) + shape, 16)
    out, _ = _nms(p, 8, 0.1)
    assert torch.equal(out, _ref(p, 8, 0.1))
    assert int((out > 0).sum()) > 0


@pytest.mark.parametrize("size_iou,reach", pc.REACH_TABLE)
def test_two_launch_every_reach(gpu_lib, size_iou, reach):
    """Reach 6 (the compile-time instance, also from a half-integer size), 3, 2, 13, 15 (62 of the 64 mask bits; also from 15.5) and 0 (nothing
    overlaps: every candidate is kept) at (70, 100): two tiles high, four wide, the last 4 columns wide."""
    size, iou = size_iou
    assert pc.plan(gpu_lib, 70, 100, size, iou)[:3] == (pc.TWO_LAUNCH, reach, 1)
    p = pc.field("a2", (2, 70, 100), 64)
    out, _ = _nms(p, size, iou, min_prob=0.1)
    assert torch.equal(out, _ref(p, size, iou, min_prob=0.1))
    if reach == 0:
        pt = torch.from_numpy(p)
        assert torch.equal(out, torch.where(pt > 0.1, pt, torch.zeros_like(pt)))
    else:
        assert 0 < int((out > 0).sum()) < int((p > 0.1).sum())


@pytest.mark.parametrize("size,iou,reach", [(16, 0.001, 15), (1, 0.1, 0)])
def test_keep_top_k_ties_at_the_fifth_score(gpu_lib, size, iou, reach):
    assert pc.plan(gpu_lib, 70, 100, size, iou)[:2] == (pc.TWO_LAUNCH, reach)
    p = pc.field("a3", (2, 70, 100), 16)
    full = _ref(p, size, iou)
    for b in range(2):
        s = torch.sort(full[b].flatten(), descending=True).values
        assert s[4] == s[5] > 0, "the input must tie at the fifth score"          # a condition on the input, from the oracle
    ref = _ref(p, size, iou, keep_top_k=5)
    out, _ = _nms(p, size, iou, keep_top_k=5)
    assert torch.equal(out, ref)
    assert [int((out[b] > 0).sum()) for b in range(2)] == [5, 5]


def test_two_launch_list_overflow(gpu_lib, refs):
    """The undecided list of every image outgrows LDS (test_cpu_postproc_plan.py proves > 19 144 of 24 576 for each) and goes to the workspace,
    each image to its own slice; the rounds that skip compaction run.  Ramp: latest index first; constant: earliest index first, a maximal tie
    chain; 4-level field."""
    _assert_plan(gpu_lib, "A4")
    p, ref = refs("a4", 8, 0.1)
    out, _ = _nms(p, 8, 0.1)
    for b in range(3):
        assert torch.equal(out[b], ref[b]), "image %d" % b
    assert ref[0, 95, 255] > 0 and ref[1, 0, 0] > 0


@pytest.mark.parametrize("size,iou", [(8, 0.1), (16, 0.001)])
def test_two_launch_bands(gpu_lib, refs, size, iou):
    """(181, 2048): 2 bands of 91 rows, the last one row short, at reach 6 and 15.  A monotone ridge down each image (highest at the bottom,
    above every field value) is a chain of decisions that crosses the band border upwards, so the upper band's finisher cannot settle it from
    the masks as its launch found them: ONE stream-ordered finisher launch must report bands left; in every mode `left == 0` means exact."""
    _assert_plan(gpu_lib, "A5")
    p, ref = refs("a5", size, iou)
    out, _ = _nms(p, size, iou)
    assert torch.equal(out, ref)
    for mode in (1, 2, 64):
        out, left = _nms(p, size, iou, mode=mode)
        print("bands, size %g: %d finisher launch(es) leave %d band(s) undecided" % (size, mode, left))
        assert left >= 0
        if mode == 1:
            assert left > 0
        if left == 0:
            assert torch.equal(out, ref), mode


def test_two_launch_bands_full_workspace_list(gpu_lib, refs):
    """Two constant (181, 2048) images: the short last band (90 of 91 rows) has every one of its pixels undecided after round 1, so its
    workspace list (positions, then scores) is as long as it can be.  It must stay inside the image's slice of the workspace: laid out by the
    band height instead of the band's own rows, image 0's scores ran into image 1's positions (and image 1's past the area)."""
    _assert_plan(gpu_lib, "A6")
    p, ref = refs("a6", 8, 0.1)
    out, _ = _nms(p, 8, 0.1)
    assert torch.equal(out, ref)
    assert ref[0, 0, 0] > 0 and ref[1, 0, 0] > 0


# ------------------------------------------------------------------------------------------------ B. sweep form
@pytest.mark.parametrize("size,iou", [(8, 0.1), (16, 0.001)])
def test_sweep_vertical_tiles(gpu_lib, refs, size, iou):
    """(200, 24): W < 32, four tiles down the image.  The ridge down columns 10-13 crosses the three tile borders, every tile waiting for the one
    below it; at size 16 the reach (15) exceeds half the width.  16-level field: ties inside rows, the tie-break's case."""
    _assert_plan(gpu_lib, "B1")
    p, ref = refs("b1", size, iou)
    out, _ = _nms(p, size, iou)
    assert torch.equal(out, ref)


def test_sweep_horizontal_tiles(gpu_lib, refs):
    """(40, 2080): 65 mask words per row, so 65 tiles in x; the ridge along rows 18-21 (highest at the right) makes every tile wait for its
    right neighbour."""
    _assert_plan(gpu_lib, "B2")
    p, ref = refs("b2", 8, 0.1)
    out, _ = _nms(p, 8, 0.1)
    assert torch.equal(out, ref)


@pytest.mark.parametrize("size,iou", [(8, 0.1), (16, 0.001)])
def test_sweep_stream_ordered(gpu_lib, refs, size, iou):
    """Stream-ordered sweeps on the vertical-tile case.  One sweep cannot finish: it derives the states from `prob` and reads no neighbour's
    state, so a ridge pixel whose higher-priority neighbour lies in the halo (below the tile border) stays undecided, and the check must say
    so.  With 64 sweeps the check reports a count; whenever it reports 0 the output is the oracle's."""
    _assert_plan(gpu_lib, "B1")
    L = _L()
    p, ref = refs("b1", size, iou)
    out, left = _nms(p, size, iou, mode=1)
    print("sweep, size %g: 1 sweep leaves %d tile(s) undecided" % (size, left))
    assert left > 0
    out, left = _nms(p, size, iou, mode=64)
    print("sweep, size %g: 64 sweeps leave %d tile(s) undecided" % (size, left))
    assert left >= 0
    if left == 0:
        assert torch.equal(out, ref)
    with pytest.raises(L.XPointHipError, match="at most 64 async sweeps"):
        _nms(p, size, iou, mode=65)


# ------------------------------------------------------------------------------------------------ C. extract_keypoints
def _extract(p, thr, m=None, cap=None, pad_rows=0, sentinel=-7):
    """xp_extract_keypoints called directly on device tensors p (B, H, W) float32 and m (B, H, W) uint8 (views allowed: the pointers decide the
    path).  kp is pre-filled with `sentinel` and has `pad_rows` extra rows after the last image.  Returns (kp (B * cap + pad_rows, 2), counts)."""
    L = _L()
    lib = L.load()
    B, H, W = p.shape
    cap = int(cap or H * W)
    kp = torch.full((B * cap + pad_rows, 2), sentinel, dtype=torch.int32, device="cuda")
    counts = torch.full((B,), sentinel, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.xp_extract_keypoints_workspace_bytes(B, H, W), dtype=torch.uint8, device="cuda")
    L.call("xp_extract_keypoints", L.ptr(p), L.ptr(m), float(thr), L.ptr(kp), L.ptr(counts), B, H, W, cap, L.ptr(ws), ws.numel(), L.current_stream())
    return kp.cpu(), counts.cpu()


def _nonzero(p, thr, m=None):
    hit = p.cpu() > torch.tensor(thr, dtype=torch.float32)          # the threshold as the kernel gets it: rounded to float32
    if m is not None:
        hit &= m.cpu() != 0
    return [torch.nonzero(hit[b]).int() for b in range(p.shape[0])]


def _offset_view(t, off):
    """A contiguous copy of t that starts `off` elements into a larger (aligned) buffer."""
    buf = torch.zeros(t.numel() + 64, dtype=t.dtype, device=t.device)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + off * t.element_size() and buf.data_ptr() % 16 == 0
    return v


def _check_full(p, thr, m=None):
    B, H, W = p.shape
    kp, counts = _extract(p, thr, m)
    ref = _nonzero(p, thr, m)
    for b in range(B):
        assert int(counts[b]) == len(ref[b]), (b, int(counts[b]), len(ref[b]))
        rows = kp[b * H * W:(b + 1) * H * W]
        assert torch.equal(rows[:len(ref[b])], ref[b]), b
        assert bool((rows[len(ref[b]):] == -7).all()), b
    return kp, counts, ref


def test_keypoints_scalar_path_with_mask(gpu_lib):
    """H * W odd: the one-pixel-per-lane kernels, with a mask about 70 % on and values exactly equal to the threshold (not hits)."""
    shape = (3, 33, 47)
    assert (33 * 47) % 4 != 0
    thr = 0.9
    p = synth.uniform("postproc/c1/p", shape, 0, 1)
    m = synth.uniform("postproc/c1/m", shape, 0, 1) > 0.3
    plant = synth.uniform("postproc/c1/plant", shape, 0, 1) > 0.9
    p[plant] = np.float32(thr)
    m[plant] = True
    assert 0.6 < m.mean() < 0.85 and plant.sum() > 100
    pd, md = torch.from_numpy(p).cuda(), torch.from_numpy(m.astype(np.uint8)).cuda()
    _, counts, ref = _check_full(pd, thr, md)
    assert min(len(r) for r in ref) > 50
    hit = torch.zeros(shape, dtype=torch.bool)
    for b in range(3):
        hit[b][ref[b][:, 0].long(), ref[b][:, 1].long()] = True
    assert not bool(hit[torch.from_numpy(plant)].any())


@pytest.mark.parametrize("p_off,m_off", [(1, 0), (0, 1), (1, 1), (2, 2), (0, None), (1, None)])
def test_keypoints_alignment(gpu_lib, p_off, m_off):
    """H * W % 4 == 0 with a heat map starting one float (or a mask starting one byte) into a buffer: the 16-byte and 4-byte loads of the
    four-pixel kernels do not apply, and the result must be that of aligned copies."""
    shape = (2, 36, 52)
    p = torch.from_numpy(synth.uniform("postproc/c2/p", shape, 0, 1)).cuda()
    m = torch.from_numpy((synth.uniform("postproc/c2/m", shape, 0, 1) > 0.3).astype(np.uint8)).cuda() if m_off is not None else None
    kp0, c0, ref = _check_full(p, 0.8, m)
    assert min(len(r) for r in ref) > 100
    pv = _offset_view(p, p_off)
    mv = _offset_view(m, m_off) if m is not None else None
    kp1, c1, _ = _check_full(pv, 0.8, mv)
    assert torch.equal(kp0, kp1) and torch.equal(c0, c1)


@pytest.mark.parametrize("shape", [(33, 47), (32, 48)])
def test_keypoints_cap_below_count(gpu_lib, shape):
    """cap = 100 with counts (above, below, above) the cap: the list stops at cap, the count does not, and nothing is written past an image's
    rows — neither into the next image's nor after the last one's.  Scalar (33 x 47) and four-pixel (32 x 48) path."""
    H, W = shape
    cap, pad = 100, 64
    p = synth.uniform("postproc/c3/%d" % W, (3, H, W), 0, 1)
    p[1] *= (p[1] > 0.98)                                            # few hits in the middle image
    pd = torch.from_numpy(p).cuda()
    kp, counts = _extract(pd, 0.8, cap=cap, pad_rows=pad)
    ref = _nonzero(pd, 0.8)
    n = [len(r) for r in ref]
    assert n[0] > cap and 0 < n[1] < cap and n[2] > cap
    assert counts.tolist() == n
    for b in range(3):
        k = min(n[b], cap)
        assert torch.equal(kp[b * cap:b * cap + k], ref[b][:k]), b
        assert bool((kp[b * cap + k:(b + 1) * cap] == -7).all()), b
    assert bool((kp[3 * cap:] == -7).all())


@pytest.mark.parametrize("shape,nseg", [((1025, 1025), 1027), ((2052, 2048), 1026)])
def test_keypoints_more_than_1024_segments(gpu_lib, shape, nseg):
    """More segments than kp_scan_kernel has threads (two per thread): scalar path with 1 027 segments of 1 024 pixels, four-pixel path with
    1 026 of 4 096.  A few hundred hits, planted in the first and the last segment and on both sides of segment borders."""
    H, W = shape
    HW = H * W
    vec4 = HW % 4 == 0
    seg = 4096 if vec4 else 1024
    assert -(-HW // seg) == nseg > 1024
    idx = (synth.uniform("postproc/c4/%d" % W, (300,), 0, 1).astype(np.float64) * HW).astype(np.int64)
    edges = [0, 1, 5, seg - 2, seg - 1, seg, seg + 1, 2 * seg - 1, 2 * seg, 513 * seg - 1, 513 * seg, 1023 * seg - 1, 1023 * seg, 1024 * seg - 1,
             1024 * seg, 1025 * seg - 1, 1025 * seg, (nseg - 1) * seg, (nseg - 1) * seg + 1, HW - 2, HW - 1]
    idx = np.unique(np.concatenate([np.minimum(idx, HW - 1), np.array([e for e in edges if e < HW])]))
    assert idx.max() == HW - 1 and 250 <= len(idx) < 400
    flat = np.full(HW, 0.25, np.float32)
    flat[idx] = 0.75
    p = torch.from_numpy(flat.reshape(1, H, W)).cuda()
    cap = 512
    kp, counts = _extract(p, 0.5, cap=cap, pad_rows=16)
    assert int(counts[0]) == len(idx)
    want = torch.from_numpy(np.stack([idx // W, idx % W], 1).astype(np.int32))
    assert torch.equal(kp[:len(idx)], want)
    assert bool((kp[len(idx):] == -7).all())


@pytest.mark.parametrize("off", [0, 1])
def test_keypoints_every_lane_hits(gpu_lib, off):
    """(2, 64, 64) of ones: 4 096 keypoints per image in raster order (off = 1: the same through the one-pixel-per-lane kernels)."""
    p = _offset_view(torch.ones(2, 64, 64, device="cuda"), off)
    kp, counts = _extract(p, 0.5)
    assert counts.tolist() == [4096, 4096]
    r = torch.arange(4096, dtype=torch.int32)
    want = torch.stack([r // 64, r % 64], 1)
    assert torch.equal(kp[:4096], want) and torch.equal(kp[4096:], want)


# ------------------------------------------------------------------------------------------------ D. xp_sample_descriptors
def _sample(kp, counts, desc_nhwc, cap, H, W, D=None):
    """xp_sample_descriptors called directly: kp (B, cap, 2) int32, counts (B), desc (B, Hc, Wc, D) -> out (B, cap, D) pre-filled with NaN.
    D: the descriptor size passed to the call, when it is not the volume's (the refusals)."""
    L = _L()
    B, Hc, Wc, Dv = desc_nhwc.shape
    D = Dv if D is None else D
    kd = torch.as_tensor(kp, dtype=torch.int32).cuda().contiguous()
    cd = torch.as_tensor(counts, dtype=torch.int32).cuda()
    dd = desc_nhwc.cuda().contiguous()
    out = torch.full((B, cap, max(D, 1)), float("nan"), device="cuda")
    L.call("xp_sample_descriptors", L.ptr(kd), L.ptr(cd), L.ptr(dd), L.ptr(out), B, cap, Hc, Wc, D, H, W, L.current_stream())
    return out.cpu()


def _sample_f64(kp, desc_hwc, H, W):
    """float64 restatement: bilinear sampling with zeros padding at i = (k / (S / 2) - 1 + 1) * (Sc - 1) / 2 (align_corners), then x / max(|x|, 1e-12)."""
    d = desc_hwc.double().numpy()
    Hc, Wc, D = d.shape
    out = np.zeros((len(kp), D))
    for n, (ky, kx) in enumerate(np.asarray(kp, dtype=np.float64)):
        iy, ix = ky / (H * 0.5) * ((Hc - 1) / 2.0), kx / (W * 0.5) * ((Wc - 1) / 2.0)
        y0, x0 = int(np.floor(iy)), int(np.floor(ix))
        for yy, wy in ((y0, y0 + 1 - iy), (y0 + 1, iy - y0)):
            for xx, wx in ((x0, x0 + 1 - ix), (x0 + 1, ix - x0)):
                if 0 <= yy < Hc and 0 <= xx < Wc:
                    out[n] += wy * wx * d[yy, xx]
        out[n] /= max(np.sqrt((out[n] ** 2).sum()), 1e-12)
    return out


def _check_sampling(out, kp, counts, desc_nhwc, H, W, what):
    """Rows < counts[b]: within 1e-6 of the oracle, and within max(1e-6, 2 x the oracle's own error) of float64 (the factor 2: the kernel sums the
    squares of the norm in another order than the oracle); rows >= counts[b]: untouched (NaN)."""
    worst = (0.0, 0.0, 0.0)
    for b in range(desc_nhwc.shape[0]):
        n = int(counts[b])
        assert bool(torch.isnan(out[b, n:]).all()), (what, b)
        if n == 0:
            continue
        k = torch.as_tensor(kp[b][:n]).long()
        orc = xo.interpolate_descriptors(k, desc_nhwc[b].permute(2, 0, 1).contiguous(), H, W)
        f64 = _sample_f64(k.numpy(), desc_nhwc[b], H, W)
        assert bool(torch.isfinite(out[b, :n]).all()), (what, b)
        e_orc = float((out[b, :n] - orc).abs().max())
        e_f64 = float(np.abs(out[b, :n].double().numpy() - f64).max())
        o_f64 = float(np.abs(orc.double().numpy() - f64).max())
        worst = tuple(max(a, c) for a, c in zip(worst, (e_orc, e_f64, o_f64)))
        assert e_orc <= 1e-6, (what, b, e_orc)
        assert e_f64 <= max(1e-6, 2 * o_f64), (what, b, e_f64, o_f64)
    print("%s: kernel vs oracle %.3g, kernel vs float64 %.3g, oracle vs float64 %.3g" % ((what,) + worst))


@pytest.mark.parametrize("D", [16, 100, 256, 512])
@pytest.mark.parametrize("cap", [64, 60])
def test_sample_descriptors_ragged_batch(gpu_lib, cap, D):
    """batch 3 with counts (0, 5, cap): cap 64 is 16 blocks per image (the XCD-aware block order, with a ragged count), cap 60 is 15 (the plain
    order); D = 256 takes the four-channels-per-lane path, 16 / 100 / 512 the general one (D = 100: a ragged last lane group)."""
    H, W, Hc, Wc = 48, 72, 6, 9
    assert (-(-cap // 4) % 8 == 0) == (cap == 64)
    desc = torch.from_numpy(synth.uniform("postproc/d1/%d" % D, (3, Hc, Wc, D), -1, 1))
    u = synth.uniform("postproc/d1/kp/%d" % cap, (3, cap, 2), 0, 1)
    kp = np.stack([np.floor(u[..., 0] * H), np.floor(u[..., 1] * W)], -1).astype(np.int32)
    kp[:, :4] = [[0, 0], [0, W - 1], [H - 1, 0], [H - 1, W - 1]]
    counts = [0, 5, cap]
    out = _sample(kp, counts, desc, cap, H, W)
    assert out.shape == (3, cap, D)
    _check_sampling(out, kp, counts, desc, H, W, "D %d cap %d" % (D, cap))


@pytest.mark.parametrize("D", [16, 256])
def test_sample_descriptors_padding_and_degenerate_volumes(gpu_lib, D):
    """Keypoints on the far border (y = H, x = W: one side weighs nothing) and beyond it (all four taps outside: an exactly zero, finite row —
    the 1e-12 clamp), an all-zero volume (zeros, not NaN), Hc = 1 and Wc = 1."""
    L = _L()
    H, W = 48, 72
    for Hc, Wc in ((6, 9), (1, 9), (6, 1)):
        desc = torch.from_numpy(synth.uniform("postproc/d2/%d/%d/%d" % (D, Hc, Wc), (2, Hc, Wc, D), -1, 1))
        desc[1] = 0
        on = [[H, 10], [7, W], [H, W], [H, 0], [0, W], [H - 1, W - 1], [0, 0], [23, 35]]
        beyond = [[2 * H, 10], [7, 2 * W], [2 * H, 2 * W], [-H, -W]]
        kp = np.array([on + beyond] * 2, dtype=np.int32)
        cap = kp.shape[1]
        out = _sample(kp, [cap, cap], desc, cap, H, W)
        _check_sampling(out, kp, [cap, cap], desc, H, W, "D %d volume %d x %d" % (D, Hc, Wc))
        assert bool((out[1] == 0).all())                                     # all-zero volume
        if Hc > 1 and Wc > 1:
            assert bool((out[0, len(on):] == 0).all())                       # beyond the border
            assert bool((out[0, :len(on)].norm(dim=1) - 1).abs().max() < 1e-5)
    desc = torch.zeros(1, 6, 9, 513)
    with pytest.raises(L.XPointHipError, match=r"D must be in \[1,512\]"):
        _sample(np.zeros((1, 4, 2), np.int32), [4], desc, 4, H, W)
    with pytest.raises(L.XPointHipError, match=r"D must be in \[1,512\]"):
        _sample(np.zeros((1, 4, 2), np.int32), [4], desc, 4, H, W, D=0)
