"""Non-trivial valid masks on the GPU, against the REAL reference (tests/golden/g25_masked_pairs.npz) and against plain references.

The reference applies `valid_mask` in three places: prob * mask BEFORE box_nms (predict_align_image_pair.py:195-204), `optical *= mask`
before the quantisation of the aligned image (:267-271), and nonzero((prob > thr) * mask) AFTER box_nms on the unmasked prob
(predict_keypoints.py:205-215).  Every other end-to-end fixture uses all-ones masks, where masking changes nothing; g25's pairs carry a
perspective quad / an uneven frame, a frame with a hole and isolated valid pixels, an all-zero optical mask, and holes punched on the
strongest detections (mask before vs after NMS).  Keypoint and match lists must equal the reference's except elements attributed one by one
to a near-tie inside the 1e-4 parity budget (tests/parity.py); the aligned image must be bit-equal to the oracle warp of the reference's
masked im_optical (rebuilt here and checked against the fixture's SHA-256)."""
import ctypes
import hashlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import xpoint_oracle as xo
from xpoint_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-4
THR = 0.015

# Measured on the MI355X (default split-fp16 dense engine): per g25 pair, (keypoints, keypoints differing from the reference,
# mutual-NN pairs, pairs differing) of the predict_align_image_pair flow, and (keypoints, differing) of the predict_keypoints flow.
PINS_ALIGN = {0: (6968, 0, 895, 0), 1: (7351, 0, 1003, 0), 2: (4037, 0, 0, 0), 3: (8101, 0, 1239, 0)}
PINS_KEYPOINTS = {0: (6889, 0), 1: (7292, 0), 2: (4037, 0), 3: (7987, 0)}


def _unpack(packed, H, W):
    return np.unpackbits(packed, count=H * W).reshape(H, W).astype(bool)


def _net(cfg):
    from xpoint_amd import models
    net = models.XPoint(cfg)
    net.load_state_dict(synth.make_torch_state_dict(cfg), strict=True)
    return net.to("cuda").eval()


@pytest.fixture(scope="module")
def env(gpu_lib, golden):
    """g25's four 480x640 pairs with their masks on the device, the model, the per-pair flow's results and the raw network outputs."""
    from xpoint_amd.predict import predict_align_image_pair
    g = golden("g25_masked_pairs.npz")
    n, H, W = [int(v) for v in g["meta"]]
    assert (n, H, W) == (4, 480, 640)
    mo = np.stack([_unpack(g[f"p{i}/mask_optical"], H, W) for i in range(n)])
    mt = np.stack([_unpack(g[f"p{i}/mask_thermal"], H, W) for i in range(n)])
    data_np = synth.with_masks(synth.make_pair_batch(0, n, H, W), mo, mt)
    data = synth.to_torch(data_np, "cuda")
    net = _net(synth.xpoint_exp1_config(H, W))
    with torch.no_grad():
        o, t, _ = net(data)
        raw = {"optical": o["prob"][:, 0].cpu().numpy(), "thermal": t["prob"][:, 0].cpu().numpy()}
        dvol = {"optical": o["desc_nhwc"].clone(), "thermal": t["desc_nhwc"].clone()}
        _, _, res = predict_align_image_pair(net, data, estimate_homography=True)
    return SimpleNamespace(g=g, B=n, H=H, W=W, data_np=data_np, data=data, net=net, raw=raw, dvol=dvol, res=res,
                           mask={"optical": mo, "thermal": mt})


def _im_optical(env, i):
    """The reference's masked, quantised im_optical of pair i (predict_align_image_pair.py:267-271, before GRAY2RGB), hash-checked."""
    img = env.data_np["optical"]["image"][i, 0]
    im = (np.clip(img * env.mask["optical"][i], 0.0, 1.0) * 255.0).astype(np.uint8)
    assert hashlib.sha256(im.tobytes()).digest() == env.g[f"p{i}/im_optical_sha256"].tobytes(), i
    return im


def _vs_g25(env, i, kp_m, matches, kind, lines):
    """Lists of pair i against g25.  kind "kp": predict_align_image_pair's flow (the keypoints come from prob * mask), with matches;
    "kpk": predict_keypoints' flow (NMS on the unmasked prob).  Returns (keypoints, differing, pairs, differing)."""
    from tests import parity
    from xpoint_amd import utils
    g, H, W = env.g, env.H, env.W
    n_kp = n_kpd = n_m = n_md = 0
    for spec in ("optical", "thermal"):
        ref = g[f"p{i}/{kind}_{spec}"].astype(np.int64).reshape(-1, 2)
        mine = np.asarray(kp_m[spec], dtype=np.int64).reshape(-1, 2)
        n_kp += len(ref)
        raw = env.raw[spec][i]
        if kind == "kp" and len(ref):
            assert float(np.abs(raw[ref[:, 0], ref[:, 1]] - g[f"p{i}/score_{spec}"]).max()) < TOL     # the reference's scores, to the parity bar
        assert bool(env.mask[spec][i][mine[:, 0], mine[:, 1]].all()), (i, spec, "keypoint on an invalid pixel")
        if np.array_equal(mine, ref):
            continue
        sel = raw * env.mask[spec][i] if kind == "kp" else raw
        rep, bad = parity.explain_keypoint_diff(mine, ref, sel, THR, 8, tol=TOL)
        n_kpd += len(rep)
        lines.append(parity.format_report(f"pair {i} {spec} {kind}", rep))
        assert not bad, parity.format_report(f"pair {i} {spec} {kind}: UNEXPLAINED keypoint differences", bad)
    if matches is None:
        return n_kp, n_kpd, n_m, n_md
    mine_m = np.asarray(matches, dtype=np.int64).reshape(-1, 2)
    ref_m = g[f"p{i}/matches"].astype(np.int64).reshape(-1, 2)
    n_m = len(ref_m)
    same_kp = all(np.array_equal(np.asarray(kp_m[s]).reshape(-1, 2), g[f"p{i}/kp_{s}"]) for s in ("optical", "thermal"))
    if not (same_kp and np.array_equal(mine_m, ref_m)):
        vol = {s: env.dvol[s][i] for s in ("optical", "thermal")}
        desc_of = lambda side, pts: utils.interpolate_descriptors_nhwc(torch.from_numpy(pts), vol[side], H, W).cpu().numpy()
        rep, bad = parity.explain_match_diff(kp_m["optical"], kp_m["thermal"], g[f"p{i}/kp_optical"], g[f"p{i}/kp_thermal"], mine_m, ref_m,
                                             desc_of, tol=TOL)
        n_md = len(rep)
        lines.append(parity.format_report(f"pair {i} mutual-NN pairs", rep))
        assert not bad, parity.format_report(f"pair {i}: UNEXPLAINED match differences", bad)
    return n_kp, n_kpd, n_m, n_md


def _same(a, b, warped=False):
    """Two PairPipeline.fetch() results, bit for bit."""
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        for k in ("kp_optical", "kp_thermal", "desc_optical", "desc_thermal"):
            assert torch.equal(x[k], y[k]), (i, k)
        for k in ("match_q", "match_t", "match_d"):
            assert np.array_equal(x[k], y[k]), (i, k)
        if warped:
            assert torch.equal(x["warped_optical"], y["warped_optical"]), i
            assert np.array_equal(x["H_est"], y["H_est"]), i


def _args(env, masks=True):
    d = env.data
    a = (d["optical"]["image"], d["thermal"]["image"])
    return a + ((d["optical"]["valid_mask"], d["thermal"]["valid_mask"]) if masks else ())


# ------------------------------------------------------------------------------------------------------------------------- kernels

@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 8, 1023, 1024, 2 * 480 * 640, 2 * 480 * 640 + 3])
def test_mul_mask_bit_exact(gpu_lib, n, offset):
    """xp_mul_mask (float4 path: n % 4 == 0 and 16-byte aligned buffers; scalar path otherwise) == torch's x * m.bool(), bit for bit:
    mask bytes 0 / 1 / 2 / 255 (nonzero = valid, as the reference's bool mask), NaN, +-inf, -0.0, denormals; nothing outside y[:n] written."""
    from xpoint_amd import _lib as L
    rng = np.random.default_rng(7 * n + offset)
    pad = 8
    x = (rng.standard_normal(n + pad) * 4).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -1e-40, 1.4e-45, -2.9e-39, 1.1754942e-38, -7.5, 3.0e38], np.float32)
    pos = rng.choice(n + pad, size=min(n + pad, 4 * len(special)), replace=False)
    x[pos] = np.resize(special, len(pos))
    x[offset:offset + min(n, len(special))] = special[:min(n, len(special))]
    m = rng.choice(np.array([0, 1, 2, 255], np.uint8), n + pad)
    xb, mb = torch.from_numpy(x).cuda(), torch.from_numpy(m).cuda()
    yb = torch.full((n + pad,), 1234.5, device="cuda")
    xs, ms, ys = xb[offset:offset + n], mb[offset:offset + n], yb[offset:offset + n]
    if offset == 0:                         # the caching allocator's blocks are 512-byte aligned: n % 4 == 0 takes the float4 path
        assert xs.data_ptr() % 16 == 0 and ys.data_ptr() % 16 == 0 and ms.data_ptr() % 4 == 0
    L.call("xp_mul_mask", L.ptr(xs), L.ptr(ms), L.ptr(ys), n, L.current_stream())
    if n == 0:                              # empty tensors (null data pointers) and live buffers with n = 0: a no-op, not an error
        L.call("xp_mul_mask", L.ptr(xb), L.ptr(mb), L.ptr(yb), 0, L.current_stream())
        with pytest.raises(L.XPointHipError):
            L.call("xp_mul_mask", L.ptr(xb), L.ptr(mb), L.ptr(yb), -1, L.current_stream())
    ref = xs * ms.bool()
    torch.cuda.synchronize()
    assert torch.equal(ys.view(torch.int32), ref.view(torch.int32)), int((ys.view(torch.int32) != ref.view(torch.int32)).sum())
    # the same against the host's IEEE arithmetic (NaN payloads aside): -0.0 / denormals / inf * 0 survive as they should
    got = ys.cpu().numpy()
    host = x[offset:offset + n] * (m[offset:offset + n] != 0)
    nan = np.isnan(host)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.int32), host[~nan].view(np.int32))
    untouched = torch.ones(n + pad, dtype=torch.bool)
    untouched[offset:offset + n] = False
    assert bool((yb.cpu()[untouched] == 1234.5).all())


def test_masked_warp_equals_oracle_and_unmasked_is_unchanged(gpu_lib):
    """xp_warp_perspective_masked (quantise-on-load mode with a valid mask) == the oracle warp of (clip(img * mask, 0, 1) * 255).astype(uint8)
    (predict_align_image_pair.py:267-271, 308), bit for bit; any nonzero mask byte is valid; an all-ones mask and no mask give the unmasked
    warp's bits; the mask is refused outside the quantise-on-load mode."""
    from xpoint_amd import _lib as L
    from xpoint_amd import utils
    H, W = 120, 200
    img = synth.uniform("maskedwarp/img", (H, W), -0.2, 1.2).astype(np.float32)        # outside [0, 1] too: the clip follows the mask
    rng = np.random.default_rng(3)
    d = torch.from_numpy(img).cuda()
    Ms = [np.eye(3), np.array([[0.94, 0.07, 11.3], [-0.05, 1.06, 6.9], [1.7e-4, -2.3e-4, 1.0]]),
          np.array([[1.3, 0.2, -20.0], [0.1, 0.8, 14.0], [4.0e-3, 2.5e-3, 1.0]])]
    for mask in (synth.mask_quad(H, W), synth.mask_frame_hole_islands(H, W), synth.mask_frame(H, W, 3, 5, 7, 9), np.zeros((H, W), bool)):
        q = xo.to_u8_image(img * mask)
        u8 = (mask * rng.choice(np.array([1, 2, 255], np.uint8), (H, W))).astype(np.uint8)
        for M in Ms:
            ref = xo.warp_perspective(np.repeat(q[..., None], 3, axis=2), M)
            got = utils.warp_perspective(d, M, quantise_u8=True, dst_channels=3, mask=torch.from_numpy(mask).cuda()).cpu().numpy()
            assert np.array_equal(got, ref), int((got != ref).sum())
            got = utils.warp_perspective(d, M, quantise_u8=True, mask=torch.from_numpy(u8).cuda()).cpu().numpy()
            assert np.array_equal(got, ref[..., 0])
    for M in Ms:
        plain = utils.warp_perspective(d, M, quantise_u8=True, dst_channels=3).cpu().numpy()
        ones = utils.warp_perspective(d, M, quantise_u8=True, dst_channels=3, mask=torch.ones((H, W), dtype=torch.bool, device="cuda")).cpu().numpy()
        ref = xo.warp_perspective(np.repeat(xo.to_u8_image(img)[..., None], 3, axis=2), M)
        assert np.array_equal(plain, ref) and np.array_equal(ones, ref)
    with pytest.raises(ValueError):
        utils.warp_perspective(d, Ms[1], mask=torch.ones((H, W), dtype=torch.bool, device="cuda"))          # not the quantise-on-load mode
    with pytest.raises(ValueError):
        utils.warp_perspective(d, Ms[1], quantise_u8=True, mask=torch.ones((H, W - 1), dtype=torch.bool, device="cuda"))
    o = torch.empty((H, W), dtype=torch.float32, device="cuda")
    mk = torch.ones((H, W), dtype=torch.uint8, device="cuda")
    Md = torch.eye(3, dtype=torch.float64, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    with pytest.raises(L.XPointHipError):
        L.call("xp_warp_perspective_masked", vp(d), vp(mk), vp(o), vp(Md), 1, H, W, H, W, 1, 1, 1, 0, L.current_stream())


# ------------------------------------------------------------------------------------------------------------- flows vs reference

def test_predict_align_image_pair_masked_vs_reference(env, capsys):
    """predict_align_image_pair with g25's masks against the REAL reference: keypoint lists and mutual-NN pairs identical except near-ties
    attributed one by one; the reference's scores at its keypoints to 1e-4; the all-zero optical mask gives no optical keypoints, no
    matches, H_est = identity and an empty matchesMask."""
    lines, counts = [], {}
    for i, r in enumerate(env.res):
        kp_m = {"optical": r["kp_optical"].cpu().numpy(), "thermal": r["kp_thermal"].cpu().numpy()}
        mine = np.array([[m.queryIdx, m.trainIdx] for m in r["matches"]], dtype=np.int64).reshape(-1, 2)
        counts[i] = _vs_g25(env, i, kp_m, mine, "kp", lines)
    r2 = env.res[2]
    assert len(r2["kp_optical"]) == 0 and len(r2["kp_thermal"]) > 0 and len(r2["matches"]) == 0
    assert np.array_equal(r2["H_est"], np.eye(3)) and r2["matchesMask"] == []
    with capsys.disabled():
        print("\ng25 predict_align_image_pair vs reference, per pair (keypoints, differing, mutual-NN pairs, differing):", counts)
        print("\n".join(lines))
    tot = np.array(list(counts.values())).sum(0)
    assert tot[1] <= tot[0] // 200 and tot[3] <= max(2, tot[2] // 50)           # attributed differences stay rare
    if PINS_ALIGN is not None:
        assert counts == PINS_ALIGN, counts


def test_predict_keypoints_masked_vs_reference(env, capsys):
    """predict_keypoints (NMS on the UNMASKED prob, the mask applied at extraction) with g25's masks against the reference's lists."""
    from xpoint_amd.predict import predict_keypoints
    with torch.no_grad():
        kpo, kpt = predict_keypoints(env.net, env.data)
    lines, counts = [], {}
    for i in range(env.B):
        n_kp, n_kpd, _, _ = _vs_g25(env, i, {"optical": kpo[i].cpu().numpy(), "thermal": kpt[i].cpu().numpy()}, None, "kpk", lines)
        counts[i] = (n_kp, n_kpd)
    assert len(kpo[2]) == 0
    with capsys.disabled():
        print("\ng25 predict_keypoints vs reference, per pair (keypoints, differing):", counts)
        print("\n".join(lines))
    if PINS_KEYPOINTS is not None:
        assert counts == PINS_KEYPOINTS, counts


def test_aligned_image_of_masked_pairs(env):
    """The aligned image of a masked pair: `warped_optical` of predict_align_image_pair and of PairPipeline(warp_optical=True) == the oracle
    warp (INTER_LINEAR, BORDER_CONSTANT) of the reference's masked im_optical (rebuilt, SHA-256 checked against g25) by the flow's own H_est.
    The staged images stay unmasked (the range guard re-encodes from them)."""
    from xpoint_amd.predict import PairPipeline
    for i, r in enumerate(env.res):
        im = _im_optical(env, i)
        ref = xo.warp_perspective(np.repeat(im[..., None], 3, axis=2), r["H_est"])
        got = r["warped_optical"].cpu().numpy()
        assert got.shape == ref.shape and np.array_equal(got, ref), (i, int((got != ref).any(-1).sum()), "pixels differ")
    assert not env.res[2]["warped_optical"].cpu().numpy().any()                  # all-zero mask, identity: a black image
    B, H, W = env.B, env.H, env.W
    with torch.no_grad():
        pipe = PairPipeline(env.net, B, H, W, cap=8192, estimate_homography=True, warp_optical=True)
        out = pipe.run(*_args(env)).fetch()
    assert torch.equal(pipe.images[:B], env.data["optical"]["image"]) and torch.equal(pipe.images[B:], env.data["thermal"]["image"])
    for i in range(B):
        im = _im_optical(env, i)
        got = out[i]["warped_optical"].numpy()
        ref = xo.warp_perspective(im, out[i]["H_est"])
        assert np.array_equal(got, ref), (i, int((got != ref).sum()), "pixels differ")
    assert np.array_equal(out[2]["H_est"], np.eye(3)) and len(out[2]["matchesMask"]) == 0 and not out[2]["warped_optical"].numpy().any()


@pytest.mark.parametrize("mask_kind", ["bool_host", "u8_device"])
@pytest.mark.parametrize("schedule", ["single", "alternate", "split2"])
def test_pair_pipeline_masked_vs_reference_and_per_pair_flow(env, schedule, mask_kind):
    """PairPipeline at B = 4, 480x640 with g25's masks: one stream, overlapped with alternating encoders, two encoder image groups; masks as
    host bool tensors (the dataset's dtype; runtime copies) and as device uint8 {0, 255} (one staging kernel, xp_stage_pair_batch).  Equal to
    the per-pair flow bit for bit, and to the reference with near-ties attributed."""
    from xpoint_amd.predict import PairPipeline
    B, H, W = env.B, env.H, env.W
    o, t, mo, mt = _args(env)
    if mask_kind == "bool_host":
        mo, mt = mo.cpu(), mt.cpu()
    else:
        mo, mt = mo.to(torch.uint8) * 255, mt.to(torch.uint8) * 255
    kw = dict(single={}, alternate=dict(overlap=True, alternate_encoders=True), split2=dict(overlap=True, split_encoder=2))[schedule]
    with torch.no_grad():
        pipe = PairPipeline(env.net, B, H, W, cap=8192, **kw)
        for _ in range(2):                 # overlapped: both buffer sets
            pipe.run(o, t, mo, mt)
        out = pipe.fetch()
    lines = []
    for i in range(B):
        r = env.res[i]
        assert torch.equal(out[i]["kp_optical"], r["kp_optical"].cpu()) and torch.equal(out[i]["kp_thermal"], r["kp_thermal"].cpu())
        np.testing.assert_allclose(out[i]["desc_optical"].numpy(), r["desc_optical"].cpu().numpy(), atol=1e-6)
        assert list(zip(out[i]["match_q"].tolist(), out[i]["match_t"].tolist())) == [(m.queryIdx, m.trainIdx) for m in r["matches"]]
        kp_m = {"optical": out[i]["kp_optical"].numpy(), "thermal": out[i]["kp_thermal"].numpy()}
        _vs_g25(env, i, kp_m, np.stack([out[i]["match_q"], out[i]["match_t"]], 1), "kp", lines)
    assert len(out[2]["kp_optical"]) == 0 and len(out[2]["match_q"]) == 0


# --------------------------------------------------------------------------------------------------- buffer reuse, capture, streaming

def test_masked_and_unmasked_steps_mixed(env):
    """Masked and unmasked steps alternate in one overlapped pipeline (depth 3: every buffer set sees a masked step after an unmasked one and
    the reverse): every unmasked step equals a fresh unmasked pipeline bit for bit, every masked step a fresh masked one — the aligned image
    included."""
    from xpoint_amd.predict import PairPipeline
    B, H, W = env.B, env.H, env.W
    kw = dict(cap=8192, estimate_homography=True, warp_optical=True)
    with torch.no_grad():
        ref_m = PairPipeline(env.net, B, H, W, **kw).run(*_args(env)).fetch()
        ref_u = PairPipeline(env.net, B, H, W, **kw).run(*_args(env, masks=False)).fetch()
        assert not all(torch.equal(a["kp_optical"], b["kp_optical"]) for a, b in zip(ref_m, ref_u))
        pipe = PairPipeline(env.net, B, H, W, overlap=True, alternate_encoders=3, **kw)
        assert pipe.depth == 3
        for step in range(2 * pipe.depth):
            masked = step % 2 == 0
            pipe.run(*_args(env, masks=masked))
            _same(pipe.fetch(), ref_m if masked else ref_u, warped=True)


@pytest.mark.parametrize("overlap", [False, True], ids=["one_stream", "overlapped"])
def test_capture_replay_with_masks(env, overlap):
    """A graph captured with masks replays NEW masks (other than the capture's) to the eager pipeline's results on them; a replay whose mask
    presence differs from the capture's raises ValueError (it would ignore the masks, or apply the ones staged by an earlier step)."""
    from xpoint_amd.predict import PairPipeline
    B, H, W = env.B, env.H, env.W
    o, t, mo, mt = _args(env)
    rot = [1, 2, 3, 0]
    kw = dict(cap=8192, estimate_homography=True, warp_optical=True)
    with torch.no_grad():
        ref_m = PairPipeline(env.net, B, H, W, **kw).run(o, t, mo, mt).fetch()
        ref_u = PairPipeline(env.net, B, H, W, **kw).run(o, t).fetch()
        sched = dict(overlap=True, alternate_encoders=True) if overlap else {}
        pipe = PairPipeline(env.net, B, H, W, **sched, **kw)
        replay = pipe.capture(o, t, mo[rot].contiguous(), mt[rot].contiguous())
        for _ in range(2):                  # overlapped: both buffer sets' graphs
            replay(o, t, mo, mt)
            _same(pipe.fetch(), ref_m, warped=True)
        with pytest.raises(ValueError, match="captured with valid masks"):
            replay(o, t)
        with pytest.raises(ValueError, match="both valid masks or neither"):
            replay(o, t, mo, None)
        replay(o, t, mo, mt)                # the refused calls left the pipeline usable
        _same(pipe.fetch(), ref_m, warped=True)
        pipe = PairPipeline(env.net, B, H, W, **sched, **kw)
        replay = pipe.capture(o, t)
        with pytest.raises(ValueError, match="captured without valid masks"):
            replay(o, t, mo, mt)
        replay(o, t)
        _same(pipe.fetch(), ref_u, warped=True)


def test_streaming_step_with_masks(env):
    """StreamingRegistrationStep (BASELINE config C5's step) with masks == the eager pipeline with masks; a replay without masks raises."""
    from xpoint_amd.predict import PairPipeline
    from xpoint_amd.streaming import StreamingRegistrationStep
    B, H, W = env.B, env.H, env.W
    o, t, mo, mt = _args(env)
    net_hm = _net(synth.xpoint_exp1_config(256, 256, hm_head=True))
    warm = synth.to_torch(synth.make_pair_batch(40, B, H, W), "cuda")
    with torch.no_grad():
        ref = PairPipeline(env.net, B, H, W, cap=8192).run(o, t, mo, mt).fetch()
        pipe = PairPipeline(env.net, B, H, W, cap=8192, overlap=True, alternate_encoders=True)
        sstep = StreamingRegistrationStep(pipe, net_hm, warm["optical"]["image"], warm["thermal"]["image"], mo.flip(0).contiguous(),
                                          mt.flip(0).contiguous())
        for _ in range(2):
            bufs, ev, hm_host, hm_ev = sstep(o.cpu().pin_memory(), t.cpu().pin_memory(), mo, mt)
            ev.synchronize(); hm_ev.synchronize()
            bufs = {k: v.clone() for k, v in bufs.items()}
            sstep.verify()
            assert not pipe.repaired
            for i in range(B):
                no, nt, nm = int(bufs["counts"][i]), int(bufs["counts"][B + i]), int(bufs["match_count"][i])
                assert torch.equal(bufs["kp"][i, :no].long(), ref[i]["kp_optical"]) and torch.equal(bufs["kp"][B + i, :nt].long(), ref[i]["kp_thermal"])
                assert bufs["match_q"][i, :nm].tolist() == ref[i]["match_q"].tolist() and bufs["match_t"][i, :nm].tolist() == ref[i]["match_t"].tolist()
        with pytest.raises(ValueError, match="captured with valid masks"):
            sstep(o, t)
