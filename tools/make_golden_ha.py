"""Generate tests/golden/g24_homographic_adaptation.npz by running the REAL reference homographic adaptation
(xpoint.utils.homographic_adaptation_multispectral / homographic_adaptation, imported from the reference tree with the
harness shims of oracle/refharness, which this tool imports and does not modify).  CPU, build container only:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_ha.py

Two stand-ins are installed on top of the harness shims, both written from the documented semantics (no OpenCV / kornia here):
  * kornia 0.1.4: geometry.transform.imgwarp.dst_norm_to_dst_norm (N_dst * M * N_src^-1, N = [[2/(w-1), 0, -1], [0, 2/(h-1), -1],
    [0, 0, 1]]) and geometry.warp.homography_warper.homography_warp (grid = torch.linspace(-1, 1, .), the projective map with a plain
    division, then the REAL torch.nn.functional.grid_sample without align_corners, i.e. align_corners=False) -- so the sampling is
    pinned to torch itself;
  * cv2: warpPerspective (INTER_NEAREST) and erode (square kernel, the default border never erodes) by OpenCV's documented scheme as
    oracle/cv_restated.py restates it, and getPerspectiveTransform (the 8 x 8 solve in float64).
sample_homography is wrapped only to RECORD the matrices it returns, compute_valid_mask to record the masks, and the nearest-mode warps
(count_sample) to record the count maps.  One thread; the file is written with fixed zip timestamps, so a re-run is byte-identical.
"""
import io
import json
import os
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import cv_restated  # noqa: E402
from oracle.refharness import build_ref, stubs  # noqa: E402
from xpoint_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g24_homographic_adaptation.npz")
SEED = 2024
_count_samples = []


# ------------------------------------------------------------------------------------------------ kornia 0.1.4 stand-in
def _normal_transform_pixel(height, width):
    tr = torch.Tensor([[1.0, 0.0, -1.0], [0.0, 1.0, -1.0], [0.0, 0.0, 1.0]])
    tr[0, 0] = tr[0, 0] * 2.0 / (width - 1.0)
    tr[1, 1] = tr[1, 1] * 2.0 / (height - 1.0)
    return tr.unsqueeze(0)


def dst_norm_to_dst_norm(dst_pix_trans_src_pix, dsize_src, dsize_dst):
    src_h, src_w = dsize_src
    dst_h, dst_w = dsize_dst
    src_norm_trans_src_pix = _normal_transform_pixel(src_h, src_w).to(dst_pix_trans_src_pix)
    dst_norm_trans_dst_pix = _normal_transform_pixel(dst_h, dst_w).to(dst_pix_trans_src_pix)
    return torch.matmul(dst_norm_trans_dst_pix, torch.matmul(dst_pix_trans_src_pix, torch.inverse(src_norm_trans_src_pix)))


def homography_warp(patch_src, dst_homo_src, dsize, mode='bilinear', padding_mode='zeros'):
    h, w = dsize
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")
    m = dst_homo_src.reshape(-1, 1, 1, 9)
    X = m[..., 0] * xs + m[..., 1] * ys + m[..., 2]
    Y = m[..., 3] * xs + m[..., 4] * ys + m[..., 5]
    Z = m[..., 6] * xs + m[..., 7] * ys + m[..., 8]
    grid = torch.stack([X / Z, Y / Z], -1)
    out = torch.nn.functional.grid_sample(patch_src, grid, mode=mode, padding_mode=padding_mode, align_corners=False)
    if mode == 'nearest':
        _count_samples.append(out.clone())
    return out


# ------------------------------------------------------------------------------------------------ cv2 stand-ins
def warp_perspective(src, M, dsize, flags=0):
    assert flags == 0, "stand-in: INTER_NEAREST only"
    return cv_restated.warp_perspective_nearest(src, M, dsize[1], dsize[0])


def erode(src, kernel, iterations=1):
    kh, kw = np.asarray(kernel).shape
    assert iterations == 1 and kh == kw and kh % 2 == 1, "stand-in: one pass of an odd square kernel"
    return cv_restated.erode(src, kh // 2)


def get_perspective_transform(src, dst):
    src = np.asarray(src, dtype=np.float32).reshape(4, 2); dst = np.asarray(dst, dtype=np.float32).reshape(4, 2)
    a = np.zeros((8, 8)); b = np.zeros(8)
    for i in range(4):
        (x, y), (u, v) = src[i], dst[i]
        a[i, 0:3] = [x, y, 1.0]; a[i + 4, 3:6] = [x, y, 1.0]
        a[i, 6], a[i, 7] = -(x * u), -(y * u)
        a[i + 4, 6], a[i + 4, 7] = -(x * v), -(y * v)
        b[i], b[i + 4] = u, v
    return np.append(np.linalg.solve(a, b), 1.0).reshape(3, 3)


def install():
    stubs.install()
    cv2 = sys.modules["cv2"]
    cv2.warpPerspective = warp_perspective; cv2.erode = erode; cv2.getPerspectiveTransform = get_perspective_transform
    cv2.INTER_NEAREST = 0
    names = ["kornia", "kornia.geometry", "kornia.geometry.warp", "kornia.geometry.warp.homography_warper", "kornia.geometry.transform",
             "kornia.geometry.transform.imgwarp"]
    mods = {}
    for n in names:
        mods[n] = types.ModuleType(n); mods[n].__path__ = []; sys.modules[n] = mods[n]
    for n in names[1:]:
        parent, child = n.rsplit(".", 1)
        setattr(mods[parent], child, mods[n])
    mods["kornia.geometry.warp.homography_warper"].homography_warp = homography_warp
    mods["kornia.geometry.transform.imgwarp"].dst_norm_to_dst_norm = dst_norm_to_dst_norm
    import xpoint.utils.homographies as H
    assert H.kornia_available
    return H


# ------------------------------------------------------------------------------------------------ cases
HOM = {'translation': True, 'rotation': True, 'scaling': True, 'perspective': True, 'scaling_amplitude': 0.2,
       'perspective_amplitude_x': 0.2, 'perspective_amplitude_y': 0.2, 'patch_ratio': 0.85, 'max_angle': 1.57, 'allow_artifacts': True}


def _cfg(**kw):
    c = {'num': 6, 'aggregation': 'prod', 'weighted_window': True, 'window_size': 3, 'erosion_radius': 2, 'mask_border': True,
         'min_count': 2, 'filter_size': 0, 'homographies': dict(HOM)}
    c.update(kw)
    return c


# name -> (H, W, B, multispectral, model kind, flow, config).  Model kinds: "reduced" (64 x 96 VMamba, EMBED_DIM 32), "full" (the XPoint-EXP1
# configuration), "exact" (ExactNet: a closed-form stand-in whose GPU twin computes the same f32 values, so that the flow's own arithmetic
# is compared with the reference free of the model's forward error)
CASES = {
    "ms_window": (64, 96, 2, True, "reduced", "multi", _cfg(aggregation='window', window_size=5)),
    "sh_window_unweighted": (64, 96, 2, False, "reduced", "multi", _cfg(aggregation='window', weighted_window=False, min_count=3)),
    "ms_prod": (64, 96, 2, True, "reduced", "multi", _cfg(aggregation='prod', mask_border=False)),
    "sh_sum": (64, 96, 2, False, "reduced", "multi", _cfg(aggregation='sum', erosion_radius=0)),
    "ms_prod_filter3": (64, 96, 2, True, "reduced", "multi", _cfg(aggregation='prod', filter_size=3)),
    "sh_single": (64, 96, 2, False, "reduced", "single", _cfg(aggregation='prod', min_count=4)),
    "full480x640": (480, 640, 1, False, "full", "multi", _cfg(num=4, aggregation='window', window_size=5, erosion_radius=3, min_count=3)),
    "ex_window": (64, 96, 2, False, "exact", "multi", _cfg(aggregation='window', window_size=5)),
    "ex_window_unweighted": (61, 83, 2, False, "exact", "multi", _cfg(aggregation='window', window_size=3, weighted_window=False)),
    "ex_prod": (64, 96, 2, False, "exact", "multi", _cfg(aggregation='prod', mask_border=False)),
    "ex_sum_filter3": (64, 96, 2, False, "exact", "multi", _cfg(aggregation='sum', filter_size=3)),
    "ex_single": (61, 83, 2, False, "exact", "single", _cfg(aggregation='prod', min_count=3)),
}
FULL_NMS = 8
# stored subsets (size budget): descriptor volumes [:, ::c, ::y, ::x], and every ROWS-th row of the full-size output maps
DESC_STRIDE = {"reduced": (2, 2, 2), "full": (4, 8, 8), "exact": (1, 1, 1)}
FULL_MAP_ROWS = 8


class ExactNet:
    """prob = 0.5 image + 0.25, desc = the image at every 8th pixel: separate f32 multiply and add, reproduced exactly by the GPU tests'
    twin (tests/test_gpu_homographic_adaptation.py ExactNet)."""

    def takes_pair(self):
        return False

    def __call__(self, data):
        img = data["image"]
        return {"prob": img * 0.5 + 0.25, "desc": img[:, :, ::8, ::8].clone()}


def model_config(H, W, multispectral, full):
    cfg = synth.xpoint_exp1_config(H, W) if full else synth.xpoint_exp1_config(H, W, vssm={"EMBED_DIM": 32})
    cfg["multispectral"] = multispectral
    cfg["takes_pair"] = False
    cfg["mixed_precision"] = False
    return cfg


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            a = np.asarray(arrays[k])
            np.lib.format.write_array(buf, np.ascontiguousarray(a) if a.ndim else a, allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    torch.set_num_threads(1)
    H_mod = install()
    import xpoint.utils as ref_utils
    out = {"provenance": np.array(json.dumps({"tool": "tools/make_golden_ha.py", "torch": torch.__version__, "seed": SEED,
                                               "numpy": np.__version__}))}
    rec_h, rec_m = [], []
    orig_sample, orig_mask = H_mod.sample_homography, H_mod.compute_valid_mask

    def sample(*a, **k):
        h = orig_sample(*a, **k); rec_h.append(np.array(h)); return h

    def mask(*a, **k):
        m = orig_mask(*a, **k); rec_m.append(np.array(m)); return m
    H_mod.sample_homography, H_mod.compute_valid_mask = sample, mask
    for ci, (name, (H, W, B, ms, kind, flow, cfg)) in enumerate(CASES.items()):
        full = kind == "full"
        if kind == "exact":
            net = ExactNet()
        else:
            mcfg = model_config(H, W, ms, full)
            net = build_ref.build_reference_xpoint(mcfg, synth.make_state_dict(mcfg))
        data = synth.to_torch(synth.make_pair_batch(10 * ci, B, H, W))
        rec_h.clear(); rec_m.clear(); _count_samples.clear()
        seed = SEED + ci
        np.random.seed(seed)
        with torch.no_grad():
            if flow == "multi":
                r = H_mod.homographic_adaptation_multispectral(data, net, json.loads(json.dumps(cfg)))
                maps = {"out": r["out"]["prob"], "out_optical": r["out_optical"]["prob"], "out_thermal": r["out_thermal"]["prob"]}
            else:
                maps = {"out": H_mod.homographic_adaptation(data["optical"], net, json.loads(json.dumps(cfg)))}
        count = torch.ones((B, 1, H, W))
        for c in _count_samples:
            count += c
        p = f"{name}/"
        out[p + "config"] = np.array(json.dumps({"model": {"H": H, "W": W, "B": B, "multispectral": ms, "full": full, "kind": kind,
                                                           "pair_index": 10 * ci},
                                                 "flow": flow, "ha": cfg, "seed": seed}))
        out[p + "homographies"] = np.stack(rec_h)
        out[p + "valid_masks"] = np.stack(rec_m).astype(np.uint8)
        out[p + "count"] = count.numpy().astype(np.uint8)
        rows = FULL_MAP_ROWS if full else 1
        out[p + "map_row_stride"] = np.array(rows)
        for k, v in maps.items():
            if v is not None:
                out[p + k] = v.numpy()[:, :, ::rows]
        if flow == "multi":
            sc, sy, sx = DESC_STRIDE[kind]
            out[p + "desc_stride"] = np.array(DESC_STRIDE[kind])
            for s in ("optical", "thermal"):
                out[p + f"desc_{s}"] = r[f"desc_{s}"].numpy()[:, ::sc, ::sy, ::sx]
        if full:
            # keypoints after the reference's box_nms; the threshold is the largest of the candidates that leaves >= 50 per image
            probs = {s: maps[f"out_{s}"] for s in ("optical", "thermal")}
            for thr in (0.015, 0.01, 0.005, 0.002, 0.001, 1e-4, 1e-5, 1e-6):
                kps = {}
                for s, pr in probs.items():
                    nms = ref_utils.box_nms(pr, FULL_NMS, thr, keep_top_k=0, on_cpu=True)
                    kps[s] = torch.nonzero(nms.squeeze() > thr).numpy()
                if min(len(v) for v in kps.values()) >= 50:
                    break
            out[p + "detection_threshold"] = np.array(thr, dtype=np.float64)
            out[p + "nms"] = np.array(FULL_NMS)
            for s, v in kps.items():
                out[p + f"keypoints_{s}"] = v.astype(np.int16)
            print(f"{name}: detection_threshold {thr}, keypoints {[len(v) for v in kps.values()]}")
        print(name, "count range", int(count.min()), int(count.max()), {k: float(v.max()) for k, v in maps.items() if v is not None})
    H_mod.sample_homography, H_mod.compute_valid_mask = orig_sample, orig_mask
    write_npz(OUT, out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
