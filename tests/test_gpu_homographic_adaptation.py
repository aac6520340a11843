"""GPU: homographic adaptation (xpoint_amd/homographies.py, csrc/homadapt.hip) against torch's grid_sample and against the REAL reference
(tests/golden/g24_homographic_adaptation.npz, tools/make_golden_ha.py): the batched warp, the valid masks, the whole flow with the
recorded homographies, chunking, and the CLI's label export."""
import json
import os

import numpy as np
import pytest
import torch

from tests import parity
from xpoint_amd import _lib, homographies as ha, models, synth, utils

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TIE = 1e-4


def _grid(m, H, W):
    """The kernel's grid formula on the CPU: torch.linspace, (X, Y, Z) = m (gx, gy, 1) with separate f32 multiplies and adds, plain division."""
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    m = m.reshape(-1, 1, 1, 9)
    X = m[..., 0] * xs + m[..., 1] * ys + m[..., 2]
    Y = m[..., 3] * xs + m[..., 4] * ys + m[..., 5]
    Z = m[..., 6] * xs + m[..., 7] * ys + m[..., 8]
    return torch.stack([X / Z, Y / Z], -1)


def _near_tie(grid, Hs, Ws):
    """Pixels whose nearest-mode source coordinate lies within TIE px of a rounding tie."""
    g = grid.double()
    ix = ((g[..., 0] + 1) * Ws - 1) / 2
    iy = ((g[..., 1] + 1) * Hs - 1) / 2
    return ((ix - ix.floor() - 0.5).abs() < TIE) | ((iy - iy.floor() - 0.5).abs() < TIE)


def _warp(src, mats, Hd, Wd, mode, padding):
    n_src, Hs, Ws = src.shape[0], src.shape[2], src.shape[3]
    n_dst = n_src * mats.shape[0]
    s = src.to(DEV).contiguous(); m = mats.to(DEV).contiguous()
    dst = torch.full((n_dst, 1, Hd, Wd), float("nan"), device=DEV)
    _lib.call("xp_ha_warp", _lib.ptr(s), _lib.ptr(dst), _lib.ptr(m), n_src, n_dst, Hs, Ws, Hd, Wd, mode, padding, _lib.current_stream())
    torch.cuda.synchronize()
    return dst.cpu()


def _hom(kind, H, W):
    if kind == "identity":
        return np.eye(3)
    if kind == "shift":
        return np.array([[1, 0, 7.25], [0, 1, -3.5], [0, 0, 1.0]])
    if kind == "rot180":
        return np.array([[-1, 0, W - 1.0], [0, -1, H - 1.0], [0, 0, 1.0]])
    if kind == "perspective":
        return ha.get_perspective_transform([[0, 0], [0, H], [W, H], [W, 0]], [[0.3 * W, 0.1 * H], [0, H], [W, 0.8 * H], [0.9 * W, 0.2 * H]])
    if kind == "outside":
        return np.array([[1.0, 0.1, 3.0 * W], [0.0, 1.0, -2.0 * H], [0.0, 1e-3, 1.0]])
    np.random.seed(int(kind[len("sampled"):]))
    return ha.sample_homography(np.array([H, W]), **ha.homography_adaptation_default_config["homographies"])


@pytest.mark.parametrize("kinds,H,W,n_src", [
    (["identity"], 64, 96, 1), (["shift"], 64, 96, 1), (["rot180"], 64, 96, 1), (["perspective"], 64, 96, 1),
    (["outside"], 64, 96, 1), (["perspective", "shift"], 37, 53, 1), (["sampled0"], 480, 640, 1),
    (["sampled1", "sampled2", "rot180", "perspective"], 61, 83, 4)])
def test_warp_kernel_vs_torch_grid_sample(gpu_lib, kinds, H, W, n_src):
    """kernel (a) against CPU grid_sample fed the kernel's grid: bilinear (zeros, reflection) to 2e-6, nearest identical away from
    rounding ties (and those differences <= 0.1 % of the pixels).  The (w - 1) normalisation puts whole rows / columns of the identity
    exactly on ties, so ties themselves are common; differences at them are not.  The last case is a 2B * K batch (n_src = 2B = 4 images, K = 4 matrices)."""
    torch.manual_seed(0)
    src = torch.rand(n_src, 1, H, W)
    mats = torch.stack([ha.sampling_matrix(torch.from_numpy(_hom(k, H, W).astype(np.float32)), H, W) for k in kinds])
    grid = _grid(mats, H, W).repeat_interleave(n_src, 0)                      # dst image i: matrix i // n_src, source i % n_src
    srcs = src.repeat(len(kinds), 1, 1, 1)
    for padding, pname in ((0, "zeros"), (1, "reflection")):
        got = _warp(src, mats, H, W, 1, padding)
        ref = torch.nn.functional.grid_sample(srcs, grid, mode="bilinear", padding_mode=pname, align_corners=False)
        assert float((got - ref).abs().max()) <= 2e-6, (kinds, pname, float((got - ref).abs().max()))
    got = _warp(src, mats, H, W, 0, 0)
    ref = torch.nn.functional.grid_sample(srcs, grid, mode="nearest", padding_mode="zeros", align_corners=False)
    tie = _near_tie(grid, H, W).unsqueeze(1)
    diff = got != ref
    assert int((diff & ~tie).sum()) == 0, (kinds, int((diff & ~tie).sum()))
    assert float(diff.float().mean()) <= 1e-3, (kinds, float(diff.float().mean()))          # differences at ties: at most 0.1 %


def _cases(g):
    return sorted({k.split("/")[0] for k in g.files if "/" in k})


def test_valid_masks_equal_the_reference_bit_for_bit(gpu_lib, golden):
    g = golden("g24_homographic_adaptation.npz")
    for case in _cases(g):
        c = json.loads(str(g[f"{case}/config"]))
        H, W = c["model"]["H"], c["model"]["W"]
        hs = torch.from_numpy(g[f"{case}/homographies"]).to(DEV).contiguous()
        K = hs.shape[0]
        mask = torch.empty((K, H, W), dtype=torch.uint8, device=DEV); tmp = torch.empty_like(mask)
        _lib.call("xp_ha_valid_mask", _lib.ptr(hs), _lib.ptr(mask), _lib.ptr(tmp), K, H, W, c["ha"]["erosion_radius"], int(c["ha"]["mask_border"]),
                  _lib.current_stream())
        ref = g[f"{case}/valid_masks"]
        got = mask.cpu().numpy()
        assert np.array_equal(got, ref), (case, int((got != ref).sum()))


_NETS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """The models (and their device workspaces) are shared by this module's tests and released after them."""
    yield
    _NETS.clear()
    torch.cuda.empty_cache()


TOL = 1e-4          # the model's bound on every forward value against the reference (tests/test_gpu_model.py)


class ExactNet:
    """GPU twin of tools/make_golden_ha.py's ExactNet: prob = 0.5 image + 0.25 (separate f32 multiply and add), desc = the image at every
    8th pixel.  With it the flow's own arithmetic meets the reference without the model's forward error in between."""

    def forward_raw(self, images, want_prob=True, want_desc=True, is_optical=None, **kw):
        x = images[:, 0]
        return {"prob": x * 0.5 + 0.25, "desc_nhwc": x[:, ::8, ::8].unsqueeze(-1).contiguous() if want_desc else None}

    @staticmethod
    def _nchw(t):
        return t.permute(0, 3, 1, 2).contiguous()


def _net(c):
    if c.get("kind") == "exact":
        return ExactNet()
    key = (c["H"], c["W"], c["multispectral"], c["full"])
    if key not in _NETS:
        cfg = synth.xpoint_exp1_config(c["H"], c["W"]) if c["full"] else synth.xpoint_exp1_config(c["H"], c["W"], vssm={"EMBED_DIM": 32})
        cfg["multispectral"] = c["multispectral"]; cfg["takes_pair"] = False; cfg["mixed_precision"] = False
        net = models.XPoint(cfg)
        net.load_state_dict(synth.make_torch_state_dict(cfg), strict=True)
        _NETS[key] = net.to(DEV).eval()
    return _NETS[key]


def _run_case(g, case, chunk=None):
    c = json.loads(str(g[f"{case}/config"]))
    m = c["model"]
    net = _net(m)
    data = synth.to_torch(synth.make_pair_batch(m["pair_index"], m["B"], m["H"], m["W"]), DEV)
    hs = list(g[f"{case}/homographies"])
    with torch.no_grad():
        if c["flow"] == "multi":
            r = utils.homographic_adaptation_multispectral(data, net, c["ha"], homographies=hs, chunk=chunk, return_count=True)
            maps = {"out": r["out"]["prob"], "out_optical": r["out_optical"]["prob"], "out_thermal": r["out_thermal"]["prob"]}
            maps.update(desc_optical=r["desc_optical"], desc_thermal=r["desc_thermal"])
            count = r["count"]
        else:
            out, count = utils.homographic_adaptation(data["optical"], net, c["ha"], homographies=hs, chunk=chunk, return_count=True)
            maps = {"out": out}
    torch.cuda.synchronize()
    return c, {k: v for k, v in maps.items() if v is not None}, count


def _tie_pixels(g, case, c):
    """Output pixels where any view's nearest-mode mask coordinate lies within TIE px of a rounding tie (count may differ there)."""
    H, W = c["model"]["H"], c["model"]["W"]
    tie = torch.zeros(H, W, dtype=torch.bool)
    for h in g[f"{case}/homographies"]:
        m = ha.sampling_matrix(torch.inverse(torch.from_numpy(h.astype(np.float32))), H, W)
        tie |= _near_tie(_grid(m[None], H, W), H, W)[0]
    return tie.numpy()


@pytest.mark.parametrize("case", ["ms_window", "sh_window_unweighted", "ms_prod", "sh_sum", "ms_prod_filter3", "sh_single", "full480x640",
                                  "ex_window", "ex_window_unweighted", "ex_prod", "ex_sum_filter3", "ex_single"])
def test_flow_vs_reference(gpu_lib, golden, case):
    g = golden("g24_homographic_adaptation.npz")
    c, maps, count = _run_case(g, case)
    cnt = count.cpu().numpy()
    ref_cnt = g[f"{case}/count"].astype(np.float32)
    tie = _tie_pixels(g, case, c)[None, None]
    diff = cnt != ref_cnt
    assert not (diff & ~tie).any(), (case, int((diff & ~tie).sum()))
    assert float(diff.mean()) <= 1e-3, (case, float(diff.mean()))
    rows = int(g[f"{case}/map_row_stride"])
    same = ~diff[:, :, ::rows]
    exact = c["model"].get("kind") == "exact"
    agg, ws = c["ha"]["aggregation"], c["ha"].get("window_size", 1)
    for k, v in maps.items():
        ref = g[f"{case}/{k}"]
        got = v.cpu().numpy()
        if k.startswith("desc"):
            sc, sy, sx = (int(t) for t in g[f"{case}/desc_stride"])
            got = got[:, ::sc, ::sy, ::sx]
            assert got.shape == ref.shape and float(np.abs(got - ref).max()) <= TOL, (case, k, float(np.abs(got - ref).max()))
            continue
        got = got[:, :, ::rows]
        assert got.shape == ref.shape, (case, k)
        m = np.broadcast_to(same, got.shape)
        if exact:
            # the flow's arithmetic against the reference's: the issue's bound
            err, bound = float(np.abs(got - ref)[m].max()), 1e-4 * float(np.abs(ref).max())
        elif c["flow"] == "multi" and agg == "prod":
            # with the model, every forward value is within TOL of the reference's; prod's output is sqrt(mean(o t)), whose sqrt multiplies
            # an error of o t by 1 / (2 sqrt(o t)) where one spectrum is near 0: compare the mean itself, |d(o t)| <= TOL (o + t) + TOL^2
            err, bound = float(np.abs(got.astype(np.float64) ** 2 - ref.astype(np.float64) ** 2)[m].max()), 2 * TOL + TOL ** 2
        elif c["flow"] == "multi" and agg == "window":
            # f = (sum of the ws x ws window of t) * o: |df| <= TOL (sum t + ws^2 o) + ws^2 TOL^2 <= 2 ws^2 TOL + ws^2 TOL^2 (probabilities <= 1)
            err, bound = float(np.abs(got - ref)[m].max()), 2 * ws * ws * TOL + ws * ws * TOL ** 2
        else:
            # single spectrum / sum: weighted means of values within TOL
            err, bound = float(np.abs(got - ref)[m].max()), TOL
        assert err <= bound, (case, k, err, bound, float(np.abs(ref).max()))
    if c["model"]["full"]:
        thr, nms = float(g[f"{case}/detection_threshold"]), int(g[f"{case}/nms"])
        for s in ("optical", "thermal"):
            p = maps[f"out_{s}"]
            kp = torch.nonzero(utils.box_nms(p, nms, thr, keep_top_k=0)[0, 0] > thr).cpu().numpy()
            rep, bad = parity.explain_keypoint_diff(kp, g[f"{case}/keypoints_{s}"], p[0, 0].cpu().numpy(), thr, nms, tol=1e-4)
            print(parity.format_report(f"{case} {s} keypoints vs reference", rep))
            assert not bad, parity.format_report(f"{case} {s}", bad)


@pytest.mark.parametrize("case", ["ms_window", "ms_prod_filter3", "sh_single", "ex_window"])
def test_chunking_is_bit_identical(gpu_lib, golden, case):
    g = golden("g24_homographic_adaptation.npz")
    num = json.loads(str(g[f"{case}/config"]))["ha"]["num"]
    base = None
    for chunk in (1, 2, num - 1, None):
        _, maps, count = _run_case(g, case, chunk)
        res = {k: v.cpu() for k, v in maps.items()}
        res["count"] = count.cpu()
        if base is None:
            base = res
            continue
        for k in base:
            assert torch.equal(res[k], base[k]), (case, chunk, k)


@pytest.mark.parametrize("gemm_mode", ["x3", "f32", "amp16f"])
@pytest.mark.parametrize("case", ["ms_window", "sh_single"])
def test_chunking_is_bit_identical_every_class(gpu_lib, golden, case, gemm_mode):
    """test_chunking_is_bit_identical's recipe in the split-bf16, exact-f32 and half-storage classes: the views go through the forward `chunk` at a
    time, so the aggregated maps rest on the model's batch invariance in the class it runs."""
    g = golden("g24_homographic_adaptation.npz")
    c = json.loads(str(g[f"{case}/config"]))
    net = _net(c["model"])
    assert isinstance(net, models.XPoint)
    num = c["ha"]["num"]
    prev = net.gemm_mode                     # the nets are shared with the other tests of this module
    try:
        net.gemm_mode = gemm_mode
        base = None
        for chunk in (1, 2, num - 1, None):
            _, maps, count = _run_case(g, case, chunk)
            assert net.effective_gemm_mode() == gemm_mode
            res = {k: v.cpu() for k, v in maps.items()}
            res["count"] = count.cpu()
            if base is None:
                base = res
                continue
            for k in base:
                assert torch.equal(res[k], base[k]), (case, gemm_mode, chunk, k)
    finally:
        net.gemm_mode = prev


def test_cli_export_equals_the_library_call(gpu_lib, tmp_path):
    from PIL import Image
    from xpoint_amd import cli
    import yaml
    H, W, n = 64, 96, 3
    for spec in ("optical", "thermal"):
        os.makedirs(tmp_path / "data" / spec)
        for i in range(n):
            img = synth.make_image(40 + i, spec, H, W)[0]
            Image.fromarray((img * 255).astype(np.uint8)).save(tmp_path / "data" / spec / f"p{i}.png")
    mcfg = synth.xpoint_exp1_config(H, W, vssm={"EMBED_DIM": 32})
    mdir = tmp_path / "model"; os.makedirs(mdir)
    yaml.safe_dump({"model": mcfg}, open(mdir / "params.yaml", "w"))
    torch.save(synth.make_torch_state_dict(mcfg), mdir / "w.model")
    ha_cfg = {"num": 5, "aggregation": "window", "weighted_window": True, "window_size": 5, "erosion_radius": 3, "mask_border": True,
              "min_count": 2, "filter_size": 0,
              "homographies": {"translation": True, "rotation": True, "scaling": True, "perspective": True, "scaling_amplitude": 0.2,
                               "perspective_amplitude_x": 0.2, "perspective_amplitude_y": 0.2, "patch_ratio": 0.85, "max_angle": 1.57,
                               "allow_artifacts": True}}
    pred = {"allow_gpu": True, "batchsize": 1, "detection_threshold": 0.015, "nms": 8, "cpu_nms": True, "topk": 0, "homographic_adaptation": ha_cfg}
    cfg_path = tmp_path / "export.yaml"
    yaml.safe_dump({"dataset": {"type": "ImagePairDataset", "foldername": str(tmp_path / "data"), "single_image": False,
                                "augmentation": {"photometric": {"enable": False}, "homographic": {"enable": False}}},
                    "prediction": pred}, open(cfg_path, "w"))
    out = tmp_path / "labels" / "labels.npz"
    cli.main(["export", "-y", str(cfg_path), "-m", str(mdir), "-v", "w", "-o", str(out), "--chunk", "2"])
    got = np.load(out)
    assert sorted(got.files) == sorted(f"p{i}.png/keypoints_{s}" for i in range(n) for s in ("optical", "thermal"))
    # the same flow through the library: seed 0, the samples in order, box_nms, threshold
    from xpoint_amd import datasets
    ds = datasets.ImagePairDataset({"foldername": str(tmp_path / "data")})
    cfg = dict(mcfg); cfg["takes_pair"] = False
    cfg["homography_regression_head"] = dict(cfg["homography_regression_head"], check=False)
    net = models.XPoint(cfg); net.load_state_dict(synth.make_torch_state_dict(mcfg), strict=False); net.to(DEV).eval()
    np.random.seed(0)
    total = 0
    with torch.no_grad():
        for i in range(n):
            batch = ds.load_batch([i], DEV)
            r = utils.homographic_adaptation_multispectral(batch, net, ha_cfg)
            for s in ("optical", "thermal"):
                p = utils.box_nms(r[f"out_{s}"]["prob"], 8, 0.015, keep_top_k=0)
                kp = torch.nonzero(p[0, 0] > 0.015).cpu().numpy()
                assert np.array_equal(got[f"p{i}.png/keypoints_{s}"], kp), (i, s)
                total += len(kp)
    assert total > 0
