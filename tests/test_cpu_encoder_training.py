"""CPU: the float64 restatement of the whole VMamba encoder (tests/encoder_f64.py) pinned against the real reference's results
(tests/golden/g33_encoder_training.npz; the reference's encoder runs as a float64 module there, tools/make_golden_encoder_training.py) at 1e-5 of each
tensor's scale — the bar of tests/test_cpu_vss_training.py — and by gradcheck of its strided layers; and the host side of
xpoint_amd.training.VSSEncoder: the reference's names, shapes and order, the from_model / load_state_dict round trip, the refusals that need no
device, the block-indexed drop-path draws, the new exports and the argument-error texts of the new entry points.

The reference's scans run in float32 inside the float64 module, so a tensor behind four blocks could miss 1e-5 through the reference's own rounding;
measured, none does: the largest disagreement over all 69 arrays of case S is 5.0e-7 of the tensor's scale (grad/encoder.layers.1.blocks.0.op.A_logs),
so every tensor keeps the 1e-5 bar and no widened bar is in use."""
import ctypes

import numpy as np
import pytest
import torch

from tests import encoder_f64 as En

TOL = 1e-5


def _close(got, ref, what, tol=TOL):
    got, ref = torch.as_tensor(np.asarray(got)).double(), torch.as_tensor(np.asarray(ref)).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, sc = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: err / scale = {err / max(sc, 1e-30):.3e}")
    assert err <= tol * max(sc, 1e-30), (what, err, sc)
    return err / max(sc, 1e-30)


def test_restatement_matches_reference():
    golden = En.golden()
    ref = En.case_reference("S")
    keys = list(golden.files)
    names = En.encoder_keys("S")
    want = [k for k in names if ".patch_embed." in "." + k or ".downsample." in k or ".layers.0.blocks.0." in k
            or k.endswith(("norm.weight", "norm.bias", "norm2.weight", "norm2.bias", "op.A_logs", "op.Ds", "op.dt_projs_weight", "op.dt_projs_bias"))]
    assert sorted(keys) == sorted(["out"] + ["grad/" + k for k in want]) and len(keys) == 69
    worst = ("", 0.0)
    for k in keys:
        g = golden[k]
        assert float(np.abs(g).max()) > 0.0, k
        e = _close(ref[k][:g.shape[0]], g, f"S/{k}")          # the largest gradient is stored as its leading output channels
        worst = max(worst, (k, e), key=lambda t: t[1])
    print(f"largest disagreement: {worst[0]} {worst[1]:.3e}")


def test_strided_layers_gradcheck():
    """the restatement's stem and stride-2 convolution + LayerNorm at tiny sizes, odd and even, against finite differences"""
    u = lambda n, s, lo=-0.5, hi=0.5: torch.from_numpy(En.synth.uniform("enc/tiny/" + n, s, lo, hi)).double().requires_grad_(True)          # noqa: E731
    for H, W in ((4, 6), (5, 3)):
        img = torch.from_numpy(En.synth.uniform(f"enc/tiny/img{H}", (2, 1, H, W), 0.0, 1.0)).double()
        args = (u("sw", (4, 3, 3, 3)), u("sb", (4,)), u("slw", (4,), 0.8, 1.2), u("slb", (4,), -0.1, 0.1))
        assert torch.autograd.gradcheck(lambda *a: En.stem64(img, *a), args, eps=1e-6, atol=1e-7, rtol=1e-5)
        args = (u(f"x{H}", (2, H, W, 4), -1.0, 1.0), u("cw", (8, 4, 3, 3)), u("cb", (8,)), u("clw", (8,), 0.8, 1.2), u("clb", (8,), -0.1, 0.1))
        assert torch.autograd.gradcheck(En.conv_s2_ln64, args, eps=1e-6, atol=1e-7, rtol=1e-5)
    x = u("d2s", (1, 2, 3, 32), -1.0, 1.0)
    assert torch.autograd.gradcheck(lambda t: En.depth_to_space_ref(t.permute(0, 3, 1, 2), 4), (x,), eps=1e-6, atol=1e-7)


def test_depth_to_space_view_is_the_references():
    from xpoint_amd.training.encoder import _depth_to_space4
    x = torch.arange(2 * 3 * 5 * 32, dtype=torch.float32).view(2, 3, 5, 32)
    assert torch.equal(_depth_to_space4(x), En.depth_to_space_ref(x.permute(0, 3, 1, 2), 4).permute(0, 2, 3, 1))


def test_encoder_host_side():
    from xpoint_amd import models, synth, training
    for case in En.CASES:
        E, depths, _ = En.CASES[case]
        cfg = En.model_config(case)
        want = [(k, tuple(shape)) for k, (shape, _) in models.XPoint(cfg).expected_keys().items() if k.startswith("encoder.")]
        enc = training.VSSEncoder(E, depths)
        assert [(k, tuple(v.shape)) for k, v in enc.state_dict().items()] == want          # the reference's names and shapes, in its order
        assert [k for k, _ in enc.named_parameters()] == [k for k, _ in want] and len(want) == 20 + 18 * sum(depths)
    # from_model / load_state_dict round trip
    cfg = En.model_config("D")
    net = models.XPoint(cfg)
    net.load_state_dict(synth.make_torch_state_dict(cfg))
    enc = training.VSSEncoder.from_model(net)
    assert enc.embed_dim == 32 and enc.depths == [2, 1, 1, 1] and enc.prefix == "encoder."
    assert enc.rates == pytest.approx(training.drop_path_rates([2, 1, 1, 1], 0.2)) and enc.rates[0] == 0.0
    sd = net.state_dict()
    for k, v in enc.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with torch.no_grad():
        enc.t("patch_embed.0.weight").add_(1.0)
        enc.t("layers.2.downsample.3.bias").add_(1.0)
    res = net.load_state_dict(enc.state_dict(), strict=False)
    assert list(res.unexpected_keys) == [] and len(res.missing_keys) == len(sd) - len(enc.state_dict())
    assert torch.equal(net.state_dict()["encoder.patch_embed.0.weight"], enc.t("patch_embed.0.weight").detach())
    assert torch.equal(net.state_dict()["encoder.layers.2.downsample.3.bias"], enc.t("layers.2.downsample.3.bias").detach())
    with pytest.raises(RuntimeError, match="holds no"):
        training.VSSEncoder.from_model(net, encoder="encoder_thermal.")
    ms = training.VSSEncoder(32, [1, 1, 1, 1], encoder="encoder_optical.")
    assert next(iter(ms.state_dict())) == "encoder_optical.patch_embed.0.weight"
    for name in ("VSSEncoder", "conv3x3_s2_wgrad", "conv3x3_s2_dgrad", "conv3x3_s2_fwd", "stem_conv", "stem_conv_wgrad"):
        assert name in training.__all__ and hasattr(training, name), name


def test_refusals_without_a_device():
    from xpoint_amd import _lib, training
    with pytest.raises(ValueError, match="encoder must be"):
        training.VSSEncoder(32, [1, 1, 1, 1], encoder="backbone.")
    with pytest.raises(ValueError, match="multiple of 8"):
        training.VSSEncoder(36, [1, 1, 1, 1])
    with pytest.raises(ValueError, match="4 stages"):
        training.VSSEncoder(32, [1, 1, 1])
    with pytest.raises(ValueError):
        training.VSSEncoder(32, [1, 1, 1, 1], drop_path_rate=1.0)
    enc = training.VSSEncoder(32, [1, 1, 1, 1])
    for mode in (enc.train, enc.eval):
        mode()
        with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
            enc(torch.zeros(1, 1, 32, 32))
    for call in (lambda: training.conv3x3_s2_wgrad(torch.zeros(1, 4, 4, 8), torch.zeros(1, 2, 2, 8)),
                 lambda: training.conv3x3_s2_dgrad(torch.zeros(1, 2, 2, 8), torch.zeros(8, 3, 3, 4), (4, 4)),
                 lambda: training.conv3x3_s2_fwd(torch.zeros(1, 4, 4, 8), torch.zeros(8, 3, 3, 8)),
                 lambda: training.stem_conv(torch.zeros(1, 1, 4, 4), torch.zeros(9, 16), torch.zeros(16)),
                 lambda: training.stem_conv_wgrad(torch.zeros(1, 1, 4, 4), torch.zeros(1, 2, 2, 16))):
        with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
            call()


def test_shape_refusals_of_the_forward():
    """H = 48 and a 3-channel image are refused before the device is looked at, with the inference model's messages (csrc/model.cpp,
    models.XPoint._forward_raw)"""
    from xpoint_amd import training
    enc = training.VSSEncoder(32, [1, 1, 1, 1])
    with pytest.raises(ValueError, match=r"H and W must be multiples of 32 for the VMamba encoder \(got 48x32\)"):
        enc(torch.zeros(1, 1, 48, 32))
    with pytest.raises(RuntimeError, match=r"image must be \(B,1,H,W\)"):
        enc(torch.zeros(1, 3, 32, 32))
    with pytest.raises(TypeError, match="float32"):
        enc(torch.zeros(1, 1, 32, 32, dtype=torch.float64))


def test_drop_path_draws_are_keyed_by_block():
    from xpoint_amd.training.encoder import drop_path_draws
    a = drop_path_draws(0.5, 7, range(16), 0, 3)
    assert a == drop_path_draws(0.5, 7, list(range(16))[::-1], 0, 3)[::-1] and set(a) == {0.0, 2.0}          # by sample id, not by position
    others = [drop_path_draws(0.5, 7, range(16), br, blk) for br in (0, 1) for blk in range(6) if (br, blk) != (0, 3)]
    assert all(a != o for o in others) and len({tuple(o) for o in others}) == len(others)
    assert a != drop_path_draws(0.5, 8, range(16), 0, 3)
    assert drop_path_draws(0.25, 1, range(64), 1, 0).count(0.0) in range(4, 30)


def test_new_exports_are_bound():
    from xpoint_amd import _lib
    names = set(_lib._SIGNATURES) | set(_lib._SIZE_QUERIES)
    for n in ("xp_conv3x3_s2_wgrad_h2", "xp_conv3x3_s2_dgrad_h2", "xp_conv3x3_s2_dgrad_h2_workspace_bytes", "xp_stem_conv", "xp_stem_conv_wgrad",
              "xp_stem_conv_wgrad_workspace_bytes"):
        assert n in names and n in _lib.exported_symbols(), n
    lib = _lib.load()
    assert lib.xp_version() == 100
    assert lib.xp_conv3x3_s2_dgrad_h2_workspace_bytes(0, 4, 4, 8, 8) == 0
    # head 4352, the rearranged weight (Ci, 32 + 64 + 64 + 128 columns at Co = 32), its split, the scaled copy of dy: each rounded up to 256 bytes
    want = 4352 + 8 * 288 * 4 + (lib.xp_split_weights_h2_bytes(8, 288) + 255) // 256 * 256 + (2 * 3 * 4 * 32 * 4 + 255) // 256 * 256
    assert lib.xp_conv3x3_s2_dgrad_h2_workspace_bytes(2, 5, 7, 8, 32) == want
    assert lib.xp_stem_conv_wgrad_workspace_bytes(48) == 64 * 9 * 48 * 8 and lib.xp_stem_conv_wgrad_workspace_bytes(0) == 0


_P = ctypes.c_void_p(256)          # a placeholder pointer, aligned: never dereferenced


def test_new_entry_argument_error_texts():
    """Every argument check of the new entry points that fails before a launch: XP_ERR_ARG and the text.  The pointers are placeholders, so the test
    does not run where a GPU is visible (the texts do not depend on the device)."""
    from xpoint_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("placeholder pointers: only where no launch can happen")
    lib = _lib.load()
    sz = ctypes.c_size_t
    cases = [
        ("xp_conv3x3_s2_wgrad_h2", (None, _P, _P, 1, 4, 4, 8, 8, None, _P, sz(1 << 20), None), "null pointer"),
        ("xp_conv3x3_s2_wgrad_h2", (_P, _P, _P, 1, 0, 4, 8, 8, None, _P, sz(1 << 20), None), "bad shape batch=1 H=0 W=4 Ci=8 Co=8"),
        ("xp_conv3x3_s2_wgrad_h2", (_P, _P, _P, 1, 4, 4, 8, 8, None, _P, sz(64), None),
         f"workspace of {lib.xp_gemm_tn_h2_workspace_bytes(4, 8, 72)} bytes, 256-byte aligned, needed (got 64)"),
        ("xp_conv3x3_s2_dgrad_h2", (_P, None, _P, 1, 4, 4, 8, 8, None, _P, sz(1 << 20), None), "null pointer"),
        ("xp_conv3x3_s2_dgrad_h2", (_P, _P, _P, 0, 4, 4, 8, 8, None, _P, sz(1 << 20), None), "bad shape batch=0 H=4 W=4 Ci=8 Co=8"),
        ("xp_conv3x3_s2_dgrad_h2", (_P, _P, _P, 1, 4, 4, 8, 6, None, _P, sz(1 << 20), None),
         "Co must be a multiple of 4 (got 6): the engine loads dy in 4-element channel groups"),
        ("xp_conv3x3_s2_dgrad_h2", (ctypes.c_void_p(260), _P, _P, 1, 4, 4, 8, 8, None, _P, sz(1 << 20), None), "dy must be 16-byte aligned"),
        ("xp_conv3x3_s2_dgrad_h2", (_P, _P, _P, 1, 4, 4, 8, 8, None, _P, sz(64), None),
         f"workspace of {lib.xp_conv3x3_s2_dgrad_h2_workspace_bytes(1, 4, 4, 8, 8)} bytes, 256-byte aligned, needed (got 64)"),
        ("xp_stem_conv", (_P, _P, None, _P, 1, 4, 4, 16, None), "null pointer"),
        ("xp_stem_conv", (_P, _P, _P, _P, 1, 4, 0, 16, None), "bad shape batch=1 H=4 W=0"),
        ("xp_stem_conv", (_P, _P, _P, _P, 1, 4, 4, 24, None), "Co must be 48 or 16 (EMBED_DIM 96 / 32), got 24"),
        ("xp_stem_conv_wgrad", (_P, None, _P, 1, 4, 4, 16, None, _P, sz(1 << 20), None), "null pointer"),
        ("xp_stem_conv_wgrad", (_P, _P, _P, 1, 4, 4, 0, None, _P, sz(1 << 20), None), "bad shape batch=1 H=4 W=4 Co=0"),
        ("xp_stem_conv_wgrad", (_P, _P, _P, 1, 4, 4, 16, None, _P, sz(64), None), f"workspace of {64 * 9 * 16 * 8} bytes needed"),
    ]
    for entry, args, text in cases:
        rc = getattr(lib, entry)(*args)
        assert rc == -1 and lib.xp_last_error().decode() == f"{entry}: {text}", (entry, rc, lib.xp_last_error())
