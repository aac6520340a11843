"""GPU: the dense training operators (csrc/train_dense.hip, csrc/train_dgrad.hip and the shared scale helper of csrc/train_scale.h) compute, bit for
bit and with the same profiled launches, what they computed while they were one file with every repeated piece written out.
tests/golden/train_dense_parent_bits.json was recorded ONCE on an MI355X by tools/make_golden_train_dense_bits.py at the commit before the split; a
mismatch is a change of results, not a reason to record again.

tests/golden/training_parent_bits.json (test_gpu_training_bits.py) pins the heads, RegNet and VSS modules; this file reaches what it does not: the
stride-2 and reflection kernels, every operator with `dy_scale=None` (the call takes its own power of two) AND with the `scale_grad` pair, the
BatchNorm / column-sum / L2 kernels at their ragged shapes, `scale_grad`'s walk with a tail, and one whole step of VSSEncoder and of XPointNet.  Shapes
are those of the operator tests (test_gpu_head_training, test_gpu_regnet_training, test_gpu_encoder_training, test_gpu_xpoint_training): every
kernel instance and every ragged edge.  A digest is the sha256 of shape, dtype and bytes; a tally is {profiler scope: launches} of one run."""
import ctypes
import json
import os

import pytest
import torch

from tests import encoder_f64 as En
from tests import test_gpu_encoder_training as TE, test_gpu_xpoint_training as TX
from tests.test_gpu_training_bits import _differences, _with_grads_and_buffers, digest
from xpoint_amd import synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_dense_parent_bits.json")
CHUNK = 256
ZP_SHAPES = [(1, 1, 1, 4, 8), (3, 9, 7, 12, 20), (1, 257, 1, 8, 4)]          # (B, H, W, Ci, Co)

# case -> (kind, parameters)
CASES = {}
for _I, _J in ((65, 256), (8, 4)):
    for _M in (1, 33, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 17):
        CASES[f"gemm_tn/{_M}x{_I}x{_J}"] = ("gemm_tn", (_M, _I, _J))
CASES["gemm_tn/column_slices"] = ("gemm_tn_slices", ())
for _s in ((1, 2, 2, 4, 8), (3, 9, 7, 48, 512)):
    CASES[f"conv3x3_wgrad/{_s}"] = ("conv3x3_wgrad", _s)
for _s in ZP_SHAPES:
    CASES[f"conv3x3_wgrad_zero_pad/{_s}"] = ("conv3x3_wgrad_zero_pad", _s)
    CASES[f"conv3x3_dgrad/{_s}"] = ("conv3x3_dgrad", _s)
for _s in TE.CONV_SHAPES:
    CASES[f"conv3x3_s2_wgrad/{_s}"] = ("conv3x3_s2_wgrad", _s)
    CASES[f"conv3x3_s2_dgrad/{_s}"] = ("conv3x3_s2_dgrad", _s)
for _s in TX.DGRAD_SHAPES:
    CASES[f"conv3x3_dgrad_reflect/{_s}"] = ("conv3x3_dgrad_reflect", _s)
for _s in ((1, 5, 7), (2, 6, 10)):
    for _Co in (16, 48):
        CASES[f"stem_conv_wgrad/{_s}/{_Co}"] = ("stem_conv_wgrad", _s + (_Co,))
for _rows in (2, 3, 1023):
    for _C in (65, 256):
        CASES[f"bn/{_rows}x{_C}"] = ("bn", (_rows, _C, 0))
CASES["bn/strided/3x65"] = ("bn", (3, 65, 7))                               # rows of a wider matrix: ld = C + 7
CASES["colsum_rows/1023x65"] = ("colsum_rows", (1023, 65))
for _rows in (1, 5):
    CASES[f"l2norm_rows_bwd/{_rows}"] = ("l2norm_rows_bwd", (_rows, 256))
for _n in (1, 255, 256, 4480, 1024 * 256 * 4 + 77):                          # one tail row; no tail; 17 rows and a tail; more rows than amax parts x 4
    CASES[f"scale_grad/{_n}"] = ("scale_grad", (_n,))
CASES["layernorm_bwd/scaled"] = ("layernorm_bwd", (33, 96))
CASES["dwconv3x3_silu_bwd/scaled"] = ("dwconv3x3_silu_bwd", (2, 5, 7, 8))
CASES["gelu_bwd/scaled"] = ("gelu_bwd", (33, 96))
CASES["step/VSSEncoder/S"] = ("encoder_step", ("S",))
CASES["step/XPointNet"] = ("model_step", ())
assert min(En.CASES, key=lambda c: En.CASES[c][0] * sum(En.CASES[c][1])) == "S"          # the smallest encoder of tests/encoder_f64.py

# the cases whose profiler tally is recorded: the whole steps, and one call with dy_scale=None of each convolution gradient
CONV_TALLIES = {"conv3x3_wgrad": (3, 9, 7, 48, 512), "conv3x3_wgrad_zero_pad": ZP_SHAPES[1], "conv3x3_dgrad": ZP_SHAPES[1],
                "conv3x3_s2_wgrad": TE.CONV_SHAPES[0], "conv3x3_s2_dgrad": TE.CONV_SHAPES[0], "conv3x3_dgrad_reflect": TX.DGRAD_SHAPES[4]}
TALLIED = [f"{k}/{s}" for k, s in CONV_TALLIES.items()] + ["stem_conv_wgrad/(1, 5, 7)/16", "step/VSSEncoder/S", "step/XPointNet"]


def _u(name, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(synth.uniform("tdb/" + name, shape, lo, hi)).cuda()


def _both(T, fn, g):
    """{'none', 'scaled'}: fn(gradient, scale) with the call's own power of two, and with scale_grad's pair."""
    gs, sc = T.scale_grad(g)
    return {"none": fn(g, None), "scaled": fn(gs, sc)}


def _s2_out(n):
    return (n - 1) // 2 + 1


def _conv_operands(kind, shape, stride=1):
    B, H, W, Ci, Co = shape
    Ho, Wo = (_s2_out(H), _s2_out(W)) if stride == 2 else (H, W)
    return (_u(f"{kind}/x{shape}", (B, H, W, Ci), -2.0, 2.0), _u(f"{kind}/w{shape}", (Co, 3, 3, Ci), -0.5, 0.5),
            _u(f"{kind}/dy{shape}", (B, Ho, Wo, Co)) * 1e-2)


def _bn(T, rows, C, pad):
    res = {}
    wide, dwide = _u(f"bn/x{rows, C, pad}", (rows, C + pad), -2.0, 2.0), _u(f"bn/dy{rows, C, pad}", (rows, C + pad)) * 1e-3
    x, dy = wide[:, pad // 2:pad // 2 + C], dwide[:, pad // 2:pad // 2 + C]
    gamma, beta = _u(f"bn/g{C}", (C,), 0.5, 1.5), _u(f"bn/b{C}", (C,), -0.2, 0.2)
    y, mean, invstd, var = T.bn_train_fwd(x, gamma, beta)
    res.update({"fwd/y": y, "fwd/mean": mean, "fwd/invstd": invstd, "fwd/var": var})
    for relu in (False, True):
        for scaled in (False, True):
            dx, dg, db, sc = T.bn_train_bwd(dy, x, gamma, mean, invstd, relu_mask=relu, scaled=scaled)
            res.update({f"bwd/relu{int(relu)}/scaled{int(scaled)}/{k}": v for k, v in (("dx", dx), ("dgamma", dg), ("dbeta", db), ("scale", sc))})
    return res


def _encoder_step():
    enc = TE._encoder("S")
    images, Rw = En.case_inputs("S")
    return _with_grads_and_buffers({"out": TE._step(enc, images, Rw)["out"]}, enc)


def _model_step():
    model = TX._model()
    got, _ = TX._step(model)
    res = {k: v for k, v in got.items() if not k.startswith("grad/")}
    return _with_grads_and_buffers(res, model)


GRADIENT_OPS = ("gemm_tn", "gemm_tn_slices", "conv3x3_wgrad", "conv3x3_wgrad_zero_pad", "conv3x3_s2_wgrad", "conv3x3_dgrad", "conv3x3_dgrad_reflect",
                "conv3x3_s2_dgrad", "stem_conv_wgrad", "colsum_rows")


def _gradient_op(T, kind, p):
    """(fn(gradient, scale), gradient) of an operator that takes a gradient operand and, optionally, its {S, 1 / S}."""
    if kind == "gemm_tn":
        M, I, J = p
        Q = _u(f"gemm/q{p}", (M, J), -4.0, 4.0)
        return (lambda g, sc: T.gemm_tn(g, Q, p_scale=sc)), _u(f"gemm/p{p}", (M, I)) * 3e-6
    if kind == "gemm_tn_slices":          # Q = columns 256..511 of a 512-wide activation, P a slice of a padded gradient
        M = CHUNK + 1
        wide = _u("gemm/wide", (M, 512), -2.0, 2.0)
        return (lambda g, sc: T.gemm_tn(g[:, :65], wide[:, 256:], p_scale=sc)), _u("gemm/pw", (M, 68)) * 1e-4
    if kind == "stem_conv_wgrad":
        B, H, W, Co = p
        img = _u(f"stem/img{p}", (B, 1, H, W), 0.0, 1.0)
        return (lambda g, sc: T.stem_conv_wgrad(img, g, dy_scale=sc)), _u(f"stem/dy{p}", (B, _s2_out(H), _s2_out(W), Co)) * 1e-2
    if kind == "colsum_rows":
        return (lambda g, sc: T.colsum_rows(g, x_scale=sc)), _u(f"colsum/x{p}", p) * 1e-3
    x, w, dy = _conv_operands(kind, p, 2 if "s2" in kind else 1)
    if kind == "conv3x3_s2_dgrad":
        return (lambda g, sc: T.conv3x3_s2_dgrad(g, w, p[1:3], dy_scale=sc)), dy
    if "dgrad" in kind:
        return (lambda g, sc: getattr(T, kind)(g, w, dy_scale=sc)), dy
    return (lambda g, sc: getattr(T, kind)(x, g, dy_scale=sc)), dy


def _run(case):
    from xpoint_amd import training as T
    kind, p = CASES[case]
    if kind in GRADIENT_OPS:
        return _both(T, *_gradient_op(T, kind, p))
    if kind == "bn":
        return _bn(T, *p)
    if kind == "l2norm_rows_bwd":
        x = _u(f"l2/x{p}", p)
        x[p[0] // 2 + 1:p[0] // 2 + 2] = 0.0          # rows = 5: row 3 is the zero row (the clamp's branch); rows = 1: no row is touched
        return {"dx": T.l2norm_rows_bwd(x, _u(f"l2/dy{p}", p) * 1e-2)}
    if kind == "scale_grad":
        g = _u(f"scale/g{p}", p) * 3e-5
        copy, sc = T.scale_grad(g)
        mine = g.clone()
        same, sc2 = T.scale_grad(mine, out=mine)
        assert same.data_ptr() == mine.data_ptr()
        return {"copy": copy, "copy/scale": sc, "in_place": same, "in_place/scale": sc2}
    if kind == "layernorm_bwd":
        dx, dg, db, sc = T.layernorm_bwd(_u("ln/dy", p) * 1e-3, _u("ln/x", p, -2.0, 2.0), _u("ln/g", p[1:], 0.5, 1.5), scaled=True)
        return {"dx": dx, "dgamma": dg, "dbeta": db, "scale": sc}
    if kind == "dwconv3x3_silu_bwd":
        dx, dw, sc = T.dwconv3x3_silu_bwd(_u("dw/x", p, -2.0, 2.0), _u("dw/w", (9, p[-1]), -0.5, 0.5), _u("dw/dy", p) * 1e-3, scaled=True)
        return {"dx": dx, "dw": dw, "scale": sc}
    if kind == "gelu_bwd":
        dx, sc = T.gelu_bwd(_u("gelu/dy", p) * 1e-3, _u("gelu/x", p, -3.0, 3.0), scaled=True)
        return {"dx": dx, "scale": sc}
    return {"encoder_step": _encoder_step, "model_step": _model_step}[kind]()


def compute_bits(case):
    """{tensor name: digest} of one case: what tools/make_golden_train_dense_bits.py records and what the test compares."""
    return {k: digest(v) for k, v in _run(case).items()}


def launch_tally(case):
    """{profiler scope: launches} of one profiled run of the case; a convolution gradient is called once, with dy_scale=None."""
    from xpoint_amd import _lib, training as T
    lib = _lib.load()
    kind, p = CASES[case]
    run = lambda: _run(case)          # noqa: E731
    if kind in GRADIENT_OPS:          # the operands are made before the profiler counts
        fn, g = _gradient_op(T, kind, p)
        run = lambda: fn(g, None)          # noqa: E731
    lib.xp_prof_reset(); lib.xp_prof_filter(None); lib.xp_prof_enable(1)
    try:
        run()
        torch.cuda.synchronize()
    finally:
        lib.xp_prof_enable(0)
    name, cnt = ctypes.create_string_buffer(96), ctypes.c_int()
    tally = {}
    for i in range(lib.xp_prof_count()):
        lib.xp_prof_get(i, name, 96, None, ctypes.byref(cnt), None, None)
        tally[name.value.decode()] = cnt.value
    lib.xp_prof_reset()
    return dict(sorted(tally.items()))


def test_the_golden_file_holds_every_case():
    gold = json.load(open(GOLDEN))
    assert sorted(k for k in gold if k != "launches") == sorted(CASES)
    assert sorted(gold["launches"]) == sorted(TALLIED) and set(TALLIED) <= set(CASES)
    assert all(gold[c] for c in CASES) and all(gold["launches"][c] for c in TALLIED)


@pytest.mark.parametrize("case", list(CASES))
def test_bits_and_launches_are_the_parents(gpu_lib, case):
    gold = json.load(open(GOLDEN))
    mine = compute_bits(case)
    differ = _differences(mine, gold[case])
    print(f"{case}: {len(mine)} tensors, {len(differ)} differ from the recorded digests: {differ}")
    assert not differ, (case, differ)
    if case in TALLIED:
        tally = launch_tally(case)
        differ = _differences(tally, gold["launches"][case])
        print(f"{case}: {sum(tally.values())} launches of {len(tally)} scopes; differing: {[(k, tally.get(k), gold['launches'][case].get(k)) for k in differ]}")
        assert not differ, (case, differ)
