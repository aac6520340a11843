"""GPU: the training SS2D core in pixel layout (xpoint_amd.training.ss2d_core; xp_ss2d_train_fwd / xp_ss2d_train_bwd, csrc/train_ss2d.hip; DESIGN.md
section 24) against the float64 restatement tests/ss2d_core_f64.py and against the routes composition (cross-scan, selective scan, cross-merge: what
training.VSSBlock runs by default) on the GPU at the same inputs: ym and all six gradients.  Every shape runs at chunk = 0 (the library's choice) and at
chunk = 2, the smallest the entry points accept, so that chunk boundaries fall inside the tiny shapes.  Bar: max |got - ref| <= 1e-4 x the scale of each
tensor; every comparison prints err / scale."""
import ctypes

import pytest
import torch

from tests import ss2d_core_f64 as S
from tests.training_cases import _bits, _close

pytestmark = pytest.mark.gpu

# (B, H, W, C): what each covers
SHAPES = [(2, 5, 7, 32),          # L = 35 odd, H != W, two samples
          (1, 8, 12, 96),         # C no multiple of 64: idle lanes in the last wave
          (2, 2, 3, 768),         # L = 6, the stage-3 width: twelve waves
          (1, 45, 46, 32),        # L = 2070: many chunks, L no multiple of any chunk length
          (1, 1, 9, 32),          # one row: the column-major route is the row-major one
          (1, 9, 1, 32),          # one column
          (3, 16, 16, 64)]        # every chunk complete
CHUNKS = [0, 2]
OUT = ("ym",) + S.GRADS


def _dev(t):
    return {k: v.cuda() for k, v in t.items()}


def _run(t, R, dims, chunk=0):
    """{'ym', 'du', ...} of training.ss2d_core and its backward on device inputs t"""
    from xpoint_amd import training as T
    leaves = [t[k].detach().clone().requires_grad_(True) for k in S.NAMES]
    ym = T.ss2d_core(*leaves[:3], R, *leaves[3:], dims, chunk=chunk)
    g = torch.autograd.grad(ym, leaves, t["dym"])
    M = t["u"].shape[0]
    assert not bool(g[2].view(M, 4, R + 2)[:, :, :R].any()), "the dt entries of xd take no gradient from the core"
    return {"ym": ym.detach(), "du": g[0], "ddtp": g[1], "dbc": g[2].view(M, 4, R + 2)[:, :, R:].contiguous(), "dA": g[3], "dD": g[4], "ddt_bias": g[5]}


def _routes(t, R, dims):
    """The same through the composition of the operator-level kernels, as the block's default path launches it"""
    from xpoint_amd.training import vss
    ym, kept = vss._core_routes_fwd(t["u"], t["dtp"], t["xd"], R, t["A"].reshape(-1, 1), t["Ds"].reshape(-1), t["dt_bias"], dims)
    du, ddtp, dbc, dA, dD, ddb = vss._core_routes_bwd(t["dym"], kept, t["A"].reshape(-1, 1), t["Ds"].reshape(-1), t["dt_bias"], dims)
    return {"ym": ym, "du": du, "ddtp": ddtp, "dbc": dbc, "dA": dA.view(4, -1), "dD": dD.view(4, -1), "ddt_bias": ddb.view(4, -1)}


def _compare(shape, variant, chunk):
    t, R = S.op_inputs(shape, variant)
    dims = tuple(shape[:3])
    ref = S.op_reference(shape, variant)
    d = _dev(t)
    got = _run(d, R, dims, chunk)
    for k in OUT:
        _close(got[k], ref[k], f"{shape} {variant} chunk {chunk}: {k} vs float64")
    other = _routes(d, R, dims)
    for k in OUT:
        _close(got[k], other[k].double(), f"{shape} {variant} chunk {chunk}: {k} vs the routes composition", scale=float(ref[k].abs().max()))


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_operator(gpu_lib, shape, chunk):
    _compare(shape, "plain", chunk)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("variant", ["dt+30", "dt-30", "smallA"])
def test_softplus_branches_and_undamped_state(gpu_lib, variant, chunk):
    _compare((2, 5, 7, 32), variant, chunk)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_gradient_range_and_zero(gpu_lib, chunk):
    shape = (2, 5, 7, 32)
    t, R = S.op_inputs(shape)
    ref = S.op_reference(shape)
    d = _dev(t)
    for f in (2.0 ** -30, 2.0 ** 10):
        got = _run(dict(d, dym=d["dym"] * f), R, shape[:3], chunk)
        for k in S.GRADS:
            _close(got[k], ref[k] * f, f"dym x {f:g} chunk {chunk}: {k}")
    zero = _run(dict(d, dym=torch.zeros_like(d["dym"])), R, shape[:3], chunk)
    for k in S.GRADS:
        assert not bool(zero[k].any()), f"all-zero dym: {k} is not exactly zero"


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("shape", [(2, 5, 7, 32), (3, 16, 16, 64), (2, 2, 3, 768)])
def test_bit_identical_and_batch_invariant(gpu_lib, shape, chunk):
    t, R = S.op_inputs(shape)
    d = _dev(t)
    B, H, W, C = shape
    L = H * W
    a = _run(d, R, shape[:3], chunk)
    b = _run(d, R, shape[:3], chunk)
    for k in OUT:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"two calls differ in {k}"
    for s in range(B):
        one = _run({k: (v[s * L:(s + 1) * L] if v.shape[0] == B * L else v) for k, v in d.items()}, R, (1, H, W), chunk)
        for k in ("ym", "du", "ddtp", "dbc"):
            assert torch.equal(_bits(one[k]), _bits(a[k][s * L:(s + 1) * L])), f"sample {s}: {k} depends on the other samples of the call"


@pytest.mark.parametrize("chunk", CHUNKS)
def test_outputs_sit_between_guard_rows(gpu_lib, chunk):
    """The entry points themselves, every output (and the workspace) a slice of a larger buffer of a bit pattern that must survive"""
    from xpoint_amd import _lib
    shape = (2, 5, 7, 32)
    B, H, W, C = shape
    t, R = S.op_inputs(shape)
    d = _dev(t)
    M, G = B * H * W, 256
    pattern = -1.2345e33

    def guarded(n):
        buf = torch.full((n + 2 * G,), pattern, dtype=torch.float32, device="cuda")
        return buf, buf[G:G + n]

    nbytes = int(_lib.load().xp_ss2d_train_workspace_bytes(B, H, W, C, chunk))
    assert nbytes % 4 == 0
    sizes = {"ym": M * C, "du": M * C, "ddtp": M * 4 * C, "dbc": M * 8, "dA": 4 * C, "dD": 4 * C, "ddt_bias": 4 * C, "ws": nbytes // 4}
    bufs = {k: guarded(n) for k, n in sizes.items()}
    assert bufs["ws"][1].data_ptr() % 256 == 0
    st = _lib.current_stream(d["u"])
    p = lambda k: ctypes.c_void_p(bufs[k][1].data_ptr())          # noqa: E731
    common = (_lib.ptr(d["u"]), _lib.ptr(d["dtp"]), ctypes.c_void_p(d["xd"].data_ptr() + 4 * R), 4 * (R + 2), R + 2, _lib.ptr(d["A"]), _lib.ptr(d["Ds"]),
              _lib.ptr(d["dt_bias"]))
    tail = (p("ws"), ctypes.c_size_t(nbytes), B, H, W, C, 1, chunk, st)
    _lib.call("xp_ss2d_train_fwd", *common, p("ym"), *tail)
    _lib.call("xp_ss2d_train_bwd", *common, _lib.ptr(d["dym"]), *(p(k) for k in S.GRADS), *tail)
    torch.cuda.synchronize()
    want = _run(d, R, shape[:3], chunk)
    shapes = {"ym": (M, C), "du": (M, C), "ddtp": (M, 4 * C), "dbc": (M, 4, 2), "dA": (4, C), "dD": (4, C), "ddt_bias": (4, C)}
    for k, (buf, mid) in bufs.items():
        n = sizes[k]
        assert bool((buf[:G] == pattern).all()) and bool((buf[G + n:] == pattern).all()), f"{k}: a guard row changed"
        if k != "ws":
            assert torch.equal(_bits(mid.view(shapes[k])), _bits(want[k])), f"{k}: the guarded call differs from the operator's"
            assert not bool((mid == pattern).any()), f"{k}: an element was left unwritten"


def test_refusals(gpu_lib):
    from xpoint_amd import _lib, training as T
    t, R = S.op_inputs((2, 5, 7, 32))
    d = _dev(t)
    args = [d[k] for k in S.NAMES]
    with pytest.raises(ValueError, match="chunk"):
        T.ss2d_core(*args[:3], R, *args[3:], (2, 5, 7), chunk=3)
    with pytest.raises(ValueError, match="dims"):
        T.ss2d_core(*args[:3], R, *args[3:], (2, 5, 8))
    with pytest.raises(ValueError, match="xd"):
        T.ss2d_core(*args[:3], R + 1, *args[3:], (2, 5, 7))
    with pytest.raises(_lib.XPointHipError, match="no CPU fallback"):
        T.ss2d_core(t["u"], *args[1:3], R, *args[3:], (2, 5, 7))
    with pytest.raises(TypeError, match="float32"):
        T.ss2d_core(d["u"].double(), *args[1:3], R, *args[3:], (2, 5, 7))
