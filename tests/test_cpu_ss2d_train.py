"""CPU: the training SS2D core in pixel layout as far as it goes without a GPU — the float64 restatement
tests/ss2d_core_f64.py pinned against the block restatement of tests/vss_f64.py (itself pinned against the real reference), the three exports and
their argument checks, and the setting's refusals."""
import ctypes

import pytest
import torch

from tests import ss2d_core_f64 as S, vss_f64 as V
from tests.training_cases import _close

KEYS = ["out", "grad/x"] + ["grad/" + k for k in V.LEAVES]


@pytest.mark.parametrize("case", list(V.CASES))
def test_restatement_reproduces_the_block(case):
    """vss_block64 rebuilt around core64 (x_proj and the dt projection in pixel layout) against the route-layout restatement: output and every gradient"""
    got, ref = S.vss_step64_core(case), V.case_reference(case)
    for k in KEYS:
        _close(got[k], ref[k], f"{case}/{k}", tol=1e-12)


def test_restatement_reads_only_the_bc_entries():
    t, R = S.op_inputs((2, 5, 7, 32))
    ref = S.op_reference((2, 5, 7, 32))
    xd = t["xd"].clone().view(-1, 4, R + 2)
    xd[:, :, :R] = 7.0
    other = S.op_step64(dict(t, xd=xd.view(-1, 4 * (R + 2))), R, (2, 5, 7))
    assert all(torch.equal(other[k], ref[k]) for k in ref)


def test_exports_are_declared_and_bound():
    from xpoint_amd import _lib
    names = {"xp_ss2d_train_workspace_bytes", "xp_ss2d_train_fwd", "xp_ss2d_train_bwd"}
    assert names <= set(_lib.exported_symbols())
    assert {"xp_ss2d_train_fwd", "xp_ss2d_train_bwd"} <= set(_lib._SIGNATURES) and "xp_ss2d_train_workspace_bytes" in _lib._SIZE_QUERIES
    lib = _lib.load()
    for n in names:
        assert getattr(lib, n) is not None


def _args(which, u=1, ws=256, nbytes=None, dstate=1, chunk=0, dims=(2, 5, 7, 32)):
    """The argument list of xp_ss2d_train_fwd / _bwd with fake (never dereferenced: every check comes before the first launch) non-null pointers"""
    B, H, W, C = dims
    from xpoint_amd import _lib
    if nbytes is None:
        nbytes = int(_lib.load().xp_ss2d_train_workspace_bytes(B, H, W, C, chunk))
    p = ctypes.c_void_p(4096)
    ptrs = [p] * (7 if which == "fwd" else 13)
    ptrs[0] = ctypes.c_void_p(4096 * u) if u else None
    return (*ptrs[:3], 16, 4, *ptrs[3:], ctypes.c_void_p(ws) if ws else None, ctypes.c_size_t(nbytes), B, H, W, C, dstate, chunk, None)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_argument_errors(which):
    from xpoint_amd import _lib
    lib = _lib.load()
    name = f"xp_ss2d_train_{which}"
    need = int(lib.xp_ss2d_train_workspace_bytes(2, 5, 7, 32, 0))
    assert need > 0 and need % 256 == 0
    for kw, text in ((dict(dstate=2), "d_state 1 only"), (dict(u=0), "null tensor pointer"), (dict(ws=0), "workspace of"),
                     (dict(nbytes=need - 1), "workspace of"), (dict(chunk=3, nbytes=need), "chunk must be 0 or a power of two"),
                     (dict(chunk=128, nbytes=need), "chunk must be"), (dict(chunk=64, dims=(1, 2, 2, 768), nbytes=1 << 30), "chunk x C"),
                     (dict(ws=128), "256-byte aligned"), (dict(dims=(16, 512, 512, 128), nbytes=1 << 40), "below 2\\^31")):
        with pytest.raises(_lib.XPointHipError, match=f"{name}: .*{text}"):
            _lib.call(name, *_args(which, **kw))


def test_workspace_query():
    from xpoint_amd import _lib
    q = _lib.load().xp_ss2d_train_workspace_bytes
    assert int(q(2, 5, 7, 32, 0)) > 0 and int(q(2, 5, 7, 32, 2)) > int(q(2, 5, 7, 32, 64)) > 0
    for bad in ((2, 5, 7, 32, 3), (2, 5, 7, 32, 1), (2, 5, 7, 32, 128), (1, 2, 2, 768, 16), (0, 5, 7, 32, 0), (2, 5, 7, 1028, 0), (16, 512, 512, 128, 0)):
        assert int(q(*bad)) == 0, bad
    assert int(q(1, 2, 2, 768, 8)) > 0 and int(q(1, 2, 2, 1024, 4)) > 0


def test_the_setting_refuses_unknown_kinds():
    from xpoint_amd import training as T
    blk = T.VSSBlock(32, dt_rank=2)
    assert blk.ss2d_core == "routes"
    with pytest.raises(ValueError, match="'nope'"):
        T.set_ss2d_core(blk, "nope")
    assert blk.ss2d_core == "routes"
    assert T.set_ss2d_core(blk, "pixel") is blk and blk.ss2d_core == "pixel"
    enc = T.VSSEncoder(32, [1, 1, 1, 1])
    assert enc.ss2d_core == "routes" and T.set_ss2d_core(enc, "pixel").ss2d_core == "pixel"
    with pytest.raises(ValueError, match="no VSS block"):
        T.set_ss2d_core(torch.nn.Linear(2, 2), "pixel")


def test_fit_checks_its_key_before_it_builds_anything(tmp_path):
    from xpoint_amd import training as T
    out = tmp_path / "never"
    with pytest.raises(ValueError, match="training.ss2d_core.*'nope'"):
        T.fit({"training": {"ss2d_core": "nope", "output_directory": str(out)}})          # no model, loss or dataset section is reached
    assert not out.exists()
