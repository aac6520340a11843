"""GPU: the three training modules of xpoint_amd.training compute, bit for bit, what they computed before the module became a package (DESIGN.md
section 17), with the same library launches.  tests/golden/training_parent_bits.json was recorded ONCE on an MI355X by tools/make_golden_training_bits.py
from the single-file xpoint_amd/training.py; a mismatch is a change of results, not a reason to record again.

A case is one forward (and, in training mode, one backward of sum(out * R)) through the public surface alone: the three classes, their forward keywords,
`.t()`, `state_dict()` and `named_parameters()`.  Inputs are those of tests/heads_f64.py, tests/regnet_f64.py and tests/vss_f64.py.  A digest is the
sha256 of shape, dtype and the raw bytes of the tensor on the host; a tally is {kernel name: launches} of one profiled step from the library's event
profiler (names and counts, never times).  `finetune_step` is not here: its results pass through the loss and Adam (test_finetune_run and
test_finetune_with_the_homography_head cover it)."""
import ctypes
import hashlib
import json
import os

import pytest
import torch

from tests import heads_f64 as Hd, regnet_f64 as Rg, vss_f64 as V

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "training_parent_bits.json")
# case -> (module, the f64 helpers' case, variant)
CASES = {
    "heads/vmamba/3x9x7/train": ("heads", "vmamba/3x9x7", "train"),        # the detector's 65 channels: the pad-to-68 path of the tail
    "heads/conv/1x2x2/train": ("heads", "conv/1x2x2", "train"),
    "heads/vmamba/3x9x7/eval": ("heads", "vmamba/3x9x7", "eval"),
    "regnet/3x16x64/masks": ("regnet", "3x16x64", "masks"),                # the recorded dropout masks of the g31 case
    "regnet/3x16x64/seed5": ("regnet", "3x16x64", "seed"),                 # seed=5, sample_ids=[4, 9, 2]
    "regnet/3x16x64/eval": ("regnet", "3x16x64", "eval"),
    "vss/A/drop_path": ("vss", "A", "drop_path"),                          # drop_path=0.3, seed=5: the scaled-branch path
    "vss/B/plain": ("vss", "B", "plain"),                                  # drop_path=0: the residual rides in the launch, R = 6
    "vss/A/no_input_grad": ("vss", "A", "no_input_grad"),                  # dx = None
    "vss/B/eval": ("vss", "B", "eval"),                                    # no_grad: the keep = False path of the MLP branch
}
TRAINING_STEPS = [c for c, (_, _, variant) in CASES.items() if variant != "eval"]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def _with_grads_and_buffers(res, mod):
    params = dict(mod.named_parameters())
    for k, p in params.items():
        res["grad/" + k] = p.grad
    for k, v in mod.state_dict().items():
        if k not in params:
            res["buffer/" + k] = v
    return res


def _heads_case(case, variant):
    from xpoint_amd import training as T
    kind = case.split("/")[0]
    sd = Hd.head_state(kind)
    heads = T.XPointHeads(in_channels=sd[Hd.DET + "1.weight"].shape[1], descriptor_size=sd[Hd.DSC + "4.weight"].shape[0])
    heads.load_state_dict(sd)
    heads = heads.cuda().train(variant == "train")
    _, (enc, r1, r2), _ = Hd.case_reference(case)
    out = heads(_nhwc(enc))
    res = {"logits": out["logits"], "desc": out["desc"]}
    if variant == "eval":
        return res
    ((out["logits"] * r1.cuda()).sum() + (out["desc"] * r2.cuda()).sum()).backward()
    return _with_grads_and_buffers(res, heads)


def _regnet_case(case, variant):
    from xpoint_amd import training as T
    (enc1, enc2, R), (m1, m2), _ = Rg.case_reference(case)
    head = T.RegNetHead()
    head.load_state_dict(Rg.head_state())
    head = head.cuda().train(variant != "eval")
    if variant == "masks":
        hm = head(_nhwc(enc1), _nhwc(enc2), dropout_masks=(m1.cuda(), m2.cuda()))
    elif variant == "seed":
        hm = head(_nhwc(enc1), _nhwc(enc2), seed=5, sample_ids=[4, 9, 2])
    else:
        hm = head(_nhwc(enc1), _nhwc(enc2))
    if variant != "eval":
        (hm * R.cuda()).sum().backward()
        assert int(head.t(Rg.HM + "layer1.1.num_batches_tracked")) == 2 and int(head.t(Rg.HM + "layer1.4.num_batches_tracked")) == 2
    return _with_grads_and_buffers({"hm": hm}, head)


def _vss_case(case, variant):
    from xpoint_amd import training as T
    (_, _, _, C), R, _, stage = V.CASES[case]
    drop = variant in ("drop_path", "no_input_grad")
    blk = T.VSSBlock(C, dt_rank=R, drop_path=0.3 if drop else 0.0, stage=stage, block=0)
    blk.load_state_dict({V.prefix(case) + k: v for k, v in V.block_state(case, torch.float32).items()})
    blk = blk.cuda().train(variant != "eval")
    x, Rw = V.case_inputs(case)
    if variant == "eval":
        with torch.no_grad():
            return {"out": blk(x.cuda())}
    x = x.cuda().requires_grad_(variant != "no_input_grad")
    out = blk(x, seed=5) if drop else blk(x)
    (out * Rw.cuda()).sum().backward()
    res = {"out": out, "grad/x": x.grad}
    res.update({"grad/" + k: blk.t(k).grad for k in V.LEAVES})
    return res


def _run(case):
    module, inner, variant = CASES[case]
    return {"heads": _heads_case, "regnet": _regnet_case, "vss": _vss_case}[module](inner, variant)


def digest(t):
    """sha256 of shape, dtype and the raw bytes on the host; an absent tensor (a gradient that is None) has the digest 'none'."""
    if t is None:
        return "none"
    a = t.detach().cpu().contiguous().numpy()
    h = hashlib.sha256(f"{tuple(a.shape)} {a.dtype} ".encode())
    h.update(a.tobytes())
    return h.hexdigest()


def compute_bits(case):
    """{tensor name: digest} of one case: what tools/make_golden_training_bits.py records and what the test compares."""
    return {k: digest(v) for k, v in _run(case).items()}


def launch_tally(case):
    """{kernel name: launches} of one profiled step of the case, from the library's event profiler."""
    from xpoint_amd import _lib
    lib = _lib.load()
    lib.xp_prof_reset(); lib.xp_prof_filter(None); lib.xp_prof_enable(1)
    try:
        _run(case)
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


def _differences(mine, recorded):
    return sorted(k for k in set(mine) | set(recorded) if mine.get(k) != recorded.get(k))


def test_the_golden_file_holds_every_case():
    gold = json.load(open(GOLDEN))
    assert sorted(k for k in gold if k != "launches") == sorted(CASES)
    assert sorted(gold["launches"]) == sorted(TRAINING_STEPS)
    assert all(gold[c] for c in CASES) and all(gold["launches"][c] for c in TRAINING_STEPS)


@pytest.mark.parametrize("case", list(CASES))
def test_bits_and_launches_are_the_parents(gpu_lib, case):
    gold = json.load(open(GOLDEN))
    mine = compute_bits(case)
    differ = _differences(mine, gold[case])
    print(f"{case}: {len(mine)} tensors, {len(differ)} differ from the recorded digests: {differ}")
    assert not differ, (case, differ)
    if case in TRAINING_STEPS:
        tally = launch_tally(case)
        differ = _differences(tally, gold["launches"][case])
        print(f"{case}: {sum(tally.values())} launches of {len(tally)} kernels; differing: {[(k, tally.get(k), gold['launches'][case].get(k)) for k in differ]}")
        assert not differ, (case, differ)
