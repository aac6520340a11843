"""The reference's two prediction flows as functions (they are scripts upstream):
  predict_align_image_pair  — reference predict_align_image_pair.py:176-264 (= benchmark_evaluation.py:16-142,
                              demo.py:30-69,427-462): forward -> prob*mask -> box_nms -> nonzero ->
                              interpolate_descriptors -> get_matches.
  predict_keypoints         — reference predict_keypoints.py:144-216: NMS on the UNMASKED prob, mask applied at
                              extraction.
plus `PairPipeline`, the batched device-resident form of the first flow used by bench.py (no host
synchronisation between stages, preallocated buffers)."""
from __future__ import annotations

import copy
import ctypes
import os

import torch

from . import _lib
from . import utils
from ._lib import c_i, ptr
from .models import take_status

# reference configs/cipdp.yaml:47-61
DEFAULT_PREDICTION = dict(detection_threshold=0.015, nms=8, cpu_nms=True, topk=0,
                          matching=dict(method="bfmatcher", knn_matches=False, method_kwargs=dict(crossCheck=True)))


def _cfg(pred):
    c = copy.deepcopy(DEFAULT_PREDICTION)
    if pred:
        utils.dict_update(c, pred)
    return c


def predict_align_image_pair(net, data, cfg_prediction=None, match_mode="strict_mnn", estimate_homography=False, warp_optical=None):
    """data: the reference pair dict ({'optical': {'image','valid_mask',...}, 'thermal': {...}}) on the GPU.
    Returns (out_optical, out_thermal, results) where results[i] = dict(kp_optical, kp_thermal (N,2) int64 (y,x),
    desc_optical, desc_thermal (N,D), matches [DMatch]).  estimate_homography=True adds the registration step of
    predict_align_image_pair.py:287-303: H_est (3,3) float64 mapping optical (x, y) to thermal (identity when fewer than
    4 matches, as the reference) and matchesMask, from `utils.find_homography` at `reprojection_threshold` (default 3), and — unless
    warp_optical=False — the script's final product (predict_align_image_pair.py:267-271, 308): `warped_optical`, the optical image multiplied
    by its valid mask and quantised to uint8 RGB as the reference builds `im_optical`, and warped by H_est into the thermal frame (`utils.warp_perspective`: INTER_LINEAR,
    BORDER_CONSTANT; (H, W, 3) uint8 on the device).  warp_optical=True without estimate_homography is an error."""
    if warp_optical and not estimate_homography:
        raise ValueError("predict_align_image_pair: warp_optical needs estimate_homography=True (the warp uses H_est)")
    if warp_optical is None:
        warp_optical = estimate_homography
    pred = _cfg(cfg_prediction)
    if net.takes_pair():
        out_o, out_t, _ = net(data)
    else:
        out_o, out_t = net(data['optical']), net(data['thermal'])
    thr = pred['detection_threshold']
    H, W = data['optical']['image'].shape[2:]
    for out, spec in ((out_o, 'optical'), (out_t, 'thermal')):
        if pred['nms'] > 0:          # the mask is applied only on the NMS branch (predict_align_image_pair.py:194-205)
            out['prob'] = utils.box_nms(out['prob'] * data[spec]['valid_mask'], pred['nms'], thr, keep_top_k=pred['topk'],
                                        on_cpu=pred['cpu_nms'])
    results = []
    for i in range(out_o['prob'].shape[0]):
        ko = torch.nonzero((out_o['prob'][i].squeeze() > thr).float())
        kt = torch.nonzero((out_t['prob'][i].squeeze() > thr).float())
        do = utils.interpolate_descriptors_nhwc(ko, out_o['desc_nhwc'][i], H, W)
        dt = utils.interpolate_descriptors_nhwc(kt, out_t['desc_nhwc'][i], H, W)
        ms = utils.get_matches(do, dt, pred['matching']['method'], pred['matching']['knn_matches'], mode=match_mode,
                               **pred['matching']['method_kwargs'])
        r = dict(kp_optical=ko, kp_thermal=kt, desc_optical=do, desc_thermal=dt, matches=ms)
        if estimate_homography:
            import numpy as np
            H_est, mask = None, None
            if len(ms) >= 4:
                qi = torch.tensor([m.queryIdx for m in ms], device=ko.device); ti = torch.tensor([m.trainIdx for m in ms], device=ko.device)
                H_est, mask = utils.find_homography(ko[qi].flip(-1).float(), kt[ti].flip(-1).float(),
                                                    float(pred.get('reprojection_threshold', 3.0)))
            r["H_est"] = H_est if H_est is not None else np.eye(3)
            r["matchesMask"] = mask.ravel().tolist() if mask is not None else []
            if warp_optical:
                # the reference masks the optical image before quantising it (predict_align_image_pair.py:267-271); data is left unchanged
                r["warped_optical"] = utils.warp_perspective(data['optical']['image'][i, 0], r["H_est"], quantise_u8=True, dst_channels=3,
                                                             mask=data['optical']['valid_mask'][i])
        results.append(r)
    return out_o, out_t, results


def predict_keypoints(net, data, cfg_prediction=None):
    """Returns ([kp per optical image], [kp per thermal image]); kp (N,2) int64 (y,x)."""
    pred = _cfg(cfg_prediction)
    if net.takes_pair():
        out_o, out_t, _ = net(data)
    else:
        out_o, out_t = net(data['optical']), net(data['thermal'])
    thr = pred['detection_threshold']
    res = []
    for out, spec in ((out_o, 'optical'), (out_t, 'thermal')):
        p = out['prob']
        if pred['nms'] > 0:
            p = utils.box_nms(p, pred['nms'], thr, keep_top_k=pred['topk'], on_cpu=pred['cpu_nms'])
        m = data[spec]['valid_mask']
        res.append([torch.nonzero((p[i].squeeze() > thr).float() * m[i].squeeze()) for i in range(p.shape[0])])
    return res[0], res[1]


class PairPipeline:
    """encode + detect + describe + match for a batch of B pairs, entirely stream-ordered on the device.

    run() enqueues: one 2B-image forward, prob*mask, box NMS (fixed number of sweeps, verified afterwards),
    keypoint extraction, descriptor sampling, mutual-NN matching.  Results stay on the GPU; `fetch()`
    synchronises, checks NMS convergence / capacity and returns host lists."""

    def __init__(self, net, batch, H, W, cap=8192, cfg_prediction=None, match_mode="strict_mnn", nms_sweeps=8, overlap=False,
                 split_encoder=False, estimate_homography=False, ransac_iters=10000, alternate_encoders=False, warp_optical=False):
        """overlap=True: two HIP streams — the encoder of call i+1 runs while the detection / matching kernels of call i
        (many small, latency-bound launches) are still in flight; encoder outputs are double-buffered.  Results of a
        call are complete after fetch() / torch.cuda.synchronize(), exactly as without overlap."""
        self.net, self.B, self.H, self.W, self.cap = net, int(batch), int(H), int(W), int(cap)
        self.overlap = bool(overlap)
        # split_encoder = S > 1: the 2B images go through the encoder as S groups on S streams (images are independent),
        # so the kernels of different groups fill each other's tails and latency-bound phases
        self.split_encoder = (int(split_encoder) if self.overlap else 0)
        if self.split_encoder in (0, 1) or (2 * self.B) % max(self.split_encoder, 1):
            self.split_encoder = 0
        # alternate_encoders: the encoders of consecutive calls run on two streams (call i on stream i & 1, whole batch, own
        # workspace), so TWO full-batch forwards are in flight next to the detection / matching of the call before — the
        # kernels keep their large-batch efficiency and fill each other's tails.  Results are those of the one-stream step.
        self.alternate = bool(alternate_encoders) and self.overlap and not self.split_encoder
        self.depth = (max(2, int(alternate_encoders)) if self.alternate else 2) if self.overlap else 1      # calls in flight = sets of input / encoder-output buffers
        self._call = 0
        self.pred = _cfg(cfg_prediction)
        self.mode = match_mode
        self.sweeps = int(nms_sweeps)
        dev = net._device if getattr(net, "_device", None) is not None and net._device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        with torch.cuda.device(dev):            # streams / events below belong to the model's device, whatever device is current
            self._init_buffers(net, H, W, estimate_homography, ransac_iters)
            # warp_optical: the registration output of predict_align_image_pair.py:308 for every pair, stream-ordered behind the robust fit —
            # the optical image (quantised to uint8 as the reference's im_optical, :271) warped by the DEVICE-resident H_est
            self.warp_optical = bool(warp_optical)
            if self.warp_optical:
                if not self.estimate_homography:
                    raise ValueError("PairPipeline: warp_optical needs estimate_homography=True")
                self.hg["warped"] = torch.empty((self.B, self.H, self.W), dtype=torch.uint8, device=dev)

    def _init_buffers(self, net, H, W, estimate_homography, ransac_iters):
        dev = self.device
        n = 2 * self.B
        lib = _lib.load()
        nbuf = self.depth
        self.images_b = [torch.empty((n, 1, H, W), device=dev) for _ in range(nbuf)]
        self.images = self.images_b[0]
        self.raw_b = [None] * nbuf
        self.mask_b = [None] * nbuf          # uint8 valid masks per buffer set: allocated by the first masked step
        self._u8_b = None                    # uint8 image staging per buffer set: allocated by the first uint8 step
        self.prob_nms = torch.empty((n, H, W), device=dev)
        self.prob_masked = torch.empty((n, H, W), device=dev)
        self.group_ws = self.alt_ws = None   # encoder workspaces of the split (one per image group) / alternating (one per buffer set) schedule
        if self.overlap:
            self.enc_stream, self.post_stream = torch.cuda.Stream(), torch.cuda.Stream()
            S = max(self.split_encoder, 1)
            n_enc = S if self.split_encoder else nbuf if self.alternate else 1         # streams that encode: one per image group / per buffer set (_streams_of)
            self.enc_streams = [self.enc_stream] + [torch.cuda.Stream() for _ in range(n_enc - 1)]
            if self.split_encoder:
                self.group_ws = [torch.empty(net.workspace_bytes(n // S, H, W), dtype=torch.uint8, device=dev) for _ in range(S)]
            if self.alternate:
                self.alt_ws = [torch.empty(net.workspace_bytes(n, H, W), dtype=torch.uint8, device=dev) for _ in range(nbuf)]
            self.enc_done = [[torch.cuda.Event() for _ in range(S)] for _ in range(nbuf)]      # [buffer set][image group]
            self.post_done = [torch.cuda.Event() for _ in range(nbuf)]
        self.nms_ws = torch.empty(lib.xp_box_nms_workspace_bytes(n, H, W, self.cap), dtype=torch.uint8, device=dev)
        self.kp = torch.zeros((n, self.cap, 2), dtype=torch.int32, device=dev)
        self.counts = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.kp_ws = torch.empty(lib.xp_extract_keypoints_workspace_bytes(n, H, W), dtype=torch.uint8, device=dev)
        D = int(net.config['descriptor_size'])
        self.D = D
        self.desc = torch.zeros((n, self.cap, D), device=dev)
        P = self.B
        self.m = dict(idx12=torch.empty((P, self.cap), dtype=torch.int32, device=dev), dist12=torch.empty((P, self.cap), device=dev),
                      idx21=torch.empty((P, self.cap), dtype=torch.int32, device=dev), dist21=torch.empty((P, self.cap), device=dev),
                      match_q=torch.empty((P, self.cap), dtype=torch.int32, device=dev),
                      match_t=torch.empty((P, self.cap), dtype=torch.int32, device=dev),
                      match_d=torch.empty((P, self.cap), device=dev), match_count=torch.zeros((P,), dtype=torch.int32, device=dev))
        self.match_ws = torch.empty(lib.xp_match_workspace_bytes(P, self.cap, self.cap, D), dtype=torch.uint8, device=dev)
        # optional registration step (predict_align_image_pair.py:283-303) on the device: one batched robust fit per pair
        self.estimate_homography = bool(estimate_homography)
        self.ransac_iters = int(ransac_iters)
        if self.estimate_homography:
            self.hg = dict(src=torch.empty((P, self.cap, 2), device=dev), dst=torch.empty((P, self.cap, 2), device=dev),
                           H=torch.empty((P, 3, 3), dtype=torch.float64, device=dev), mask=torch.empty((P, self.cap), dtype=torch.uint8, device=dev),
                           n_inliers=torch.zeros((P,), dtype=torch.int32, device=dev),
                           ws=torch.empty(lib.xp_find_homography_workspace_bytes(P) // 8 + 1, dtype=torch.float64, device=dev))
        self.raw = None
        self.repaired = False        # set by verify(): the latest call was recomputed (range guard): earlier host downloads of it are stale
        self._last = None            # (buffer set, masked) of the latest call: what verify() re-runs when the range guard trips
        self._graphs = None
        self._capture_masked = None
        # range guard of the dense engine (status_word, _note_engine, _settle_engine)
        self._status = torch.zeros(1, dtype=torch.int32, device=dev)
        self._engine_enqueued = None   # dense engine of the forward enqueued last
        self._h2_pending = False       # some forward enqueued on "h2" has not been judged yet
        self._graph_engine = None      # dense engine the graphs were captured on
        # download_async: pinned host buffer sets (allocated by its first call) and their rotation
        self._copy_engine_d2h = os.environ.get("XP_D2H_COPY_ENGINE", "0") == "1"      # A/B: the runtime's copy engines for the result lists
        self.host_sets = max(2, self.depth + 1)
        self._host = self._host_src = self._host_ev = None
        self._host_i = 0

    def run(self, optical, thermal, mask_optical=None, mask_thermal=None):
        """Input contract (also of capture() / the replay callable): optical and thermal are (B, 1, H, W) / (B, H, W) images of the SAME dtype —
        float32 in [0, 1] (device-resident: staged by one kernel; host / pinned: copied), or uint8 gray 0..255 (a quarter of the PCIe bytes; divided by 255
        on the device, the same f32 division the reference's loader does on the host).  A uint8 / float mix raises ValueError.  Masks: both or neither."""
        if (mask_optical is None) != (mask_thermal is None):
            raise ValueError("PairPipeline.run: pass both valid masks or neither")
        with torch.cuda.device(self.device):
            return self._step(optical, thermal, mask_optical, mask_thermal)

    def _step(self, optical, thermal, mask_optical, mask_thermal, replay=False):
        """Enqueue one step: THE schedule, for eager steps and (replay=True) for steps replayed from the captured graphs.  The two bodies it runs —
        the encoder on image group h of buffer set k, detection / matching on buffer set k — are eager calls or graph replays; the waits and records
        around them are the same ("PairPipeline's step schedule")."""
        masked = mask_optical is not None
        if not self.overlap:                                    # one stream: everything in the caller's stream order
            self._stage_inputs(0, optical, thermal, mask_optical, mask_thermal)
            self._last = (0, masked)
            if replay:
                self._note_engine(self._graph_engine)
                self._graphs.replay()
            else:
                self._encode_group(0)
                self._post(0, masked)
            return self
        k = self._call % self.depth
        self._call += 1
        self._last = (k, masked)
        cur = torch.cuda.current_stream()
        # inputs are taken over on the CALLER's stream (so the caller may reuse its tensors right after the call returns),
        # once the step `depth` calls ago has finished with buffer set k
        cur.wait_event(self.post_done[k])
        self._stage_inputs(k, optical, thermal, mask_optical, mask_thermal)
        enc_g, post_g = self._graphs[k] if replay else (None, None)
        if self.split_encoder and self.raw_b[k] is None:        # first (eager) step on this buffer set: one whole-batch forward allocates the outputs the groups write into
            self.enc_stream.wait_stream(cur)
            with torch.cuda.stream(self.enc_stream):
                self._encode_group(k)
            cur.wait_stream(self.enc_stream)
        for h, stream in enumerate(self._streams_of(k)):
            stream.wait_stream(cur)
            with torch.cuda.stream(stream):
                if replay:
                    self._note_engine(self._graph_engine)
                    enc_g[h].replay()
                else:
                    self._encode_group(k, h)
                self.enc_done[k][h].record()
            self.post_stream.wait_event(self.enc_done[k][h])
        with torch.cuda.stream(self.post_stream):
            if replay:
                post_g.replay()
                self.raw, self.images = self.raw_b[k], self.images_b[k]      # (what _post sets)
            else:
                self._post(k, masked)
            self.post_done[k].record()
        return self

    def _flags(self):
        """multispectral models: the first B images of the batch are optical, the last B thermal."""
        if not self.net.config.get('multispectral', False):
            return None
        return [True] * self.B + [False] * self.B

    def _stage_inputs(self, k, optical, thermal, mask_optical, mask_thermal):
        B, H, W = self.B, self.H, self.W
        img = self.images_b[k]
        masked = mask_optical is not None
        if masked and self.mask_b[k] is None:
            self.mask_b[k] = torch.empty((2 * B, H, W), dtype=torch.uint8, device=img.device)
        n = B * H * W

        def resident(t, dtype):
            return t.is_cuda and t.device == img.device and t.dtype == dtype and t.is_contiguous() and t.numel() == n
        if resident(optical, torch.float32) and resident(thermal, torch.float32) and \
                (not masked or (resident(mask_optical, torch.uint8) and resident(mask_thermal, torch.uint8))):
            # device-resident inputs: one launch instead of four runtime blits (a 9.8 MB image block takes the blit kernel 76 us)
            _lib.check(_lib.load().xp_stage_pair_batch(ptr(optical), ptr(thermal), ptr(img), ptr(mask_optical) if masked else None,
                                                       ptr(mask_thermal) if masked else None, ptr(self.mask_b[k]) if masked else None, n,
                                                       _lib.current_stream()), "xp_stage_pair_batch")
            return
        if (optical.dtype == torch.uint8) != (thermal.dtype == torch.uint8):
            # a uint8 image means "0..255 gray, divide by 255 on the device"; a float image means "already in [0, 1]".  One of each would put the two spectra
            # on different scales without any error: refuse it
            raise ValueError(f"PairPipeline: optical is {optical.dtype} and thermal is {thermal.dtype} — pass both images as uint8 (0..255, normalised on the "
                             "device) or both as float32 in [0, 1]")
        if optical.dtype == torch.uint8 and (optical.numel() != n or thermal.numel() != n):
            raise ValueError(f"PairPipeline: uint8 images must hold exactly {self.B} x {H} x {W} pixels each (got {optical.numel()} and {thermal.numel()})")
        if optical.dtype == torch.uint8:
            # 8-bit gray images (what a camera / decoder delivers): a quarter of the bytes over PCIe, gray / 255 on the device — the same f32 division the
            # reference's loader does on the host (xpoint/datasets/ImagePairDataset.py:254-274), so the staged images are the same bits
            if self._u8_b is None:
                self._u8_b = [torch.empty((2 * B, H, W), dtype=torch.uint8, device=img.device) for _ in range(self.depth)]
            u8 = self._u8_b[k]
            u8[:B].copy_(optical.reshape(B, H, W), non_blocking=True)
            u8[B:].copy_(thermal.reshape(B, H, W), non_blocking=True)
            _lib.check(_lib.load().xp_u8_to_unit_f32(ctypes.c_void_p(u8.data_ptr()), ptr(img), 2 * n, _lib.current_stream()), "xp_u8_to_unit_f32")
        else:
            img[:B].copy_(optical, non_blocking=True)           # host (pinned) inputs, other dtypes / layouts: the runtime's copy engines
            img[B:].copy_(thermal, non_blocking=True)
        if masked:
            self.mask_b[k][:B].copy_(mask_optical.reshape(B, H, W))
            self.mask_b[k][B:].copy_(mask_thermal.reshape(B, H, W))

    def _encode_group(self, k, h=None):
        """Enqueue the encoder + heads on image group h of buffer set k, on the current stream.  h=None, or a schedule with one group: the whole batch
        (also what the allocating first step of the split schedule and a range-guard repair run)."""
        fl = self._flags()
        whole = h is None or not self.split_encoder
        if whole:
            img, out, ws = self.images_b[k], self.raw_b[k], self.alt_ws[k] if self.alternate else None
        else:
            g = 2 * self.B // self.split_encoder
            sl = slice(h * g, (h + 1) * g)
            img, ws, fl = self.images_b[k][sl], self.group_ws[h], None if fl is None else fl[sl]
            out = {kk: (v[sl] if v is not None else None) for kk, v in self.raw_b[k].items()}      # the group writes into views of the full-batch outputs
        # check=False: stream-ordered, no host synchronisation here; the forward's status word is read in verify() / fetch() / download_async()
        self._note_engine()
        res = self.net.forward_raw(img, want_prob=True, want_desc=True, out=out, workspace=ws, is_optical=fl, check=False, status=self._status)
        if whole:
            self.raw_b[k] = res

    def _post(self, k, masked=False):
        B, H, W, n = self.B, self.H, self.W, 2 * self.B
        lib = _lib.load()
        st = _lib.current_stream()
        raw = self.raw_b[k]
        self.raw = raw
        self.images = self.images_b[k]
        prob = raw["prob"]
        thr = float(self.pred['detection_threshold'])
        if self.pred['nms'] > 0:
            if masked:          # the mask is applied on the NMS branch only, like predict_align_image_pair.py:194-205 (and predict_align_image_pair above)
                _lib.check(lib.xp_mul_mask(ptr(prob), ptr(self.mask_b[k]), ptr(self.prob_masked), n * H * W, st), "xp_mul_mask")
                prob = self.prob_masked
            _lib.check(lib.xp_box_nms(ptr(prob), ptr(self.prob_nms), ptr(self.nms_ws), self.nms_ws.numel(), n, H, W,
                                      float(self.pred['nms']), thr, 0.1, int(self.pred['topk']), self.cap, self.sweeps, None, st),
                       "xp_box_nms")
            prob = self.prob_nms
        _lib.check(lib.xp_extract_keypoints(ptr(prob), None, thr, ptr(self.kp), ptr(self.counts), n, H, W, self.cap, ptr(self.kp_ws),
                                            self.kp_ws.numel(), st),
                   "xp_extract_keypoints")
        d = raw["desc_nhwc"]
        _lib.check(lib.xp_sample_descriptors(ptr(self.kp), ptr(self.counts), ptr(d), ptr(self.desc), n, self.cap, d.shape[1],
                                             d.shape[2], self.D, H, W, st), "xp_sample_descriptors")
        m = self.m
        _lib.check(lib.xp_match_mnn(ptr(self.desc[:B]), ptr(self.desc[B:]), ptr(self.counts), 1, 0, B, B, self.cap, self.cap, self.D,
                                    utils.MATCH_MODES[self.mode], ptr(m["idx12"]), ptr(m["dist12"]), ptr(m["idx21"]), ptr(m["dist21"]),
                                    ptr(m["match_q"]), ptr(m["match_t"]), ptr(m["match_d"]), ptr(m["match_count"]),
                                    ptr(self.match_ws), self.match_ws.numel(), st), "xp_match_mnn")
        if self.estimate_homography:
            h = self.hg
            _lib.check(lib.xp_gather_match_points(ptr(self.kp), ptr(m["match_q"]), ptr(m["match_t"]), ptr(m["match_count"]), B, self.cap,
                                                  ptr(h["src"]), ptr(h["dst"]), st), "xp_gather_match_points")
            _lib.check(lib.xp_find_homography(ptr(h["src"]), ptr(h["dst"]), ptr(m["match_count"]), B, self.cap,
                                              float(self.pred.get('reprojection_threshold', 3.0)), self.ransac_iters, 0, ptr(h["H"]), ptr(h["mask"]),
                                              ptr(h["n_inliers"]), ptr(h["ws"]), h["ws"].numel() * 8, st), "xp_find_homography")
            if self.warp_optical:
                # masked steps: the optical image times its mask, quantised (predict_align_image_pair.py:267-271) — by the warp's load, so the staged
                # images stay unmasked (a range-guard repair re-encodes the latest step from them, _settle_engine)
                _lib.check(lib.xp_warp_perspective_masked(ptr(self.images_b[k]), ctypes.c_void_p(self.mask_b[k].data_ptr()) if masked else None,
                                                          ctypes.c_void_p(h["warped"].data_ptr()), ctypes.c_void_p(h["H"].data_ptr()),
                                                          B, H, W, H, W, 1, 1, 2, 0, st), "xp_warp_perspective_masked")
        return self

    def match_stats(self):
        """Nomination statistics of the latest step's matcher call (xp_match_stats): what its run time depends on (clustered descriptors nominate
        more), never its result.  Synchronises."""
        with torch.cuda.device(self.device):
            torch.cuda.synchronize()
            lib = _lib.load()
            out = torch.zeros(4, dtype=torch.int64, device=self.device)
            _lib.check(lib.xp_match_stats(ptr(self.match_ws), ptr(self.counts), 1, 0, self.B, self.B, self.cap, self.cap, self.D, ptr(out),
                                          _lib.current_stream()), "xp_match_stats")
            s, mx, ov, rows = (int(v) for v in out.cpu())
        return dict(mean=round(s / max(rows, 1), 3), max=mx, overflow_rows=ov, rows=rows, inline_capacity=int(lib.xp_match_cand_cap()))

    def wait(self):
        """Make the caller's current stream wait for everything run() has enqueued so far (overlapped mode: the
        detection / matching stream); after it, stream-ordered reads of the result tensors are safe."""
        if self.overlap and self._call:
            torch.cuda.current_stream().wait_event(self.post_done[(self._call - 1) % self.depth])
        return self

    def capture(self, optical, thermal, mask_optical=None, mask_thermal=None):
        """Capture the step into hipGraphs (fixed shapes, preallocated buffers) and return a replay callable that takes the same
        arguments as run().  The input copies stay outside the graphs (so the caller may pass different tensors, e.g. pinned
        host memory, at every replay).
        One stream: one graph of encoder + detection + matching.  Overlapped pipeline: per output buffer (two of them), one
        graph per encoder image group and one for the detection / matching kernels, each replayed on its own stream and
        chained by the same events as the eager schedule — the cross-step overlap survives capture.
        Masks: the graphs are captured with or without the masking kernel, as the capture call is; every replay must match that
        (both masks when captured with masks — new ones at every replay are fine — neither when captured without) and raises
        ValueError otherwise, instead of ignoring the masks or applying those staged by an earlier step.  Capture a second pipeline
        for the other case."""
        with torch.cuda.device(self.device):
            for _ in range(self.depth):                         # warm-up outside capture: one-time allocations, every buffer set
                self._step(optical, thermal, mask_optical, mask_thermal)
            torch.cuda.synchronize()
            self._settle_engine()                               # a range-guard trip during warm-up switches the engine BEFORE anything is captured
            self._capture_masked = mask_optical is not None
            self._capture_graphs()

        def replay(optical, thermal, mask_optical=None, mask_thermal=None):
            self._check_replay_masks(mask_optical, mask_thermal)
            with torch.cuda.device(self.device):
                return self._step(optical, thermal, mask_optical, mask_thermal, replay=True)
        return replay

    def _check_replay_masks(self, mask_optical, mask_thermal):
        if (mask_optical is None) != (mask_thermal is None):
            raise ValueError("PairPipeline replay: pass both valid masks or neither")
        if (mask_optical is not None) != self._capture_masked:
            raise ValueError("PairPipeline replay: the graphs were captured " + ("with" if self._capture_masked else "without") +
                             " valid masks and this replay passes " + ("none" if self._capture_masked else "masks") +
                             " — a replay cannot change whether the step masks; capture another pipeline for that")

    def _streams_of(self, k):
        return self.enc_streams if self.split_encoder else [self.enc_streams[k] if self.alternate else self.enc_stream]

    def _capture_graphs(self):
        """(Re)capture the step's graphs with the dense engine in force now; buffers exist (warm-up done), device synchronised."""
        masked = self._capture_masked
        self._graph_engine = self.net.effective_gemm_mode()     # what every replay enqueues (_note_engine)
        pend = self._h2_pending
        if not self.overlap:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._encode_group(0)
                self._post(0, masked)
            self._graphs = g
            self._h2_pending = pend                             # (capturing enqueues nothing)
            return
        graphs = []
        for k in range(self.depth):
            enc_g = []
            for h, stream in enumerate(self._streams_of(k)):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=stream):
                    self._encode_group(k, h)
                enc_g.append(g)
            pg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(pg, stream=self.post_stream):
                self._post(k, masked)
            graphs.append((enc_g, pg))
        self._graphs = graphs
        self._h2_pending = pend                                 # (capturing enqueues nothing)
        torch.cuda.synchronize()

    def status_word(self):
        """This pipeline's OWN forward status word (int32[1] on its device): its forwards OR their XP_STATUS_* bits into it and only its own
        verify() / fetch() reads and clears it — another pipeline on the same model, or an eager forward, cannot consume a trip raised by a step
        that is still in flight here."""
        return self._status

    def _note_engine(self, engine=None):
        """Record the dense engine of the forwards this pipeline enqueues (eager: the model's engine now; graph replay: the engine the graphs were
        captured on): a status trip is judged against THAT engine, not against whatever the shared model has been switched to since (_settle_engine)."""
        if engine is None:
            engine = self.net.effective_gemm_mode()
        if engine == "h2":
            self._h2_pending = True
        self._engine_enqueued = engine

    def _settle_engine(self):
        """After a device-wide synchronisation: read and clear the forward status word.  Non-zero on the split-fp16 engine = an operand left
        the fp16 range: the model switches to "x3" for this weight set (warning), captured graphs are re-captured on it, and the latest call
        is computed again from its staged inputs — the results the caller reads next are never the overflowed ones.  Non-zero on any other
        engine raises (models.XPoint.handle_status).  Returns True when it re-ran."""
        word = self._status
        st = take_status(word)
        if st == 0:
            self._h2_pending = False                           # (device-wide synchronisation done: nothing enqueued on h2 is still in flight)
            return False
        # judged against the engine the pending forwards were enqueued with (some step in flight on "h2" -> recoverable, even when another user of
        # the same model has already switched it to "x3"); raises unless the h2 -> x3 switch applies
        pending = "h2" if self._h2_pending else self._engine_enqueued
        self._h2_pending = False
        retry = None
        if self._last is not None:
            def retry():          # the latest call's forward again (eager, from its staged inputs) on the model's current settings -> its status
                self._encode_group(self._last[0])
                torch.cuda.synchronize()
                return take_status(word)
        # round 6: on "h2" the model first tries to LOCALISE the trip (only the out-of-range launches move to the x3 planes) before giving up the engine
        self.net.handle_status(st, "PairPipeline", pending, retry=retry)
        self._h2_pending = False                               # (the localisation's forwards were synchronised and read by retry())
        if self._graphs is not None:
            self._capture_graphs()
        if self._last is not None:
            k, masked = self._last
            self._encode_group(k)
            self._post(k, masked)
            torch.cuda.synchronize()
            self._h2_pending = False
            self.net.handle_status(take_status(word), "PairPipeline, second run")
        return True

    def download_async(self):
        """Streaming use: enqueue — right behind the detection / matching kernels of the last run() / replay — the copies of its result
        lists (keypoint counts and coordinates, match counts and index lists, distances; the homography fields when estimated) into
        pinned host buffers, and return (buffers, event).  The buffers are valid after event.synchronize(); the NEXT run() may be enqueued
        before that, so the device-to-host traffic of step i overlaps the steps behind it (`self.host_sets` = depth + 1 buffer sets rotate: a caller
        may keep `depth` steps in flight and must consume a set before the host_sets-th call after it).  The copies are ordered on the stream that
        writes the results, ahead of the next step's kernels."""
        with torch.cuda.device(self.device):
            if self._host is None:
                def pin(t):
                    return torch.empty(t.shape, dtype=t.dtype, device="cpu").pin_memory()
                src = dict(counts=self.counts, kp=self.kp, match_count=self.m["match_count"], match_q=self.m["match_q"], match_t=self.m["match_t"],
                           match_d=self.m["match_d"])
                src["status"] = self._status                               # XP_STATUS_* bits of THIS pipeline's forwards so far: non-zero = call verify()
                if self.estimate_homography:
                    src.update(H_est=self.hg["H"], n_inliers=self.hg["n_inliers"], matchesMask=self.hg["mask"])
                self._host_src = src
                self._host = [{k: pin(v) for k, v in src.items()} for _ in range(self.host_sets)]
                self._host_ev = [torch.cuda.Event() for _ in range(self.host_sets)]
            i = self._host_i
            self._host_i = (i + 1) % self.host_sets
            stream = self.post_stream if self.overlap else torch.cuda.current_stream()
            with torch.cuda.stream(stream):
                for k, v in self._host_src.items():
                    self.copy_to_pinned(v, self._host[i][k])
                self._host_ev[i].record()
            return self._host[i], self._host_ev[i]

    def copy_to_pinned(self, v, h):
        """Enqueue the copy of device tensor v into pinned host tensor h on the current stream.
        By a kernel, not by the copy engines: a device-to-host copy queued behind this step's kernels would hold up the NEXT steps' image
        uploads in the engines' queue (xp_copy_to_mapped_host; bench.py's streaming loop: 1 553 -> see profiles/r5_streaming_parts.txt).  Tensors the
        kernel does not take (non-contiguous, empty, not 16-byte aligned) and XP_D2H_COPY_ENGINE=1 (A/B) go through the runtime's copy."""
        if v.is_contiguous() and v.numel() > 0 and v.data_ptr() % 16 == 0 and h.data_ptr() % 16 == 0 and not self._copy_engine_d2h:
            _lib.check(_lib.load().xp_copy_to_mapped_host(ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(h.data_ptr()), v.numel() * v.element_size(),
                                                          _lib.current_stream()), "xp_copy_to_mapped_host")
        else:
            h.copy_(v, non_blocking=True)

    def verify(self):
        """After a synchronisation point: the async NMS must have reached its fixed point and no list may have
        overflowed its capacity.  Raises otherwise (the caller can re-run with more sweeps / capacity).  Also settles the dense engine's
        range guard (see _settle_engine): never raises for an fp16-range overflow, falls back instead."""
        lib = _lib.load()
        # range guard of the split-fp16 dense engine (include/xpoint_hip.h, xp_xpoint_forward_ex): the forwards' status word.  A trip re-runs the
        # latest call on "x3" (and keeps that engine), so the checks below — and the caller — see the repaired results.
        # SCOPE of the repair: only the LATEST call (self._last) is recomputed; earlier calls still in flight when the guard tripped (depth 2-3
        # bursts, streaming) ran on the overflowed engine and are NOT recomputed — a caller that keeps several steps in flight must treat every step
        # since its last verify() as suspect.  Host buffers already filled by download_async() are stale after a repair: `self.repaired` is set and the
        # caller must call download_async() again for the latest step (bufs["status"] != 0 is the trigger, see download_async).
        self.repaired = self._settle_engine()
        if self.pred['nms'] > 0:
            left = c_i(-1)
            _lib.check(lib.xp_box_nms_check(ptr(self.nms_ws), 2 * self.B, self.H, self.W, ctypes.byref(left), _lib.current_stream()),
                       "xp_box_nms_check")
            while left.value != 0:
                # The stream-ordered NMS enqueues a fixed number of sweeps (sweeps past the fixed point exit at once); an image whose suppression
                # chains need more is NOT an error of the data: raise the count (kept for later calls), recompute the latest call's detection /
                # matching stages from its encoder outputs, and check again — the caller never sees a half-converged heat map.
                if self.sweeps >= 64 or self._last is None:
                    raise RuntimeError(f"PairPipeline: NMS not converged after {self.sweeps} sweeps ({left.value} tiles undecided)")
                import warnings
                warnings.warn(f"PairPipeline: NMS needed more than {self.sweeps} sweeps ({left.value} tiles undecided); re-running the step's "
                              f"post-processing with {min(64, 2 * self.sweeps)} and keeping that count", RuntimeWarning, stacklevel=2)
                self.sweeps = min(64, 2 * self.sweeps)
                if self._graphs is not None:
                    self._capture_graphs()
                k, masked = self._last
                self._post(k, masked)
                torch.cuda.synchronize()
                _lib.check(lib.xp_box_nms_check(ptr(self.nms_ws), 2 * self.B, self.H, self.W, ctypes.byref(left), _lib.current_stream()),
                           "xp_box_nms_check")
        mx = int(self.counts.max().item())
        if mx > self.cap:
            raise RuntimeError(f"PairPipeline: {mx} keypoints exceed capacity {self.cap}")

    def fetch(self):
        torch.cuda.synchronize()        # device-wide: covers both streams of the overlapped mode
        self.verify()
        B = self.B
        counts = self.counts.cpu().numpy()
        mc = self.m["match_count"].cpu().numpy()
        out = []
        for i in range(B):
            no, nt, nm = int(counts[i]), int(counts[B + i]), int(mc[i])
            extra = {}
            if self.estimate_homography:
                extra = dict(H_est=self.hg["H"][i].cpu().numpy(), matchesMask=self.hg["mask"][i, :nm].cpu().numpy(),
                             n_inliers=int(self.hg["n_inliers"][i].item()))
                if self.warp_optical:
                    extra["warped_optical"] = self.hg["warped"][i].cpu()
            out.append(dict(extra, kp_optical=self.kp[i, :no].cpu().long(), kp_thermal=self.kp[B + i, :nt].cpu().long(),
                            desc_optical=self.desc[i, :no].cpu(), desc_thermal=self.desc[B + i, :nt].cpu(),
                            match_q=self.m["match_q"][i, :nm].cpu().numpy(), match_t=self.m["match_t"][i, :nm].cpu().numpy(),
                            match_d=self.m["match_d"][i, :nm].cpu().numpy(),
                            idx12=self.m["idx12"][i, :no].cpu().numpy(), idx21=self.m["idx21"][i, :nt].cpu().numpy()))
        return out
