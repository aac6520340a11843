"""training.Adam: torch.optim.Adam (L2 weight decay, amsgrad off) as three kinds of launch of the HIP library (csrc/optim.hip),
with an optional global-norm clip and a DEVICE-SIDE guard against non-finite gradients.

    optimizer = training.Adam(model.parameters(), lr=1e-4, weight_decay=5e-4)
    loss, components = training.train_step(model, data, loss_fn, optimizer, seed=step)
    optimizer.last_step()          # {'grad_norm', 'skipped', 'step', 'skipped_steps'}: ONE synchronisation, on demand only

A step is: xp_optim_grad_sumsq (one f64 partial per workgroup, fixed slots), xp_optim_step_header (one workgroup: norm^2, finite, clip
coefficient, the step counter and both bias corrections in a 64-byte device record), xp_optim_adam_apply (reads the record; when the norm is not
finite and `skip_nonfinite` holds it writes nothing, so parameters and moments keep their bits and the counter does not advance).  step() never
reads anything back.  The pointer tables travel by value in the kernel arguments, 64 tensors per launch, and are rebuilt every step from the current
`.grad`s, so `zero_grad(set_to_none=True)` stays the cheap path.

Both moments live in two flat f32 buffers; `state[p]['exp_avg']` / `['exp_avg_sq']` are views into them and `state_dict()` has torch.optim.Adam's
layout, so either optimiser loads the other's.  Differences from torch.optim.Adam, all stated: ONE step counter for every parameter (torch keeps
one per parameter; they differ only for a parameter that has had no gradient in some step); one parameter group; float32 parameters on one GPU; no
amsgrad, maximize, capturable, foreach or fused switches.  No CPU fallback."""
import ctypes
import math

import torch

from .. import _lib

_HEADER_WORDS = 8          # f64 norm2, bc1, bc2, clip_coef | i64 t, skipped, finite, applied


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_norm=None, skip_nonfinite=True):
        if not 0.0 <= float(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_norm is not None and not max_norm > 0.0:
            raise ValueError(f"Invalid max_norm value: {max_norm} (None switches clipping off)")
        # the keys torch.optim.Adam's groups carry, with the values this class fixes, so that a state_dict moves between the two
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None, capturable=False,
                        differentiable=False, fused=None, max_norm=max_norm, skip_nonfinite=bool(skip_nonfinite))
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError("training.Adam: one parameter group only")
        self._params = list(self.param_groups[0]['params'])
        for p in self._params:          # CPU parameters are refused by step(): the state (and its exchange with torch.optim.Adam) needs no GPU
            if p.dtype != torch.float32 or p.device != self._params[0].device or not p.is_contiguous():
                raise TypeError("training.Adam: parameters must be contiguous float32 tensors on one device")
        self._flat = None

    # ---- the flat state
    def _init_state(self):
        """The two flat moment buffers, the header record and the norm workspace: once, at the first step or load.  Tensors whose size is a multiple
        of four floats come first, so that one odd-sized tensor does not push every later one off the 16-byte path."""
        if self._flat is not None:
            return
        dev = self._params[0].device
        order = sorted(range(len(self._params)), key=lambda i: self._params[i].numel() % 4 != 0)
        offsets, total = {}, 0
        for i in order:
            offsets[i] = total
            total += self._params[i].numel()
        lib = _lib.load()
        self._exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self._exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        self._header = torch.zeros(_HEADER_WORDS, dtype=torch.float64, device=dev)
        assert int(lib.xp_optim_header_bytes()) == 8 * _HEADER_WORDS
        self._workspace = torch.empty(max(int(lib.xp_optim_workspace_bytes(len(self._params), total)), 256), dtype=torch.uint8, device=dev)
        self._total = total
        self._offsets = [offsets[i] for i in range(len(self._params))]
        self._flat = True
        for i, p in enumerate(self._params):
            o, n = self._offsets[i], p.numel()
            self.state[p] = {'step': torch.tensor(0.0, dtype=torch.float32), 'exp_avg': self._exp_avg[o:o + n].view_as(p),
                             'exp_avg_sq': self._exp_avg_sq[o:o + n].view_as(p)}

    def _read_header(self):
        """The record on the host (one synchronisation)."""
        f = self._header.cpu()
        i = f.view(torch.int64)
        return {'norm2': float(f[0]), 'bc1': float(f[1]), 'bc2': float(f[2]), 'clip_coef': float(f[3]), 't': int(i[4]), 'skipped': int(i[5]),
                'finite': bool(i[6]), 'applied': bool(i[7])}

    # ---- the step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        if len(self.param_groups) != 1 or len(group['params']) != len(self._params) or any(a is not b for a, b in zip(group['params'], self._params)):
            raise ValueError("training.Adam: one parameter group, with the parameters it was built with")
        if not self._params[0].is_cuda:
            raise _lib.XPointHipError("training.Adam: parameters must live on the GPU (xpoint_amd has no CPU fallback)")
        self._init_state()
        ps, gs, offs, ns, keep = [], [], [], [], []
        for i, p in enumerate(self._params):
            g = p.grad
            if g is None:
                continue
            if g.is_sparse or g.dtype != torch.float32 or g.device != p.device:
                raise TypeError("training.Adam: gradients must be dense float32 tensors on the parameters' device")
            if not g.is_contiguous():
                g = g.contiguous()          # one copy; the table holds its pointer until the launches below are enqueued
                keep.append(g)
            ps.append(p.data_ptr()); gs.append(g.data_ptr()); offs.append(self._offsets[i]); ns.append(p.numel())
        if not ps:
            return loss
        n = len(ps)
        vp, vl = ctypes.c_void_p * n, ctypes.c_int64 * n
        c_p, c_g, c_o, c_n = vp(*ps), vp(*gs), vl(*offs), vl(*ns)
        beta1, beta2 = group['betas']
        max_norm = group['max_norm']
        dev = self._params[0].device
        stream = _lib.current_stream(dev)
        parts = ctypes.c_int64(0)
        ws, hdr = ctypes.c_void_p(self._workspace.data_ptr()), ctypes.c_void_p(self._header.data_ptr())
        with torch.cuda.device(dev):
            _lib.call("xp_optim_grad_sumsq", c_g, c_n, n, ws, ctypes.c_size_t(self._workspace.numel()), ctypes.byref(parts), stream)
            _lib.call("xp_optim_step_header", ws, parts.value, hdr, float(beta1), float(beta2), 0.0 if max_norm is None else float(max_norm),
                      int(bool(group['skip_nonfinite'])), stream)
            _lib.call("xp_optim_adam_apply", c_p, c_g, c_o, c_n, n, ctypes.c_void_p(self._exp_avg.data_ptr()),
                      ctypes.c_void_p(self._exp_avg_sq.data_ptr()), self._total, hdr, float(group['lr']), float(group['weight_decay']), float(beta1),
                      float(beta2), float(group['eps']), stream)
        return loss

    def last_step(self):
        """What the last step() did, read from the device record: {'grad_norm': the global L2 norm of the gradients BEFORE clipping (inf / nan when a
        gradient was not finite), 'skipped': the step was not applied, 'step': steps applied so far, 'skipped_steps': steps not applied so far}.
        One synchronisation: call it on demand, not every step."""
        self._init_state()
        h = self._read_header()
        return {'grad_norm': math.sqrt(h['norm2']) if h['norm2'] >= 0.0 else float('nan'), 'skipped': not h['applied'] and (h['t'] + h['skipped']) > 0,
                'step': h['t'], 'skipped_steps': h['skipped']}

    # ---- torch.optim.Adam's state layout, both ways
    def state_dict(self):
        if self._flat is not None:
            t = float(self._read_header()['t'])
            for p in self._params:
                self.state[p]['step'] = torch.tensor(t, dtype=torch.float32)
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)          # casts the moments to the parameters' device and dtype; replaces self.state
        if len(self.param_groups) != 1 or len(self.param_groups[0]['params']) != len(self._params):
            raise ValueError("training.Adam: one parameter group only")
        group = self.param_groups[0]
        for k, v in self.defaults.items():          # a torch.optim.Adam state_dict has no max_norm / skip_nonfinite
            group.setdefault(k, v)
        if group.get('amsgrad') or group.get('maximize'):
            raise ValueError("training.Adam: a state with amsgrad or maximize set is not supported")
        self._params = list(group['params'])
        loaded = dict(self.state)
        self._flat = None
        self.state.clear()
        self._init_state()
        steps = set()
        for p in self._params:
            st = loaded.get(p)
            if not st:          # torch holds no state for a parameter that never had a gradient: zero moments
                continue
            if st['exp_avg'].shape != p.shape or st['exp_avg_sq'].shape != p.shape:
                raise ValueError("training.Adam: a loaded moment does not have its parameter's shape")
            self.state[p]['exp_avg'].copy_(st['exp_avg'])
            self.state[p]['exp_avg_sq'].copy_(st['exp_avg_sq'])
            steps.add(int(round(float(st['step']))))
        if len(steps) > 1:
            raise ValueError(f"training.Adam keeps ONE step counter; the loaded state holds several ({sorted(steps)})")
        t = steps.pop() if steps else 0
        self._header.view(torch.int64)[4] = t
        for p in self._params:
            self.state[p]['step'] = torch.tensor(float(t), dtype=torch.float32)
