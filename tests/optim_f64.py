"""A numpy float64 restatement of the optimiser step of xpoint_amd.training.Adam (csrc/optim.hip): global gradient norm, clip coefficient, the skip
of a non-finite step, torch's Adam with L2 weight decay.  tests/test_cpu_optim.py pins it against torch.optim.Adam run in float64 on the CPU (with
torch.nn.utils.clip_grad_norm_ in front when clipping); tests/test_gpu_optim.py pins the kernels against it.  Nothing here calls the library."""
import numpy as np

# element counts of the tensors of the shared case: one element, below / at / above one 16-byte group, an odd count, the three around 4096, and one
# just over one workgroup's span of 8192 elements (two workgroups, the second with a single element)
SIZES = (1, 3, 4, 5, 65, 4095, 4096, 4097, 8193)
MANY = (300, 7)          # more tensors than one kernel-argument table of 64 holds; every flat offset but each fourth is off the 16-byte grid
STEPS = 5


def uniform(name, n, lo=-1.0, hi=1.0):
    """n float32-representable values in [lo, hi), keyed by name (the same on every machine)."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return (rng.random(n) * (hi - lo) + lo).astype(np.float32)


def case(sizes=SIZES, steps=STEPS, tag="optim"):
    """(parameters, [gradients of step 1, ...]) as lists of float32 arrays: what both the restatement and the kernels start from."""
    params = [uniform(f"{tag}/p{i}/{n}", n) for i, n in enumerate(sizes)]
    grads = [[uniform(f"{tag}/g{s}/{i}/{n}", n, -0.1, 0.1) for i, n in enumerate(sizes)] for s in range(steps)]
    return params, grads


class AdamF64:
    """The state of the restatement: parameters, both moments and the step counter, float64."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None, skip_nonfinite=True):
        self.p = [np.asarray(p, np.float64).copy() for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.t, self.skipped = 0, 0
        self.lr, self.betas, self.eps, self.wd, self.max_norm, self.skip_nonfinite = lr, betas, eps, weight_decay, max_norm, skip_nonfinite
        self.grad_norm = None

    def step(self, grads):
        """grads: one array or None per parameter.  Returns True when the step was applied."""
        live = [i for i, g in enumerate(grads) if g is not None]
        with np.errstate(invalid="ignore", over="ignore"):
            norm2 = float(sum(np.sum(np.asarray(grads[i], np.float64) ** 2) for i in live))
        self.grad_norm = float(np.sqrt(norm2)) if norm2 >= 0.0 else float("nan")
        if not np.isfinite(norm2) and self.skip_nonfinite:
            self.skipped += 1
            return False
        clip = 1.0 if self.max_norm is None else min(1.0, self.max_norm / (np.sqrt(norm2) + 1e-6))
        self.t += 1
        b1, b2 = self.betas
        bc1, bc2 = 1.0 - b1 ** self.t, 1.0 - b2 ** self.t
        for i in live:
            g = clip * np.asarray(grads[i], np.float64) + self.wd * self.p[i]
            self.m[i] = b1 * self.m[i] + (1.0 - b1) * g
            self.v[i] = b2 * self.v[i] + (1.0 - b2) * g * g
            self.p[i] = self.p[i] - (self.lr / bc1) * self.m[i] / (np.sqrt(self.v[i]) / np.sqrt(bc2) + self.eps)
        return True
