"""Cases for the tests of the torch-evaluated callback route: `_GenericHMC` (hamiltorch_amd/samplers.py) and the state kernels of
csrc/hmc_pieces.hip.  Plain numpy, no GPU.  Shared by tests/test_generic_cases_cpu.py (which checks everything the GPU tests rely on),
tests/test_gpu_pieces.py (the kernels one by one through hamiltorch_amd/_abi.py) and tests/test_gpu_generic.py (the engine).

TARGETS are numpy twins with batched `logp(theta)` / `grad(theta)` whose arithmetic follows theta's dtype and calls no BLAS (every sum
is numpy's pairwise sum over a contiguous last axis, so the float32 figures do not depend on the BLAS at hand), each with a torch
closure over device tensors (`closure(dtype, device)`) that no recogniser of the library can see through.

BOUNDS.  float64: 1e-12 relative to the data's scale for one kernel, 1e-9 end to end with 3 % of the chains exempt (a flipped accept
decision) - the project's bounds.  float32, one kernel: 4 x the distance of the SAME numpy formula evaluated in float32 from its
float64 value on the same float32 inputs, at least 4 ulp of the case's scale (`f32_bound`); the distances are recorded in
F32_PIECES and measured again by the CPU tests.  float32, end to end: 4 x the largest difference of the float32 oracle from the
float64 oracle on the chains that kept their accept decisions, at least 2e-6 (`Run.bound`); the differences are recorded in
F32_ORACLE_ERR and measured again by the CPU tests.  Nothing here is fitted to what a GPU returned."""
import math

import numpy as np
import torch

import hmc_oracle as O

NP = {torch.float32: np.float32, torch.float64: np.float64}
TAG = {torch.float64: "f64", torch.float32: "f32"}
F64_PIECE, F64_RUN = 1e-12, 1e-9
BAND_F32 = 2e-4                     # the project's end-to-end band in float32 (the funnel rows, see Run.bound)
MAX_FLIPPED = 0.03
ULP32 = float(np.finfo(np.float32).eps)


def rand_spd(D, seed, lo=0.5, hi=1.5):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    P = (Q * np.linspace(lo, hi, D)) @ Q.T
    return 0.5 * (P + P.T)


def matvec(x, A):
    """x[..., D] -> (A x)[..., D] = x @ A.T without BLAS: products summed over the contiguous last axis in numpy's pairwise order."""
    if x.ndim == 2 and x.shape[0] * A.size > (1 << 24):          # a large batch in slices: the same sums, less memory
        return np.concatenate([matvec(x[i:i + 64], A) for i in range(0, x.shape[0], 64)])
    return (x[..., None, :] * A).sum(-1)


def _t(a, dtype, device):
    return torch.tensor(np.asarray(a), dtype=dtype, device=device)


# ---- targets ---------------------------------------------------------------------------------------------------------------------------
class DenseGaussian:
    """log p = -1/2 (theta - mu)^T P (theta - mu): a random SPD precision with eigenvalues in [0.5, 1.5] (D = 1: P = 1.3), mu != 0."""

    def __init__(self, D, seed=0):
        self.D = D
        self.P = rand_spd(D, 100 + seed) if D > 1 else np.array([[1.3]])
        self.mu = 0.2 * np.random.default_rng(200 + seed).standard_normal(D)

    def logp(self, th):
        d = th - self.mu.astype(th.dtype)
        return (th.dtype.type(-0.5) * (d * matvec(d, self.P.astype(th.dtype))).sum(-1)).astype(th.dtype)

    def grad(self, th):
        return -matvec(th - self.mu.astype(th.dtype), self.P.astype(th.dtype))

    def closure(self, dtype, device):
        P, mu = _t(self.P, dtype, device), _t(self.mu, dtype, device)

        def f(w):
            d = w - mu
            return -0.5 * (d * (P @ d)).sum()
        return f

    def grad_closure(self, dtype, device):
        """The gradient as a callable of its own (what `pass_grad` takes)."""
        P, mu = _t(self.P, dtype, device), _t(self.mu, dtype, device)
        return lambda w: -(P @ (w - mu))


class Funnel(O.FunnelTarget):
    """The oracle's 11-D funnel (unit scales) with the closure of the reference's notebook."""

    def __init__(self, D=11):
        super().__init__(D)

    def logp(self, th):
        return super().logp(th).astype(th.dtype)

    def grad(self, th):
        return super().grad(th).astype(th.dtype)

    def closure(self, dtype, device):
        hl2p = 0.5 * math.log(2.0 * math.pi)

        def f(w):
            v, x = w[0], w[1:]
            return (-v * v / 18.0 - math.log(3.0) - hl2p) + (-0.5 * torch.exp(v) * (x * x).sum() + 0.5 * x.numel() * v - x.numel() * hl2p)
        return f


class Ball:
    """log p = -|theta|^2 / 2 inside the ball |theta|^2 < R^2 and NaN outside it (gradient 0 there): a proposal that ends outside is
    non-finite and must be a rejection for that chain only."""

    def __init__(self, D=4, R=2.5):
        self.D, self.R2 = D, R * R

    def logp(self, th):
        r2 = (th * th).sum(-1)
        return np.where(r2 < self.R2, th.dtype.type(-0.5) * r2, np.nan).astype(th.dtype)

    def grad(self, th):
        r2 = (th * th).sum(-1)
        return np.where((r2 < self.R2)[..., None], -th, 0).astype(th.dtype)

    def closure(self, dtype, device):
        R2 = self.R2

        def f(w):
            r2 = (w * w).sum()
            return torch.where(r2 < R2, -0.5 * r2, torch.full_like(r2, float("nan")))
        return f


class Branching:
    """log p = -|theta|^2 / 2 - [theta_0 < 0] theta_0^4 / 4, written with a Python `if` on the argument: torch.func.vmap refuses it and
    the engine evaluates it chain by chain."""

    def __init__(self, D=4):
        self.D = D

    def logp(self, th):
        t0 = th[..., 0]
        return (th.dtype.type(-0.5) * (th * th).sum(-1) - np.where(t0 < 0, th.dtype.type(0.25) * t0 ** 4, 0)).astype(th.dtype)

    def grad(self, th):
        g = -th.copy()
        g[..., 0] -= np.where(th[..., 0] < 0, th[..., 0] ** 3, 0)
        return g

    def closure(self, dtype, device):
        def f(w):
            if w[0] < 0:
                return -0.5 * (w * w).sum() - 0.25 * w[0] ** 4
            return -0.5 * (w * w).sum()
        return f


class Mixed:
    """log p of one target, gradient of another: what sample(pass_grad=...) integrates (S:61-63).  `grad_of` is a target or a constant
    vector (a tensor `pass_grad`)."""

    def __init__(self, logp_of, grad_of):
        self.logp_of, self.grad_of = logp_of, grad_of

    def logp(self, th):
        return self.logp_of.logp(th)

    def grad(self, th):
        if isinstance(self.grad_of, np.ndarray):
            return np.broadcast_to(self.grad_of.astype(th.dtype), th.shape).copy()
        return self.grad_of.grad(th)


# ---- mass matrices ---------------------------------------------------------------------------------------------------------------------
MASSES = ("none", "diag", "full")
KIND = {"none": 0, "diag": 1, "full": 2, "nonsym": 2}


def inv_mass(mass, D, dtype=np.float64):
    """none | diag: uniform(0.5, 2) | full: random SPD, eigenvalues in [0.5, 1.5] | nonsym: that plus a strictly upper triangle of
    N(0, 0.3^2) - NOT a mass matrix, for the kick/drift kernel alone: the oracle's M^-1 p is p @ inv_mass.T, and the transposed
    index gives other numbers."""
    rng = np.random.default_rng(7000 + D)
    diag = rng.uniform(0.5, 2.0, D)
    if mass == "none":
        return None
    if mass == "diag":
        return diag.astype(dtype)
    full = rand_spd(D, 7 + D)
    if mass == "nonsym":
        full = full + np.triu(0.3 * rng.standard_normal((D, D)), 1)
    return full.astype(dtype)


# ---- kernel-level cases (tests/test_gpu_pieces.py) ---------------------------------------------------------------------------------------
PIECE_D = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 130, 257)      # every lane-group size 1 .. 64, a ragged and a full last pass
PIECE_C = (1, 37, 70)                                                        # C G is no multiple of the 256-thread block
FULL_MAX_D = 130
KICK, DRIFT = 0.35, 0.6


def piece_inputs(D, C=70, dtype=np.float64):
    """theta, p, grad ~ N(0, 1) and log p ~ N(0, D) for C chains: rounded to `dtype` first, so that both dtypes' references start from
    the numbers the kernel gets.  The first C' < C rows are the inputs of the smaller batch."""
    rng = np.random.default_rng(9000 + D)
    x = {k: rng.standard_normal((70, D)) for k in ("theta", "p", "grad")}
    x["logp"] = math.sqrt(D) * rng.standard_normal(70)
    if C > 70:
        rng = np.random.default_rng(9500 + D + C)
        x = {k: rng.standard_normal((C, D)) for k in ("theta", "p", "grad")}
        x["logp"] = math.sqrt(D) * rng.standard_normal(C)
    return {k: v[:C].astype(dtype) for k, v in x.items()}


def ref_hamiltonian(x, im, with_logp, dt):
    """O.hmc_hamiltonian's arithmetic (O.kinetic) in `dt`, M^-1 p without BLAS."""
    p = x["p"].astype(dt)
    v = p if im is None else (im.astype(dt) * p if im.ndim == 1 else matvec(p, im.astype(dt)))
    kin = dt(0.5) * (p * v).sum(-1)
    return ((-x["logp"].astype(dt) if with_logp else 0) + kin).astype(dt)


def ref_kick_drift(x, im, kick, drift, with_grad, dt):
    """One explicit step of S:281-298: p += kick grad, then theta += drift M^-1 p (the updated p)."""
    th, p = x["theta"].astype(dt), x["p"].astype(dt)
    if with_grad:
        p = p + dt(kick) * x["grad"].astype(dt)
    if drift != 0:
        v = p if im is None else (im.astype(dt) * p if im.ndim == 1 else matvec(p, im.astype(dt)))
        th = th + dt(drift) * v
    return th, p


def normals32(seed, chain_ids, draw, D):
    """O.philox_normals with the Box-Muller arithmetic in float32 (the float64 routine rounds once at the end)."""
    f = np.float32
    chain_ids = np.asarray(chain_ids, dtype=np.uint64).reshape(-1, 1)
    nblk = (D + 3) // 4
    x = O.philox4x32(np.arange(nblk, dtype=np.uint64).reshape(1, -1), np.uint64(draw), chain_ids, np.uint64(O.PURPOSE_MOMENTUM),
                     seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u = [O._u24(xx).astype(f) for xx in x]
    out = np.empty((chain_ids.shape[0], nblk, 4), dtype=f)
    for a in (0, 2):
        r = np.sqrt(f(-2.0) * np.log(u[a]))
        ang = f(2.0 * np.pi) * u[a + 1]
        out[:, :, a], out[:, :, a + 1] = r * np.cos(ang), r * np.sin(ang)
    return out.reshape(chain_ids.shape[0], nblk * 4)[:, :D]


RS_SEED, RS_OFF, RS_DRAW = 987654321012, 1000, 5


def factor(mass, D, dtype=np.float64):
    """An explicit momentum factor: diag uniform(0.3, 3); full: lower-triangular, N(0, 1 / D) below a diagonal in [0.5, 1.5]."""
    rng = np.random.default_rng(8000 + D)
    if mass == "none":
        return None
    if mass == "diag":
        return rng.uniform(0.3, 3.0, D).astype(dtype)
    return (np.tril(rng.standard_normal((D, D)) / math.sqrt(D), -1) + np.diag(rng.uniform(0.5, 1.5, D))).astype(dtype)


def ref_resample(mass, D, C, dt):
    """p = factor . z on the Philox stream (RS_SEED, RS_OFF + c, RS_DRAW) in `dt`: z from the float32 Box-Muller or from
    O.philox_normals."""
    ids = RS_OFF + np.arange(C)
    z = normals32(RS_SEED, ids, RS_DRAW, D) if dt == np.float32 else O.philox_normals(RS_SEED, ids, RS_DRAW, D, dtype=np.float64)
    mf = factor(mass, D)
    if mf is None:
        return z
    return (mf.astype(dt) * z) if mf.ndim == 1 else matvec(z, mf.astype(dt))


def f32_distance(name, mass, D, C=70):
    """How far the numpy formula of a kernel-level case is in float32 from its float64 value on the same float32 inputs, and the
    scale of the case (largest magnitude of the result): what F32_PIECES records."""
    if name == "resample":
        a = ref_resample(mass, D, C, np.float32)
        mf = factor(mass, D)
        z = O.philox_normals(RS_SEED, RS_OFF + np.arange(C), RS_DRAW, D, dtype=np.float64)
        mf = None if mf is None else mf.astype(np.float32).astype(np.float64)
        b = z if mf is None else (mf * z if mf.ndim == 1 else matvec(z, mf))
        return float(np.abs(a - b).max()), float(np.abs(b).max())
    x = piece_inputs(D, C, np.float32)
    im = inv_mass(mass, D, np.float32)
    if name == "hamiltonian":
        a, b = ref_hamiltonian(x, im, True, np.float32), ref_hamiltonian(x, im, True, np.float64)
        return float(np.abs(a - b).max()), float(np.abs(b).max())
    assert name == "kick_drift"
    (ta, pa), (tb, pb) = ref_kick_drift(x, im, KICK, DRIFT, True, np.float32), ref_kick_drift(x, im, KICK, DRIFT, True, np.float64)
    return float(max(np.abs(ta - tb).max(), np.abs(pa - pb).max())), float(max(np.abs(tb).max(), np.abs(pb).max()))


def f32_bound(name, mass, D, C=70):
    """4 x the recorded float32 distance of the case, at least 4 ulp of its scale.  (Batches of fewer than 70 chains are the first
    rows of the 70: the bound of the 70 holds for them.)"""
    dist, scale = F32_PIECES[(name, mass, D, max(C, 70))]
    return max(4.0 * dist, 4.0 * ULP32 * scale)


def piece_cases():
    """(kernel, mass, D, C) of every kernel-level float32 bound."""
    out = []
    for D in PIECE_D:
        for mass in MASSES + ("nonsym",):
            if mass in ("full", "nonsym") and D > FULL_MAX_D:
                continue
            if mass != "nonsym":
                out.append(("hamiltonian", mass, D, 70))
            out.append(("kick_drift", mass, D, 70))
    out += [("resample", m, D, 70) for D in RESAMPLE_D for m in MASSES]
    out += [("kick_drift", m) + STRIDE_KICK[::-1] for m in MASSES] + [("resample", m) + STRIDE_RESAMPLE[::-1] for m in ("none", "diag")]
    return out + [("resample", "full") + STRIDE_RESAMPLE_FULL[::-1]]


RESAMPLE_D = (5, 65, 129, 257)       # full: the three block sizes 64 / 128 / 256 of resample_full_kernel
# grid-stride sizes: one case each (C, D, what the launch code strides beyond)
STRIDE_KICK = (2100, 257)            # kick_drift / drift_full: C D = 539 700 > 2048 blocks x 256 threads
STRIDE_RESAMPLE = (8100, 257)        # resample: C ceil(D / 4) = 526 500 > 524 288; run_begin: 2 081 700 words > 4096 x 256
STRIDE_RESAMPLE_FULL = (4100, 5)     # resample_full: one block per chain, 4096 blocks

# (kernel, mass, D, C) -> (float32 distance, scale), measured on the CPU by f32_distance (tests/test_generic_cases_cpu.py measures again)
F32_PIECES = {
    ('hamiltonian', 'none', 1, 70): (1.1e-07, 2.44),
    ('kick_drift', 'none', 1, 70): (9.4e-08, 2.61),
    ('hamiltonian', 'diag', 1, 70): (1.7e-07, 2.62),
    ('kick_drift', 'diag', 1, 70): (1.8e-07, 2.7),
    ('hamiltonian', 'full', 1, 70): (1.3e-07, 2.46),
    ('kick_drift', 'full', 1, 70): (1.2e-07, 2.54),
    ('kick_drift', 'nonsym', 1, 70): (1.2e-07, 2.54),
    ('hamiltonian', 'none', 2, 70): (3.9e-07, 5.41),
    ('kick_drift', 'none', 2, 70): (2.2e-07, 3.89),
    ('hamiltonian', 'diag', 2, 70): (3.8e-07, 6.38),
    ('kick_drift', 'diag', 2, 70): (2.6e-07, 4.62),
    ('hamiltonian', 'full', 2, 70): (4.1e-07, 6.31),
    ('kick_drift', 'full', 2, 70): (1.9e-07, 3.51),
    ('kick_drift', 'nonsym', 2, 70): (3.2e-07, 3.51),
    ('hamiltonian', 'none', 3, 70): (4.9e-07, 7.15),
    ('kick_drift', 'none', 3, 70): (2e-07, 3.63),
    ('hamiltonian', 'diag', 3, 70): (3.8e-07, 7.12),
    ('kick_drift', 'diag', 3, 70): (3.4e-07, 3.86),
    ('hamiltonian', 'full', 3, 70): (2.7e-07, 9.05),
    ('kick_drift', 'full', 3, 70): (2.3e-07, 3.66),
    ('kick_drift', 'nonsym', 3, 70): (3.4e-07, 3.02),
    ('hamiltonian', 'none', 4, 70): (3.3e-07, 13.7),
    ('kick_drift', 'none', 4, 70): (2.1e-07, 3.44),
    ('hamiltonian', 'diag', 4, 70): (8.3e-07, 19.2),
    ('kick_drift', 'diag', 4, 70): (2.5e-07, 3.81),
    ('hamiltonian', 'full', 4, 70): (8.2e-07, 10.3),
    ('kick_drift', 'full', 4, 70): (3.7e-07, 3.41),
    ('kick_drift', 'nonsym', 4, 70): (3.7e-07, 3.41),
    ('hamiltonian', 'none', 5, 70): (4.1e-07, 8.58),
    ('kick_drift', 'none', 5, 70): (2e-07, 3.42),
    ('hamiltonian', 'diag', 5, 70): (6.3e-07, 9.47),
    ('kick_drift', 'diag', 5, 70): (2.8e-07, 3.42),
    ('hamiltonian', 'full', 5, 70): (6.8e-07, 9.27),
    ('kick_drift', 'full', 5, 70): (3.1e-07, 3.42),
    ('kick_drift', 'nonsym', 5, 70): (2.5e-07, 3.55),
    ('hamiltonian', 'none', 8, 70): (9.2e-07, 11.9),
    ('kick_drift', 'none', 8, 70): (2.5e-07, 4.38),
    ('hamiltonian', 'diag', 8, 70): (1.3e-06, 18.7),
    ('kick_drift', 'diag', 8, 70): (4.2e-07, 4.94),
    ('hamiltonian', 'full', 8, 70): (1e-06, 11.9),
    ('kick_drift', 'full', 8, 70): (3.3e-07, 4.38),
    ('kick_drift', 'nonsym', 8, 70): (3.7e-07, 4.38),
    ('hamiltonian', 'none', 9, 70): (8.9e-07, 14.9),
    ('kick_drift', 'none', 9, 70): (2.9e-07, 3.79),
    ('hamiltonian', 'diag', 9, 70): (1.4e-06, 15.4),
    ('kick_drift', 'diag', 9, 70): (3.1e-07, 3.79),
    ('hamiltonian', 'full', 9, 70): (1.2e-06, 16.7),
    ('kick_drift', 'full', 9, 70): (3.5e-07, 3.84),
    ('kick_drift', 'nonsym', 9, 70): (6.4e-07, 5.76),
    ('hamiltonian', 'none', 16, 70): (8.4e-07, 23.9),
    ('kick_drift', 'none', 16, 70): (2.1e-07, 4.18),
    ('hamiltonian', 'diag', 16, 70): (1.8e-06, 34.4),
    ('kick_drift', 'diag', 16, 70): (3.5e-07, 4.6),
    ('hamiltonian', 'full', 16, 70): (2e-06, 22.7),
    ('kick_drift', 'full', 16, 70): (3e-07, 4.22),
    ('kick_drift', 'nonsym', 16, 70): (4.1e-07, 4.65),
    ('hamiltonian', 'none', 17, 70): (1.3e-06, 20.1),
    ('kick_drift', 'none', 17, 70): (2.7e-07, 3.9),
    ('hamiltonian', 'diag', 17, 70): (2.2e-06, 23.5),
    ('kick_drift', 'diag', 17, 70): (3.1e-07, 4.39),
    ('hamiltonian', 'full', 17, 70): (1.1e-06, 21.6),
    ('kick_drift', 'full', 17, 70): (3.5e-07, 3.94),
    ('kick_drift', 'nonsym', 17, 70): (4.8e-07, 4.52),
    ('hamiltonian', 'none', 32, 70): (2.8e-06, 34.4),
    ('kick_drift', 'none', 32, 70): (2.6e-07, 3.88),
    ('hamiltonian', 'diag', 32, 70): (2.6e-06, 39.6),
    ('kick_drift', 'diag', 32, 70): (6.5e-07, 4.61),
    ('hamiltonian', 'full', 32, 70): (3e-06, 35.7),
    ('kick_drift', 'full', 32, 70): (3.8e-07, 3.88),
    ('kick_drift', 'nonsym', 32, 70): (5e-07, 5.32),
    ('hamiltonian', 'none', 33, 70): (3e-06, 37.6),
    ('kick_drift', 'none', 33, 70): (4e-07, 4.17),
    ('hamiltonian', 'diag', 33, 70): (4.5e-06, 44.5),
    ('kick_drift', 'diag', 33, 70): (5e-07, 4.4),
    ('hamiltonian', 'full', 33, 70): (3.5e-06, 36),
    ('kick_drift', 'full', 33, 70): (3.6e-07, 4.35),
    ('kick_drift', 'nonsym', 33, 70): (7.8e-07, 5.15),
    ('hamiltonian', 'none', 63, 70): (8.3e-06, 54.3),
    ('kick_drift', 'none', 63, 70): (2.9e-07, 4.67),
    ('hamiltonian', 'diag', 63, 70): (1.1e-05, 68.7),
    ('kick_drift', 'diag', 63, 70): (6.4e-07, 5.14),
    ('hamiltonian', 'full', 63, 70): (1.1e-05, 54.4),
    ('kick_drift', 'full', 63, 70): (6.5e-07, 4.41),
    ('kick_drift', 'nonsym', 63, 70): (8.9e-07, 7.25),
    ('hamiltonian', 'none', 64, 70): (5.9e-06, 56.3),
    ('kick_drift', 'none', 64, 70): (3e-07, 5.32),
    ('hamiltonian', 'diag', 64, 70): (6e-06, 69.1),
    ('kick_drift', 'diag', 64, 70): (3.6e-07, 5.04),
    ('hamiltonian', 'full', 64, 70): (5.3e-06, 53.3),
    ('kick_drift', 'full', 64, 70): (5e-07, 5.18),
    ('kick_drift', 'nonsym', 64, 70): (7.2e-07, 6.33),
    ('hamiltonian', 'none', 65, 70): (4.5e-06, 50.9),
    ('kick_drift', 'none', 65, 70): (3e-07, 4.51),
    ('hamiltonian', 'diag', 65, 70): (5e-06, 62.8),
    ('kick_drift', 'diag', 65, 70): (4.7e-07, 5.38),
    ('hamiltonian', 'full', 65, 70): (5.7e-06, 52.4),
    ('kick_drift', 'full', 65, 70): (4.4e-07, 4.69),
    ('kick_drift', 'nonsym', 65, 70): (8.7e-07, 6.85),
    ('hamiltonian', 'none', 130, 70): (9.4e-06, 96.1),
    ('kick_drift', 'none', 130, 70): (2.7e-07, 4.66),
    ('hamiltonian', 'diag', 130, 70): (1.1e-05, 113),
    ('kick_drift', 'diag', 130, 70): (4.7e-07, 5.71),
    ('hamiltonian', 'full', 130, 70): (1.3e-05, 99.6),
    ('kick_drift', 'full', 130, 70): (6.2e-07, 4.83),
    ('kick_drift', 'nonsym', 130, 70): (1.3e-06, 9.76),
    ('hamiltonian', 'none', 257, 70): (1.6e-05, 166),
    ('kick_drift', 'none', 257, 70): (3e-07, 4.58),
    ('hamiltonian', 'diag', 257, 70): (2.5e-05, 202),
    ('kick_drift', 'diag', 257, 70): (4.4e-07, 5.68),
    ('resample', 'none', 5, 70): (8.5e-07, 3.08),
    ('resample', 'diag', 5, 70): (2.4e-06, 8.64),
    ('resample', 'full', 5, 70): (1.2e-06, 4.34),
    ('resample', 'none', 65, 70): (1.1e-06, 3.78),
    ('resample', 'diag', 65, 70): (2.5e-06, 7.85),
    ('resample', 'full', 65, 70): (1.4e-06, 6.45),
    ('resample', 'none', 129, 70): (1.1e-06, 3.78),
    ('resample', 'diag', 129, 70): (2.8e-06, 9.37),
    ('resample', 'full', 129, 70): (1.7e-06, 5.38),
    ('resample', 'none', 257, 70): (1.3e-06, 3.78),
    ('resample', 'diag', 257, 70): (3e-06, 10.1),
    ('resample', 'full', 257, 70): (1.6e-06, 7.19),
    ('kick_drift', 'none', 257, 2100): (5.1e-07, 5.64),
    ('kick_drift', 'diag', 257, 2100): (6.8e-07, 7.42),
    ('kick_drift', 'full', 257, 2100): (1.1e-06, 5.81),
    ('resample', 'none', 257, 8100): (1.6e-06, 5.57),
    ('resample', 'diag', 257, 8100): (4.2e-06, 13.9),
    ('resample', 'full', 5, 4100): (1.6e-06, 5.26),
}


# ---- Metropolis select cases ----------------------------------------------------------------------------------------------------------
MH_SEED, MH_OFF, MH_BURN = 20240611, 29, 5
MH_N = (MH_BURN - 1, MH_BURN, MH_BURN + 1, MH_BURN + 2)
MH_SENTINEL = -77.25
MH_GUARD = 1e-5
NONFINITE = {3: ("Hn", np.nan), 11: ("Hn", np.inf), 19: ("Ho", np.nan), 27: ("lp", -np.inf), 35: ("lp", np.nan)}


def mh_inputs(C, dtype):
    """Energies and log p of the proposals for C <= 70 chains in five classes by chain index: c % 7 == 0 a sure accept (H_new = H_old
    - 5), c % 7 == 1 a sure reject (H_new = H_old + 50: log u >= log 2^-24 = -16.6), c in NONFINITE one non-finite value with the
    other two finite, every other chain H_new = H_old + N(0, 1).  -> Ho, Hn, lp, klass ('a' | 'r' | 'n' | 'x')."""
    rng = np.random.default_rng(555)
    Ho = 3.0 * rng.standard_normal(70)
    Hn = Ho + rng.standard_normal(70)
    lp = -np.abs(3.0 * rng.standard_normal(70))
    klass = np.array(["x"] * 70)
    c = np.arange(70)
    Hn[c % 7 == 0] = Ho[c % 7 == 0] - 5.0; klass[c % 7 == 0] = "a"
    Hn[c % 7 == 1] = Ho[c % 7 == 1] + 50.0; klass[c % 7 == 1] = "r"
    for k, (which, v) in NONFINITE.items():
        {"Ho": Ho, "Hn": Hn, "lp": lp}[which][k] = v
        if which == "lp":
            Hn[k] = Ho[k] - 5.0                    # the energies alone would accept
        klass[k] = "n"
    return Ho[:C].astype(dtype), Hn[:C].astype(dtype), lp[:C].astype(dtype), klass[:C]


def mh_uniform(n, C, dtype):
    return O.PhiloxDraws(MH_SEED, MH_OFF + np.arange(C), dtype).mh_uniform(n)


def mh_expected(cur, prop, init, Ho, Hn, lp, n, burn, u, rej0):
    """O.mh_accept + the LogProbError rule (S:1045-1057) + the update rule of O.sample_chain_driver for ONE trajectory ->
    (accept, new cur, row or None, reject counts)."""
    acc, _ = O.mh_accept(Ho, Hn, u)
    if lp is not None:
        acc = acc & np.isfinite(lp)
    a = acc[:, None]
    # n > burn: np.where(a, new, ret[-1]) with ret[-1] = params_init at n = burn + 1 (Q2), the chain's last row afterwards;
    # n <= burn: np.where(a, new, burn_prev)
    new = np.where(a, prop, init if n == burn + 1 else cur)
    return acc, new, (new if n > burn else None), rej0 + (~acc)


def mh_margin(Ho, Hn, u):
    """|rho - log u| / (1 + |H_old| + |H_new|) in float64: below MH_GUARD a decision may differ on the last bit of a float32 log."""
    with np.errstate(invalid="ignore"):
        rho = np.minimum(0.0, (Ho - Hn).astype(np.float64))
        return np.abs(rho - np.log(u.astype(np.float64))) / (1.0 + np.abs(Ho.astype(np.float64)) + np.abs(Hn.astype(np.float64)))


# ---- engine runs (tests/test_gpu_generic.py) --------------------------------------------------------------------------------------------
class _Upcast:
    """The float32 draws handed to float64 arithmetic: the same numbers, no rounding of their own."""

    def __init__(self, draws):
        self.draws = draws

    def normals(self, n, D, sub=0):
        return self.draws.normals(n, D, sub).astype(np.float64)

    def mh_uniform(self, n):
        return self.draws.mh_uniform(n).astype(np.float64)

    def split_perm(self, n, M):
        return self.draws.split_perm(n, M)


SPLIT_KINDS = {"SPLITTING": "symmetric", "SPLITTING_RAND": "rand", "SPLITTING_KMID": "kmid"}


class Run:
    """One sample() run: target (or a list of three for the split integrators), start, mass matrix, and the oracle's result
    (computed once per dtype, shared, left unchanged)."""

    def __init__(self, name, target, D, L, eps, mass="none", burn=0, C=70, N=12, seed=4242, off=17, scale=0.3, split=None, band=False):
        self.name, self.target, self.D, self.L, self.eps, self.mass, self.burn = name, target, D, L, eps, mass, burn
        self.C, self.N, self.seed, self.off, self.scale, self.split, self.band = C, N, seed, off, scale, split, band
        self._oracle = {}

    def start(self, dtype):
        z = O.philox_normals(self.seed, self.off + np.arange(self.C), 0, self.D, O.PURPOSE_INIT, dtype=np.float64)
        return (self.scale * z).astype(NP[dtype])

    def inv_mass(self, dtype):
        return inv_mass(self.mass, self.D, NP[dtype])

    def kwargs(self):
        return dict(num_samples=self.N, num_steps_per_sample=self.L, step_size=self.eps, burn=self.burn, seed=self.seed,
                    chain_offset=self.off, debug=2, verbose=False, native=False)

    def oracle(self, dtype, exact=False):
        """O.sample_hmc on the Philox draws of (seed, chain offset) -> (rows [n, C, D], info).  exact=True: float64 arithmetic on
        the start, mass matrix and draws of the float32 run - that run without its rounding."""
        key = (dtype, exact)
        if key not in self._oracle:
            draws = O.PhiloxDraws(self.seed, self.off + np.arange(self.C), NP[dtype])
            th0, im = self.start(dtype), self.inv_mass(dtype)
            if exact:
                assert dtype == torch.float32
                draws, th0, im = _Upcast(draws), th0.astype(np.float64), None if im is None else im.astype(np.float64)
            if self.split:
                ref, info = O.sample_hmc(None, th0, self.N, self.L, self.eps, self.burn, im, draws, grad_fns=[t.grad for t in self.target],
                                         logp_fns=[t.logp for t in self.target], split_kind=SPLIT_KINDS[self.split])
            else:
                ref, info = O.sample_hmc(self.target, th0, self.N, self.L, self.eps, self.burn, im, draws)
            ref = np.stack(ref)
            assert ref.dtype == (np.float64 if exact else NP[dtype])
            self._oracle[key] = (ref, info)
        return self._oracle[key]

    def bound(self, dtype):
        """float64: 1e-9.  float32: 4 x the recorded error of the float32 oracle, at least 2e-6; `band` rows (the funnel: its error is
        amplified along the neck, up to 3.9e-4 on one chain of the float32 oracle itself) the project's band of 2e-4."""
        if dtype == torch.float64:
            return F64_RUN
        return BAND_F32 if self.band else max(4.0 * F32_ORACLE_ERR[self.name], 2e-6)


def deviation(a, b):
    """Largest difference per chain of two runs [n, C, D]."""
    return np.abs(a.astype(np.float64) - b.astype(np.float64)).max(axis=(0, 2))


MASS_ROWS = (("none", 0), ("diag", 3), ("full", -1))    # the Q2 trajectory (burn + 1) on the capture warm-up, inside replay, first eager
# D, L, step size: at every (mass, burn) row the oracle takes both Metropolis branches at trajectory burn + 1 (the CPU tests assert it)
_GAUSS = ((1, 5, 0.9), (5, 5, 0.55), (11, 5, 0.45), (65, 5, 0.3), (130, 4, 0.25))
RUNS = {}
for _D, _L, _eps in _GAUSS:
    for _mass, _burn in MASS_ROWS:
        RUNS["gauss%d_%s" % (_D, _mass)] = Run("gauss%d_%s" % (_D, _mass), DenseGaussian(_D), _D, _L, _eps, _mass, _burn)
for _mass, _burn in MASS_ROWS:
    RUNS["funnel_%s" % _mass] = Run("funnel_%s" % _mass, Funnel(11), 11, 8, 0.2, _mass, _burn, scale=0.5, band=True)
ORACLE_RUNS = sorted(RUNS)
# carry: a step size at which the oracle rejects 30 - 70 % of the proposals, so that the carried pair is used on both branches
RUNS["carry"] = Run("carry", DenseGaussian(11), 11, 5, 1.0, "diag", 3)
RUNS["chunks"] = Run("chunks", DenseGaussian(5), 5, 5, 0.7, "diag", 3)
SPLIT_RUNS = []
for _kind in SPLIT_KINDS:
    for _D, _eps in ((5, 0.8), (65, 0.25)):
        for _mass, _burn in MASS_ROWS:
            _n = "split_%s_%d_%s" % (SPLIT_KINDS[_kind], _D, _mass)
            RUNS[_n] = Run(_n, [DenseGaussian(_D, s) for s in (1, 2, 3)], _D, 3, _eps, _mass, _burn, split=_kind)
            SPLIT_RUNS.append(_n)
RUNS["loop"] = Run("loop", Branching(4), 4, 4, 0.9, "none", 1, C=9)
_PG = DenseGaussian(5, 4)
PASS_GRAD_OTHER = DenseGaussian(5, 5)                                   # the gradient handed in is NOT the callable's own
PASS_GRAD_CONST = 0.3 * np.random.default_rng(31).standard_normal(5)
RUNS["pass_grad_callable"] = Run("pass_grad_callable", Mixed(_PG, PASS_GRAD_OTHER), 5, 4, 0.3, "diag", 1)
RUNS["pass_grad_tensor"] = Run("pass_grad_tensor", Mixed(_PG, PASS_GRAD_CONST), 5, 4, 0.3, "none", 1)
RUNS["ball"] = Run("ball", Ball(4, 2.5), 4, 5, 0.5, "none", 1, scale=0.6)
F32_RUNS = ORACLE_RUNS + ["carry", "chunks"] + SPLIT_RUNS + ["pass_grad_callable", "pass_grad_tensor"]

# run -> largest difference of the float32 oracle from the float64 oracle on the chains that kept their decisions (none flipped),
# measured on the CPU (tests/test_generic_cases_cpu.py measures again)
F32_ORACLE_ERR = {
    'funnel_diag': 0.00012,
    'funnel_full': 6.3e-05,
    'funnel_none': 7.5e-05,
    'gauss11_diag': 1.7e-06,
    'gauss11_full': 9.9e-07,
    'gauss11_none': 8.8e-07,
    'gauss130_diag': 8.2e-07,
    'gauss130_full': 1.4e-06,
    'gauss130_none': 5.8e-07,
    'gauss1_diag': 1.5e-06,
    'gauss1_full': 1.2e-06,
    'gauss1_none': 1.1e-06,
    'gauss5_diag': 7.7e-07,
    'gauss5_full': 1.1e-06,
    'gauss5_none': 9.6e-07,
    'gauss65_diag': 9.2e-07,
    'gauss65_full': 1.1e-06,
    'gauss65_none': 8.7e-07,
    'carry': 2.2e-06,
    'chunks': 9.3e-07,
    'split_symmetric_5_none': 5.2e-07,
    'split_symmetric_5_diag': 6.2e-07,
    'split_symmetric_5_full': 7.5e-07,
    'split_symmetric_65_none': 5.3e-07,
    'split_symmetric_65_diag': 6.4e-07,
    'split_symmetric_65_full': 6.7e-07,
    'split_rand_5_none': 6.9e-07,
    'split_rand_5_diag': 1.2e-06,
    'split_rand_5_full': 7.7e-07,
    'split_rand_65_none': 4.3e-07,
    'split_rand_65_diag': 5.2e-07,
    'split_rand_65_full': 6.1e-07,
    'split_kmid_5_none': 5.9e-07,
    'split_kmid_5_diag': 2.6e-06,
    'split_kmid_5_full': 1.3e-06,
    'split_kmid_65_none': 4.4e-07,
    'split_kmid_65_diag': 5.3e-07,
    'split_kmid_65_full': 7.3e-07,
    'pass_grad_callable': 5.8e-07,
    'pass_grad_tensor': 5.9e-07,
}

# leapfrog() with a (D,) input: D, steps, step size; float32 distance per (D, mass) as for the kernels
LEAPFROG = {65: (6, 0.3), 130: (6, 0.25)}
F32_LEAPFROG = {
    (65, 'none'): (4.1e-07, 2.96),
    (65, 'diag'): (5e-07, 3.73),
    (65, 'full'): (4.4e-07, 3),
    (130, 'none'): (3.7e-07, 3.04),
    (130, 'diag'): (3.7e-07, 3.72),
    (130, 'full'): (4.2e-07, 3.22),
}


def leapfrog_start(D):
    """One chain: start and momentum ~ N(0, 1)."""
    rng = np.random.default_rng(600 + D)
    return rng.standard_normal(D), rng.standard_normal(D)


def leapfrog_path(D, mass, run_dtype, dt):
    """The oracle's path ([steps, D] of theta, of p) in `dt` from the start, momentum and mass matrix rounded to `run_dtype`."""
    (th, p), tgt, (steps, eps) = leapfrog_start(D), DenseGaussian(D), LEAPFROG[D]
    th, p = th.astype(run_dtype).astype(dt), p.astype(run_dtype).astype(dt)
    im = inv_mass(mass, D, run_dtype)
    pt, pp = O.hmc_leapfrog(th[None], p[None], tgt.grad, steps, eps, None if im is None else im.astype(dt), return_path=True)
    return np.stack(pt)[:, 0], np.stack(pp)[:, 0]
