"""Shared by tests/test_diag_rank_cases_cpu.py and tests/test_gpu_diag_rank.py: the table of shapes and data variants of the
rank-normalised diagnostics, and their reference - scipy's rankdata(method="average") and special.ndtri, numpy's sort and quantile,
followed by the numpy restatement of tests/diag_cases.py on the derived series.

Per coordinate, over x[S, C] with N = S C (hamiltorch_amd/diagnostics.py: rank_summary): a coordinate holding a NaN or an infinity is
NaN in every field; r = average rank among all N draws (-0.0 ties with +0.0), z = ndtri((r - 3/8) / (N + 1/4)); ess_bulk = E(z),
rhat_bulk = R(z); med = 0.5 (x_((N-1)//2) + x_(N//2)), zf the same z of |x - med|, rhat_folded = R(zf), rhat the larger one;
I05 = 1[x <= x_((N-1)//20)], I95 = 1[x <= x_(19 (N-1)//20)], ess_tail = min(E(I05), E(I95)); q05 / median / q95 = numpy.quantile of the
draws in float64.  E and R are diag_cases.restate's ess and rhat.

The shapes: T = the sort's tile (keys per block and pass).  N = S C in {4, 5, T-1, T, T+1, 2T+3} as one long chain, and 257 x 70.
T is a multiple of 256, so T-1, T+1 and 2T+3 have no divisor 4 or 5: the many-short-chains forms (S = 4 or 5) sit at N = T, at the
nearest multiples on both sides of the tile edges (T-3, T+2, 2T+4), and T-1 = 23 x 89 and T+1 = 683 x 3 appear with those chain shapes.
D in {1, 3, 67, 130}, both dtypes.  The data variants:
  a  diag_cases.generate as is
  b  quantised to multiples of 0.5: tie runs of hundreds of draws across tile and digit boundaries
  c  coordinate 0 mixes -0.0 and +0.0, negative values, float32 denormals and neighbours in the last mantissa bit
  d  coordinate 1 constant, coordinate 3 with one NaN, coordinate 5 with one +inf, among good coordinates
  e  float64 only: 1 + 1e-10 generate - the draws differ only below float32 precision (a 32-bit key would tie them all)"""
import functools
from collections import namedtuple

import numpy as np

import diag_cases as T0
from hamiltorch_amd import diagnostics as DG

T = DG.RANK_TILE

Case = namedtuple("Case", "S C D dtype variant seed")

_SHAPES = [
    (4, 1, 1, "f32", "a"), (4, 1, 3, "f64", "a"), (4, 1, 130, "f32", "a"), (5, 1, 3, "f32", "b"), (5, 1, 67, "f64", "a"),
    (T - 1, 1, 3, "f32", "a"), (T - 1, 1, 1, "f64", "b"), (T, 1, 1, "f32", "b"), (T, 1, 3, "f64", "e"),
    (T + 1, 1, 3, "f32", "b"), (T + 1, 1, 3, "f64", "a"), (2 * T + 3, 1, 3, "f32", "a"), (2 * T + 3, 1, 1, "f64", "b"),
    (4, T // 4, 67, "f32", "a"), (4, T // 4, 130, "f64", "b"), (5, (T - 3) // 5, 3, "f64", "a"), (5, (T + 2) // 5, 130, "f32", "b"),
    (4, (2 * T + 4) // 4, 67, "f64", "d"), (5, (2 * T + 4) // 5, 3, "f32", "c"),
    (23, (T - 1) // 23, 67, "f32", "d"), ((T + 1) // 3, 3, 3, "f64", "c"),
    (257, 70, 3, "f32", "a"), (257, 70, 3, "f64", "e"), (5, 3598, 3, "f32", "b"), (4, 4500, 1, "f64", "c"),
]
CASES = [Case(S, C, D, np.float32 if t == "f32" else np.float64, v, 2000 + i) for i, (S, C, D, t, v) in enumerate(_SHAPES)]
IDS = ["S%d-C%d-D%d-%s-%s" % (c.S, c.C, c.D, "f32" if c.dtype == np.float32 else "f64", c.variant) for c in CASES]

CONSTANT, WITH_NAN, WITH_INF = 1, 3, 5            # the degenerate coordinates of variant d


def generate(S, C, D, dtype, variant, seed):
    x = T0.generate(S, C, D, np.float64, seed)
    rng = np.random.default_rng(seed + 7)
    if variant == "b":
        x = np.round(x * 2.0) / 2.0
    elif variant == "c":
        x = x.astype(dtype)
        one = dtype(1.0)
        special = np.array([-0.0, 0.0, -0.0, 0.0, 1e-40, -1e-40, 3e-45, -3e-45, one, np.nextafter(one, dtype(2.0)), np.nextafter(one, dtype(0.0)),
                            -one, np.nextafter(-one, dtype(-2.0)), -2.5, 2.5], dtype=dtype)
        pick = rng.random((S, C)) < 0.4
        x[:, :, 0] = np.where(pick, special[rng.integers(0, len(special), (S, C))], x[:, :, 0] - x[:, :, 0].mean())
    elif variant == "d":
        x[:, :, CONSTANT] = 2.5
        x[S // 2, C // 3, WITH_NAN] = np.nan
        x[S - 1, C - 1, WITH_INF] = np.inf
    elif variant == "e":
        assert dtype == np.float64
        x = 1.0 + 1e-10 * x
    return np.ascontiguousarray(x.astype(dtype))


def samples(case):
    return generate(*case)


Reference = namedtuple("Reference", "ess_bulk ess_tail rhat rhat_bulk rhat_folded q05 median q95 sd small z i05 i95 zf")


def normal_scores(v):
    """v[S, C] -> ndtri((r - 3/8) / (N + 1/4)) with r the average ranks among all S C values."""
    from scipy import special, stats
    r = stats.rankdata(v.ravel(), method="average").reshape(v.shape)
    return special.ndtri((r - 0.375) / (v.size + 0.25))


def derive(x):
    """x[S, C, D] -> (z, i05, i95, zf) [S, C, D] float64 and the mask of the coordinates holding a NaN or an infinity (NaN there)."""
    x = np.asarray(x).astype(np.float64) + 0.0
    S, C, D = x.shape
    N = S * C
    z, i05, i95, zf = (np.full((S, C, D), np.nan) for _ in range(4))
    bad = ~np.isfinite(x).all(axis=(0, 1))
    for d in np.flatnonzero(~bad):
        col = x[:, :, d]
        srt = np.sort(col.ravel())
        z[:, :, d] = normal_scores(col)
        zf[:, :, d] = normal_scores(np.abs(col - 0.5 * (srt[(N - 1) // 2] + srt[N // 2])))
        i05[:, :, d] = col <= srt[(N - 1) // 20]
        i95[:, :, d] = col <= srt[19 * (N - 1) // 20]
    return z, i05, i95, zf, bad


def _min_nan(a, b):
    return np.where(np.isnan(a) | np.isnan(b), np.nan, np.minimum(a, b))


def _max_nan(a, b):
    return np.where(np.isnan(a) | np.isnan(b), np.nan, np.maximum(a, b))


def reference(x, max_lag=None):
    """Everything rank_summary() reports, per coordinate, from scipy / numpy and diag_cases.restate; `small`: the smallest |pair sum|
    on the Geyer walks of z, I05 and I95; `sd`: the standard deviation of the draws (the scale of the quantiles' absolute tolerance)."""
    x = np.asarray(x)
    z, i05, i95, zf, bad = derive(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        rz, r05, r95 = T0.restate(z, max_lag), T0.restate(i05, max_lag), T0.restate(i95, max_lag)
        rhat_folded = np.array([T0.rhat_split_np(zf[:, :, d]) for d in range(x.shape[2])])
    x64 = x.astype(np.float64)
    q = np.full((3, x.shape[2]), np.nan)
    q[:, ~bad] = np.quantile(x64[:, :, ~bad].reshape(-1, int((~bad).sum())), [0.05, 0.5, 0.95], axis=0)
    with np.errstate(invalid="ignore"):
        sd = np.where(bad, np.nan, x64.reshape(-1, x.shape[2]).std(axis=0))
    return Reference(rz.ess, _min_nan(r05.ess, r95.ess), _max_nan(rz.rhat, rhat_folded), rz.rhat, rhat_folded, q[0], q[1], q[2], sd,
                     np.minimum(np.minimum(rz.small, r05.small), r95.small), z, i05, i95, zf)


@functools.lru_cache(maxsize=None)
def _reference(i):
    return reference(samples(CASES[i]))


def referenced(case):
    """The reference of a case of the table (computed once per process; treat as read-only)."""
    return _reference(CASES.index(case))
