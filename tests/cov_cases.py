"""Shared by tests/test_cov_cases_cpu.py and tests/test_gpu_cov.py: the cases of the running covariance (csrc/covariance.hip,
diagnostics.RunningCovariance), a numpy float64 restatement of update / merge / finish in the kernels' own order of operations, an
np.longdouble two-pass computation of the same quantities, and the error band the kernels are held to.

The band: per case and quantity the error of the float64 restatement against the longdouble computation, MEASURED below; the
kernels get 4 x that, with a floor of 1e-15 (BAND) - the rule of tests/moments_cases.py.  Errors are relative to the quantity's
scale: the largest |x| of the case for the means, the largest reference entry for the co-moments and the matrices, the value
itself for R-hat.

    python tests/cov_cases.py          prints the MEASURED table (float64 restatement against longdouble, this file's cases)
"""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

if __name__ == "__main__":                   # (run as a script: the package is one directory up)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hamiltorch_amd import diagnostics as DG  # noqa: E402

SLICES = DG.MOMENTS_CHAIN_SLICES
REG_N, REG_FLOOR = 5.0, 1e-3

Case = namedtuple("Case", "name kind S C D dtype seed")

#: (S, C, D): one series; one coordinate; a chain-slice edge; many chains; more than two row segments; T = 153, no multiple of
#: the wave; T = 2080, a chain's pairs over several passes of its workgroup; the limit D = 256
SHAPES = [(1, 1, 1), (5, 3, 1), (7, 65, 3), (4, 1025, 2), (600, 2, 3), (9, 3, 17), (5, 3, 64), (3, 2, 256)]
_T = {"f32": np.float32, "f64": np.float64}
CASES = [Case("S%d-C%d-D%d-%s" % (S, C, D, t), "random", S, C, D, _T[t], 500 + 2 * i + j)
         for i, (S, C, D) in enumerate(SHAPES) for j, t in enumerate(("f32", "f64"))]
CASES += [Case("offset-%s" % t, "offset", 1000, 3, 2, _T[t], 600 + j) for j, t in enumerate(("f32", "f64"))]     # mean 1e6, sd 1
CASES += [Case("constant-f32", "constant", 40, 3, 2, np.float32, 700), Case("nan-f64", "nan", 20, 4, 3, np.float64, 701)]
IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
NAN_AT = (7, 2, 1)                           # the one NaN draw of the "nan" case: row, chain, coordinate

QUANTITIES = ("chain_mean", "chain_q", "mean", "cov_within", "cov_total", "rhat", "inv_mass")


def pairs(D):
    """(i, j) of the packed upper triangle, row-major over i <= j."""
    return np.triu_indices(D)


@functools.lru_cache(maxsize=None)
def _samples(i):
    c = CASES[i]
    rng = np.random.default_rng(c.seed)
    mix = np.eye(c.D) + 0.5 * rng.standard_normal((c.D, c.D)) / np.sqrt(c.D)          # correlated coordinates
    if c.kind == "offset":
        x = 1e6 + rng.standard_normal((c.S, c.C, c.D)) @ mix
    elif c.kind == "constant":
        x = np.broadcast_to(np.array([2.5, -0.1])[None, None, :] + np.arange(c.C)[None, :, None], (c.S, c.C, c.D)).copy()
    else:
        x = ((np.linspace(0.5, 3.0, c.D) * rng.standard_normal((c.S, c.C, c.D))) @ mix + np.linspace(-100.0, 100.0, c.D)
             + 0.3 * rng.standard_normal((c.C, c.D)))
        if c.kind == "nan":
            x[NAN_AT] = np.nan
    x = x.astype(c.dtype)
    x.setflags(write=False)
    return x


def samples(case):
    """x[S, C, D] of a case in its dtype (computed once per process; read-only)."""
    return _samples(CASES.index(case))


def chunkings(S):
    """The ways a case's S rows are fed: at once, (1, S - 1), and uneven thirds."""
    out = [(S,)]
    if S >= 2:
        out.append((1, S - 1))
    if S >= 4:
        a, b = max(1, S // 3 - 1), S // 3 + 1
        out.append((a, b, S - a - b))
    return out


# ---- the float64 restatement ----------------------------------------------------------------------------------------------------
def chan(na, ma, qa, nb, mb, qb):
    """Chan et al. over means [C, D] and packed co-moments [C, T], counts as floats: (na, ma, qa) + (nb, mb, qb) with nb > 0."""
    if na == 0.0:
        return nb, mb.copy(), qb.copy()
    iu, ju = pairs(ma.shape[1])
    n = na + nb
    dl = mb - ma
    return n, ma + dl * (nb / n), qa + qb + dl[:, iu] * dl[:, ju] * (na * nb / n)


def recurrence(x):
    """x[S, C, D] float64 -> (mean [C, D], q [C, T]) in row order: delta = x - m, m += delta / k, q_ij += delta_i (x_j - m_j)
    with the updated m_j.  (A lane of the kernel carries m_i and m_j itself; they are the entries of this m.)"""
    iu, ju = pairs(x.shape[2])
    m, q = np.zeros(x.shape[1:]), np.zeros((x.shape[1], iu.size))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(x.shape[0]):
            dl = x[k] - m
            m = m + dl / float(k + 1)
            q = q + dl[:, iu] * (x[k] - m)[:, ju]
    return m, q


class State:
    """hta_cov_update / RunningCovariance.merge / hta_cov_finish in numpy float64, in the kernels' order of operations."""

    def __init__(self):
        self.n, self.mean, self.q = 0, None, None

    def _store(self, n, m, q):
        iu, ju = pairs(m.shape[1])
        with np.errstate(invalid="ignore", over="ignore"):
            if self.n:
                _, m, q = chan(float(self.n), self.mean, self.q, float(n), m, q)
        q = np.where(np.isfinite(m[:, iu]) & np.isfinite(m[:, ju]) & np.isfinite(q), q, np.nan)
        self.mean, self.q = np.where(np.isfinite(q[:, iu == ju]), m, np.nan), q
        self.n += n
        return self

    def update(self, x):
        x = np.asarray(x, dtype=np.float64)
        S, C, D = x.shape
        R = DG.moments_segment_rows(S, C, D)
        n, m, q = 0.0, None, None
        with np.errstate(invalid="ignore", over="ignore"):
            for r0 in range(0, S, R):
                mb, qb = recurrence(x[r0:r0 + R])
                n, m, q = chan(n, m, q, float(min(S, r0 + R) - r0), mb, qb)
        return self._store(S, m, q)

    def merge(self, other):
        return self._store(other.n, other.mean, other.q)

    @staticmethod
    def stack(parts):
        out = State()
        out.n = parts[0].n
        out.mean, out.q = np.concatenate([p.mean for p in parts], 0), np.concatenate([p.q for p in parts], 0)
        return out

    def finish(self, reg_n=REG_N, reg_floor=REG_FLOOR):
        return finish(self.n, self.mean, self.q, reg_n, reg_floor, slices=SLICES)


def _over_chains(a, slices):
    """sum over axis 0 of a[C, ...]: slice k adds the chains k, k + slices, ... in order, the slices are added in order."""
    if slices is None:
        return a.sum(axis=0)
    parts = []
    for k in range(slices):
        s = np.zeros(a.shape[1:], a.dtype)
        for c in range(k, a.shape[0], slices):
            s = s + a[c]
        parts.append(s)
    tot = parts[0]
    for p in parts[1:]:
        tot = tot + p
    return tot


def _full(tri, D):
    """packed [T] -> the full symmetric [D, D]."""
    iu, ju = pairs(D)
    out = np.empty((D, D), tri.dtype)
    out[iu, ju] = tri
    out[ju, iu] = tri
    return out


def finish(n, mean_c, q_c, reg_n=REG_N, reg_floor=REG_FLOOR, slices=None):
    """The pooled statistics from per-chain means [C, D] and packed co-moments [C, T] of n draws, in the dtype of the inputs."""
    ft = mean_c.dtype.type
    C, D = mean_c.shape
    iu, ju = pairs(D)
    dg = iu == ju
    n_, nc = ft(n), ft(C)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mean = _over_chains(mean_c, slices) / nc
        m2 = _over_chains(q_c, slices)
        dm = mean_c - mean
        ssb = _over_chains(dm[:, iu] * dm[:, ju], slices)
        cw = m2 / (n_ - ft(1)) / nc
        N = n_ * nc
        ct = (m2 + n_ * ssb) / (N - ft(1))
        vw = cw[dg]
        vb = ssb[dg] / (nc - ft(1)) if C > 1 else np.zeros_like(ssb[dg])
        rh = np.full(mean.shape, np.nan, mean_c.dtype)
        if n >= 2:
            pos = vw > 0
            rh = np.where(pos, np.sqrt(((n_ - ft(1)) / n_ * vw + vb) / np.where(pos, vw, ft(1))), np.where(vb > 0, np.inf, np.nan))
            rh = np.where(np.isnan(vw) | np.isnan(vb), np.nan, rh)
        im = ct * (N / (N + ft(reg_n)))
        im = np.where(dg, im + ft(reg_floor) * (ft(reg_n) / (N + ft(reg_n))), im)
    return dict(chain_mean=mean_c, chain_q=q_c, mean=mean, cov_within=_full(cw, D), cov_total=_full(ct, D), rhat=rh, inv_mass=_full(im, D))


def restate(x, chunks):
    """The restatement's quantities of x[S, C, D] fed in `chunks` rows at a time."""
    st, r0 = State(), 0
    for k in chunks:
        st.update(x[r0:r0 + k])
        r0 += k
    assert r0 == x.shape[0]
    return st.finish()


def exact(x):
    """The same quantities in np.longdouble: two passes over the rows per chain, plain sums over chains."""
    xl = np.asarray(x, dtype=np.longdouble)
    iu, ju = pairs(xl.shape[2])
    with np.errstate(invalid="ignore"):
        m = xl.sum(axis=0) / np.longdouble(xl.shape[0])
        d = xl - m
        q = (d[:, :, iu] * d[:, :, ju]).sum(axis=0)
    return finish(xl.shape[0], m, q)


def errors(got, ref, x):
    """{quantity: error of `got` against `ref`} on the scales of the module docstring; inf where the non-finite entries differ
    or a quantity whose reference is all zero is not zero."""
    finite = np.abs(np.asarray(x, dtype=np.float64)[np.isfinite(x)])
    xs = float(finite.max()) if finite.size and finite.max() > 0 else 1.0
    out = {}
    for k in QUANTITIES:
        g, r = np.asarray(got[k], dtype=np.longdouble), np.asarray(ref[k], dtype=np.longdouble)
        if g.shape != r.shape or not (np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(np.isinf(g), np.isinf(r))
                                      and np.array_equal(g[np.isinf(g)], r[np.isinf(r)])):
            out[k] = np.inf
            continue
        ok = np.isfinite(r)
        if not ok.any():
            out[k] = 0.0
            continue
        d = np.abs(g[ok] - r[ok])
        if k in ("chain_mean", "mean"):
            out[k] = float(d.max() / xs)
        elif k == "rhat":
            out[k] = float((d / np.abs(r[ok])).max())
        else:
            top = np.abs(r[ok]).max()
            out[k] = float(d.max() / top) if top > 0 else (0.0 if d.max() == 0 else np.inf)
    return out


def measure(case):
    """{quantity: the largest error of the float64 restatement against longdouble over the case's chunkings}."""
    x = samples(case)
    ref = exact(x)
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for chunks in chunkings(case.S):
        e = errors(restate(x, chunks), ref, x)
        worst = {k: max(worst[k], e[k]) for k in QUANTITIES}
    return worst


FLOOR = 1e-15

#: measured by `python tests/cov_cases.py` (x86-64: np.longdouble is the 80-bit format), rounded up to two digits;
#: tests/test_cov_cases_cpu.py::test_the_band_is_the_measured_error_of_the_restatement measures them again
MEASURED = {
    "S1-C1-D1-f32": {"chain_mean": 0.0, "chain_q": 0.0, "mean": 0.0, "cov_within": 0.0, "cov_total": 0.0, "rhat": 0.0, "inv_mass": 0.0},
    "S1-C1-D1-f64": {"chain_mean": 0.0, "chain_q": 0.0, "mean": 0.0, "cov_within": 0.0, "cov_total": 0.0, "rhat": 0.0, "inv_mass": 0.0},
    "S5-C3-D1-f32": {"chain_mean": 5.7e-17, "chain_q": 3.6e-15, "mean": 2.9e-17, "cov_within": 3.6e-15, "cov_total": 1.6e-15, "rhat": 2e-15, "inv_mass": 1.8e-15},
    "S5-C3-D1-f64": {"chain_mean": 8.5e-17, "chain_q": 1.2e-14, "mean": 9.4e-17, "cov_within": 6.4e-15, "cov_total": 7e-15, "rhat": 8.1e-16, "inv_mass": 7e-15},
    "S7-C65-D3-f32": {"chain_mean": 1.3e-16, "chain_q": 1.4e-15, "mean": 3e-16, "cov_within": 1.6e-16, "cov_total": 1.5e-16, "rhat": 5.3e-16, "inv_mass": 2.1e-16},
    "S7-C65-D3-f64": {"chain_mean": 1.9e-16, "chain_q": 2.1e-15, "mean": 1.2e-16, "cov_within": 2.4e-16, "cov_total": 1.2e-16, "rhat": 6.6e-16, "inv_mass": 1.2e-16},
    "S4-C1025-D2-f32": {"chain_mean": 0.0, "chain_q": 9.8e-16, "mean": 8.3e-18, "cov_within": 3.4e-17, "cov_total": 3.9e-17, "rhat": 3.9e-17, "inv_mass": 7e-17},
    "S4-C1025-D2-f64": {"chain_mean": 1.2e-16, "chain_q": 6.9e-16, "mean": 1.6e-16, "cov_within": 2.3e-16, "cov_total": 7.3e-17, "rhat": 2e-16, "inv_mass": 1.9e-16},
    "S600-C2-D3-f32": {"chain_mean": 1.4e-16, "chain_q": 9.5e-16, "mean": 1.1e-16, "cov_within": 6.9e-16, "cov_total": 1.8e-15, "rhat": 9.9e-16, "inv_mass": 1.7e-15},
    "S600-C2-D3-f64": {"chain_mean": 2e-16, "chain_q": 7e-16, "mean": 3.5e-17, "cov_within": 4.2e-16, "cov_total": 4.5e-16, "rhat": 2.2e-15, "inv_mass": 3.5e-16},
    "S9-C3-D17-f32": {"chain_mean": 1.4e-16, "chain_q": 1.6e-15, "mean": 1.2e-16, "cov_within": 7.4e-16, "cov_total": 8.2e-16, "rhat": 2.2e-15, "inv_mass": 8.2e-16},
    "S9-C3-D17-f64": {"chain_mean": 1.4e-16, "chain_q": 2.4e-15, "mean": 1.8e-16, "cov_within": 1.5e-15, "cov_total": 2.3e-15, "rhat": 1.1e-14, "inv_mass": 2.4e-15},
    "S5-C3-D64-f32": {"chain_mean": 8.1e-17, "chain_q": 7.6e-16, "mean": 1.9e-16, "cov_within": 5.4e-16, "cov_total": 1.3e-15, "rhat": 2.9e-15, "inv_mass": 1.3e-15},
    "S5-C3-D64-f64": {"chain_mean": 1.4e-16, "chain_q": 1.9e-15, "mean": 2e-16, "cov_within": 1.3e-15, "cov_total": 1.5e-15, "rhat": 4.6e-15, "inv_mass": 1.5e-15},
    "S3-C2-D256-f32": {"chain_mean": 4.4e-17, "chain_q": 3.9e-16, "mean": 8.7e-17, "cov_within": 5e-16, "cov_total": 1.3e-15, "rhat": 6.3e-15, "inv_mass": 1.4e-15},
    "S3-C2-D256-f64": {"chain_mean": 9.1e-17, "chain_q": 1.6e-15, "mean": 1.6e-16, "cov_within": 1.6e-15, "cov_total": 2.4e-15, "rhat": 1.2e-14, "inv_mass": 2.5e-15},
    "offset-f32": {"chain_mean": 2.1e-16, "chain_q": 1.6e-11, "mean": 1.6e-16, "cov_within": 5.2e-12, "cov_total": 7.4e-12, "rhat": 2e-12, "inv_mass": 7.4e-12},
    "offset-f64": {"chain_mean": 2.5e-16, "chain_q": 1.3e-11, "mean": 2.6e-16, "cov_within": 8.2e-12, "cov_total": 9.3e-12, "rhat": 1.1e-12, "inv_mass": 9.3e-12},
    "constant-f32": {"chain_mean": 0.0, "chain_q": 0.0, "mean": 0.0, "cov_within": 0.0, "cov_total": 9.1e-17, "rhat": 0.0, "inv_mass": 1.4e-16},
    "nan-f64": {"chain_mean": 2.4e-16, "chain_q": 2.3e-15, "mean": 1.1e-16, "cov_within": 1.2e-15, "cov_total": 1.2e-15, "rhat": 2.3e-15, "inv_mass": 1.2e-15},
}


def band(case):
    """{quantity: what the kernels may differ from the restatement by}: 4 x MEASURED, at least FLOOR."""
    return {k: max(4.0 * MEASURED[case.name][k], FLOOR) for k in QUANTITIES}


def _round_up(v):
    if v == 0.0 or not np.isfinite(v):
        return v
    e = int(np.floor(np.log10(v))) - 1
    return float("%.1e" % (np.ceil(v / 10.0 ** e) * 10.0 ** e))


if __name__ == "__main__":
    print("MEASURED = {")
    for c in CASES:
        m = measure(c)
        print('    "%s": {%s},' % (c.name, ", ".join('"%s": %r' % (k, _round_up(m[k])) for k in QUANTITIES)))
    print("}")
