"""Shared by tests/test_moments_cases_cpu.py and tests/test_gpu_moments.py: the cases of the running moments (csrc/moments.hip,
diagnostics.RunningMoments), a numpy float64 restatement of update / merge / finish in the kernels' own order of operations, an
np.longdouble two-pass computation of the same quantities, and the error band the kernels are held to.

The band: per case and quantity the error of the float64 restatement against the longdouble computation, MEASURED below; the
kernels get 4 x that, with a floor of 1e-15 (BAND).  Errors are relative to the quantity's scale: the largest |x| of the case for
the means, the largest reference value over the entries for M2 and the variances, the value itself for R-hat.

    python tests/moments_cases.py          prints the MEASURED table (float64 restatement against longdouble, this file's cases)
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

#: (S, C, D): one series; one coordinate; a chain tile edge; D over two lane tiles; many chains; more than two row segments at a tiny C D
SHAPES = [(1, 1, 1), (5, 3, 1), (7, 65, 3), (33, 64, 130), (4, 1025, 2), (600, 2, 3)]
_T = {"f32": np.float32, "f64": np.float64}
CASES = [Case("S%d-C%d-D%d-%s" % (S, C, D, t), "random", S, C, D, _T[t], 100 + 2 * i + j)
         for i, (S, C, D) in enumerate(SHAPES) for j, t in enumerate(("f32", "f64"))]
CASES += [Case("offset-%s" % t, "offset", 1000, 3, 2, _T[t], 200 + j) for j, t in enumerate(("f32", "f64"))]     # mean 1e6, sd 1
CASES += [Case("constant-f32", "constant", 40, 3, 2, np.float32, 300), Case("nan-f64", "nan", 20, 4, 3, np.float64, 301)]
IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
NAN_AT = (7, 2, 1)                           # the one NaN draw of the "nan" case: row, chain, coordinate

QUANTITIES = ("chain_mean", "chain_m2", "mean", "var_within", "var_between", "var_total", "rhat", "inv_mass")


@functools.lru_cache(maxsize=None)
def _samples(i):
    c = CASES[i]
    rng = np.random.default_rng(c.seed)
    if c.kind == "offset":
        x = 1e6 + rng.standard_normal((c.S, c.C, c.D))
    elif c.kind == "constant":
        x = np.broadcast_to(np.array([2.5, -0.1])[None, None, :] + np.arange(c.C)[None, :, None], (c.S, c.C, c.D)).copy()
    else:
        x = (np.linspace(0.5, 3.0, c.D) * rng.standard_normal((c.S, c.C, c.D)) + np.linspace(-100.0, 100.0, c.D)
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
    """Chan et al., elementwise over [C, D], counts as floats: (na, ma, qa) + (nb, mb, qb) with nb > 0."""
    if na == 0.0:
        return nb, mb.copy(), qb.copy()
    n = na + nb
    dl = mb - ma
    return n, ma + dl * (nb / n), qa + qb + dl * dl * (na * nb / n)


def welford(x):
    """x[S, C, D] float64 -> (mean, M2)[C, D]: Welford's recurrence in row order."""
    m, q = np.zeros(x.shape[1:]), np.zeros(x.shape[1:])
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(x.shape[0]):
            dl = x[k] - m
            m = m + dl / float(k + 1)
            q = q + dl * (x[k] - m)
    return m, q


class State:
    """hta_moments_update / RunningMoments.merge / hta_moments_finish in numpy float64, in the kernels' order of operations."""

    def __init__(self):
        self.n, self.mean, self.m2 = 0, None, None

    def _store(self, n, m, q):
        with np.errstate(invalid="ignore", over="ignore"):
            if self.n:
                _, m, q = chan(float(self.n), self.mean, self.m2, float(n), m, q)
        bad = ~(np.isfinite(m) & np.isfinite(q))
        self.mean, self.m2 = np.where(bad, np.nan, m), np.where(bad, np.nan, q)
        self.n += n
        return self

    def update(self, x):
        x = np.asarray(x, dtype=np.float64)
        S, C, D = x.shape
        R = DG.moments_segment_rows(S, C, D)
        n, m, q = 0.0, None, None
        with np.errstate(invalid="ignore", over="ignore"):
            for r0 in range(0, S, R):
                mb, qb = welford(x[r0:r0 + R])
                n, m, q = chan(n, m, q, float(min(S, r0 + R) - r0), mb, qb)
        return self._store(S, m, q)

    def merge(self, other):
        return self._store(other.n, other.mean, other.m2)

    @staticmethod
    def stack(parts):
        out = State()
        out.n = parts[0].n
        out.mean, out.m2 = np.concatenate([p.mean for p in parts], 0), np.concatenate([p.m2 for p in parts], 0)
        return out

    def finish(self, reg_n=REG_N, reg_floor=REG_FLOOR):
        return finish(self.n, self.mean, self.m2, reg_n, reg_floor, slices=SLICES)


def _over_chains(a, slices):
    """sum over axis 0 of a[C, D]: slice k adds the chains k, k + slices, ... in order, the slices are added in order."""
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


def finish(n, mean_c, m2_c, reg_n=REG_N, reg_floor=REG_FLOOR, slices=None):
    """The pooled statistics from per-chain (mean, M2)[C, D] of n draws, in the dtype of the inputs."""
    ft = mean_c.dtype.type
    C = mean_c.shape[0]
    n_, nc = ft(n), ft(C)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mean = _over_chains(mean_c, slices) / nc
        m2 = _over_chains(m2_c, slices)
        dm = mean_c - mean
        ssb = _over_chains(dm * dm, slices)
        vw = m2 / (n_ - ft(1)) / nc
        vb = ssb / (nc - ft(1)) if C > 1 else np.zeros_like(ssb)
        N = n_ * nc
        vt = (m2 + n_ * ssb) / (N - ft(1))
        rh = np.full(mean.shape, np.nan, mean_c.dtype)
        if n >= 2:
            pos = vw > 0
            rh = np.where(pos, np.sqrt(((n_ - ft(1)) / n_ * vw + vb) / np.where(pos, vw, ft(1))), np.where(vb > 0, np.inf, np.nan))
            rh = np.where(np.isnan(vw) | np.isnan(vb), np.nan, rh)
        im = vt * (N / (N + ft(reg_n))) + ft(reg_floor) * (ft(reg_n) / (N + ft(reg_n)))
    return dict(chain_mean=mean_c, chain_m2=m2_c, mean=mean, var_within=vw, var_between=vb, var_total=vt, rhat=rh, inv_mass=im)


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
    with np.errstate(invalid="ignore"):
        m = xl.sum(axis=0) / np.longdouble(xl.shape[0])
        q = ((xl - m) ** 2).sum(axis=0)
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

#: measured by `python tests/moments_cases.py` (x86-64: np.longdouble is the 80-bit format), rounded up to two digits;
#: tests/test_moments_cases_cpu.py::test_the_band_is_the_measured_error_of_the_restatement measures them again
MEASURED = {
    "S1-C1-D1-f32": {"chain_mean": 0.0, "chain_m2": 0.0, "mean": 0.0, "var_within": 0.0, "var_between": 0.0, "var_total": 0.0, "rhat": 0.0, "inv_mass": 0.0},
    "S1-C1-D1-f64": {"chain_mean": 0.0, "chain_m2": 0.0, "mean": 0.0, "var_within": 0.0, "var_between": 0.0, "var_total": 0.0, "rhat": 0.0, "inv_mass": 0.0},
    "S5-C3-D1-f32": {"chain_mean": 2.9e-17, "chain_m2": 5.3e-15, "mean": 8.5e-17, "var_within": 3.5e-15, "var_between": 6.9e-15, "var_total": 1.8e-15, "rhat": 2.1e-15, "inv_mass": 1.8e-15},
    "S5-C3-D1-f64": {"chain_mean": 1.2e-16, "chain_m2": 1.9e-14, "mean": 3.8e-17, "var_within": 5.2e-15, "var_between": 1.5e-14, "var_total": 7.6e-15, "rhat": 5.1e-15, "inv_mass": 7.4e-15},
    "S7-C65-D3-f32": {"chain_mean": 1.4e-16, "chain_m2": 1.2e-15, "mean": 1.8e-16, "var_within": 1.3e-16, "var_between": 1.5e-15, "var_total": 3.3e-16, "rhat": 5e-16, "inv_mass": 3.9e-16},
    "S7-C65-D3-f64": {"chain_mean": 1.7e-16, "chain_m2": 2.8e-15, "mean": 1.4e-16, "var_within": 2.8e-16, "var_between": 1.6e-15, "var_total": 3.2e-16, "rhat": 1.2e-15, "inv_mass": 2.4e-16},
    "S33-C64-D130-f32": {"chain_mean": 4.3e-16, "chain_m2": 2.7e-15, "mean": 2.3e-16, "var_within": 3.1e-16, "var_between": 1.1e-14, "var_total": 5.6e-16, "rhat": 2.2e-15, "inv_mass": 6.7e-16},
    "S33-C64-D130-f64": {"chain_mean": 4.7e-16, "chain_m2": 3.1e-15, "mean": 2.8e-16, "var_within": 3.7e-16, "var_between": 9.8e-15, "var_total": 4.9e-16, "rhat": 2.4e-15, "inv_mass": 5.4e-16},
    "S4-C1025-D2-f32": {"chain_mean": 0.0, "chain_m2": 7.3e-16, "mean": 4e-17, "var_within": 1.1e-17, "var_between": 4.7e-17, "var_total": 1.5e-16, "rhat": 7.1e-17, "inv_mass": 6.3e-17},
    "S4-C1025-D2-f64": {"chain_mean": 1.3e-16, "chain_m2": 1.2e-15, "mean": 5.6e-17, "var_within": 1.5e-16, "var_between": 4e-16, "var_total": 3.3e-16, "rhat": 5.2e-17, "inv_mass": 3.9e-16},
    "S600-C2-D3-f32": {"chain_mean": 2.3e-16, "chain_m2": 2.9e-16, "mean": 2.1e-16, "var_within": 2.9e-16, "var_between": 1.1e-13, "var_total": 7.1e-16, "rhat": 7.9e-15, "inv_mass": 7e-16},
    "S600-C2-D3-f64": {"chain_mean": 2.3e-16, "chain_m2": 9.7e-16, "mean": 1.4e-16, "var_within": 3.1e-16, "var_between": 7.7e-14, "var_total": 5.1e-16, "rhat": 8.6e-15, "inv_mass": 4.3e-16},
    "offset-f32": {"chain_mean": 2.7e-16, "chain_m2": 2.3e-11, "mean": 3.5e-17, "var_within": 1e-11, "var_between": 4.9e-09, "var_total": 1.8e-11, "rhat": 6e-12, "inv_mass": 1.8e-11},
    "offset-f64": {"chain_mean": 2.5e-16, "chain_m2": 1.5e-11, "mean": 1.2e-16, "var_within": 1.3e-11, "var_between": 3e-09, "var_total": 1.5e-11, "rhat": 4.5e-12, "inv_mass": 1.5e-11},
    "constant-f32": {"chain_mean": 0.0, "chain_m2": 0.0, "mean": 0.0, "var_within": 0.0, "var_between": 5.6e-17, "var_total": 9.1e-17, "rhat": 0.0, "inv_mass": 1.3e-16},
    "nan-f64": {"chain_mean": 1.9e-16, "chain_m2": 8.3e-16, "mean": 9e-17, "var_within": 5.4e-16, "var_between": 7.3e-14, "var_total": 6.3e-16, "rhat": 1.2e-14, "inv_mass": 6.3e-16},
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
