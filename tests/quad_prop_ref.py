"""numpy restatement of the quad route's propagated trajectory (hamiltorch_amd/csrc/quad_prop.hpp, quad_body: PROP), shared by
tests/test_quad_prop_coeffs.py, tests/test_quad_prop_cases_cpu.py and tests/test_gpu_quad_prop.py.  Nothing of the library runs here.

coeffs(): the half kick, the L steps  y += eps r ; r += nel y  and the closing half kick in float64 (Python floats: IEEE double, one
rounding per multiply and per add, no contraction) on the basis inputs (1, 0) and (0, 1), from the float32 constants eps,
nel = -(eps lam), hl = (0.5 eps) lam promoted to double; the results rounded to float32.

eig_block(): eig_small_kernel's outputs (hmc_gauss_small_dev.hpp) - lam, Qt, Tin, Tout of the whitened precision matrix - from
numpy's float64 eigh, rounded to float32.  The kernel diagonalises with a float64 Jacobi: the two agree to float64 rounding up to the
order and sign of the eigenvectors, which the trajectory does not depend on.

propagated_run(): sample() of a case of tests/gauss_traj_cases.py as the propagator twins compute it, in float32 numpy: the state
carried in the eigenbasis, energies doubled, records [Qt z, 2 log u], the Q2 rule, rows q = mu + Tout y of accepted proposals."""
import numpy as np

import hmc_oracle as O

F32 = np.float32


def lane_constants(eps, lam):
    """(eps, nel, hl) of a live lane as quad_body forms them in float32."""
    eps, lam = F32(eps), F32(lam)
    return eps, F32(-(eps * lam)), F32(F32(F32(0.5) * eps) * lam)


def coeffs(eps32, nel32, hl32, L):
    """(a, b, c, d) in float32: y = a yc + b z, r = c yc + d z."""
    eps, nel, hl = float(F32(eps32)), float(F32(nel32)), float(F32(hl32))
    out = []
    for yc, z in ((1.0, 0.0), (0.0, 1.0)):
        y, r = yc, z - hl * yc
        for _ in range(int(L)):
            y = y + eps * r
            r = r + nel * y
        r = r + hl * y
        out.append((y, r))
    with np.errstate(over="ignore", invalid="ignore"):
        return F32(out[0][0]), F32(out[1][0]), F32(out[0][1]), F32(out[1][1])


def eig_block(P32, mass_kind, mass_factor32):
    """(lam[D], Qt[D, D], Tin[D, D], Tout[D, D]) in float32."""
    D = P32.shape[0]
    A = 0.5 * (P32.astype(np.float64) + P32.astype(np.float64).T)
    if mass_kind == 0:
        Lm = np.eye(D)
    elif mass_kind == 1:
        Lm = np.diag(mass_factor32.astype(np.float64))
    else:
        Lm = np.tril(mass_factor32.astype(np.float64))
    Li = np.linalg.inv(Lm)
    A = Li @ A @ Li.T
    lam, Q = np.linalg.eigh(0.5 * (A + A.T))
    return lam.astype(F32), Q.T.astype(F32), (Q.T @ Lm.T).astype(F32), (Li.T @ Q).astype(F32)


def _matvec32(M, v):
    """M[D, D] (float32) times v[C, D] (float32), accumulated in float32 in the kernels' order (first product, then fused adds; numpy
    has no fma: one more rounding per term, inside every band this is held to)."""
    acc = M[None, :, 0] * v[:, 0:1]
    for i in range(1, M.shape[1]):
        acc = (acc + M[None, :, i] * v[:, i:i + 1]).astype(F32)
    return acc.astype(F32)


def propagated_run(G, case, chains=None):
    """(rows[T - burn, c, D], h_old[T, c], h_new[T, c], accept[T, c], rejected[c], cur[c, D]) in float32 / bool of `case` (G:
    tests/gauss_traj_cases.py) on `chains` (default: its probe chains)."""
    chains = G.probe_chains(case) if chains is None else np.asarray(chains)
    D, L = case.D, case.L
    P, mu = G.inputs_of(D)
    kind, _, mf = G.mass_operands(case, F32)
    lam, Qt, Tin, Tout = eig_block(P, kind, mf)
    eps = F32(G.eps_of(case))
    co = np.array([coeffs(*lane_constants(eps, lam[k]), L) for k in range(D)], dtype=F32)      # [D, 4]
    a, b, c, d = (co[None, :, j] for j in range(4))
    log_norm = F32(G.log_norm(D))
    th0 = G.starts(case, chains)
    draws = O.PhiloxDraws(case.seed, G.CHAIN_OFFSET + chains, F32)
    to_y = lambda q: _matvec32(Tin, (q - mu[None, :]).astype(F32))      # noqa: E731
    st = {"yc": to_y(th0)}
    st["potc"] = (lam[None, :] * st["yc"] * st["yc"]).astype(F32)
    h_old, h_new, accept = [], [], []

    def propose(n, cur):
        yc, potc = st["yc"], st["potc"]
        z = _matvec32(Qt, draws.normals(n, D).astype(F32))
        lu2 = (F32(2.0) * np.log(draws.mh_uniform(n).astype(F32))).astype(F32)
        with np.errstate(over="ignore", invalid="ignore"):
            eo = (z * z + potc).astype(F32)
            y = (b * z + (a * yc).astype(F32)).astype(F32)
            r = (d * z + (c * yc).astype(F32)).astype(F32)
            pot1 = ((lam[None, :] * y).astype(F32) * y).astype(F32)
            en = (r * r + pot1).astype(F32)
            dH = (eo - en).astype(F32).sum(axis=1, dtype=F32)
            acc = dH >= lu2                                             # (NaN and -inf reject)
        h_old.append((F32(0.5) * eo.sum(axis=1, dtype=F32) - log_norm).astype(F32))
        h_new.append((F32(0.5) * en.sum(axis=1, dtype=F32) - log_norm).astype(F32))
        accept.append(acc.copy())
        yc = np.where(acc[:, None], y, yc)
        potc = np.where(acc[:, None], pot1, potc)
        if n == case.burn + 1:                                          # Q2: a rejection goes back to params_init itself
            y0 = to_y(th0)
            yc = np.where(acc[:, None], yc, y0)
            potc = np.where(acc[:, None], potc, (lam[None, :] * y0 * y0).astype(F32))
        st["yc"], st["potc"] = yc.astype(F32), potc.astype(F32)
        with np.errstate(over="ignore", invalid="ignore"):
            return (mu[None, :] + _matvec32(Tout, y)).astype(F32), acc

    # oracle/hmc_oracle.py:sample_chain_driver's bookkeeping, with the state handed back kept as well
    rows, cur, burn_prev = [th0.copy()], th0.copy(), th0.copy()
    rejected = np.zeros(len(chains), dtype=np.int64)
    for n in range(case.ntraj):
        new, acc = propose(n, cur)
        rejected += ~acc
        if n > case.burn:
            cur = np.where(acc[:, None], new, rows[-1])
            rows.append(cur)
        else:
            burn_prev = np.where(acc[:, None], new, burn_prev)
            cur = burn_prev
    return np.stack(rows), np.stack(h_old), np.stack(h_new), np.stack(accept), rejected, cur
