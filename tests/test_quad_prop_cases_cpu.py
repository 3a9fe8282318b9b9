"""CPU: do the oracle bands of tests/gauss_traj_cases.py hold for the quad route's PROPAGATED trajectory (quad_body: PROP - the L steps
applied as one precomputed linear map)?  Decided here without a GPU: tests/quad_prop_ref.py:propagated_run restates the twins'
arithmetic in float32 numpy, and every case of the table that reaches a quad kernel (D <= 4 with a workspace: the routes quad_diag,
quad_two, quad_one) is held to the float64 oracle exactly as tests/test_gpu_gauss_traj.py holds the kernels:
  - H_old and H_new of trajectory 0 on every compared chain inside h_tol;
  - rows and the state handed back inside row_band, on every chain (the restatement has no borderline chain to excuse: see below);
  - accept[T, c], the reject counts and the acceptance rate equal to the oracle's on every chain whose guard_margin, at every
    trajectory, is above the band: above the row band as a plain number (margin and band are both relative quantities), or, in the
    margin's own unit, further from its threshold than the two energies of that trajectory may be off together
    (h_tol(H_old) + h_tol(H_new)) - the second admits more chains and is the one a decision can actually feel.  The number of
    compared chains is printed; at least half of every case's chains must qualify.
The bands, the cases and the reference are the table's own; nothing here is fitted to an output."""
import numpy as np
import pytest

import gauss_traj_cases as G
import quad_prop_ref as R

QUAD_ROUTES = ("quad_diag", "quad_two", "quad_one")
IDS = [c.id for c in G.TABLE if any(r in QUAD_ROUTES and G.expected_route(c, r).startswith("hmc_gauss_quad") for r in c.routes)]


def test_the_cases_are_the_tables_quad_cases():
    assert set(IDS) == {"r1", "r2", "r3", "r4", "r3d", "r3f", "r3bm1", "r3b0", "r3b7", "q15", "q16", "q17", "qo1", "qo2", "qo3", "qo4"}


@pytest.mark.parametrize("cid", IDS)
def test_propagated_trajectory_is_inside_the_oracle_bands(cid):
    case = G.CASES[cid]
    ref = G.reference(cid)
    rows, h_old, h_new, accept, rejected, cur = R.propagated_run(G, case)
    name = "hmc_gauss_quad_kernel"
    band = G.row_band("f32", name, case.D, ref.rows)
    # energies of trajectory 0
    for got, want, what in ((h_old[0], ref.h_old[0], "H_old"), (h_new[0], ref.h_new[0], "H_new")):
        tol = G.h_tol("f32", case, want)
        share = float((np.abs(got - want) / tol).max())
        print("%s %s: largest share of its tolerance %.3g" % (cid, what, share))
        assert share <= 1.0, (cid, what, share)
    # rows and the state handed back
    out = G.outside(rows.astype(np.float64), cur.astype(np.float64), ref, band)
    err = max(float(np.abs(rows - ref.rows).max()), float(np.abs(cur - ref.cur).max()))
    print("%s rows: largest error %.3g, band %.3g, chains outside %d of %d" % (cid, err, band, int(out.sum()), out.size))
    assert not out.any(), (cid, err, band)
    # decisions: every chain has its margin, and every decision is the oracle's
    margin = G.guard_margin(ref)
    scale = np.maximum(1.0, np.maximum(np.abs(ref.h_old), np.abs(ref.h_new)))
    clear = ((margin > band) | (margin * scale > G.h_tol("f32", case, ref.h_old) + G.h_tol("f32", case, ref.h_new))).all(axis=0)
    print("%s decisions: %d of %d chains compared, closest compared decision %.3g max(1, |H|)" % (cid, int(clear.sum()), clear.size, float(margin[:, clear].min())))
    assert 2 * int(clear.sum()) >= clear.size, (cid, int(clear.sum()))
    assert np.array_equal(accept[:, clear], ref.accept[:, clear]), cid
    assert np.array_equal(rejected[clear], ref.rejected[clear]), cid
    assert np.array_equal(1.0 - rejected[clear] / float(case.ntraj), ref.acc_rate[clear]), cid
