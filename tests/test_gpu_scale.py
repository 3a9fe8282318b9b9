"""GPU parity at the chain counts the published sweeps run at (README: `bench.py --sweep` 2^14 ... 2^22 chains, the compiled-callback rows
at 65 536 chains): the launches whose shape the small-shape suite never reaches - 32-bit lane offsets next to their guards, grids of 10^5
workgroups, grid-stride loops past their clamp, the host's chunking by WS_CAP / PREDRAW_CAP, sample rows past element 2^31.

Philox streams are keyed by the global chain id, so the oracle reproduces any subset of the chains of a launch: every case is checked chain by
chain on the probe set of tests/scale_cases.py (first lanes / waves / blocks, last chains, both sides of every power of two and of every
route threshold, 64 fixed random ids).  The GPU result is reduced to the probe chains on the device (index_select) before it is copied.

Tolerances are the ones the small-shape test of the same route and type uses (named next to each number): the arithmetic of a chain does not
depend on the chain count - read from the kernels (one chain per quad / lane / wave, no reduction across chains), not measured.  Chains
allowed outside the band: 0.5 % of the probe chains and at most 2 (scale_cases.allowed_share: none below 200 probe chains);
tests/test_scale_cases.py holds the cases away from borderline Metropolis decisions on the CPU.  Chains outside the band are printed with
their ids: a launch-shape error shows as a run of adjacent or all-high ids, a borderline decision as an isolated one.  Every case asserts the
route it ran on (hta_last_route()).
"""
import numpy as np
import pytest
import torch

import hmc_oracle as O
import scale_cases as SC
from test_gpu_hmc import _compare_runs

pytestmark = pytest.mark.gpu
NP = {torch.float32: np.float32, torch.float64: np.float64}


@pytest.fixture(scope="module")
def ht():
    import hamiltorch_amd
    assert torch.cuda.is_available()
    return hamiltorch_amd


def dev():
    return torch.device("cuda:0")


def route():
    from hamiltorch_amd import _abi
    return _abi.last_route()


def init_state_device(C, D, scale):
    """scale_cases.init_state for ALL chains, on the device, bit for bit (float64)"""
    c = torch.arange(C, dtype=torch.int64, device=dev())[:, None]
    j = torch.arange(D, dtype=torch.int64, device=dev())[None, :]
    m = (c * 2654435761 + j * 40503) % 65521
    return ((m.to(torch.float64) * 2.0 / 65521.0) - 1.0) * float(scale)


def probe_rows(out, idt):
    """[rows, probe chains, D] of a sample() result, reduced on the device (the lazy list's backing tensor where there is one)"""
    if hasattr(out, "tensor") and not getattr(out, "_done", True):
        return out.tensor.index_select(1, idt)
    return torch.stack([r.index_select(0, idt) for r in out])


def check(tag, ids, rows, ref, tol, final=None, rejected=None, rej_ref=None):
    """rows [S, n, D] (device) against the oracle's list `ref` on the probe chains `ids`: _compare_runs of tests/test_gpu_hmc.py with the
    scale tests' share; then the final state against the oracle's last row and the reject counts of the chains inside the band."""
    share = SC.allowed_share(len(ids))
    got = rows.cpu().numpy(); want = np.stack(ref)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    err = np.abs(got - want).max(axis=(0, 2))
    out = ~(err <= tol)
    print("%s: %d probe chains, largest difference %.3g, outside %.1e: %s" % (tag, len(ids), np.nanmax(err), tol, ids[out].tolist()))
    bad = _compare_runs(list(rows), ref, tol, share)
    if final is not None:
        _compare_runs([final], [ref[-1]], tol, share)
    if rejected is not None:
        np.testing.assert_array_equal(np.asarray(rejected)[~bad], np.asarray(rej_ref)[~bad], err_msg=tag + ": reject counts")
    return bad


# =====================================================================================================================================
# Gaussian HMC
# =====================================================================================================================================
def _ws_chunk(C, D, N):
    """Trajectories per launch of _GaussianHMC.advance for this shape (the cap is read from samplers.py)"""
    from hamiltorch_amd import _abi, samplers
    cap = samplers._GaussianHMC.WS_CAP
    fixed = _abi.gaussian_workspace_bytes(C, D, 0, 4)
    per = _abi.gaussian_workspace_bytes(C, D, 1, 4) - fixed
    assert fixed + per <= cap
    return max(1, min(N, (cap - fixed) // per))


def _gauss_case(ht, case, monkeypatch):
    from hamiltorch_amd import _abi
    C, D, N, L, burn, eps, seed = (case[k] for k in ("C", "D", "N", "L", "burn", "eps", "seed"))
    off = case.get("off", 0)
    ids = SC.probe_ids(C)
    idt = torch.from_numpy(ids).to(dev())
    P, mu = SC.gauss_model(D)
    t = ht.GaussianTarget(torch.tensor(mu, dtype=torch.float32, device=dev()), precision=torch.tensor(P, dtype=torch.float32, device=dev()),
                          normalized=False)
    th0 = init_state_device(C, D, 0.5).float().contiguous()
    assert np.array_equal(th0.index_select(0, idt).cpu().numpy(), SC.gauss_start(case, ids).astype(np.float32))
    ref, info = SC.gauss_oracle(case, ids)
    rej_ref = np.rint((1.0 - info["acc_rate"]) * N).astype(np.int64)
    tol = 2e-4                      # tests/test_gpu_hmc.py::test_sample_fused_vs_oracle, float32
    for k, v in case.get("tuning", {}).items():
        _abi.set_tuning(k, v)
    try:
        # ---- the C ABI, with a caller's workspace
        chunk = case.get("abi_chunk", N)
        chunk = _ws_chunk(C, D, N) if chunk == "sample" else chunk
        cur = th0.clone()
        samples = torch.empty(SC.num_rows(N, burn), C, D, device=dev())
        samples[0].copy_(th0)
        rej = torch.zeros(C, dtype=torch.int32, device=dev())
        ws = torch.empty(_abi.gaussian_workspace_bytes(C, D, chunk, 4), dtype=torch.uint8, device=dev())
        if case.get("prepared"):
            _abi.hmc_gaussian_prepare(th0, t.precision, 0, None, C, D, chunk, ws)
        routes = set()
        for start in range(0, N, chunk):
            _abi.hmc_gaussian_sample(cur, th0, t.precision, t.mean, t.log_norm, 0, None, None, L, eps, min(chunk, N - start), start, burn,
                                     seed, off, samples, rej, workspace=ws)
            routes.add(route())
        torch.cuda.synchronize()
        if case.get("prepared"):
            _abi.hmc_gaussian_forget(ws)
        assert routes == {case["abi"]}, (case["id"], routes)
        rows, fin, rj = samples.index_select(1, idt), cur.index_select(0, idt), rej.index_select(0, idt).cpu().numpy()
        del samples, ws, cur, rej
        check(case["id"] + " / C ABI", ids, rows, ref, tol, fin, rj, rej_ref)
        # ---- sample()
        launches = []
        real = _abi.hmc_gaussian_sample

        def counted(*a, **k):
            launches.append(a[10])
            return real(*a, **k)
        monkeypatch.setattr(_abi, "hmc_gaussian_sample", counted)
        out, acc = ht.sample(t, th0, num_samples=N, num_steps_per_sample=L, step_size=eps, burn=burn, debug=2, verbose=False, seed=seed,
                             chain_offset=off)
        monkeypatch.setattr(_abi, "hmc_gaussian_sample", real)
        assert route() == case["sample"], (case["id"], route())
        print("%s / sample(): trajectories per launch %s" % (case["id"], launches))
        assert sum(launches) == N and len(launches) >= case.get("min_launches", 1), launches
        rows = probe_rows(out, idt)
        rj = np.rint((1.0 - acc.index_select(0, idt).cpu().numpy()) * N).astype(np.int64)
        del out
        check(case["id"] + " / sample()", ids, rows, ref, tol, rows[-1], rj, rej_ref)
    finally:
        _abi.reset_tuning()
        t.__dict__.pop("_hta_hmc_ws", None)
        _abi.free_scratch(0)
        torch.cuda.empty_cache()


@pytest.mark.parametrize("case", SC.GAUSS_CASES, ids=[c["id"] for c in SC.GAUSS_CASES])
def test_gaussian_hmc_at_scale_vs_oracle(ht, case, monkeypatch):
    """BASELINE config 2's target (and D = 1 / 4 / 64 variants) through the C ABI and through sample() at the sweep's chain counts and on
    both sides of every route threshold: samples, final state and reject counts of the probe chains against oracle.sample_hmc."""
    _gauss_case(ht, case, monkeypatch)


def test_gaussian_rows_past_2_31_elements(ht, monkeypatch):
    """514 rows of 2^20 chains x 4 coordinates: the sample tensor passes element 2^31 (row 512) and byte 2^32 (row 256) / 2^33; every row of
    the probe chains is compared, so the first and the last row and the rows on both sides of those marks are.  Needs ~11 GB; skipped only
    when less than three times that is free."""
    case = SC.BIG_CASE
    C, D, N = case["C"], case["D"], case["N"]
    rows = SC.num_rows(N, case["burn"])
    assert rows * C * D > 1 << 31 and (rows - 1) * C * D * 4 > 1 << 33
    from hamiltorch_amd import _abi
    need = rows * C * D * 4 + _abi.gaussian_workspace_bytes(C, D, case["abi_chunk"], 4) + 4 * C * D * 4
    free, total = torch.cuda.mem_get_info()
    if free < 3 * need:
        pytest.skip("%.1f GB of device memory free, the case needs %.1f GB and asks for three times that" % (free / 1e9, need / 1e9))
    _gauss_case(ht, case, monkeypatch)


# =====================================================================================================================================
# compiled callbacks at the published 65 536 chains
# =====================================================================================================================================
def _funnel():
    from test_gpu_jit import funnel_device
    return funnel_device


def _cb_run(ht, case, dtype, idt, th0):
    out, acc = ht.sample(_funnel(), th0, num_samples=case["N"], num_steps_per_sample=case["L"], step_size=case["eps"], burn=case["burn"],
                         debug=2, verbose=False, seed=case["seed"])
    r = route()
    assert "hta_cb_hmc_kernel<D=11,%s,mass=0," % ("f32" if dtype == torch.float32 else "f64") in r, r
    rows = probe_rows(out, idt)
    return rows, acc.index_select(0, idt).cpu(), r


# tolerances: tests/test_gpu_jit.py::test_compiled_funnel_vs_oracle
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-4), (torch.float64, 1e-9)], ids=["f32", "f64"])
@pytest.mark.parametrize("case", SC.CB_HMC_CASES, ids=[c["id"] for c in SC.CB_HMC_CASES])
def test_compiled_hmc_at_scale_vs_oracle(ht, case, dtype, tol, monkeypatch):
    """hta_cb_hmc_kernel on the 11-D funnel at 65 536 chains (records pre-drawn) and at 131 136 (past PREDRAW_MAX_CHAINS: drawn in the
    lane), 8 x 25 steps: probe chains against the oracle; where both forms are allowed the two are equal bit for bit."""
    from hamiltorch_amd import samplers
    C = case["C"]
    ids = SC.probe_ids(C)
    idt = torch.from_numpy(ids).to(dev())
    th0 = init_state_device(C, SC.CB_D, SC.CB_SCALE).float().to(dtype).contiguous()
    ref, info = SC.cb_hmc_oracle(case, ids, NP[dtype])
    rej_ref = np.rint((1.0 - info["acc_rate"]) * case["N"])
    rows, acc, r = _cb_run(ht, case, dtype, idt, th0)
    pre = C <= samplers._CompiledHMC.PREDRAW_MAX_CHAINS
    assert (",predrawn>" in r) == pre, r
    check("%s %s (%s)" % (case["id"], dtype, r), ids, rows, ref, tol, rows[-1], np.rint((1.0 - acc.numpy()) * case["N"]), rej_ref)
    if pre:
        monkeypatch.setenv("HAMILTORCH_AMD_JIT_PREDRAW", "0")
        rows2, acc2, r2 = _cb_run(ht, case, dtype, idt, th0)
        assert "predrawn" not in r2, r2
        diff = (rows != rows2).any(dim=2).any(dim=0).cpu().numpy()
        print("pre-drawn against in-lane draws: probe chains that differ %s" % ids[diff].tolist())
        assert torch.equal(rows, rows2) and torch.equal(acc, acc2)


def test_compiled_hmc_predraw_cap_chunks(ht, monkeypatch):
    """100 trajectories of 65 536 chains: PREDRAW_CAP cuts the run into launches; equal bit for bit to the same run with the draws in the lane
    (one launch), and within tolerance of the oracle (burn-in and the Q2 reset inside the first launch)."""
    from hamiltorch_amd import samplers
    from hamiltorch_amd.jit import runtime
    case, dtype = SC.CB_CAP_CASE, torch.float32
    C, N = case["C"], case["N"]
    per = runtime.hmc_predraw_bytes(C, SC.CB_D, 1, 4)
    assert samplers._CompiledHMC.PREDRAW_CAP // per < N, "the run must not fit one launch's records"
    ids = SC.probe_ids(C)
    idt = torch.from_numpy(ids).to(dev())
    th0 = init_state_device(C, SC.CB_D, SC.CB_SCALE).float().contiguous()
    launches = []
    real = runtime.hmc_sample

    def counted(*a, **k):
        launches.append(a[8])
        return real(*a, **k)
    monkeypatch.setattr(runtime, "hmc_sample", counted)
    rows, acc, r = _cb_run(ht, case, dtype, idt, th0)
    assert ",predrawn>" in r and len(launches) > 1 and sum(launches) == N, (r, launches)
    print("trajectories per launch: %s" % launches)
    ref, info = SC.cb_hmc_oracle(case, ids, np.float32)
    check(case["id"], ids, rows, ref, 2e-4, rows[-1], np.rint((1.0 - acc.numpy()) * N), np.rint((1.0 - info["acc_rate"]) * N))
    del launches[:]
    monkeypatch.setenv("HAMILTORCH_AMD_JIT_PREDRAW", "0")
    rows2, acc2, r2 = _cb_run(ht, case, dtype, idt, th0)
    assert "predrawn" not in r2 and launches == [N], (r2, launches)
    diff = (rows != rows2).any(dim=2).any(dim=0).cpu().numpy()
    print("chunked pre-drawn run against the one-launch in-lane run: probe chains that differ %s" % ids[diff].tolist())
    assert torch.equal(rows, rows2) and torch.equal(acc, acc2)


@pytest.mark.parametrize("case", SC.SPLIT_CASES, ids=[c["id"] for c in SC.SPLIT_CASES])
def test_compiled_split_at_scale_vs_oracle(ht, case):
    """hta_cb_split_kernel, the logistic list of tests/test_gpu_jit_split.py (M = 3, L = 8) at 65 536 chains; 2e-4: test_compiled_list_vs_oracle"""
    import test_gpu_jit_split as TS
    dtype, C = torch.float32, case["C"]
    ids = SC.probe_ids(C)
    idt = torch.from_numpy(ids).to(dev())
    th0 = init_state_device(C, SC.SPLIT_D, SC.SPLIT_SCALE).float().contiguous()
    out, acc = ht.sample(TS.logistic_closures(dtype), th0, num_samples=case["N"], num_steps_per_sample=case["L"], step_size=case["eps"],
                         burn=case["burn"], integrator=TS.integrator(ht, case["kind"]), debug=2, verbose=False, seed=case["seed"])
    r = route()
    assert "hta_cb_split_kernel<D=6,M=3,f32,mass=0,kind=%s," % case["kind"] in r, r
    ref, info = SC.split_oracle(case, ids, np.float32, lambda dt: TS.logistic_oracle(dtype))
    rows = probe_rows(out, idt)
    check(case["id"], ids, rows, ref, 2e-4, rows[-1], np.rint((1.0 - acc.index_select(0, idt).cpu().numpy()) * case["N"]),
          np.rint((1.0 - info["acc_rate"]) * case["N"]))


# tolerances: tests/test_gpu_jit.py::test_fused_rmhmc_kernel_vs_oracle
@pytest.mark.parametrize("case", SC.RMHMC_CASES, ids=[c["id"] for c in SC.RMHMC_CASES])
def test_compiled_rmhmc_at_scale_vs_oracle(ht, case):
    """hta_cb_rmhmc_kernel on the 11-D funnel (jitter 1e-3, alpha = 1): 65 536 chains in float32, 4096 in float64, 3 trajectories"""
    from test_gpu_jit import scaled_funnel
    dtype, tol = (torch.float32, 5e-3) if case["dtype"] == "f32" else (torch.float64, 1e-7)
    C, D = case["C"], SC.CB_D
    ids = SC.probe_ids(C)
    idt = torch.from_numpy(ids).to(dev())
    th0 = init_state_device(C, D, SC.RMHMC_SCALE).float().to(dtype).contiguous()
    out, acc = ht.sample(scaled_funnel(np.ones(D - 1)), th0, num_samples=case["N"], num_steps_per_sample=case["L"], step_size=case["eps"],
                         burn=case["burn"], jitter=case["jitter"], softabs_const=case["alpha"], explicit_binding_const=case["omega"],
                         sampler=ht.Sampler.RMHMC, integrator=ht.Integrator.EXPLICIT, metric=ht.Metric.SOFTABS, debug=2, verbose=False,
                         seed=case["seed"])
    r = route()
    assert "hta_cb_rmhmc_kernel<D=11,%s,jitter=1," % case["dtype"] in r, r
    ref, info = SC.rmhmc_oracle(case, ids, NP[dtype])
    rows = probe_rows(out, idt)
    check(case["id"], ids, rows, ref, tol, rows[-1], np.rint((1.0 - acc.index_select(0, idt).cpu().numpy()) * case["N"]),
          np.rint((1.0 - info["acc_rate"]) * case["N"]))


# =====================================================================================================================================
# hta_net_forward: the grid-stride over samples past the grid.y clamp of 32 768
# =====================================================================================================================================
def _forward64(dims, act, th, X):
    """out[S, N, O] of the flattened nets th[S, P] (per Linear: weight [out, in] row-major, then bias) in float64"""
    f = {"relu": lambda z: np.maximum(z, 0.0), "tanh": np.tanh, "sigmoid": lambda z: 1.0 / (1.0 + np.exp(-z))}[act]
    h = np.broadcast_to(X.astype(np.float64), (th.shape[0],) + X.shape)
    off = 0
    for l in range(len(dims) - 1):
        i, o = dims[l], dims[l + 1]
        W = th[:, off:off + o * i].reshape(-1, o, i).astype(np.float64); b = th[:, off + o * i:off + o * i + o].astype(np.float64)
        off += o * i + o
        h = np.einsum("sni,soi->sno", h, W) + b[:, None, :]
        if l < len(dims) - 2:
            h = f(h)
    assert off == th.shape[1]
    return h


@pytest.mark.parametrize("N", [65, 1])
@pytest.mark.parametrize("dims,act", [([3, 9, 1], "relu"), ([2, 300, 2], "tanh"), ([4, 3], "relu")], ids=["3-9-1", "2-300-2-streamed", "4-3-no-hidden"])
def test_net_forward_past_the_grid_clamp(ht, dims, act, N):
    """40 000 parameter rows (grid.y is clamped to 32 768: rows 32 768 ... 39 999 are the second pass of the loop over samples): rows 0,
    32 767, 32 768, 39 999 and 16 random ones against a float64 forward pass (oracle.MLPRegressionTarget.predict for the one-output net);
    tolerance of tests/test_gpu_predict.py::test_native_regression_predict_vs_oracle_and_torch_path.  [4, 3]: a net with no hidden layer."""
    from hamiltorch_amd import _abi
    S = 40000
    Dp = sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))
    g = torch.Generator(device=dev()).manual_seed(7)
    th = 0.4 * torch.randn(S, Dp, generator=g, device=dev())
    X = torch.randn(N, dims[0], generator=g, device=dev())
    out = torch.full((S, N, dims[-1]), float("nan"), device=dev())
    _abi.net_forward(th, dims, act, X, out)
    assert route() == "net_forward_kernel<float>", route()
    assert bool(torch.isfinite(out).all()), "every (sample, point, output) is written"
    rows = np.unique(np.concatenate([[0, 32767, 32768, S - 1], np.random.default_rng(3).integers(0, S, 16)]))
    rt = torch.from_numpy(rows).to(dev())
    got = out.index_select(0, rt).cpu().numpy()
    thr, Xh = th.index_select(0, rt).cpu().numpy(), X.cpu().numpy()
    want = _forward64(dims, act, thr, Xh)
    if dims[-1] == 1:
        o = O.MLPRegressionTarget(dims, Xh, np.zeros((N, 1), np.float32), [1.0] * (2 * (len(dims) - 1)), 1.0, 1.0, act)
        want_o = o.predict(thr.astype(np.float64))
        np.testing.assert_allclose(want, want_o, rtol=1e-12, atol=1e-12)
        want = want_o
    tol = 2e-4
    np.testing.assert_allclose(got, want, rtol=tol, atol=tol * max(1.0, np.abs(want).max()))
