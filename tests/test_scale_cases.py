"""CPU: the case list of tests/test_gpu_scale.py (tests/scale_cases.py) - the probe set, and that no case rests on a borderline
Metropolis decision: the oracle in fp32 and the oracle in fp64 take the same accept decisions on every case's probe chains and stay
well inside the band the GPU comparison uses, so a chain outside the band on the GPU is the kernel's and not the case's."""
import numpy as np
import pytest

import scale_cases as SC


def _powers(C):
    e, out = 1 << 12, []
    while e < C:
        out.append(e)
        e <<= 1
    return out


@pytest.mark.parametrize("C", [64, 1000, 4096, 4104, 1 << 14, 1 << 16, 65544, (1 << 17) + 64, 1 << 18, 1 << 20, (1 << 20) + 64, 1 << 22])
def test_probe_ids(C):
    ids = SC.probe_ids(C)
    assert ids.dtype == np.int64 and np.all(np.diff(ids) > 0), "sorted, unique"
    assert ids[0] == 0 and ids[-1] == C - 1, "first and last chain"
    assert ids.min() >= 0 and ids.max() < C and len(ids) <= 400
    have = set(ids.tolist())
    for want in [0, 1, 15, 16, 63, 64, 255, 256, 1023, 1024, C - 1, C - 2, C - 64, C - 65]:
        assert want in have or not (0 <= want < C), want
    for e in _powers(C) + list(SC.EDGES):
        for want in (e - 1, e, e + 1):
            assert want in have or want >= C, (e, want)
    # the random part is there and is the same from call to call
    assert len(have - set(SC.probe_ids(C, edges=()).tolist())) <= 3 * len(SC.EDGES)
    assert np.array_equal(ids, SC.probe_ids(C))
    if C >= 1 << 14:
        assert len(ids) >= 64


def test_init_state_is_a_pure_function_of_the_chain_id():
    a = SC.init_state(np.arange(100), 4, 0.5)
    b = SC.init_state(np.array([7, 99]), 4, 0.5)
    assert np.array_equal(a[[7, 99]], b) and np.abs(a).max() <= 0.5 and len(np.unique(a[:, 0])) == 100
    big = SC.init_state(np.array([(1 << 22) - 1]), 3, 0.5)          # (no int64 overflow at the largest launch)
    m = ((((1 << 22) - 1) * 2654435761) % 65521)
    assert big[0, 0] == ((m * 2.0 / 65521.0) - 1.0) * 0.5


def _decisions(run, case):
    ids = SC.probe_ids(case["C"])
    r32, i32 = run(case, ids, np.float32)
    r64, i64 = run(case, ids, np.float64)
    dev = np.abs(np.stack(r32).astype(np.float64) - np.stack(r64)).max(axis=(0, 2))
    same = np.array_equal(np.stack(i32["accept"]), np.stack(i64["accept"]))
    return ids, same, dev


def _split_oracle(case, ids, dtype):
    import torch
    from test_gpu_jit_split import logistic_oracle
    return SC.split_oracle(case, ids, dtype, lambda dt: logistic_oracle(torch.float32 if dt == np.float32 else torch.float64))


FP32_CASES = ([(SC.gauss_oracle, c, 2e-4) for c in SC.GAUSS_CASES + [SC.BIG_CASE]]
              + [(SC.cb_hmc_oracle, c, 2e-4) for c in SC.CB_HMC_CASES + [SC.CB_CAP_CASE]]
              + [(_split_oracle, c, 2e-4) for c in SC.SPLIT_CASES]
              + [(SC.rmhmc_oracle, c, 5e-3) for c in SC.RMHMC_CASES if c["dtype"] == "f32"])


@pytest.mark.parametrize("run,case,tol", FP32_CASES, ids=[c["id"] for _, c, _ in FP32_CASES])
def test_scale_cases_have_no_borderline_decisions(run, case, tol):
    """Every fp32 case: identical accept decisions of the oracle in fp32 and in fp64 on the probe chains (same fp32 start, same Philox
    streams), and the two runs within a quarter of the band the GPU comparison allows - the other three quarters are the kernel's
    (contracted multiply-adds, another summation order)."""
    ids, same, dev = _decisions(run, case)
    print("%s: %d probe chains, fp32 against fp64 oracle: largest difference %.3g" % (case["id"], len(ids), dev.max()))
    assert same, "a probe chain of %s takes different decisions in fp32 and fp64: change the case's seed" % case["id"]
    assert dev.max() <= 0.25 * tol, "chains %s of %s" % (ids[dev > 0.25 * tol].tolist(), case["id"])
