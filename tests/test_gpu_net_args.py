"""The argument checks of the deep-net sampler entry points (csrc/mlp_hmc.hip, mlp3_mfma.hip, netn_hmc.hip), text by text: each
case hands one bad argument to an otherwise valid call through the C ABI and expects HTA_ERR_INVALID with the message the
source spells out.  Every case of test_bad_argument_text is refused before any launch; the tensors still have the sizes a valid
call needs, and one more test makes each of those calls with nothing wrong (one trajectory or one evaluation of one chain)."""
import pytest
import torch

from hamiltorch_amd import _abi

pytestmark = pytest.mark.gpu

N = 65
MLP3_DIMS = (1, 72, 72, 1)            # csrc/mlp3_mfma.hip takes it (a width beyond the small-net kernel's 64)
MLP3_WORKSPACE = 7 * 448 * 4 * 4      # one workgroup (C = 1): 7 blocks of 448 float4


def _tensors(dtype, D, n_in):
    z = lambda *shape: torch.zeros(*shape, dtype=dtype, device="cuda:0")
    return dict(theta=z(1, D), theta_init=z(1, D), X=z(N, n_in), Y=z(N))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _call(name, like, args):
    fn = getattr(_abi.load(), "%s_%s" % (name, "f32" if like.dtype == torch.float32 else "f64"))
    with torch.cuda.device(like.device):
        _abi._check(fn(*args, _abi._stream(like)), name)


def _mlp(dtype, eval_only, **bad):
    n_in, H = 2, 4
    t = _tensors(dtype, H * n_in + 2 * H + 1, n_in)
    a = dict(M=1, Nb=1, N=N, mass_kind=_abi.MASS_NONE, integrator=_abi.SPLIT_SYMMETRIC, split=0, theta=t["theta"])
    a.update(bad)
    tau4 = _abi._tau4(t["theta"], [1.0] * 4)
    if eval_only:
        _call("hta_mlp_logp_grad", t["X"], [_ptr(a["theta"]), 1, n_in, H, 0, 0, _ptr(t["X"]), _ptr(t["Y"]), a["N"], a["M"], a["Nb"],
                                            a["split"], tau4, 1.0, 1.0, None, None])
    else:
        _call("hta_mlp_hmc_sample", t["X"], [_ptr(a["theta"]), _ptr(t["theta_init"]), 1, n_in, H, 0, 0, _ptr(t["X"]), _ptr(t["Y"]), a["N"],
                                             a["M"], a["Nb"], tau4, 1.0, 1.0, a["mass_kind"], None, None, a["integrator"], 1, 0.01, 1,
                                             0, 0, 1, 0, None, None, None, None, None])


def _netn(dtype, eval_only, dims=(2, 4, 1), **bad):
    D = sum(dims[i] * dims[i + 1] + dims[i + 1] for i in range(len(dims) - 1))
    t = _tensors(dtype, D, dims[0])
    nl, cd, ct = _abi._net_operands(t["theta"], dims, [1.0] * (2 * (len(dims) - 1)))
    ws = torch.zeros(MLP3_WORKSPACE, dtype=torch.uint8, device="cuda:0") if dims == MLP3_DIMS else None
    a = dict(M=1, Nb=1, N=N, mass_kind=_abi.MASS_NONE, integrator=_abi.SPLIT_SYMMETRIC, split=0, theta=t["theta"],
             workspace_bytes=0 if ws is None else ws.numel())
    a.update(bad)
    if eval_only:
        _call("hta_netn_logp_grad", t["X"], [_ptr(a["theta"]), 1, nl, cd, 0, 0, _ptr(t["X"]), _ptr(t["Y"]), a["N"], a["M"], a["Nb"],
                                             a["split"], ct, 1.0, 1.0, None, None, _ptr(ws), a["workspace_bytes"]])
    else:
        _call("hta_netn_hmc_sample", t["X"], [_ptr(a["theta"]), _ptr(t["theta_init"]), 1, nl, cd, 0, 0, _ptr(t["X"]), _ptr(t["Y"]), a["N"],
                                              a["M"], a["Nb"], ct, 1.0, 1.0, a["mass_kind"], None, None, a["integrator"], 1, 0.01, 1,
                                              0, 0, 1, 0, None, None, None, None, None, _ptr(ws), a["workspace_bytes"]])


f32, f64 = torch.float32, torch.float64
# entry -> (caller, the name its checks print)
ENTRIES = {
    "hta_mlp_hmc_sample_f32": (lambda **b: _mlp(f32, False, **b), "hta_mlp_hmc"),
    "hta_mlp_logp_grad_f32": (lambda **b: _mlp(f32, True, **b), "hta_mlp_hmc"),
    "hta_netn_hmc_sample_f32": (lambda **b: _netn(f32, False, **b), "hta_netn_hmc"),
    "hta_netn_hmc_sample_f64": (lambda **b: _netn(f64, False, **b), "hta_netn_hmc"),
    "hta_netn_logp_grad_f32": (lambda **b: _netn(f32, True, **b), "hta_netn_hmc"),
    "hta_netn_hmc_sample_f32[mlp3]": (lambda **b: _netn(f32, False, MLP3_DIMS, **b), "hta_netn_hmc"),
    "hta_netn_logp_grad_f32[mlp3]": (lambda **b: _netn(f32, True, MLP3_DIMS, **b), "hta_netn_hmc"),
}
SAMPLERS = [e for e in ENTRIES if "sample" in e]
EVALS = [e for e in ENTRIES if "logp_grad" in e]

# (case, entries it applies to, the bad arguments, the literal of the source with %s = the entry's name)
CASES = [
    ("splits_exceed_N", list(ENTRIES), dict(M=2, Nb=33), "%s: M=2 splits of Nb=33 points exceed N=65"),
    ("dense_mass", [e for e in SAMPLERS if "mlp3" not in e], dict(mass_kind=_abi.MASS_FULL),
     "%s: only identity / diagonal inv_mass are supported natively"),
    # a dense mass keeps the model off the matrix-core route, and the small-net kernel refuses its widths first
    ("dense_mass", ["hta_netn_hmc_sample_f32[mlp3]"], dict(mass_kind=_abi.MASS_FULL), "%s: layer width 72 not in [1, 64]"),
    ("diag_mass_without_operands", ["hta_netn_hmc_sample_f32[mlp3]"], dict(mass_kind=_abi.MASS_DIAG),
     "%s: diagonal mass needs inv_mass and mass_factor"),
    ("diag_mass_without_operands", [e for e in SAMPLERS if "mlp3" not in e], dict(mass_kind=_abi.MASS_DIAG),
     "%s: only identity / diagonal inv_mass are supported natively"),
    ("eval_split_is_M", EVALS, dict(M=2, Nb=1, split=2), "%s: split 2 not in [0, 2)"),
    ("integrator_3", SAMPLERS, dict(integrator=3), "%s: unknown integrator 3"),
    ("rand_M_65", SAMPLERS, dict(integrator=_abi.SPLIT_RAND, M=65, Nb=1), "%s: SPLITTING_RAND supports at most 64 subsets natively (M=65)"),
    ("kmid_M_1", SAMPLERS, dict(integrator=_abi.SPLIT_KMID, M=1), "%s: SPLITTING_KMID needs at least 2 subsets"),
    ("null_theta", list(ENTRIES), dict(theta=None), "%s: NULL pointer / empty batch"),
    ("short_workspace", ["hta_netn_hmc_sample_f32[mlp3]"], dict(workspace_bytes=MLP3_WORKSPACE - 1),
     "%%s (mlp3): workspace of %d bytes required (hta_netn_hmc_workspace_bytes)" % MLP3_WORKSPACE),
]
PARAMS = [pytest.param(entry, bad, text, id="%s-%s" % (entry, case)) for case, entries, bad, text in CASES for entry in entries]


@pytest.mark.parametrize("entry,bad,text", PARAMS)
def test_bad_argument_text(entry, bad, text):
    call, who = ENTRIES[entry]
    if "split" in bad:                 # the one check that names the evaluation entry point
        who = who.replace("_hmc", "_logp_grad")
    with pytest.raises(_abi.InvalidArguments) as e:
        call(**bad)
    assert str(e.value).endswith("(-1): " + text % who), str(e.value)


def test_the_calls_are_valid_without_the_bad_argument():
    """Each caller above, with nothing wrong, samples one trajectory / evaluates one split: a case that raises does so for its own
    bad argument, not for the harness's."""
    for entry, (call, _) in ENTRIES.items():
        call()
    torch.cuda.synchronize()
