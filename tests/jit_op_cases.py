"""Case table of the callback compiler's lowering (hamiltorch_amd/jit/trace.py), op by op - a helper module for
tests/test_jit_ops.py (CPU: coverage of the lowering table, parity with torch.autograd, hipRTC builds) and
tests/test_gpu_jit_ops.py (the compiled device code).

Each case applies one op (or one family of overloads) to the traced vector's own coordinates, so that a wrong entry of the
gradient points at the op, and lists rows of points that hit the op where kernels go wrong: kinks and ties hit exactly, tails,
overflow, zeros and poles, non-default keyword arguments.  torch.autograd of the callable is the oracle.

Fields of a case:
  rows       float64 points (value, gradient and - where `hess` - Hessian compared with autograd);
  rows32     float32 points (None: the rows whose finite entries are all <= 30 in size - inf / NaN entries stay);
  hess       the graph forms the Hessian (False only where a second derivative needs digamma', refused by ir.Unsupported);
  third      smooth: the third derivatives are compared too;
  refuse     the fragment of the ir.Unsupported reason the trace (or its gradient) must raise - nothing else is compared;
  example    a benign example point for the trace (None: the first row);
  tol32      float32 bound, relative to 1 + |ref|;
  rtol64     the device's float64 bound where ocml's special functions differ from glibc / torch by a few ulp (None: the exact rule);
  tol_cpu    the bound of the numpy model in float64 (default 1e-12 relative to 1 + |ref|), stated where it is wider;
  grad_only_rows   rows where only the value and the gradient are compared: torch's double backward forms 0 * inf or
             exp(1600) there and returns NaN (or uses >= where its backward uses >), the graph gives the limit; `note` says which.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

INF, NAN = math.inf, math.nan


@dataclass
class Case:
    name: str
    fn: object
    D: int
    rows: list
    hess: bool = True
    third: bool = False
    refuse: str | None = None
    example: list | None = None
    rows32: list | None = None
    tol32: float = 1e-5
    rtol64: float | None = None
    tol_cpu: float = 1e-12
    note: str = ""
    grad_only_rows: list = field(default_factory=list)

    @property
    def example_point(self):
        return self.example if self.example is not None else self.rows[0]

    @property
    def f32_rows(self):
        if self.rows32 is not None:
            return self.rows32
        return [r for r in self.rows if all(abs(v) <= 30 or not math.isfinite(v) for v in r)]


CASES: list[Case] = []


def case(name, D, rows, **kw):
    def deco(fn):
        CASES.append(Case(name, fn, D, [list(map(float, r)) for r in rows], **kw))
        return fn
    return deco


def _c(w, *vals):
    """A constant of the traced vector's dtype (closed-over tensors trace as constants)."""
    return torch.tensor(vals, dtype=w.dtype)


# ---- kinks and ties, hit exactly -------------------------------------------------------------------------------------------
@case("relu", 2, [[0, 0.5], [-0.5, 0], [1, -1], [NAN, 1]], example=[0.3, -0.4])
def _relu(w):
    return (F.relu(w) * _c(w, 1.0, 2.0)).sum()


@case("abs_sign", 2, [[0, 1], [-1, 0], [0.5, -2]], example=[0.3, -0.4])
def _abs_sign(w):
    return w[0].abs() * 3 + torch.absolute(w[1]) + (torch.sign(w) * w).sum() + torch.sgn(w[0]) * 2


@case("clamp_scalar", 3, [[-1, 2, 0.5], [2, -1, 0], [-3, 3, 1.5], [NAN, 0.5, NAN]], example=[0.2, 0.4, 0.6])
def _clamp_scalar(w):
    return (torch.clamp(w, -1.0, 2.0) * _c(w, 1.0, 2.0, 3.0)).sum() + torch.clip(w[2], 0.0, 1.0) * 5


@case("clamp_tensor", 3, [[0.5, 0.5, 1.0], [1.0, 0.5, 1.0], [0.2, 0.5, 1.0], [1.5, 0.5, 1.0], [0.0, 2.0, 1.0], [0.2, 0.5, 0.5],
                          [0.7, 0.5, 0.5], [0.5, 0.5, 0.5], [NAN, 0.5, 1.0], [0.7, NAN, 1.0], [0.7, 0.5, NAN]], example=[0.7, 0.5, 1.0])
def _clamp_tensor(w):
    return torch.clamp(w[0:1], w[1:2], w[2:3]).sum() * 2 + torch.clamp_min(w[0:1], w[1:2]).sum() + torch.clamp_max(w[0:1], w[2:3]).sum() * 3


@case("clamp_min_max", 2, [[0.5, -0.5], [0, 0.25], [-1, 1]], example=[0.7, 0.1])
def _clamp_min_max(w):
    return torch.clamp_min(w, 0.5).sum() + 2 * torch.clamp_max(w, 0.25).sum() + torch.clamp(w, min=0.0).pow(2).sum()


@case("hardtanh", 2, [[-1, 1], [0.5, -2], [2, 0], [NAN, 0.5]], example=[0.3, -0.4])
def _hardtanh(w):
    return F.hardtanh(w[0]) * 2 + F.hardtanh(w[1], -0.5, 1.5) + F.hardtanh(w, -2.0, 0.5).sum()


@case("leaky_elu_at_zero", 2, [[0, 0], [0.5, -0.5], [-2, 3]], example=[0.3, -0.4], grad_only_rows=[[0, 0]],
      note="at 0 torch's elu backward takes the negative branch (x <= 0) and its double backward the positive one (x < 0)")
def _leaky_elu(w):
    # (no celu: torch's native celu kernel rounds 1 / alpha to float32, 4e-8 off in float64 - not the lowering's business)
    return (F.leaky_relu(w[0]) + F.leaky_relu(w[1], 0.2) + F.elu(w[0]) + F.elu(w[1], alpha=0.7) + F.selu(w[0]) + F.selu(w[1]) * 2)


@case("elu_kwargs", 2, [[0, 0], [0.5, -0.5], [-2, 3]], example=[0.3, -0.4], grad_only_rows=[[0, 0]],
      note="at 0 torch's backward takes the negative branch (x <= 0) and its double backward the positive one (x < 0)")
def _elu_kwargs(w):
    return torch.ops.aten.elu(w, 0.7, 1.5, 2.0).sum()


@case("maximum_minimum", 2, [[1, 1], [0, 0], [1, 2], [3, -1]], example=[0.3, -0.4])
def _maximum(w):
    return torch.maximum(w[0], w[1]) * 2 + torch.minimum(w[0], w[1]) + torch.max(w[0], w[1]) * 0.5 + torch.min(w[1], w[0]) * 0.25


@case("fmax_fmin", 2, [[1, 1], [1, 2], [3, -1]], example=[0.3, -0.4])
def _fmax(w):
    return torch.fmax(w[0], w[1]) * 2 + torch.fmin(w[0], w[1])


@case("fmax_nan", 2, [[1, 2], [-1, 0.5]], example=[0.3, -0.4])
def _fmax_nan(w):
    n = _c(w, NAN)[0]
    return torch.fmax(w[0], n) + torch.fmin(n, w[1]) * 2 + torch.fmax(w, w.flip(0)).sum()


@case("maximum_nan", 2, [[NAN, 1.0], [-2.0, NAN], [NAN, NAN], [1.0, 1.0]], example=[0.3, -0.4])
def _maximum_nan(w):
    return torch.maximum(w[0], w[1]) + torch.minimum(w[1], w[0]) * 2


@case("reduce_max_ties", 4, [[1, 1, 1, 0], [1, 1, 0.5, 0], [2, 1, 2, -3], [0, 0, 0, 0], [-1, -1, -1, -1]], example=[0.1, 0.4, -0.3, 0.2])
def _reduce_max(w):
    return w.amax() * 2 + w.max() + w.amin() * 3 + w.min() * 0.5


@case("reduce_max_dims", 4, [[1, 1, 1, 1], [1, 2, 2, 1], [0.5, 0.5, -1, 3]], example=[0.1, 0.4, -0.3, 0.2])
def _reduce_max_dims(w):
    m = w.reshape(2, 2)
    return ((m.amax(0) * _c(w, 1.0, 2.0)).sum() + (m.amin(1, keepdim=True) * _c(w, 3.0, 5.0)[:, None]).sum()
            + (torch.amax(m, (0, 1)) * 7))


@case("reduce_max_inf", 3, [[INF, 1, 0], [INF, INF, 0], [-INF, -INF, -INF]], example=[0.1, 0.4, -0.3])
def _reduce_max_inf(w):
    return w.amax() + w.amin()


@case("reduce_max_exact", 3, [[0.3, 0.3, 0.3], [1.1, 1.1, 1.1], [0.3, 1.1, 1.1], [-0.7, 0.2, -0.7]], example=[0.1, 0.4, -0.3],
      note="the extreme of a 3-way tie is the entry itself, exactly: x == x.amax() holds and amax - amin of a constant vector is 0")
def _reduce_max_exact(w):
    r = (w == w.amax()).to(w.dtype).sum() * w[0] + (w == w.max()).to(w.dtype).sum() + (w == w.amin()).to(w.dtype).sum() * 2
    return r + (w.amax() == w.amin()).to(w.dtype) * 5 + (w.abs() == torch.linalg.vector_norm(w, INF)).to(w.dtype).sum() * w[1]


@case("max_dim", 3, [[1, 1, 0], [0, 2, 2], [5, 5, 5], [-1, 0, 1]], example=[0.1, 0.4, -0.3])
def _max_dim(w):
    m = torch.stack([w, w.flip(0)])
    return (w.max(0).values * 2 + w.min(0).values + (m.max(1, keepdim=True).values * _c(w, 1.0, 3.0)[:, None]).sum()
            + (m.min(0).values * _c(w, 1.0, 2.0, 4.0)).sum())


@case("where_masked_fill", 2, [[0, 1], [0.5, -0.5], [-1, 0]], example=[0.3, -0.4])
def _where(w):
    a = torch.where(w > 0, w * w, -w).sum() + torch.where(w[0] >= w[1], w[0], 2 * w[1])
    b = w.masked_fill(w < 0, 0.5).sum() + w.masked_fill(w <= 0, w[1] * 3).sum()
    return a + b + torch.where(w > 0, w, 0.0).sum() + torch.where(w < 0, 1.0, w).sum() + torch.where(w > 0, 2.0, 3.0).sum()


@case("rounding", 2, [[0.5, 1.5], [2.5, -0.5], [-1.5, 0.25], [1, -2]], example=[0.3, -0.4])
def _rounding(w):
    return ((torch.floor(w) + torch.ceil(w) * 2 + torch.round(w) * 3 + torch.trunc(w) * 5) * w).sum()


@case("div_rounding_mode", 2, [[1.5, 0.5], [-3, 2], [2.5, -1], [7, 0.5]], example=[1.3, 0.4])
def _div_mode(w):
    return (torch.div(w[0], w[1], rounding_mode="floor") + torch.div(w[0], w[1], rounding_mode="trunc") * 2 + torch.div(w, 2.0, rounding_mode="floor").sum()
            + torch.div(w[0], w[1]) + (torch.floor_divide(w[0].detach(), w[1].detach()) * 0.5 + w.detach()[0] // 2.0) * w[1])


# ---- tails and overflow ------------------------------------------------------------------------------------------------
_TAILS = [[30, -30], [100, -100], [800, -800], [0, 1e-9], [-1, 2]]
_TAILS32 = [[30, -30], [90, -90], [0, 1e-5], [-1, 2]]


@case("softplus_default", 2, _TAILS, rows32=_TAILS32, third=True, example=[0.3, -0.4])
def _softplus(w):
    return F.softplus(w).sum()


@case("softplus_kwargs", 2, [[0.5, 1], [1, 2], [1.5, 1.7], [5, -1], [2, 1.5], [-3, 0]], example=[0.3, -0.4], grad_only_rows=[[1, 2]],
      note="at beta x == threshold torch's backward is softplus' (>) and its double backward the identity's (>=)")
def _softplus_kw(w):
    return F.softplus(w[0], threshold=1) + F.softplus(w[1], beta=3, threshold=5) * 2 + F.softplus(w, beta=0.5).sum()


@case("log_sigmoid", 2, _TAILS, rows32=_TAILS32, third=True, example=[0.3, -0.4])
def _logsig(w):
    return F.logsigmoid(w).sum()


@case("sigmoid_silu", 2, _TAILS, rows32=_TAILS32, third=True, example=[0.3, -0.4])
def _sigmoid(w):
    return torch.sigmoid(w).sum() + F.silu(w).sum() * 0.5


@case("logaddexp", 2, [[1, 1], [0, 0], [30, -30], [100, 100], [800, -800], [-800, -800], [-1, 2]], rows32=[[1, 1], [90, -90], [-1, 2]],
      third=True, example=[0.3, -0.4], grad_only_rows=[[800, -800], [90, -90]],
      note="torch's double backward forms exp(1600) (exp(180) in float32)")
def _logaddexp(w):
    return torch.logaddexp(w[0], w[1])


@case("logaddexp_neginf", 1, [[0.5], [-2.0]], third=True, example=[0.3])
def _logaddexp_ninf(w):
    return torch.logaddexp(w[0], _c(w, -INF)[0]) + torch.logaddexp(_c(w, -INF)[0], -w[0]) * 2


@case("logsumexp_softmax", 3, [[1, 1, 1], [30, -30, 0], [100, -100, 100], [800, -800, 0], [-800, -800, -800], [0.5, -1, 2]],
      rows32=[[1, 1, 1], [90, -90, 0], [0.5, -1, 2]], third=True, example=[0.3, -0.4, 0.1])
def _lse(w):
    wt = _c(w, 1.0, 2.0, 3.0)
    return (torch.logsumexp(w, 0) + (F.log_softmax(w, 0) * wt).sum() + (F.softmax(w, 0) * wt).sum()
            + (torch.softmax(w, -1) * wt).sum() + torch.log_softmax(w.reshape(1, 3), 1)[0, 1])


@case("logsumexp_neginf", 2, [[0.5, -1], [0, 0]], third=True, example=[0.3, -0.4])
def _lse_ninf(w):
    return torch.logsumexp(torch.cat([w, _c(w, -INF)]), 0) + torch.logsumexp(torch.stack([w, w * 2]), 0, keepdim=True).sum()


@case("erfc_tail", 1, [[4], [6], [9], [0], [-3]], rows32=[[4], [6], [9], [0], [-3]], third=True, rtol64=4e-15, tol_cpu=1e-10, example=[0.3],
      note="the third derivative of log erfc(x) cancels terms of size x^3 (700 at x = 9): 1e-10")
def _erfc(w):
    return torch.log(torch.erfc(w[0])) + torch.special.erfc(w[0]) * 0.5


@case("erf_gelu", 2, [[0, 1], [3, -3], [-0.5, 6]], third=True, rtol64=4e-15, example=[0.3, -0.4])
def _erf(w):
    return torch.erf(w).sum() + F.gelu(w).sum() + F.gelu(w, approximate="tanh").sum() * 2 + torch.special.erf(w[0])


@case("exp_family_small", 2, [[1e-9, -1e-9], [1e-5, -1e-5], [0, 0.5]], third=True, example=[0.3, -0.4])
def _exp_small(w):
    return (torch.expm1(w) * 3 + torch.log1p(w) + torch.sinh(w) * 5 + torch.tanh(w) * 7 + torch.cosh(w)).sum()


@case("sinh_small", 2, [[1e-9, 1e-5], [-1e-9, 2e-7]], rows32=[[1e-5, 2e-7], [-1e-5, 1e-6]], tol32=2e-5, example=[0.3, -0.4],
      grad_only_rows=[[1e-9, 1e-5], [-1e-9, 2e-7], [1e-5, 2e-7], [-1e-5, 1e-6]],
      note="sinh near 0 scaled to O(1): (e^x - e^-x) / 2 loses every digit there; the Hessian (sinh again, as the derivative of cosh's "
           "(e^x + e^-x) / 2 form) cancels the same way, so only the value and the gradient are compared")
def _sinh_small(w):
    return torch.sinh(w[0]) * 1e9 + torch.sinh(w[1]) * 1e5


@case("sinh_cosh_tanh_large", 2, [[30, -30], [100, -100], [800, -800], [700, -700]], rows32=[[30, -30], [80, -80]], third=True, example=[0.3, -0.4],
      grad_only_rows=[[800, -800]], note="sinh, cosh overflow: torch's double backward multiplies inf by 0")
def _exp_large(w):
    return (torch.sinh(w) * 1e-300 + torch.cosh(w) * 1e-300 + torch.tanh(w) + torch.exp(-w * w * 1e-6)).sum()


@case("exp_log_overflow", 2, [[709, -745], [710, -746], [0, 1]], rows32=[[88, -103], [89, -104], [0, 1]], third=True, example=[0.3, -0.4],
      grad_only_rows=[[710, -746]], note="exp overflows: torch's double backward multiplies inf by 0")
def _exp_over(w):
    return torch.exp(w[0]) + torch.exp(w[1]) * 3 + torch.exp2(w[1] * 0.5) + torch.log2(w[0] * w[0] + 1) + torch.log10(w[0] * w[0] + 2)


@case("trig", 2, [[0, 0.5], [3, -2], [1e-9, 100]], third=True, rtol64=4e-15, example=[0.3, -0.4])
def _trig(w):
    return (torch.sin(w) + torch.cos(w) * 2 + torch.atan(w) * 3 + torch.arctan(w[0]) + torch.tan(w * 0.5)).sum()


# ---- zeros and poles ---------------------------------------------------------------------------------------------------
@case("norm2_zero", 3, [[0, 0, 0], [0, 3, 4], [1e-200, 0, 0], [1, -2, 2]], third=True, example=[0.3, -0.4, 0.5],
      grad_only_rows=[[0, 0, 0], [1e-200, 0, 0]], note="at (and next to) a zero norm torch's double backward is 0 / 0")
def _norm2(w):
    return -torch.linalg.vector_norm(w) - 0.5 * torch.norm(w[:2]) + torch.linalg.norm(w[1:]) * 0.25


@case("norm_ords", 3, [[0, 0, 0], [0, -3, 3], [1, -2, 0.5], [0.3, -0.3, 0.5]], example=[0.3, -0.4, 0.5],
      note="ord 1 / inf / -inf: piecewise linear (their Hessians are 0 where defined); gradients with ties and zero entries")
def _norm_ords(w):
    return (torch.linalg.vector_norm(w, 1) + torch.linalg.vector_norm(w, INF) * 2 + torch.linalg.vector_norm(w, -INF) * 3
            + torch.norm(w, p=1) * 0.5)


@case("norm_minf_value", 3, [[1, -0.3, 0.5], [0.3, -0.3, 2]], third=True, example=[0.7, -0.4, 0.5])
def _norm_minf(w):
    return torch.linalg.vector_norm(w, -INF) * 1.5


@case("norm3_dims", 4, [[0, 0, 0, 0], [0, 1, 0, -2], [1, -2, 0.5, 3]], third=True, example=[0.3, -0.4, 0.5, 0.6],
      grad_only_rows=[[0, 0, 0, 0], [0, 1, 0, -2]], note="at a zero norm (of a column) torch's double backward is 0 / 0")
def _norm3(w):
    m = w.reshape(2, 2)
    return (torch.linalg.vector_norm(w, 3) + (torch.linalg.vector_norm(m, 2, dim=1) * _c(w, 1.0, 2.0)).sum()
            + torch.linalg.vector_norm(m, 1, dim=0, keepdim=True).sum() + torch.norm(m, 2.5, 0).sum())


@case("norm_ord0", 2, [[1, 0]], refuse="order 0")
def _norm0(w):
    return torch.linalg.vector_norm(w, 0)


@case("var_std", 3, [[1, 1, 1], [0, 0, 0], [1, 2, 4], [-1, 0.5, 3]], third=True, example=[0.3, -0.4, 0.5])
def _var_std(w):
    m = w.reshape(3, 1)
    return (w.var() + w.std() * 2 + torch.var(w, unbiased=False) * 3 + torch.std(w, correction=0) * 5 + torch.std(w, unbiased=True) * 0.5
            + m.var(0, keepdim=True).sum() * 7 + torch.std(m, dim=0).sum() * 11 + torch.var(w, correction=2) * 13)


@case("var_correction_ge_n", 3, [[1, 2, 4], [1, 1, 1]], example=[0.3, -0.4, 0.5],
      note="correction >= n: torch divides by max(0, n - correction) = 0 (value inf, or NaN at a constant input)")
def _var_big_corr(w):
    return torch.var(w, correction=3) + torch.std(w, correction=5)


@case("sqrt_rsqrt_log_recip", 4, [[0, 0, 0, 0], [1, 4, 0.5, 2], [-1, -1, -1, -1]], third=True, example=[0.3, 0.4, 0.5, 0.6],
      grad_only_rows=[[0, 0, 0, 0]], note="at the poles torch's double backward puts 0 * inf = NaN into the off-diagonal entries")
def _poles(w):
    return torch.sqrt(w[0]) + torch.rsqrt(w[1]) * 2 + torch.log(w[2]) * 3 + torch.reciprocal(w[3]) * 5


@case("pow_scalar_exponent", 4, [[0, 0, 0, 0], [-2, -2, -2, -0.5], [2, 3, 0.25, 1.5]], third=True, example=[0.3, 0.4, 0.5, 0.6],
      grad_only_rows=[[0, 0, 0, 0]], note="at 0 torch's double backward puts 0 * inf = NaN into the off-diagonal entries")
def _pow_scalar(w):
    return (w[0] ** 2 + w[1] ** 3 * 2 + w[2] ** 0.5 * 3 + w[3] ** -1 * 5 + w[0] ** 0 + torch.pow(w[1], 1.5) * 0.5
            + torch.square(w[2]) + w[3] ** 2.5 * 0.1 + w[0] ** -2 * 0.01 + w[1] ** 4 * 0.1 + w[1] ** -0.5)


@case("pow_tensor_exponent", 4, [[0, 2, 0, 0.5], [0, 0, 0, -1], [-2, 3, 2, 1.5], [1.5, 0.5, 3, -0.5], [0, 1, -2, 2]], third=True,
      example=[0.3, 2.0, 0.5, 0.6], grad_only_rows=[[0, 2, 0, 0.5], [0, 0, 0, -1], [0, 1, -2, 2]],
      note="at x = 0 torch's double backward of pow forms log(0) * 0")
def _pow_tensor(w):
    return torch.pow(w[0], w[1]) + torch.pow(w[2], w[3]) * 2 + torch.pow(_c(w, 2.0)[0], w[1]) * 0.5 + torch.pow(2.0, w[3])


@case("pow_zero_base_scalar", 2, [[0, 1], [0.5, -1]], third=True, example=[0.3, 2.0], grad_only_rows=[[0, 1], [0.5, -1]],
      note="pow(0, y): torch's double backward forms log(0) * 0")
def _pow_zero_base(w):
    return torch.pow(0.0, w[0]) + torch.pow(_c(w, 0.0)[0], w[1] * w[1])


@case("xlogy", 2, [[0, 3], [0.5, 2], [2, 0], [1, 1e-300], [0, 0], [0, INF], [0, -1], [NAN, 2], [0, NAN]], third=True, example=[0.3, 2.0],
      grad_only_rows=[[1, 1e-300], [0, 0], [0, INF], [0, -1]],
      note="at y = 1e-300, y = 0, y = inf and y < 0 torch's double backward forms 0 * inf or log of a negative number")
def _xlogy(w):
    return torch.xlogy(w[0], w[1]) + torch.xlogy(w[0], 2.5) * 2


@case("xlogy_scalar", 1, [[0], [1], [0.5]], third=True, example=[0.3])
def _xlogy_scalar(w):
    return torch.xlogy(w[0], _c(w, 0.0)[0]) * 0.5 + torch.xlogy(w[0], _c(w, 3.0)[0]) + torch.xlogy(2.0, w[0] + 1)


@case("lgamma", 2, [[0.5, 1e-8], [-0.5, -2.5], [0, -1], [3, 10]], hess=False, rtol64=1e-13, tol32=2e-5, example=[0.3, 2.0])
def _lgamma(w):
    return torch.lgamma(w[0]) + torch.lgamma(w[1]) * 2


@case("digamma_refused", 1, [[0.5]], refuse="derivative of digamma")
def _digamma(w):
    return torch.digamma(w[0])


@case("digamma_value", 2, [[0.5, 1e-8], [-0.5, -2.5], [0, -1], [3, 10]], hess=False, rtol64=1e-13, tol32=2e-5, example=[0.3, 2.0],
      note="digamma under a detach: its value is compiled, its derivative (trigamma) is not needed")
def _digamma_value(w):
    return torch.digamma(w.detach()).sum() * w[0] + torch.lgamma(w[1])


@case("prod_zeros", 3, [[0, 2, 3], [0, 0, 3], [1, 2, 3], [0, 0, 0]], third=True, example=[0.3, -0.4, 0.5])
def _prod(w):
    return w.prod() + torch.prod(w.reshape(1, 3), 1).sum() * 2 + torch.prod(w.reshape(3, 1), 0, keepdim=True).sum()


@case("nan_to_num", 2, [[INF, -INF], [-INF, NAN], [NAN, INF], [1e300, -2], [0.5, NAN]],
      rows32=[[INF, -INF], [-INF, NAN], [NAN, INF], [3e38, -2], [0.5, NAN]], example=[0.3, -0.4],
      note="the default replacements of +-inf are the largest finite value of the dtype: float64's or float32's")
def _nan_to_num(w):
    return (torch.nan_to_num(w[0]) * 0.5 + torch.nan_to_num(w[1], nan=0.5, posinf=3.0, neginf=-4.0) + torch.nan_to_num(w[1], neginf=-1.0)
            + torch.nan_to_num(w[0], nan=2.0, posinf=5.0) * 0.25)


@case("nan_to_num_scaled", 1, [[1.0], [-1.0], [0.5]], rows32=[[1.0], [-1.0], [0.5]], example=[0.3],
      note="1e300 * 1e300 * w is inf: nan_to_num gives the dtype's largest finite value (float32's in float32, where 1e300 is inf too)")
def _nan_to_num_scaled(w):
    return torch.nan_to_num(w[0] * 1e300 * 1e300) + torch.nan_to_num(w * 1e300, nan=1.0).sum() * 0.5


@case("isnan_isinf", 2, [[INF, 1], [NAN, -INF], [0.5, -0.5]], example=[0.3, -0.4])
def _isnan(w):
    f = w.isfinite().to(w.dtype) * 2 + w.isnan().to(w.dtype) * 3 + torch.isinf(w).to(w.dtype) * 5
    return (f + torch.where(torch.isfinite(w), w, 0.0)).sum()


# ---- non-default keyword arguments ----------------------------------------------------------------------------------------
@case("activations", 2, [[0.5, -0.5], [2, -3], [-1, 1]], third=True, rtol64=4e-15, example=[0.3, -0.4])
def _activations(w):
    return (F.gelu(w, approximate="tanh") + F.mish(w) + F.elu(w, 0.5) + F.selu(w) + F.celu(w, 0.5)).sum()


@case("addmm_family", 4, [[0.5, -1, 2, 0.25], [1, 1, 1, 1]], third=True, example=[0.3, -0.4, 0.5, 0.6])
def _addmm(w):
    m = w.reshape(2, 2)
    v = w[:2]
    return (torch.addmm(m, m, m.t(), beta=0.5, alpha=2.0).sum() + torch.addmv(v, m, v, beta=3.0, alpha=-1.5).sum()
            + torch.baddbmm(m[None], m[None], m[None], beta=0.25, alpha=4.0).sum() + torch.addmm(m, m, m).sum() * 0.5)


@case("triangular_solves", 4, [[2, 0.5, -1, 3], [1, 1, 1, 1]], third=True, example=[2.0, 0.4, 0.5, 1.6])
def _tri(w):
    A = torch.stack([torch.stack([w[0], w[1] * 0]), torch.stack([w[1], w[3]])])
    U = A.t()
    b = torch.stack([w[2], w[0]]).reshape(2, 1)
    r = torch.linalg.solve_triangular(A, b, upper=False).sum() + torch.linalg.solve_triangular(U, b, upper=True).sum() * 2
    r = r + torch.linalg.solve_triangular(A, b, upper=False, unitriangular=True).sum() * 3
    r = r + torch.triangular_solve(b, U, upper=True).solution.sum() * 5 + torch.triangular_solve(b, A, upper=False, transpose=True).solution.sum() * 7
    return r + torch.triangular_solve(b, U, upper=True, unitriangular=True).solution.sum()


@case("lerp_addc", 3, [[0.5, -1, 2], [0, 0, 1]], third=True, example=[0.3, -0.4, 0.5])
def _lerp(w):
    return (torch.lerp(w[0], w[1], 0.25) + torch.lerp(w[0], w[1], w[2]) * 2 + torch.addcmul(w[0], w[1], w[2], value=0.5)
            + torch.addcdiv(w[0], w[1], w[2] + 3, value=-2.0))


@case("arith_overloads", 3, [[0.5, -1, 2], [1, 1, 1]], third=True, example=[0.3, -0.4, 0.5])
def _arith(w):
    r = torch.add(w[0], w[1], alpha=2.0) + torch.sub(w[1], w[2], alpha=0.5) + torch.rsub(w[0], w[2], alpha=3.0) + (2.0 - w[1])
    r = r + w[0] * 3.0 + w[1] / 4.0 + torch.true_divide(w[2], w[0] + 5) + -w[0] + torch.negative(w[1]) + (+w[2])
    return r + torch.add(w, 1).sum() + torch.sub(w, 2.0).sum() * w[0]


@case("compare_logic", 3, [[0.5, 0.5, 1], [0, -1, 1], [2, 2, 2]], example=[0.3, -0.4, 0.5])
def _compare(w):
    a, b = w[0], w[1]
    m = ((a > b) & (b >= 0)) | ~(a < w[2]) | torch.logical_and(a <= b, b != w[2]) | torch.logical_or(a == b, torch.logical_not(b < 0))
    m2 = torch.ne(w, 0.5) & torch.eq(w, w)
    s = torch.greater(a, b).to(w.dtype) + torch.greater_equal(a, 0.5).to(w.dtype) + torch.less(a, b).to(w.dtype) + torch.less_equal(b, 0.5).to(w.dtype)
    s = s + torch.not_equal(a, b).to(w.dtype) + torch.bitwise_and(w > 0, w < 1).to(w.dtype).sum() + torch.bitwise_or(w > 1, w < 0).to(w.dtype).sum()
    s = s + torch.bitwise_not(w > 0).to(w.dtype).sum() + torch.lt(w, 1).to(w.dtype).sum() + torch.le(w, 1).to(w.dtype).sum()
    return torch.where(m, w[2], -w[2]) * 2 + (m2.to(w.dtype) * w).sum() + s * w[0]


# ---- structure ops, once each ----------------------------------------------------------------------------------------------
_M = torch.tensor([[0.5, -1.0, 2.0, 0.25], [1.5, 0.75, -0.5, 1.0], [0.3, 0.2, -0.1, 0.4]], dtype=torch.float64)


@case("views", 4, [[0.5, -1, 2, 0.25]], third=True, example=[0.3, -0.4, 0.5, 0.6])
def _views(w):
    m = w.reshape(2, 2)
    r = (m.t() * _c(w, 1.0, 2.0)).sum() + (m.transpose(0, 1) @ m).sum() + m.permute(1, 0)[0, 1] * 3 + w.view(4, 1).squeeze(1)[2] * 5
    r = r + w.unsqueeze(0).expand(3, 4).sum(0)[1] + w.flatten()[3] + m.flatten(0, 1)[0] + m.mT[0, 1] * 7 + m.mH[1, 0] + m.adjoint()[1, 1]
    r = r + w.reshape(1, 4).squeeze()[0] + w.reshape(1, 2, 2).squeeze(0)[1, 1] + w.reshape(2, 1, 2).squeeze((1,))[0, 1]
    r = r + w.flip(0)[0] * 11 + w.repeat(2)[5] + w.narrow(0, 1, 2).sum() + w.contiguous()[0] + m.expand_as(torch.empty(2, 2))[1, 0]
    r = r + w.clone()[1] + torch.broadcast_to(w[0], (3,)).sum()
    return r + m.diagonal().sum() + torch.diagonal(m, 1).sum() + m.trace() * 2 + torch.positive(w)[0] + w.resolve_conj()[1] + w.conj()[2]


@case("indexing", 4, [[0.5, -1, 2, 0.25]], third=True, example=[0.3, -0.4, 0.5, 0.6])
def _indexing(w):
    idx = torch.tensor([3, 0, 0, 2])
    m = torch.stack([w, w * 2])
    r = (w[idx] * w).sum() + w.index_select(0, torch.tensor([1, 3])).prod() + torch.gather(m, 1, torch.tensor([[0, 2], [3, 1]])).sum()
    r = r + m[1, 2:][0] + m[:, 1].sum() * 3 + m[torch.tensor([1, 0]), torch.tensor([0, 3])].sum() + w[1:3].sum() + w[::2].sum() * 2
    return r + torch.select(m, 1, 3).sum() + m[-1][-1]


@case("scatters", 4, [[0.5, -1, 2, 0.25]], third=True, example=[0.3, -0.4, 0.5, 0.6])
def _scatters(w):
    out = torch.zeros(6, dtype=w.dtype)
    out[1:5] = w * w
    out[0] = w[2] * 3
    out[torch.tensor([5])] = w[0:1]
    acc = out.clone()
    acc[torch.tensor([1, 3])] += w[3]
    acc = acc.index_put((torch.tensor([2, 4]),), w[:2], accumulate=True)
    m = torch.zeros(2, 3, dtype=w.dtype)
    m[1] = w[:3]
    m[:, 0] = w[2:]
    return (out * _c(w, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0)).sum() + acc.pow(2).sum() + (m * m).sum()


@case("concat_split", 4, [[0.5, -1, 2, 0.25]], third=True, example=[0.3, -0.4, 0.5, 0.6])
def _cat(w):
    a, b = w.split(2)
    c = torch.cat([a, b * 2, torch.empty(0, dtype=w.dtype)])
    d = torch.concat([w[:1], w[2:]])
    p, q = torch.split(w, [1, 3])
    x0, x1, x2, x3 = w.unbind()
    h = torch.chunk(w, 2)
    s = torch.stack([a, b], 1)
    return (c * w).sum() + d.prod() + p.sum() * q.sum() + x0 * x3 - x1 * x2 + h[0].sum() * h[1].sum() * 0.5 + (s[:, 0] * s[:, 1]).sum()


@case("cumsum_tri_diag", 4, [[0.5, -1, 2, 0.25]], third=True, example=[0.3, -0.4, 0.5, 0.6])
def _tri(w):
    m = w.reshape(2, 2)
    cs = torch.cumsum(w, 0)
    return ((cs * cs).sum() + torch.tril(m).sum() * 2 + torch.triu(m, 1).sum() * 3 + torch.diag(w[:2]).pow(2).sum() + torch.diag(m).sum()
            + torch.diag_embed(w[:2]).sum() * 5 + torch.diag(w[:3], 1)[0, 1] + torch.cumsum(m, 1)[1, 1] * 7)


@case("creation", 3, [[0.5, -1, 2]], third=True, example=[0.3, -0.4, 0.5])
def _creation(w):
    e = torch.eye(3, dtype=w.dtype)
    r = (e @ w).sum() + (torch.eye(3, 2, dtype=w.dtype).t() @ w).sum() * 2 + (torch.arange(3, dtype=w.dtype) * w).sum()
    r = r + (torch.arange(1, 4).to(w.dtype) * w).sum() + (torch.arange(0, 6, 2, dtype=w.dtype) * w).sum() + (torch.full((3,), 0.5, dtype=w.dtype) * w).sum()
    r = r + (torch.zeros(3, dtype=w.dtype) + w).sum() + (torch.ones(3, dtype=w.dtype) * w).prod() + (torch.ones_like(w) * 3 + w).pow(2).sum()
    r = r + (torch.zeros_like(w) + w).prod() + torch.full_like(w, 2.0).dot(w) + w.new_zeros(3).add(w).sum() + w.new_ones(3).dot(w)
    r = r + w.new_full((3,), 4.0).dot(w) + torch.scalar_tensor(2.0, dtype=w.dtype) * w[0] + torch.empty_like(w).fill_(1.0).dot(w)
    return r + w.new_empty(3).fill_(2.0).dot(w) + torch.full((3,), 1.0, dtype=w.dtype).dot(w.type_as(w)) + w.to(w.dtype)[1]


@case("matmul_shapes", 4, [[0.5, -1, 2, 0.25]], third=True, example=[0.3, -0.4, 0.5, 0.6])
def _matmul(w):
    m = w.reshape(2, 2)
    A = _M.to(w.dtype)
    r = (A @ w).sum() + (w @ A.t()).sum() + (m @ m).sum() + torch.mm(m, m.t()).sum() + torch.mv(m, w[:2]).sum()
    r = r + torch.bmm(m[None], m[None]).sum() + torch.matmul(m[None].expand(2, 2, 2), w[:2]).sum() + w.dot(w) + torch.inner(w, w) * 2
    r = r + torch.vdot(w, w) + torch.outer(w[:2], w[2:]).sum() + torch.ger(w[:2], w[:2]).sum() + F.linear(w, A, A[:, 0]).sum()
    return r + F.linear(w, A).sum() * 0.5 + torch.matmul(w, w)


@case("reductions", 4, [[0.5, -1, 2, 0.25]], third=True, example=[0.3, -0.4, 0.5, 0.6])
def _reductions(w):
    m = w.reshape(2, 2)
    return (w.sum() * w.mean() + m.sum(0).prod() + m.sum(1, keepdim=True).sum() + m.mean(0).pow(2).sum() + m.mean(1, keepdim=True).pow(3).sum()
            + w.sum(dtype=w.dtype) * 2)


@case("detach_casts", 3, [[0.5, -1, 2]], third=True, example=[0.3, -0.4, 0.5])
def _detach(w):
    b = (w > 0).to(w.dtype)
    return (w * w.detach()).sum() + (b * w).sum() + w.to(torch.float64).to(w.dtype).sum() + (w > 0).float().to(w.dtype).sum() * w[0] + w.type(w.dtype)[1]


@case("distributions", 3, [[0.5, -1, 2], [0.25, 0.5, 0.75]], third=True, rtol64=1e-14, example=[0.3, 0.4, 0.5])
def _dists(w):
    d = torch.float64
    mu = torch.tensor([0.1, -0.2, 0.3], dtype=d)
    L = torch.tensor([[1.0, 0, 0], [0.5, 1.5, 0], [-0.3, 0.2, 0.8]], dtype=d)
    r = torch.distributions.MultivariateNormal(mu, scale_tril=L).log_prob(w)
    r = r + torch.distributions.Normal(mu, torch.tensor(2.0, dtype=d)).log_prob(w).sum()
    r = r + torch.distributions.Laplace(torch.tensor(0.0, dtype=d), torch.tensor(1.5, dtype=d)).log_prob(w[0] + 3)
    r = r + torch.distributions.Cauchy(torch.tensor(0.0, dtype=d), torch.tensor(2.0, dtype=d)).log_prob(w[1])
    r = r + torch.distributions.StudentT(torch.tensor(4.0, dtype=d)).log_prob(w[2])
    return r + torch.distributions.LogNormal(torch.tensor(0.0, dtype=d), torch.tensor(1.0, dtype=d)).log_prob(torch.exp(w[0]))


@case("distributions_lgamma", 3, [[0.5, 0.25, 2], [0.25, 0.5, 0.75]], hess=False, rtol64=1e-13, tol32=2e-5, example=[0.3, 0.4, 0.5],
      note="Beta / Gamma / Dirichlet / Poisson log_probs: lgamma of the argument, no Hessian")
def _dists_lgamma(w):
    d = torch.float64
    r = torch.distributions.Beta(torch.tensor(2.0, dtype=d), torch.tensor(3.0, dtype=d)).log_prob(w[1])
    r = r + torch.distributions.Gamma(torch.tensor(2.0, dtype=d), torch.tensor(3.0, dtype=d)).log_prob(w[2])
    r = r + torch.distributions.Dirichlet(torch.tensor([1.5, 2.5], dtype=d)).log_prob(torch.stack([w[1], 1 - w[1]]))
    return r + torch.distributions.Poisson(w[2]).log_prob(torch.tensor(3.0, dtype=d)) + torch.distributions.Gamma(w[2], 1.0).log_prob(torch.tensor(2.0, dtype=d))


@case("distributions_discrete", 3, [[0.5, -1, 2]], third=True, example=[0.3, 0.4, 0.5])
def _dists_discrete(w):
    r = torch.distributions.Bernoulli(logits=w[0]).log_prob(torch.tensor(1.0, dtype=w.dtype))
    r = r + torch.distributions.Categorical(logits=w).log_prob(torch.tensor(2))
    return r + torch.distributions.Bernoulli(logits=w[1:]).log_prob(torch.tensor([0.0, 1.0], dtype=w.dtype)).sum()


@case("narrowing_cast", 2, [[0.5, 1.5], [2.0, 0.3]], third=True, tol_cpu=2e-6, rtol64=2e-6, example=[0.7, 1.2],
      note="Gamma(2.0, 3.0) with float32 parameters casts the argument to float32 inside a float64 callable: the graph does not "
           "model narrowing casts, so it stays in float64 and differs from torch by float32 rounding (stated bound 2e-6)")
def _narrowing(w):
    return torch.distributions.Gamma(torch.tensor(2.0), torch.tensor(3.0)).log_prob(w).sum()


# ---- what the table refuses ------------------------------------------------------------------------------------------------
@case("asinh_refused", 2, [[0.5, 1]], refuse="not in the lowering table")
def _asinh(w):
    return torch.asinh(w).sum()


@case("atan2_refused", 2, [[0.5, 1]], refuse="not in the lowering table")
def _atan2(w):
    return torch.atan2(w[0], w[1])


@case("cumprod_refused", 2, [[0.5, 1]], refuse="not in the lowering table")
def _cumprod(w):
    return torch.cumprod(w, 0).sum()


@case("logdet_refused", 4, [[2, 0.5, 0.5, 2]], refuse="")
def _logdet(w):
    return torch.logdet(w.reshape(2, 2))



# ---- overloads Python spells differently: called through torch.ops.aten ------------------------------------------------------
@case("aten_scalar_overloads", 3, [[0.5, -1, 2], [1, 2, 0.5]], third=True, example=[0.3, -0.4, 0.5])
def _aten_scalar(w):
    a = torch.ops.aten
    r = a.add.Scalar(w, 1.5).sum() + a.sub.Scalar(w, 0.5, 2).prod() + a.mul.Scalar(w, 3.0).pow(2).sum() + a.div.Scalar(w, 4.0).sum()
    r = r + a.norm.Scalar(w, 2) + a.norm.ScalarOpt_dim(w, 3, [0]) + a.alias.default(w)[1] * 2 + (w == 0.5).to(w.dtype).sum()
    return r + a.detach_.default(w.detach() * 1.0).sum() * w[0]


@case("aten_scalar_rounding", 2, [[1.5, 0.5], [-3, 2], [2.5, -1]], example=[1.3, 0.4])
def _aten_scalar_round(w):
    a = torch.ops.aten
    return (a.div.Scalar_mode(w, 2.0, rounding_mode="floor") * w).sum() + (a.floor_divide.Scalar(w.detach(), 0.5) * w).sum()


@case("asserts", 2, [[0.5, -1]], third=True, example=[0.3, -0.4])
def _asserts(w):
    torch._assert_async(w[0] > -1e300)
    torch.ops.aten._assert_async.msg(w[1] > -1e300, "finite")
    return (w * w * w).sum()


CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
