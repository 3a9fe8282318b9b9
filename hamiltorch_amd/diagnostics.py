"""Convergence diagnostics of the chains ``sample()`` returns, computed where the samples are: bulk effective sample size
and split R-hat of every coordinate of ``samples[S, C, D]`` on the GPU (csrc/diagnostics.hip).

The definitions are those of ``hamiltorch_amd/ess.py`` (linear autocovariance with divisor S, Geyer's initial positive
sequence, the multi-chain variance of Vehtari et al. 2021 without rank-normalisation; split R-hat of Gelman et al. 2013), in
fp64 whatever the sample dtype.  ``ess.py`` works one coordinate per Python iteration through an FFT and a host loop; here
one moments pass and a few rounds of lag blocks cover all D coordinates:

    out = hamiltorch_amd.sample(target, params_init, num_samples=1000, ...)      # list, row 0 = params_init
    s = hamiltorch_amd.diagnostics.summary(out, skip=1)
    s.ess_bulk, s.rhat, s.mean, s.sd                                             # [D] float64 tensors
    s.min_ess(), s.max_rhat()

The host loop: the first round computes ``LAG_BLOCK`` lags, every later round twice the lags of the one before; after each
round the finish kernel resumes every coordinate's Geyer walk and counts the coordinates still walking into one int32.
Reading that int32 is the only synchronisation.  Coordinates are processed in chunks sized by ``plan`` so that the
workspace stays within ``workspace_bytes``; results do not depend on the chunking (nor on strides), bit for bit.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import torch

from . import _abi
from .samplelist import as_tensor

#: lags per lag block B and rows of S per grid segment R (csrc/diagnostics.hip: DIAG_LAG_BLOCK, DIAG_SEGMENT_ROWS), the
#: chain groups of the lag kernel and the lag blocks one launch takes
LAG_BLOCK = 16
SEGMENT_ROWS = 256
CHAIN_GROUPS = 1024
MAX_LAG_BLOCKS = 32

Plan = namedtuple("Plan", "chunks n_segments chain_groups lags_per_launch bytes_per_coordinate")


def _lags_per_launch(S):
    return LAG_BLOCK * min(MAX_LAG_BLOCKS, -(-int(S) // LAG_BLOCK))


def workspace_bytes_for(S, C, D, n_lags):
    """Bytes of the workspace of hta_diag_* for D coordinates and launches of up to `n_lags` lags (the layout of
    csrc/diagnostics.hip: diag_layout, restated; the library checks the size it is given against its own)."""
    S, C, D, n_lags = int(S), int(C), int(D), int(n_lags)
    nseg = -(-S // SEGMENT_ROWS)
    P = nseg * min(C, CHAIN_GROUPS)
    return 8 * (3 * D + 2 * ((D + 1) // 2) + C * D + 4 * nseg * C * D + n_lags * D + n_lags * P * D)


def plan(S, C, D, itemsize=4, cap=256 << 20):
    """How summary() walks samples[S, C, D] under a workspace of at most `cap` bytes: the coordinate chunks [(d0, d1), ...]
    (they cover [0, D) once, in order, sizes as equal as they come), the segments S is cut into, the chain groups of the lag
    kernel, and the lags one launch takes.  Pure: no library, no device.  (`itemsize` of the samples does not enter - the
    workspace is fp64 for both sample dtypes.)  ValueError when `cap` cannot hold one coordinate."""
    S, C, D, cap = int(S), int(C), int(D), int(cap)
    if S < 1 or C < 1 or D < 1:
        raise ValueError("diagnostics.plan: bad shape (S=%d C=%d D=%d)" % (S, C, D))
    n_lags = _lags_per_launch(S)
    per = workspace_bytes_for(S, C, 2, n_lags) // 2                        # (two coordinates: the int32 state arrays pair up)
    dmax = D
    if workspace_bytes_for(S, C, D, n_lags) > cap:
        dmax = cap // per
        while dmax > 0 and workspace_bytes_for(S, C, dmax, n_lags) > cap:
            dmax -= 1
        if dmax < 1:
            raise ValueError("diagnostics: workspace_bytes=%d cannot hold one coordinate of samples[%d, %d, .] (%d bytes)"
                             % (cap, S, C, workspace_bytes_for(S, C, 1, n_lags)))
    n = -(-D // dmax)
    size = -(-D // n)
    chunks = [(d0, min(D, d0 + size)) for d0 in range(0, D, size)]
    return Plan(chunks, -(-S // SEGMENT_ROWS), min(C, CHAIN_GROUPS), n_lags, per)


class Summary:
    """Per-coordinate diagnostics of samples[S, C, D]: [D] tensors on the samples' device (float64 but `lags_used` int64 and
    `truncated` bool).  `truncated`: the Geyer walk of the coordinate ended by itself (a negative pair sum, the end of the
    series, or no spread at all) and was not stopped by `max_lag`."""
    __slots__ = ("mean", "sd", "ess_bulk", "rhat", "tau", "lags_used", "truncated", "n_draws", "n_chains")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def min_ess(self):
        """min over coordinates of ess_bulk (NaN if any coordinate has none, like ess.ess_min)."""
        v = self.ess_bulk
        return float("nan") if bool(torch.isnan(v).any()) else float(v.min())

    def max_rhat(self):
        """max over coordinates of rhat, NaN coordinates ignored (like ess.rhat_max)."""
        v = self.rhat[~torch.isnan(self.rhat)]
        return float(v.max()) if v.numel() else float("nan")

    def to(self, device):
        return Summary(**{k: (getattr(self, k).to(device) if torch.is_tensor(getattr(self, k)) else getattr(self, k)) for k in self.__slots__})

    def __repr__(self):
        return ("Summary(%d draws x %d chains x %d coordinates: min ess_bulk %.1f, max rhat %.4f)"
                % (self.n_draws, self.n_chains, self.mean.numel(), self.min_ess(), self.max_rhat()))


def _as_samples(samples):
    """The accepted inputs as one [S, C, D] tensor (a view wherever the input is a tensor or sample()'s lazy list)."""
    if not torch.is_tensor(samples):
        samples = list(samples) if not isinstance(samples, list) else samples
        if len(samples) and not torch.is_tensor(samples[0]):                # (a SampleList answers [0] from its backing tensor)
            samples = [torch.as_tensor(r) for r in samples]
        samples = as_tensor(samples)
    if samples.dim() == 2:
        samples = samples.unsqueeze(1)
    if samples.dim() != 3:
        raise ValueError("diagnostics: samples must be [S, C, D] or [S, D], got shape %s" % (tuple(samples.shape),))
    if not samples.is_floating_point():
        raise ValueError("diagnostics: samples must be floating point, got %s" % samples.dtype)
    return samples


def summary(samples, skip=0, max_lag=None, workspace_bytes=256 << 20):
    """Diagnostics of `samples` ([S, C, D] tensor, [S, D] tensor = one chain, the list sample() returns, or a plain list of rows)
    after dropping the first `skip` rows (row 0 of sample()'s list is params_init: pass skip=1).  `max_lag`: the Geyer walks
    use lags below it only (default: as far as they go).  CPU samples are staged to the GPU and the results come back on the
    CPU.  Returns a Summary."""
    x = _as_samples(samples)
    skip = int(skip)
    if skip < 0:
        raise ValueError("diagnostics: skip=%d" % skip)
    S, C, D = x.shape[0] - skip, x.shape[1], x.shape[2]
    if S < 4:
        raise ValueError("diagnostics: %d draws after skip=%d; at least 4 are needed" % (S, skip))
    if C < 1 or D < 1:
        raise ValueError("diagnostics: no chains or no coordinates in samples of shape %s" % (tuple(x.shape),))
    if max_lag is not None and int(max_lag) < 2:
        raise ValueError("diagnostics: max_lag=%r; a Geyer pair needs two lags" % (max_lag,))
    if x.dtype not in (torch.float32, torch.float64):
        x = x.to(torch.float32)                                             # half / bfloat16 samples: exact in float32
    pl = plan(S, C, D, x.element_size(), workspace_bytes)
    host = not x.is_cuda
    if host:
        from .host import _device
        x = x.to(_device())
    _abi.require_device(x, "samples")
    x = x[skip:]
    if x.stride(2) != 1 or x.stride(1) < D or x.stride(0) < (C - 1) * x.stride(1) + D:
        x = x.contiguous()
    out = _run(x, pl, S if max_lag is None else min(S, int(max_lag)))
    return out.to("cpu") if host else out


def _run(x, pl, lag_limit):
    lib = _abi.load()
    S, C, D = x.shape
    dev = x.device
    suf = _abi._suffix(x)
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    mean, sd, rhat, tau, ess = (torch.empty(D, **f64) for _ in range(5))
    lags, done = torch.empty(D, **i32), torch.empty(D, **i32)
    count = torch.zeros(1, **i32)
    moments, lag_fn = getattr(lib, "hta_diag_moments_" + suf), getattr(lib, "hta_diag_lags_" + suf)
    ss, sc, item = x.stride(0), x.stride(1), x.element_size()
    vp = ctypes.c_void_p
    with torch.cuda.device(dev):
        width = max(d1 - d0 for d0, d1 in pl.chunks)
        nbytes = int(lib.hta_diag_workspace_bytes(S, C, width, pl.lags_per_launch))
        ws = _abi.scratch(x, nbytes, "diag")
        wsp, st = vp(ws.data_ptr()), _abi._stream(x)
        for d0, d1 in pl.chunks:
            k = d1 - d0
            xp = vp(x.data_ptr() + d0 * item)
            at = lambda t: vp(t.data_ptr() + d0 * t.element_size())            # noqa: E731
            _abi._check(moments(xp, ss, sc, S, C, k, at(mean), at(sd), at(rhat), wsp, nbytes, st), "hta_diag_moments")
            t0, round_lags = 0, LAG_BLOCK
            while True:
                end = min(t0 + round_lags, -(-lag_limit // LAG_BLOCK) * LAG_BLOCK)
                while t0 < end:
                    n = min(end - t0, pl.lags_per_launch)
                    _abi._check(lag_fn(xp, ss, sc, S, C, k, t0, n, wsp, nbytes, st), "hta_diag_lags")
                    _abi._check(lib.hta_diag_finish(S, C, k, t0, n, lag_limit, at(tau), at(ess), at(lags), at(done), vp(count.data_ptr()),
                                                    wsp, nbytes, st), "hta_diag_finish")
                    t0 += n
                if int(count.item()) == 0 or t0 >= lag_limit:                   # the one read-back of a round
                    break
                round_lags *= 2
    return Summary(mean=mean, sd=sd, ess_bulk=ess, rhat=rhat, tau=tau, lags_used=lags.to(torch.int64), truncated=done.to(torch.bool),
                   n_draws=int(S), n_chains=int(C))


def ess(samples, skip=0, max_lag=None, workspace_bytes=256 << 20):
    """[D] bulk effective sample sizes of samples (see summary)."""
    return summary(samples, skip, max_lag, workspace_bytes).ess_bulk


def rhat(samples, skip=0, workspace_bytes=256 << 20):
    """[D] split R-hat of samples (see summary; the moments pass and one round of lags)."""
    return summary(samples, skip, LAG_BLOCK, workspace_bytes).rhat


def ess_min(samples, skip=0, max_lag=None, workspace_bytes=256 << 20):
    """min over coordinates of the bulk effective sample size (ess.ess_min for all coordinates at once)."""
    return summary(samples, skip, max_lag, workspace_bytes).min_ess()


def rhat_max(samples, skip=0, workspace_bytes=256 << 20):
    """max over coordinates of split R-hat, NaN coordinates ignored (ess.rhat_max)."""
    return summary(samples, skip, LAG_BLOCK, workspace_bytes).max_rhat()
