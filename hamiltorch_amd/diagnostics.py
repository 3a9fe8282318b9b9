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

``rank_summary`` adds the rank-normalised half of Vehtari et al. 2021 (csrc/diagnostics_rank.hip): the draws of all chains of a
coordinate are ranked together by a segmented radix sort on the device, mapped to normal scores, and the scores, the folded
draws' scores and the 5 % / 95 % indicators go through the same stages:

    r = hamiltorch_amd.diagnostics.rank_summary(out, skip=1)
    r.ess_bulk, r.ess_tail, r.rhat, r.rhat_bulk, r.rhat_folded, r.q05, r.median, r.q95

``RunningMoments`` is the streaming half (csrc/moments.hip): per-chain mean and M2 of every coordinate, updated chunk by chunk, for
mean, sd, within / between variance and R-hat of runs that are never held in memory at once - and the pooled variance the
cross-chain warm-up takes its diagonal mass from (hamiltorch_amd/adapt.py):

    acc = hamiltorch_amd.diagnostics.RunningMoments()
    acc.update(out, skip=1)                                                       # as often as chunks arrive
    m = acc.result(reg_n=5)
    m.mean, m.sd, m.var_within, m.var_between, m.var_total, m.rhat, m.inv_mass

``RunningCovariance`` (csrc/covariance.hip) keeps the off-diagonal too - per chain the co-moments of every pair of coordinates,
D <= COVARIANCE_MAX_D -, with the same surface; its result has cov_within, cov_total, corr and a [D, D] inv_mass, the dense mass
of warmup(mass="dense").
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


# ---- rank-normalised diagnostics (csrc/diagnostics_rank.hip) -------------------------------------------------------------------------
#: keys per block and pass of the segmented radix sort (csrc/diagnostics_rank.hip: DIAG_RANK_TILE)
RANK_TILE = 2048

RankPlan = namedtuple("RankPlan", "chunks n_tiles lags_per_launch bytes_per_coordinate")


def _r8(n):
    return -(-n // 8) * 8


def rank_workspace_bytes_for(S, C, D, key_bytes=8):
    """Bytes of the workspace of hta_diag_rank* for D coordinates (the layout of csrc/diagnostics_rank.hip: diag_rank_layout,
    restated): keys and uint32 payloads, twice each for the ping-pong of the passes, and 256 digit counts per tile."""
    N, D, key_bytes = int(S) * int(C), int(D), int(key_bytes)
    return 2 * _r8(N * D * key_bytes) + 2 * _r8(N * D * 4) + D * -(-N // RANK_TILE) * 1024


def rank_bytes_for(S, C, D, n_lags):
    """Everything rank_summary() holds on the device for D coordinates at a time: the sort's workspace (8-byte keys: the fold's),
    the derived series z[S, C, D] (fp64; zf reuses it) and I05 / I95 (float), and the workspace of the existing stages."""
    S, C, D = int(S), int(C), int(D)
    return rank_workspace_bytes_for(S, C, D, 8) + 16 * S * C * D + workspace_bytes_for(S, C, D, n_lags)


def rank_plan(S, C, D, itemsize=4, cap=256 << 20):
    """plan() for rank_summary(): the coordinate chunks [(d0, d1), ...] under which keys, payloads, their ping-pong buffers, the
    digit counts, the derived series and the existing stages' workspace together stay within `cap` bytes.  Pure.  (`itemsize` does
    not enter: the fold sorts 8-byte keys for both sample dtypes.)  ValueError when `cap` cannot hold one coordinate."""
    S, C, D, cap = int(S), int(C), int(D), int(cap)
    if S < 1 or C < 1 or D < 1:
        raise ValueError("diagnostics.rank_plan: bad shape (S=%d C=%d D=%d)" % (S, C, D))
    if S * C >= 1 << 31:
        raise ValueError("diagnostics: %d x %d draws per coordinate; the ranking takes fewer than 2^31" % (S, C))
    n_lags = _lags_per_launch(S)
    per = rank_bytes_for(S, C, 2, n_lags) // 2
    dmax = D
    if rank_bytes_for(S, C, D, n_lags) > cap:
        dmax = cap // per
        while dmax > 0 and rank_bytes_for(S, C, dmax, n_lags) > cap:
            dmax -= 1
        if dmax < 1:
            raise ValueError("diagnostics: workspace_bytes=%d cannot hold one coordinate of samples[%d, %d, .] with its ranks (%d bytes)"
                             % (cap, S, C, rank_bytes_for(S, C, 1, n_lags)))
    n_tiles = -(-(S * C) // RANK_TILE)
    dmax = min(dmax, max(1, ((1 << 31) - 1) // n_tiles))                   # (coordinates x tiles is one grid axis)
    n = -(-D // dmax)
    size = -(-D // n)
    return RankPlan([(d0, min(D, d0 + size)) for d0 in range(0, D, size)], n_tiles, n_lags, per)


class RankSummary:
    """Rank-normalised diagnostics of samples[S, C, D] (Vehtari et al. 2021): [D] float64 tensors on the samples' device.
    `ess_bulk` / `rhat_bulk`: ESS and split R-hat of the rank-normalised draws z; `rhat_folded`: split R-hat of the rank-normalised
    |x - median|; `rhat` = max(rhat_bulk, rhat_folded); `ess_tail` = min of the ESS of the indicators of the 5 % and 95 % order
    statistics; `q05`, `median`, `q95`: numpy's linear-interpolation quantiles over all draws.  A coordinate holding a NaN or an
    infinity is NaN in every field; a constant one is NaN in every ESS and R-hat (its quantiles are the constant).  `route`: the
    sort kernel the ranking dispatched to."""
    __slots__ = ("ess_bulk", "ess_tail", "rhat", "rhat_bulk", "rhat_folded", "q05", "median", "q95", "n_draws", "n_chains", "route")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def min_ess(self):
        """min over coordinates of ess_bulk and ess_tail (NaN if any coordinate has none)."""
        v = torch.minimum(self.ess_bulk, self.ess_tail)
        return float("nan") if bool(torch.isnan(v).any()) else float(v.min())

    def max_rhat(self):
        """max over coordinates of rhat, NaN coordinates ignored."""
        v = self.rhat[~torch.isnan(self.rhat)]
        return float(v.max()) if v.numel() else float("nan")

    def to(self, device):
        return RankSummary(**{k: (getattr(self, k).to(device) if torch.is_tensor(getattr(self, k)) else getattr(self, k)) for k in self.__slots__})

    def __repr__(self):
        return ("RankSummary(%d draws x %d chains x %d coordinates: min ess %.1f, max rhat %.4f)"
                % (self.n_draws, self.n_chains, self.rhat.numel(), self.min_ess(), self.max_rhat()))


def rank_summary(samples, skip=0, max_lag=None, workspace_bytes=256 << 20):
    """Rank-normalised diagnostics of `samples`: the inputs, `skip`, `max_lag` and the CPU-in, CPU-out rule of summary().  Per
    coordinate the S C draws of all chains are ranked together (ties averaged, -0.0 = +0.0) and mapped to normal scores
    z = Phi^-1((r - 3/8) / (S C + 1/4)); ESS and split R-hat of z, of the folded draws' z and of the tail indicators are those of
    summary() (the ESS on unsplit chains - ArviZ splits the chains for its ESS first, so its numbers differ slightly).  Returns a
    RankSummary."""
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
        x = x.to(torch.float32)
    pl = rank_plan(S, C, D, x.element_size(), workspace_bytes)
    host = not x.is_cuda
    if host:
        from .host import _device
        x = x.to(_device())
    _abi.require_device(x, "samples")
    x = x[skip:]
    if x.stride(2) != 1 or x.stride(1) < D or x.stride(0) < (C - 1) * x.stride(1) + D:
        x = x.contiguous()
    out = _run_rank(x, pl, S if max_lag is None else min(S, int(max_lag)))
    return out.to("cpu") if host else out


def _run_rank(x, pl, lag_limit):
    lib = _abi.load()
    S, C, D = x.shape
    dev = x.device
    suf = _abi._suffix(x)
    f64 = dict(dtype=torch.float64, device=dev)
    ess_b, ess_t, rh, rh_b, rh_f, q05, med, q95, centre = (torch.empty(D, **f64) for _ in range(9))
    bad = torch.empty(D, dtype=torch.int32, device=dev)
    rank_fn, fold_fn = getattr(lib, "hta_diag_rank_" + suf), getattr(lib, "hta_diag_rank_folded_" + suf)
    ss, sc, item = x.stride(0), x.stride(1), x.element_size()
    vp = ctypes.c_void_p
    route = ""
    with torch.cuda.device(dev):
        width = max(d1 - d0 for d0, d1 in pl.chunks)
        wsb = int(lib.hta_diag_rank_workspace_bytes(S, C, width, 8))
        ws = _abi.scratch(x, wsb + 16 * S * C * width, "diag_rank")
        st = _abi._stream(x)
        for d0, d1 in pl.chunks:
            k = d1 - d0
            n = S * C * k
            z = ws[wsb:wsb + 8 * n].view(torch.float64).view(S, C, k)
            i05 = ws[wsb + 8 * n:wsb + 12 * n].view(torch.float32).view(S, C, k)
            i95 = ws[wsb + 12 * n:wsb + 16 * n].view(torch.float32).view(S, C, k)
            one = Plan([(0, k)], -(-S // SEGMENT_ROWS), min(C, CHAIN_GROUPS), pl.lags_per_launch, 0)
            xp = vp(x.data_ptr() + d0 * item)
            at = lambda t: vp(t.data_ptr() + d0 * t.element_size())            # noqa: E731
            _abi._check(rank_fn(xp, ss, sc, S, C, k, vp(z.data_ptr()), vp(i05.data_ptr()), vp(i95.data_ptr()), at(q05), at(med), at(q95), at(centre),
                                at(bad), vp(ws.data_ptr()), wsb, st), "hta_diag_rank")
            route = _abi.last_route()
            sz = _run(z, one, lag_limit)
            ess_b[d0:d1], rh_b[d0:d1] = sz.ess_bulk, sz.rhat
            ess_t[d0:d1] = torch.minimum(_run(i05, one, lag_limit).ess_bulk, _run(i95, one, lag_limit).ess_bulk)
            _abi._check(fold_fn(xp, ss, sc, S, C, k, at(centre), vp(z.data_ptr()), at(bad), vp(ws.data_ptr()), wsb, st), "hta_diag_rank_folded")
            rh_f[d0:d1] = _moments_rhat(z)
    torch.maximum(rh_b, rh_f, out=rh)
    return RankSummary(ess_bulk=ess_b, ess_tail=ess_t, rhat=rh, rhat_bulk=rh_b, rhat_folded=rh_f, q05=q05, median=med, q95=q95, n_draws=int(S),
                       n_chains=int(C), route=route)


def _moments_rhat(x):
    """[D] split R-hat of the contiguous series x[S, C, D]: the moments stage alone."""
    lib = _abi.load()
    S, C, D = x.shape
    mean, sd, rhat_ = (torch.empty(D, dtype=torch.float64, device=x.device) for _ in range(3))
    nbytes = int(lib.hta_diag_workspace_bytes(S, C, D, 0))
    ws = _abi.scratch(x, nbytes, "diag")
    vp = ctypes.c_void_p
    _abi._check(getattr(lib, "hta_diag_moments_" + _abi._suffix(x))(vp(x.data_ptr()), x.stride(0), x.stride(1), S, C, D, vp(mean.data_ptr()), vp(sd.data_ptr()),
                                                                    vp(rhat_.data_ptr()), vp(ws.data_ptr()), nbytes, _abi._stream(x)), "hta_diag_moments")
    return rhat_


def ess_tail(samples, skip=0, max_lag=None, workspace_bytes=256 << 20):
    """[D] tail effective sample sizes of samples (see rank_summary)."""
    return rank_summary(samples, skip, max_lag, workspace_bytes).ess_tail


def rhat_rank(samples, skip=0, workspace_bytes=256 << 20):
    """[D] rank-normalised R-hat of samples: the larger of the bulk and the folded statistic (see rank_summary)."""
    return rank_summary(samples, skip, LAG_BLOCK, workspace_bytes).rhat


# ---- running moments (csrc/moments.hip) -------------------------------------------------------------------------------------
#: rows of S per grid segment of the update kernel, its lower limit, the grid size below which segments are halved, the lanes
#: of a workgroup, and the chain slices of the finish kernel (csrc/moments.hip: MOM_*)
MOMENTS_SEGMENT_ROWS = 256
MOMENTS_MIN_SEGMENT_ROWS = 32
MOMENTS_TARGET_BLOCKS = 512
MOMENTS_THREADS = 256
MOMENTS_CHAIN_SLICES = 16


def moments_segment_rows(S, C, D):
    """Rows per segment of an update with a chunk x[S, C, D] (csrc/moments.hip: moments_segment_rows, restated).  Pure."""
    bx = -(-int(C) * int(D) // MOMENTS_THREADS)
    R = MOMENTS_SEGMENT_ROWS
    while R > MOMENTS_MIN_SEGMENT_ROWS and bx * -(-int(S) // R) < MOMENTS_TARGET_BLOCKS:
        R //= 2
    return R


class MomentsResult:
    """Pooled statistics of a RunningMoments: [D] float64 tensors on the samples' device.  `mean`: the mean of the chain means;
    `var_within`: the mean over chains of their unbiased variances; `var_between`: the unbiased variance of the chain means;
    `var_total`: the unbiased variance of all draws of all chains around `mean`; `sd` = sqrt(var_total); `rhat`: R-hat of the
    unsplit chains (stack() the accumulators of a run's halves for split R-hat); `inv_mass` ([D], `dtype`): the regularised
    `var_total`, or None when no `reg_n` was given."""
    __slots__ = ("mean", "sd", "var_within", "var_between", "var_total", "rhat", "inv_mass", "n_draws", "n_chains")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def max_rhat(self):
        """max over coordinates of rhat, NaN coordinates ignored."""
        v = self.rhat[~torch.isnan(self.rhat)]
        return float(v.max()) if v.numel() else float("nan")

    def to(self, device):
        return MomentsResult(**{k: (getattr(self, k).to(device) if torch.is_tensor(getattr(self, k)) else getattr(self, k)) for k in self.__slots__})

    def __repr__(self):
        return "MomentsResult(%d draws x %d chains x %d coordinates)" % (self.n_draws, self.n_chains, self.mean.numel())


class RunningMoments:
    """Per-chain mean and M2 of every coordinate of samples that arrive chunk by chunk, in fp64 on the device (csrc/moments.hip):

        acc = hamiltorch_amd.diagnostics.RunningMoments()
        for _ in range(100):
            out = hamiltorch_amd.sample(target, start, num_samples=50, ...)        # rows never held together
            acc.update(out, skip=1)
            start = out[-1]
        r = acc.result()
        r.mean, r.sd, r.rhat                                                        # [D] float64 tensors

    `RunningMoments(C, D, device)` fixes the shape at once; without arguments the first update() does.  The state is
    `state[2, C, D]` (means, M2) and the host integer `n_draws`.  CPU samples are staged to the GPU chunk by chunk like in
    summary(), and the results of an accumulator fed from the CPU come back on the CPU."""

    def __init__(self, C=None, D=None, device=None):
        self.state, self.n_draws, self._host = None, 0, False
        if (C is None) != (D is None):
            raise ValueError("RunningMoments: give both C and D, or neither")
        if C is not None:
            if int(C) < 1 or int(D) < 1:
                raise ValueError("RunningMoments: bad shape (C=%d D=%d)" % (C, D))
            dev = torch.device("cuda" if device is None else device)
            self._host = dev.type != "cuda"
            if self._host:
                from .host import _device
                dev = _device()
            self.state = torch.zeros((2, int(C), int(D)), dtype=torch.float64, device=dev)

    @property
    def n_chains(self):
        return None if self.state is None else int(self.state.shape[1])

    @property
    def n_coordinates(self):
        return None if self.state is None else int(self.state.shape[2])

    def reset(self):
        """Forget every draw (the shape stays)."""
        self.n_draws = 0
        return self

    def update(self, samples, skip=0):
        """Add the rows of `samples` after the first `skip` ([S, C, D] tensor, [S, D] tensor = one chain, the list sample()
        returns - row 0 is params_init: skip=1 -, or a plain list of rows).  Returns self."""
        x = _as_samples(samples)
        skip = int(skip)
        if skip < 0:
            raise ValueError("RunningMoments: skip=%d" % skip)
        S, C, D = x.shape[0] - skip, x.shape[1], x.shape[2]
        if C < 1 or D < 1:
            raise ValueError("RunningMoments: no chains or no coordinates in samples of shape %s" % (tuple(x.shape),))
        if S < 1:
            return self
        if x.dtype not in (torch.float32, torch.float64):
            x = x.to(torch.float32)
        if not x.is_cuda:
            from .host import _device
            if self.state is None:
                self._host = True
            x = x.to(self.state.device if self.state is not None else _device())
        _abi.require_device(x, "samples")
        if self.state is None:
            self.state = torch.empty((2, C, D), dtype=torch.float64, device=x.device)
        if (C, D) != tuple(self.state.shape[1:]) or x.device != self.state.device:
            raise ValueError("RunningMoments: samples of %d chains x %d coordinates on %s; the accumulator holds %d x %d on %s"
                             % (C, D, x.device, self.state.shape[1], self.state.shape[2], self.state.device))
        x = x[skip:]
        if x.stride(2) != 1 or x.stride(1) < D or x.stride(0) < (C - 1) * x.stride(1) + D:
            x = x.contiguous()
        lib = _abi.load()
        vp = ctypes.c_void_p
        with torch.cuda.device(x.device):
            nbytes = int(lib.hta_moments_workspace_bytes(S, C, D))
            ws = _abi.scratch(x, nbytes, "moments")
            _abi._check(getattr(lib, "hta_moments_update_" + _abi._suffix(x))(vp(x.data_ptr()), x.stride(0), x.stride(1), S, C, D, self.n_draws,
                                                                             vp(self.state.data_ptr()), None if ws is None else vp(ws.data_ptr()), nbytes,
                                                                             _abi._stream(x)), "hta_moments_update")
        self.n_draws += S
        return self

    def merge(self, other):
        """Add the draws another accumulator of the same chains has seen, chain by chain (Chan's formula; the counts may differ).
        Returns self."""
        if other.state is None or other.n_draws == 0:
            return self
        if self.state is None:
            self.state, self._host = torch.empty_like(other.state), other._host
        if self.state.shape != other.state.shape or self.state.device != other.state.device:
            raise ValueError("RunningMoments.merge: %s on %s and %s on %s" % (tuple(self.state.shape[1:]), self.state.device,
                                                                               tuple(other.state.shape[1:]), other.state.device))
        if self.n_draws == 0:
            self.state.copy_(other.state)
        else:
            na, nb = float(self.n_draws), float(other.n_draws)
            delta = other.state[0] - self.state[0]
            self.state[1] += other.state[1] + delta * delta * (na * nb / (na + nb))
            self.state[0] += delta * (nb / (na + nb))
            bad = ~(torch.isfinite(self.state[0]) & torch.isfinite(self.state[1]))
            self.state[:, bad] = float("nan")
        self.n_draws += other.n_draws
        return self

    @classmethod
    def stack(cls, parts):
        """A new accumulator whose chains are the chains of `parts` side by side (equal draw counts and coordinates).  Of the
        accumulators of a run's first and last half it is the accumulator of the 2 C half chains: its rhat is split R-hat."""
        parts = list(parts)
        if not parts or any(p.state is None for p in parts):
            raise ValueError("RunningMoments.stack: an accumulator without a shape")
        if len({p.n_draws for p in parts}) != 1 or len({(p.state.shape[2], p.state.device) for p in parts}) != 1:
            raise ValueError("RunningMoments.stack: the parts differ in draws, coordinates or device")
        out = cls()
        out.state = torch.cat([p.state for p in parts], dim=1).contiguous()
        out.n_draws, out._host = parts[0].n_draws, all(p._host for p in parts)
        return out

    def result(self, reg_n=None, reg_floor=1e-3, dtype=None):
        """The pooled statistics of the draws seen so far (a MomentsResult).  With `reg_n` also `inv_mass` of `dtype` (default
        float32): var_total N / (N + reg_n) + reg_floor reg_n / (N + reg_n), N = n_draws x chains (Stan: reg_n = 5)."""
        if self.state is None or self.n_draws < 1:
            raise ValueError("RunningMoments.result: no draws yet")
        lib = _abi.load()
        _, C, D = self.state.shape
        dev = self.state.device
        mean, vw, vb, vt, rh = (torch.empty(D, dtype=torch.float64, device=dev) for _ in range(5))
        im = None
        if reg_n is not None:
            dtype = torch.float32 if dtype is None else dtype
            if dtype not in (torch.float32, torch.float64):
                raise TypeError("RunningMoments.result: inv_mass in float32 or float64, got %s" % dtype)
            im = torch.empty(D, dtype=dtype, device=dev)
        vp = ctypes.c_void_p
        p = lambda t: vp(t.data_ptr())                                           # noqa: E731
        with torch.cuda.device(dev):
            _abi._check(lib.hta_moments_finish(C, D, self.n_draws, p(self.state), p(mean), p(vw), p(vb), p(vt), p(rh),
                                               0.0 if reg_n is None else float(reg_n), float(reg_floor),
                                               p(im) if im is not None and im.dtype == torch.float32 else None,
                                               p(im) if im is not None and im.dtype == torch.float64 else None,
                                               _abi._stream(self.state)), "hta_moments_finish")
        out = MomentsResult(mean=mean, sd=torch.sqrt(vt), var_within=vw, var_between=vb, var_total=vt, rhat=rh, inv_mass=im,
                            n_draws=int(self.n_draws), n_chains=int(C))
        return out.to("cpu") if self._host else out


# ---- running covariance (csrc/covariance.hip) -------------------------------------------------------------------------------
#: the largest D of RunningCovariance (include/hamiltorch_amd.h: HTA_COV_MAX_D): the state holds D (D + 1) / 2 co-moments per
#: chain, 270 MB at 1024 chains and D = 256
COVARIANCE_MAX_D = 256


class CovarianceResult:
    """Pooled statistics of a RunningCovariance: float64 tensors on the samples' device.  `mean` [D]: the mean of the chain
    means; `cov_within` [D, D]: the mean over chains of their unbiased covariances; `cov_total` [D, D]: the unbiased covariance
    of all draws of all chains around `mean`; `sd` = sqrt(diag(cov_total)); `corr` = cov_total / (sd sd^T); `rhat` [D]: R-hat of
    the unsplit chains; `inv_mass` ([D, D], `dtype`): the regularised `cov_total`, or None when no `reg_n` was given.  The
    matrices are exactly symmetric; the diagonals, `mean` and `rhat` are MomentsResult's values of the same feed, bit for bit."""
    __slots__ = ("mean", "sd", "cov_within", "cov_total", "corr", "rhat", "inv_mass", "n_draws", "n_chains")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def max_rhat(self):
        """max over coordinates of rhat, NaN coordinates ignored."""
        v = self.rhat[~torch.isnan(self.rhat)]
        return float(v.max()) if v.numel() else float("nan")

    def to(self, device):
        return CovarianceResult(**{k: (getattr(self, k).to(device) if torch.is_tensor(getattr(self, k)) else getattr(self, k)) for k in self.__slots__})

    def __repr__(self):
        return "CovarianceResult(%d draws x %d chains x %d coordinates)" % (self.n_draws, self.n_chains, self.mean.numel())


class RunningCovariance:
    """Per-chain means and co-moments of every pair of coordinates of samples that arrive chunk by chunk, in fp64 on the device
    (csrc/covariance.hip) - RunningMoments with the off-diagonal kept:

        acc = hamiltorch_amd.diagnostics.RunningCovariance()
        for _ in range(100):
            out = hamiltorch_amd.sample(target, start, num_samples=50, ...)
            acc.update(out, skip=1)
            start = out[-1]
        r = acc.result(reg_n=5)
        r.cov_total, r.corr, r.inv_mass                                             # [D, D]

    `RunningCovariance(C, D, device)` fixes the shape at once; without arguments the first update() does.  D is at most
    COVARIANCE_MAX_D.  The state is one float64 buffer - `means` [C, D] followed by `comoments` [C, T], T = D (D + 1) / 2, the
    pairs i <= j packed row-major - and the host integer `n_draws`.  CPU samples are staged to the GPU, and the results of an
    accumulator fed from the CPU come back on the CPU."""

    def __init__(self, C=None, D=None, device=None):
        self.state, self.n_draws, self._host, self._shape = None, 0, False, None
        if (C is None) != (D is None):
            raise ValueError("RunningCovariance: give both C and D, or neither")
        if C is not None:
            if int(C) < 1 or int(D) < 1:
                raise ValueError("RunningCovariance: bad shape (C=%d D=%d)" % (C, D))
            self._check_d(int(D))
            dev = torch.device("cuda" if device is None else device)
            self._host = dev.type != "cuda"
            if self._host:
                from .host import _device
                dev = _device()
            self._allocate(int(C), int(D), dev, zero=True)

    @staticmethod
    def _check_d(D):
        if D > COVARIANCE_MAX_D:
            raise ValueError("RunningCovariance: D=%d is beyond the limit of %d coordinates (COVARIANCE_MAX_D)" % (D, COVARIANCE_MAX_D))

    def _allocate(self, C, D, dev, zero=False):
        self._shape = (C, D)
        n = C * (D + D * (D + 1) // 2)
        self.state = (torch.zeros if zero else torch.empty)(n, dtype=torch.float64, device=dev)

    @property
    def n_chains(self):
        return None if self.state is None else self._shape[0]

    @property
    def n_coordinates(self):
        return None if self.state is None else self._shape[1]

    @property
    def means(self):
        """[C, D] view of the state: the chains' means."""
        C, D = self._shape
        return self.state[:C * D].view(C, D)

    @property
    def comoments(self):
        """[C, T] view of the state: the chains' co-moments, the pairs i <= j packed row-major."""
        C, D = self._shape
        return self.state[C * D:].view(C, -1)

    def reset(self):
        """Forget every draw (the shape stays)."""
        self.n_draws = 0
        return self

    def update(self, samples, skip=0):
        """Add the rows of `samples` after the first `skip` (the inputs of RunningMoments.update).  Returns self."""
        x = _as_samples(samples)
        skip = int(skip)
        if skip < 0:
            raise ValueError("RunningCovariance: skip=%d" % skip)
        S, C, D = x.shape[0] - skip, x.shape[1], x.shape[2]
        if C < 1 or D < 1:
            raise ValueError("RunningCovariance: no chains or no coordinates in samples of shape %s" % (tuple(x.shape),))
        self._check_d(D)
        if S < 1:
            return self
        if x.dtype not in (torch.float32, torch.float64):
            x = x.to(torch.float32)
        if not x.is_cuda:
            from .host import _device
            if self.state is None:
                self._host = True
            x = x.to(self.state.device if self.state is not None else _device())
        _abi.require_device(x, "samples")
        if self.state is None:
            self._allocate(C, D, x.device)
        if (C, D) != self._shape or x.device != self.state.device:
            raise ValueError("RunningCovariance: samples of %d chains x %d coordinates on %s; the accumulator holds %d x %d on %s"
                             % (C, D, x.device, self._shape[0], self._shape[1], self.state.device))
        x = x[skip:]
        if x.stride(2) != 1 or x.stride(1) < D or x.stride(0) < (C - 1) * x.stride(1) + D:
            x = x.contiguous()
        lib = _abi.load()
        vp = ctypes.c_void_p
        with torch.cuda.device(x.device):
            nbytes = int(lib.hta_cov_workspace_bytes(S, C, D))
            ws = _abi.scratch(x, nbytes, "covariance")
            _abi._check(getattr(lib, "hta_cov_update_" + _abi._suffix(x))(vp(x.data_ptr()), x.stride(0), x.stride(1), S, C, D, self.n_draws,
                                                                         vp(self.state.data_ptr()), None if ws is None else vp(ws.data_ptr()), nbytes,
                                                                         _abi._stream(x)), "hta_cov_update")
        self.n_draws += S
        return self

    def merge(self, other):
        """Add the draws another accumulator of the same chains has seen, chain by chain (Chan's formula; the counts may differ).
        Returns self."""
        if other.state is None or other.n_draws == 0:
            return self
        if self.state is None:
            self.state, self._host, self._shape = torch.empty_like(other.state), other._host, other._shape
        if self._shape != other._shape or self.state.device != other.state.device:
            raise ValueError("RunningCovariance.merge: %s on %s and %s on %s" % (self._shape, self.state.device, other._shape, other.state.device))
        if self.n_draws == 0:
            self.state.copy_(other.state)
        else:
            na, nb = float(self.n_draws), float(other.n_draws)
            D = self._shape[1]
            iu, ju = torch.triu_indices(D, D, device=self.state.device)
            delta = other.means - self.means
            self.comoments.add_(other.comoments).add_(delta[:, iu] * delta[:, ju] * (na * nb / (na + nb)))
            self.means.add_(delta * (nb / (na + nb)))
            q = self.comoments
            q[~torch.isfinite(self.means[:, iu] + self.means[:, ju] + q)] = float("nan")
            self.means[torch.isnan(q[:, iu == ju])] = float("nan")
        self.n_draws += other.n_draws
        return self

    @classmethod
    def stack(cls, parts):
        """A new accumulator whose chains are the chains of `parts` side by side (equal draw counts and coordinates).  Of the
        accumulators of a run's first and last half it is the accumulator of the 2 C half chains: its rhat is split R-hat."""
        parts = list(parts)
        if not parts or any(p.state is None for p in parts):
            raise ValueError("RunningCovariance.stack: an accumulator without a shape")
        if len({p.n_draws for p in parts}) != 1 or len({(p._shape[1], p.state.device) for p in parts}) != 1:
            raise ValueError("RunningCovariance.stack: the parts differ in draws, coordinates or device")
        out = cls()
        out.state = torch.cat([p.means.reshape(-1) for p in parts] + [p.comoments.reshape(-1) for p in parts])
        out._shape = (sum(p._shape[0] for p in parts), parts[0]._shape[1])
        out.n_draws, out._host = parts[0].n_draws, all(p._host for p in parts)
        return out

    def result(self, reg_n=None, reg_floor=1e-3, dtype=None):
        """The pooled statistics of the draws seen so far (a CovarianceResult).  With `reg_n` also `inv_mass` [D, D] of `dtype`
        (default float32): cov_total N / (N + reg_n) + reg_floor reg_n / (N + reg_n) I, N = n_draws x chains (Stan: reg_n = 5)."""
        if self.state is None or self.n_draws < 1:
            raise ValueError("RunningCovariance.result: no draws yet")
        lib = _abi.load()
        C, D = self._shape
        dev = self.state.device
        mean, rh = (torch.empty(D, dtype=torch.float64, device=dev) for _ in range(2))
        cw, ct = (torch.empty((D, D), dtype=torch.float64, device=dev) for _ in range(2))
        im = None
        if reg_n is not None:
            dtype = torch.float32 if dtype is None else dtype
            if dtype not in (torch.float32, torch.float64):
                raise TypeError("RunningCovariance.result: inv_mass in float32 or float64, got %s" % dtype)
            im = torch.empty((D, D), dtype=dtype, device=dev)
        vp = ctypes.c_void_p
        p = lambda t: vp(t.data_ptr())                                           # noqa: E731
        with torch.cuda.device(dev):
            _abi._check(lib.hta_cov_finish(C, D, self.n_draws, p(self.state), p(mean), p(cw), p(ct), p(rh),
                                           0.0 if reg_n is None else float(reg_n), float(reg_floor),
                                           p(im) if im is not None and im.dtype == torch.float32 else None,
                                           p(im) if im is not None and im.dtype == torch.float64 else None,
                                           _abi._stream(self.state)), "hta_cov_finish")
        sd = torch.sqrt(ct.diagonal())
        out = CovarianceResult(mean=mean, sd=sd, cov_within=cw, cov_total=ct, corr=ct / (sd[:, None] * sd[None, :]), rhat=rh, inv_mass=im,
                               n_draws=int(self.n_draws), n_chains=int(C))
        return out.to("cpu") if self._host else out
