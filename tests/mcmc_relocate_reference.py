"""A plain numpy model of lfs_mcmc_relocate (the contract in include/lfs_gsplat.h: MCMC::relocate_gs of the reference without a host round trip), in fp64 and
independent of the kernels: no blocks, no scans, no search loop - a cumsum, a searchsorted and the relocation formula (Eq. 9 of "3D Gaussian Splatting as
Markov Chain Monte Carlo", as oracle/oracle_ops.hpp writes it). Shared by tests/test_gpu_mcmc_relocate.py and its emulated twin.

What is float32 here is what the contract makes float32: the opacity sigmoid(raw) that decides dead / alive and is the sampling weight (the same float32
numpy arithmetic as relocation_uniforms of tests/test_gpu_strategy_reference.py), |q|^2 against 1e-8, and the two clamp bounds."""
import math

import numpy as np

N_MAX = 51
MIN_OPACITY = 0.005
OPACITY_CAP = np.float32(1 - 1e-7)      # mcmc.cpp:155
PARAM_WIDTHS = (3, 3, None, 3, 4, 1)    # means, sh0, shN (free), raw_scales, raw_quats, raw_opacities


def binoms(n_max=N_MAX):
    b = np.zeros((n_max, n_max), np.float32)   # mcmc.cpp:459-472
    for a in range(n_max):
        for k in range(a + 1):
            b[a, k] = math.comb(a, k)
    return b


def sigmoid32(raw_o):
    raw_o = np.asarray(raw_o, np.float32)
    with np.errstate(over="ignore"):
        return (np.float32(1) / (np.float32(1) + np.exp(-raw_o))).astype(np.float32)


class Sampling:
    """dead mask, weights, CDF and - for given uniforms - the source of every dead row"""

    def __init__(self, raw_o, raw_q, min_opacity=MIN_OPACITY):
        self.o32 = sigmoid32(raw_o).reshape(-1)
        q = np.asarray(raw_q, np.float32)
        self.dead = (self.o32 <= np.float32(min_opacity)) | ((q * q).sum(-1) < np.float32(1e-8))
        self.N = len(self.o32)
        self.n_dead = int(self.dead.sum())
        self.w = np.where(self.dead, 0.0, self.o32.astype(np.float64))
        self.cdf = np.cumsum(self.w)
        self.total = float(self.cdf[-1]) if self.N else 0.0
        idx = np.arange(self.N)
        self.last_alive_at_or_before = np.maximum.accumulate(np.where(self.dead, -1, idx))                      # -1: none
        self.first_alive_at_or_after = np.minimum.accumulate(np.where(self.dead, self.N, idx)[::-1])[::-1]    # N: none

    def sources(self, u):
        """[N] int64: the first j with cdf[j] > u_i * total for dead i (a dead j - only a target at or above the total finds one - gives way to the last alive
        row before it); -1 for alive rows, and for every row when nothing is alive"""
        src = np.full(self.N, -1, np.int64)
        if self.total <= 0.0:
            return src
        j = np.minimum(np.searchsorted(self.cdf, np.asarray(u, np.float64) * self.total, side="right"), self.N - 1)
        back = self.last_alive_at_or_before[j]
        j = np.where(back >= 0, back, self.first_alive_at_or_after[j])
        src[self.dead] = j[self.dead]
        return src

    def margin(self, u):
        """[N] float64: the distance of every target u_i * total to the nearest CDF value (0, the start of the first cell, included). A source is
        unambiguous when the two sides' CDFs and targets cannot differ by as much."""
        t = np.asarray(u, np.float64) * self.total
        edges = np.concatenate([[0.0], self.cdf])
        k = np.searchsorted(edges, t, side="right")
        below = t - edges[np.maximum(k - 1, 0)]
        above = np.where(k <= self.N, edges[np.minimum(k, self.N)] - t, np.inf)
        return np.minimum(np.abs(below), np.abs(above))


def relocation(o, scales, n, b, n_max=N_MAX):
    """fp64: new opacity 1 - (1 - o)^(1/n) and scale * o / sum_{a=1..n} sum_{k<a} C(a-1,k) (-1)^k / sqrt(k+1) new_o^(k+1), for o [M], scales [M,3], n [M]"""
    o, scales, n = np.asarray(o, np.float64), np.asarray(scales, np.float64), np.asarray(n, np.int64)
    b = np.asarray(b, np.float64).reshape(n_max, n_max)
    new_o = 1.0 - np.power(1.0 - o, 1.0 / n)
    denom = np.zeros_like(o)
    for a in range(1, int(n.max()) + 1 if len(n) else 1):
        take = n >= a
        for k in range(a):
            denom[take] += b[a - 1, k] * (((-1.0) ** k / math.sqrt(k + 1)) * new_o[take] ** (k + 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        return new_o, scales * (o / denom)[:, None]


class Expected:
    """everything lfs_mcmc_relocate leaves behind, for params = the six tensors [N, width] (float32, order of PARAM_WIDTHS) and uniforms u [N]"""

    def __init__(self, params, u, b=None, n_max=N_MAX, min_opacity=MIN_OPACITY):
        b = binoms(n_max) if b is None else b
        self.sampling = s = Sampling(params[5], params[4], min_opacity)
        self.source = s.sources(u)
        self.counts = np.bincount(self.source[self.source >= 0], minlength=s.N).astype(np.int64)
        self.drawn = self.counts > 0                       # the rows whose Adam moments are zeroed
        self.n = np.minimum(self.counts + 1, n_max)
        j = np.nonzero(self.drawn)[0]
        self.new_opacity = np.full(s.N, np.nan)
        self.new_scale = np.full((s.N, 3), np.nan)
        raw_s = np.asarray(params[3], np.float64)
        no, ns = relocation(s.w[j], np.exp(raw_s[j]), self.n[j], b, n_max)
        self.new_opacity[j] = np.clip(no, float(np.float32(min_opacity)), float(OPACITY_CAP))
        self.new_scale[j] = ns
        self.params = [np.array(p, np.float64).reshape(s.N, -1) for p in params]
        with np.errstate(divide="ignore", invalid="ignore"):
            self.params[3][j] = np.log(ns)
            self.params[5][j, 0] = np.log(self.new_opacity[j] / (1.0 - self.new_opacity[j]))
        i = np.nonzero(self.source >= 0)[0]
        for p in self.params:                              # dead <- the (updated) row of its source
            p[i] = p[self.source[i]]
