"""GPU: lfs_mcmc_relocate (csrc/mcmc.hip: block sums -> scan of the block sums -> CDF -> inverse-CDF sample -> values -> apply) against the exact host model
of tests/mcmc_relocate_reference.py, through the C ABI with plain tensors, at the sizes where a prefix-sum / inverse-CDF pipeline goes wrong: more than 256
blocks (the carry of the block scan), ragged tails (N % 4 != 0, a last block of one element), targets at 0, just below the total and exactly on a CDF value,
one source drawn 130 times, rows dead by their quaternion, nothing alive, NULL moments, a zero-width shN and the argument checks.

Every row is tagged: means[j] = (j, 0, 0) (exact in fp32 up to 2^24) and all Adam moments are non-zero, so after the call means[i, 0] IS the source of a dead row
i and a zeroed moment row IS a drawn source - the workspace is never read."""
import ctypes as C

import numpy as np
import pytest
import torch

import mcmc_relocate_reference as R
from gpu_util import n, t

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# 262 145 and 524 293: two and three passes of the block scan, each with a one-element last block. At 262 145 the second pass holds that one block, whose only
# cdf value the search never reads (mid < N - 1): the pass is seen through the total alone. 263 171 = 257 * 1024 + 3 puts two blocks into it, the first one full.
EXACT_SIZES = [1, 3, 1023, 1025, 4099, 262145, 263171, 524293]
U_TOP = np.nextafter(1.0, 0.0)


# ---- inputs and the call ---------------------------------------------------------------------------------------------------------------------------------
def make_rows(raw_o, raw_q, seed, shn_width=6):
    """-> (params, exp_avg, exp_avg_sq): six float32 [N, width] arrays each, rows tagged by means[:, 0], no zero among the moments"""
    rng = np.random.default_rng(seed)
    N = len(raw_o)
    means = np.zeros((N, 3), np.float32)
    means[:, 0] = np.arange(N)
    params = [means, rng.standard_normal((N, 3), np.float32), rng.standard_normal((N, shn_width), np.float32),
              (np.log(0.02) + 0.5 * rng.standard_normal((N, 3))).astype(np.float32), np.asarray(raw_q, np.float32).reshape(N, 4),
              np.asarray(raw_o, np.float32).reshape(N, 1)]
    exp_avg = [(((np.arange(p.size) % 7) + 1) * np.float32(0.125)).astype(np.float32).reshape(p.shape) for p in params]
    exp_avg_sq = [(((np.arange(p.size) % 5) + 1) * np.float32(0.25)).astype(np.float32).reshape(p.shape) for p in params]
    return params, exp_avg, exp_avg_sq


class Result:
    pass


def relocate(params, exp_avg, exp_avg_sq, u, *, n_max=R.N_MAX, min_opacity=R.MIN_OPACITY, want_n_dead=True, N=None, widths=None, binoms="default",
             workspace_short_by=0):
    """one lfs_mcmc_relocate on device copies of the arrays -> Result(rc, params, exp_avg, exp_avg_sq, n_dead) read back (moments None when not given)"""
    from lichtfeld_studio_amd import capi
    lib = capi.load_library()
    rows_N = len(params[0])
    N = rows_N if N is None else N
    dp = [t(p) for p in params]
    da = [None] * 6 if exp_avg is None else [t(p) for p in exp_avg]
    ds = [None] * 6 if exp_avg_sq is None else [t(p) for p in exp_avg_sq]
    du = None if u is None else t(np.asarray(u, np.float64), torch.float64)
    db = t(R.binoms(n_max if n_max > 0 else R.N_MAX)) if isinstance(binoms, str) else binoms
    dn = torch.full((1,), -7, dtype=torch.int32, device=DEV) if want_n_dead else None
    rows = (capi.ParamRows * 6)()
    for k in range(6):
        width = params[k].shape[1] if widths is None else widths[k]
        nonempty = dp[k].numel() > 0
        rows[k].param = dp[k].data_ptr() if nonempty else None
        rows[k].exp_avg = da[k].data_ptr() if da[k] is not None and nonempty else None
        rows[k].exp_avg_sq = ds[k].data_ptr() if ds[k] is not None and nonempty else None
        rows[k].width = width
    need = int(lib.lfs_mcmc_relocate_workspace_bytes(C.c_uint32(rows_N)))
    ws = capi.workspace(need, DEV, "test_mcmc_relocate")
    r = Result()
    r.rc = int(lib.lfs_mcmc_relocate(C.c_uint32(N), rows, capi.ptr(du), capi.ptr(db), C.c_int32(n_max), C.c_float(min_opacity), capi.ptr(dn),
                                     capi.ptr(ws), C.c_size_t(need - workspace_short_by), capi.stream()))
    torch.cuda.synchronize()
    r.params = [n(p) for p in dp]
    r.exp_avg = None if exp_avg is None else [n(p) for p in da]
    r.exp_avg_sq = None if exp_avg_sq is None else [n(p) for p in ds]
    r.n_dead = int(dn[0]) if want_n_dead else None
    return r


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def assert_nothing_changed(res, params, exp_avg, exp_avg_sq):
    for k in range(6):
        assert same_bits(res.params[k], params[k]), k
        if res.exp_avg is not None:
            assert same_bits(res.exp_avg[k], exp_avg[k]) and same_bits(res.exp_avg_sq[k], exp_avg_sq[k]), k


def check_structure(res, params, exp_avg, exp_avg_sq, exp):
    """what holds bit for bit whatever the values are: sources, n_dead, dead row = the updated row of its source, untouched rows, which moments are zero"""
    s = exp.sampling
    dead_idx = np.nonzero(s.dead)[0]
    got_src = res.params[0][dead_idx, 0].astype(np.int64)
    assert np.array_equal(got_src, exp.source[dead_idx]), (dead_idx[got_src != exp.source[dead_idx]][:8], got_src[got_src != exp.source[dead_idx]][:8])
    assert not s.dead[got_src].any()
    if res.n_dead is not None:
        assert res.n_dead == s.n_dead
    untouched = ~s.dead & ~exp.drawn
    for k in range(6):
        assert same_bits(res.params[k][dead_idx], res.params[k][got_src]), k           # (the source's row AFTER its own update)
        assert same_bits(res.params[k][untouched], params[k][untouched]), k
        if k not in (3, 5):                                                              # a drawn source changes in scale and opacity only
            assert same_bits(res.params[k][exp.drawn], params[k][exp.drawn]), k
        if res.exp_avg is not None:
            for got, before in ((res.exp_avg[k], exp_avg[k]), (res.exp_avg_sq[k], exp_avg_sq[k])):
                assert not bits(got[exp.drawn]).any(), k                                  # +0.0 on exactly the drawn sources
                assert same_bits(got[~exp.drawn], before[~exp.drawn]), k                 # dead rows keep their own moments (the reference does not touch them)


def check_values(res, exp, opacity_bar=(2e-5, 1e-7), scale_rtol=2e-3, max_n=12):
    """relocated opacity and scale of the drawn sources with n = count + 1 <= 12 (above that the alternating binomial sum cancels in fp32, in the reference as
    well: tests/test_gpu_small_ops.py) against the fp64 model, at the project's bars for the relocation kernel"""
    j = np.nonzero(exp.drawn & (exp.n <= max_n))[0]
    got_o = 1.0 / (1.0 + np.exp(-res.params[5][j, 0].astype(np.float64)))
    got_s = np.exp(res.params[3][j].astype(np.float64))
    print(f"relocated values of {len(j)} sources: opacity worst {np.abs(got_o - exp.new_opacity[j]).max():.3e} abs, "
          f"scale worst {np.abs(got_s / exp.new_scale[j] - 1).max():.3e} rel")
    np.testing.assert_allclose(got_o, exp.new_opacity[j], rtol=opacity_bar[0], atol=opacity_bar[1])
    np.testing.assert_allclose(got_s, exp.new_scale[j], rtol=scale_rtol)
    return len(j)


# ---- 1. exact tier -----------------------------------------------------------------------------------------------------------------------------------------
def exact_inputs(N):
    """raw opacities 0 (sigmoid = 0.5 exactly), 20 (1.0 exactly: 1 + expf(-20) rounds to 1) and -8 (dead), a few rows dead by quaternion: every weight is 0, 0.5
    or 1, every partial sum exact in fp64 in ANY order, so the source of every dead row is exact for any u. -> (raw_o, raw_q, u, placed) with placed = the rows
    whose u was put on an edge: {row: expected source}"""
    rng = np.random.default_rng(1000 + N)
    raw_q = rng.standard_normal((N, 4)).astype(np.float32)
    u = rng.random(N)
    if N == 1:                                  # one alive row: nothing to do
        return np.array([0.0], np.float32), raw_q, u, {}
    if N == 3:                                  # dead (u = 0), alive, dead (u just below 1)
        u[0], u[2] = 0.0, U_TOP
        return np.array([-8.0, 0.0, -8.0], np.float32), raw_q, u, {0: 1, 2: 1}
    m = int(np.floor(np.log2(0.6 * N)))         # total weight 2^m: u = cdf[j] / total and u * total are exact
    ones, halves = int(0.6 * 2 ** m), 2 * (2 ** m - int(0.6 * 2 ** m))
    inner = N - 6                               # rows 0..2 and N-3..N-1 are dead
    assert ones + halves + 3 + 64 < inner
    mid = np.full(inner, -8.0, np.float32)
    mid[:ones], mid[ones:ones + halves] = 20.0, 0.0
    mid = mid[rng.permutation(inner)]
    raw_o = np.concatenate([np.full(3, -8.0, np.float32), mid, np.full(3, -8.0, np.float32)])
    qdead = rng.choice(np.nonzero(raw_o == -8.0)[0][3:-3], 3, replace=False)    # dead by quaternion, opacity 1.0
    raw_o[qdead], raw_q[qdead] = 20.0, 1e-5
    s = R.Sampling(raw_o, raw_q)
    assert s.total == 2.0 ** m and s.dead[qdead].all()
    alive = np.nonzero(~s.dead)[0]
    u[0], u[N - 1] = 0.0, U_TOP
    placed = {0: int(alive[0]), N - 1: int(alive[-1])}
    # targets exactly ON a CDF value: the strict > must pick the NEXT alive row. Half of the j are followed by a dead row, some are dead rows themselves
    before_dead = alive[:-1][np.diff(alive) > 1]
    js = np.concatenate([rng.choice(before_dead, 32, replace=False), rng.choice(alive[:-1], 24, replace=False), rng.choice(np.nonzero(s.dead)[0][3:-3], 8, replace=False)])
    hosts = rng.choice(np.nonzero(s.dead)[0][3:-3], 64, replace=False)
    for i, j in zip(hosts, js):
        u[i] = s.cdf[j] / s.total
        assert u[i] * s.total == s.cdf[j]
        placed[int(i)] = int(s.first_alive_at_or_after[j + 1])
    return raw_o, raw_q, u, placed


def exact_tier(N):
    raw_o, raw_q, u, placed = exact_inputs(N)
    params, exp_avg, exp_avg_sq = make_rows(raw_o, raw_q, seed=N)
    exp = R.Expected(params, u)
    s = exp.sampling
    halves = np.where(s.dead, 0, np.where(raw_o == 20.0, 2, 1))
    assert np.array_equal(s.cdf * 2, np.cumsum(halves).astype(np.float64))            # the model's CDF is the integer count of halves: exact
    for i, j in placed.items():
        assert exp.source[i] == j, (i, j, exp.source[i])
    if N > 3:
        assert s.margin(u)[list(placed)[2:]].max() == 0.0                              # (those targets sit ON a CDF value)
        assert int((s.dead & (raw_o == 20.0)).sum()) == 3 and s.n_dead > N // 10             # three rows dead by quaternion alone
    res = relocate(params, exp_avg, exp_avg_sq, u)
    assert res.rc == 0
    check_structure(res, params, exp_avg, exp_avg_sq, exp)
    if s.n_dead:
        assert check_values(res, exp) > 0
    else:
        assert_nothing_changed(res, params, exp_avg, exp_avg_sq)
    again = relocate(params, exp_avg, exp_avg_sq, u)                                   # fresh copies of the inputs: identical bits
    for k in range(6):
        assert same_bits(again.params[k], res.params[k]) and same_bits(again.exp_avg[k], res.exp_avg[k]) and same_bits(again.exp_avg_sq[k], res.exp_avg_sq[k]), k
    assert again.n_dead == res.n_dead


@pytest.mark.parametrize("N", EXACT_SIZES)
def test_exact_weights_give_the_models_sources_bit_for_bit(lfs, N):
    exact_tier(N)


# ---- 2. general weights ------------------------------------------------------------------------------------------------------------------------------------
def general_inputs(N, seed):
    """raw opacities random in [-6, 6], a tenth forced dead (by opacity or by quaternion); every u is built from the model as (cdf[s-1] + f w_s) / total for a
    source s drawn in proportion to its weight, f from {0.02, 0.5, 0.98} (0.5 for a source too light for the margin below at the outer two)"""
    rng = np.random.default_rng(seed)
    raw_o = rng.uniform(-6.0, 6.0, N).astype(np.float32)
    raw_q = rng.standard_normal((N, 4)).astype(np.float32)
    forced = rng.random(N) < 0.1
    by_q = forced & (rng.random(N) < 0.3)
    raw_o[forced & ~by_q] = -8.0
    raw_q[by_q] = 1e-5
    s = R.Sampling(raw_o, raw_q)
    # the two sides' weights may differ by a few ulp each (device expf against the float32 numpy sigmoid; weights < 1: ulp <= 2^-24), so the two CDFs differ by
    # at most n_alive 2^-22 - and so do the two totals, hence the targets u * total: a source is certain when the target is further than TWICE that from the
    # nearest CDF value of the model. (The fp64 sums themselves are exact on both sides: fp32 weights above 2^-8, total < 2^22.)
    bound = (N - s.n_dead) * 2.0 ** -22
    dead_idx, alive_idx = np.nonzero(s.dead)[0], np.nonzero(~s.dead)[0]
    src = rng.choice(alive_idx, len(dead_idx), p=s.w[alive_idx] / s.w[alive_idx].sum())
    f = rng.choice([0.02, 0.5, 0.98], len(dead_idx))
    f[0.02 * s.w[src] <= 4 * bound] = 0.5
    u = rng.random(N)
    u[dead_idx] = (s.cdf[src] - s.w[src] + f * s.w[src]) / s.total
    assert np.abs(s.o32 - np.float32(R.MIN_OPACITY)).min() > 1e-7                       # no row whose dead / alive could depend on the last bit of expf
    assert s.margin(u)[dead_idx].min() > 2 * bound, (s.margin(u)[dead_idx].min(), bound)
    assert np.array_equal(s.sources(u)[dead_idx], src)
    assert len(set(f)) == 3 and np.bincount(src).max() >= 2
    return raw_o, raw_q, u


def general_tier(N, oracle_mod):
    raw_o, raw_q, u = general_inputs(N, seed=N)
    params, exp_avg, exp_avg_sq = make_rows(raw_o, raw_q, seed=N, shn_width=9)
    b = R.binoms()
    exp = R.Expected(params, u, b)
    # the bars of check_values are the project's bars for the relocation kernel; before they are used, the fp32 oracle (the reference's arithmetic) has to meet
    # them against the fp64 model on these inputs
    j = np.nonzero(exp.drawn & (exp.n <= 12))[0]
    assert len(j) > 50 and exp.n[j].max() >= 3
    oo, os_ = oracle_mod.relocation(exp.sampling.o32[j], np.exp(params[3][j]), exp.n[j].astype(np.int32), b, R.N_MAX)
    oo = np.clip(oo, np.float32(R.MIN_OPACITY), R.OPACITY_CAP)
    print(f"fp32 oracle against the fp64 model: opacity worst {np.abs(oo - exp.new_opacity[j]).max():.3e} abs, scale worst {np.abs(os_ / exp.new_scale[j] - 1).max():.3e} rel")
    np.testing.assert_allclose(oo, exp.new_opacity[j], rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(os_, exp.new_scale[j], rtol=2e-3)
    res = relocate(params, exp_avg, exp_avg_sq, u)
    assert res.rc == 0
    check_structure(res, params, exp_avg, exp_avg_sq, exp)
    assert check_values(res, exp) == len(j)
    k = np.nonzero(exp.drawn)[0]                                                         # every drawn source: finite raw opacity inside the clamp
    assert np.isfinite(res.params[5][k]).all()


@pytest.mark.parametrize("N", [1027, 2051])
def test_general_weights_sources_exact_and_values_within_the_relocation_bars(lfs, oracle_mod, N):
    general_tier(N, oracle_mod)


# ---- 3. block-boundary probe -------------------------------------------------------------------------------------------------------------------------------
def test_targets_on_block_boundaries_never_draw_a_dead_source(lfs):
    """The block sums (thread-sequential + tree) and the CDF (Hillis-Steele) add the same weights in different orders; were their fp64 results to differ in the
    last bit, cdf would step across the dead first row of a block and a target in that window would find the dead row. Every block of 1024 starts with a dead
    row here and one dead row per block aims at cdf[1024 b - 1]. The model cannot say which neighbour wins, so this asserts the property: the source is alive
    and is the last alive row before the boundary or the first after it.
    (Found: no dead source - and none is possible at this size: fp32 weights above 2^-8 and a total below 2^22 make every fp64 partial sum exact in any
    order. Above 2^22 the sums do round; relocate_sample_kernel decides aliveness from the weight for that reason.)"""
    N = 262145
    rng = np.random.default_rng(3)
    w = rng.uniform(0.006, 0.999, N)
    raw_o = np.log(w / (1 - w)).astype(np.float32)
    raw_q = rng.standard_normal((N, 4)).astype(np.float32)
    heads = np.arange(0, N, 1024)
    raw_o[heads] = -8.0
    extra = rng.choice(np.setdiff1d(np.arange(N), heads), 2000, replace=False)         # other dead rows, random u
    raw_o[extra] = -8.0
    s = R.Sampling(raw_o, raw_q)
    assert len(heads) == 257 and s.dead[heads].all()
    u = rng.random(N)
    u[heads] = np.concatenate([[0.0], s.cdf[heads[1:] - 1]]) / s.total
    params, exp_avg, exp_avg_sq = make_rows(raw_o, raw_q, seed=3)
    res = relocate(params, exp_avg, exp_avg_sq, u)
    assert res.rc == 0 and res.n_dead == s.n_dead
    dead_idx = np.nonzero(s.dead)[0]
    src = res.params[0][dead_idx, 0].astype(np.int64)
    assert not s.dead[src].any()
    got = res.params[0][heads, 0].astype(np.int64)
    before = np.where(heads > 0, s.last_alive_at_or_before[np.maximum(heads - 1, 0)], -1)
    after = s.first_alive_at_or_after[heads]
    ok = (got == before) | ((got == after) & (after < N))
    assert ok.all(), (heads[~ok], got[~ok])
    print(f"boundary targets: {int((got == before).sum())} took the row before, {int((got == after).sum())} the row after")
    for k in range(6):                                                                  # and the dead rows are copies of those sources
        assert same_bits(res.params[k][dead_idx], res.params[k][src]), k


# ---- 4. count clamp ----------------------------------------------------------------------------------------------------------------------------------------
def test_a_source_drawn_130_times_is_relocated_with_n_max(lfs):
    N, alive = 131, 65
    raw_o = np.full(N, -8.0, np.float32)
    raw_o[alive] = 0.0
    rng = np.random.default_rng(4)
    raw_q = rng.standard_normal((N, 4)).astype(np.float32)
    u = rng.random(N)
    u[0], u[N - 1] = 0.0, U_TOP
    params, exp_avg, exp_avg_sq = make_rows(raw_o, raw_q, seed=4)
    exp = R.Expected(params, u)
    assert exp.counts[alive] == 130 and exp.n[alive] == 51
    res = relocate(params, exp_avg, exp_avg_sq, u)
    assert res.rc == 0 and res.n_dead == 130
    check_structure(res, params, exp_avg, exp_avg_sq, exp)
    assert (res.params[0][:, 0] == alive).all()                                         # every dead row became a copy of the alive one
    got_o = 1.0 / (1.0 + np.exp(-float(res.params[5][alive, 0])))
    np.testing.assert_allclose(got_o, 1.0 - 0.5 ** (1.0 / 51.0), rtol=2e-5)             # n = n_max = 51; n = 131 would give 0.0053 < 0.0135
    np.testing.assert_allclose(got_o, exp.new_opacity[alive], rtol=2e-5)
    assert np.isfinite(res.params[3][alive]).all()


# ---- 5. nothing alive --------------------------------------------------------------------------------------------------------------------------------------
def test_nothing_alive_changes_nothing(lfs):
    raw_o = np.array([-8.0, 20.0, -8.0, 0.0, -30.0], np.float32)
    raw_q = np.random.default_rng(5).standard_normal((5, 4)).astype(np.float32)
    raw_q[[1, 3]] = 1e-5                                                                # the two opaque rows are dead by their quaternion
    params, exp_avg, exp_avg_sq = make_rows(raw_o, raw_q, seed=5)
    assert R.Sampling(raw_o, raw_q).n_dead == 5
    res = relocate(params, exp_avg, exp_avg_sq, np.array([0.0, 0.3, 0.5, 0.9, U_TOP]))
    assert res.rc == 0 and res.n_dead == 5
    assert_nothing_changed(res, params, exp_avg, exp_avg_sq)


# ---- 6. optional pointers ----------------------------------------------------------------------------------------------------------------------------------
def test_optional_pointers_do_not_change_the_result(lfs):
    N = 1029
    raw_o, raw_q, u = general_inputs(N, seed=6)
    params, exp_avg, exp_avg_sq = make_rows(raw_o, raw_q, seed=6, shn_width=9)
    full = relocate(params, exp_avg, exp_avg_sq, u)
    assert full.rc == 0 and full.n_dead > 50
    bare = relocate(params, None, None, u)                                               # no Adam moments at all
    no_count = relocate(params, exp_avg, exp_avg_sq, u, want_n_dead=False)
    assert bare.rc == 0 and no_count.rc == 0 and bare.n_dead == full.n_dead
    for k in range(6):
        assert same_bits(bare.params[k], full.params[k]), k
        assert same_bits(no_count.params[k], full.params[k]) and same_bits(no_count.exp_avg[k], full.exp_avg[k]) and same_bits(no_count.exp_avg_sq[k], full.exp_avg_sq[k]), k
    cut = lambda rows: [p if k != 2 else np.zeros((N, 0), np.float32) for k, p in enumerate(rows)]   # shN of width 0 behind a NULL pointer
    res = relocate(cut(params), cut(exp_avg), cut(exp_avg_sq), u)
    assert res.rc == 0 and res.n_dead == full.n_dead
    for k in (0, 1, 3, 4, 5):
        assert same_bits(res.params[k], full.params[k]) and same_bits(res.exp_avg[k], full.exp_avg[k]) and same_bits(res.exp_avg_sq[k], full.exp_avg_sq[k]), k


# ---- 7. argument checks ------------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(lfs):
    N = 9
    raw_o = np.array([-8.0, 0.0, 20.0] * 3, np.float32)
    raw_q = np.random.default_rng(7).standard_normal((N, 4)).astype(np.float32)
    params, exp_avg, exp_avg_sq = make_rows(raw_o, raw_q, seed=7)
    u = np.full(N, 0.5)
    cases = {
        "N = 2^24 + 1": (dict(N=(1 << 24) + 1), -1),
        "n_max = 0": (dict(n_max=0), -1),
        "means of width 4": (dict(widths=[4, 3, 6, 3, 4, 1]), -1),
        "raw_opacities of width 2": (dict(widths=[3, 3, 6, 3, 4, 2]), -1),
        "NULL binoms": (dict(binoms=None), -1),
        "a workspace one byte short": (dict(workspace_short_by=1), -3),
        "N = 0": (dict(N=0), 0),
    }
    for name, (kw, rc) in cases.items():
        res = relocate(params, exp_avg, exp_avg_sq, u, **kw)
        assert res.rc == rc, (name, res.rc)
        assert res.n_dead == -7, name                                                    # not even the count was cleared
        assert_nothing_changed(res, params, exp_avg, exp_avg_sq)
    res = relocate(params, exp_avg, exp_avg_sq, None)
    assert res.rc == -1 and res.n_dead == -7
    assert_nothing_changed(res, params, exp_avg, exp_avg_sq)
    assert relocate(params, exp_avg, exp_avg_sq, u).rc == 0                             # and the same arrays are accepted as they are
