"""GPU: visible-only Adam (csrc/adam_visible.hip) - lfs_adam_step_multi_visible, lfs_fastgs_view_visibility and GutTrainer(visible_adam=True).

No tolerance anywhere in the operator tests: a visible row must hold the bits of the dense kernel (ops.adam_step_wrapper, itself bit-exact against the oracle in
tests/test_gpu_small_ops.py), an invisible row the bits it had before the call. Gradient rows of invisible Gaussians are filled with NaN: a single load of one of
them that reaches a store shows up as a NaN.

Sizes: 1 (one lane), 31 / 33 (the word edge), 63 / 65 (the edge of a wave's block of 64 Gaussians), 257 (the workgroup edge), 5000 (several workgroups, a ragged last
block), 70 001 with 15 rest coefficients (the launch shares 2048 workgroups between the tensors: means gets 105 of them for 52 500 float4, so the flat path's
grid-stride loop takes a second trip) and 450 001 (7032 blocks of 64 rows against the 1563 workgroups x 4 waves of shN: the compaction path's second trip; a wave
covers 64 x 45 floats per trip, so no smaller model reaches it). Row widths: 1, 3, 4 (flat 16-byte path: a float4 covers four, one-and-a-bit, one Gaussian) and 45 / 72 (compaction path; R = 0: the tensor is skipped).
Bodies 1 - 3 also run on the emulated library (tests/test_emulated_adam_visible.py)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LRS = [1.6e-4, 2.5e-3, 1.25e-4, 5e-3, 1e-3, 5e-2]       # the six learning rates of test_adam_multi_equals_per_tensor
BC = (1 / (1 - 0.9 ** 5), 1 / math.sqrt(1 - 0.999 ** 5))
MASKS = ["all", "none", "first", "last", "alternating", "blocks64", "iid"]
NAMES = ["means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opacities"]


def _mask(kind, N):
    i = np.arange(N)
    if kind == "all":
        return np.ones(N, bool)
    if kind == "none":
        return np.zeros(N, bool)
    if kind == "first":
        return i == 0
    if kind == "last":
        return i == N - 1
    if kind == "alternating":
        return i % 2 == 1
    if kind == "blocks64":
        return (i // 64) % 2 == 0
    if kind == "iid":
        return np.random.default_rng(900 + N).random(N) < 0.1
    raise ValueError(kind)


def _pack(mask, extra_words=0):
    """bool [N] -> int32 device tensor of ceil(N / 32) (+ extra) words, bit i of word i // 32"""
    N = len(mask)
    words = (N + 31) // 32
    padded = np.zeros((words + extra_words) * 32, bool)
    padded[:N] = mask
    packed = np.packbits(padded.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)
    return torch.from_numpy(packed.view(np.int32).copy()).to(DEV)


def _unpack(bits, N):
    b = np.unpackbits(bits.detach().cpu().numpy().view(np.uint8), bitorder="little")
    return b[:N].astype(bool), b[N:]


def _shapes(N, R):
    return [(N, 3), (N, 1, 3), (N, R, 3), (N, 3), (N, 4), (N,)]


def _tensors(N, R, seed, offset=0):
    """four lists (param, exp_avg, exp_avg_sq, grad) of six tensors; with offset > 0 each is a view `offset` floats into a flat buffer, returned as well"""
    g = torch.Generator().manual_seed(seed)
    out, flats = [], []
    for scale, positive in ((1.0, False), (0.1, True), (0.01, True), (1.0, False)):
        row, frow = [], []
        for s in _shapes(N, R):
            numel = int(np.prod(s))
            flat = torch.randn(numel + offset, generator=g) * scale
            flat = (flat.abs() if positive else flat).to(DEV)
            frow.append(flat)
            row.append(flat[offset:].view(s))
        out.append(row)
        flats.append(frow)
    return out, flats


def _entries(p, m, v, g):
    return [(p[i], m[i], v[i], g[i], LRS[i], 0.9, 0.999, 1e-15, *BC) for i in range(6)]


def _check_case(N, R, kind, offset=0):
    from lichtfeld_studio_amd import ops
    (p, m, v, g), flats = _tensors(N, R, 31 * N + R, offset)
    mask_np = _mask(kind, N)
    mask = torch.from_numpy(mask_np).to(DEV)
    before = [[x.clone() for x in row] for row in (p, m, v)]
    flats_before = [[x.clone() for x in row] for row in flats[:3]]
    # the dense twin: the same tensors through the existing kernel, tensor by tensor, on clean gradients
    p2, m2, v2 = [[x.clone() for x in row] for row in (p, m, v)]
    for i in range(6):
        ops.adam_step_wrapper(p2[i], m2[i], v2[i], g[i].clone(), LRS[i], 0.9, 0.999, 1e-15, *BC)
    if kind == "all" and offset == 0:
        p3, m3, v3 = [[x.clone() for x in row] for row in (p, m, v)]
        ops.adam_step_multi(_entries(p3, m3, v3, g))
    for x in g:
        x[~mask] = float("nan")      # an invisible gradient row must not be read into anything that is stored
    ops.adam_step_multi_visible(_entries(p, m, v, g), _pack(mask_np), N)
    for got, twin, old in zip(p + m + v, p2 + m2 + v2, before[0] + before[1] + before[2]):
        assert torch.isfinite(got).all(), (N, R, kind, tuple(got.shape))
        assert torch.equal(got[mask], twin[mask]), (N, R, kind, tuple(got.shape))
        assert torch.equal(got[~mask], old[~mask]), (N, R, kind, tuple(got.shape))
    if kind == "all" and offset == 0:
        for got, multi in zip(p + m + v, p3 + m3 + v3):
            assert torch.equal(got, multi), (N, R, tuple(got.shape))
    if offset:
        for frow, brow in zip(flats[:3], flats_before):
            for f, b in zip(frow, brow):
                assert torch.equal(f[:offset], b[:offset])   # nothing before the view was touched
    if mask_np.any() and kind != "none":
        assert any(not torch.equal(a, b) for a, b in zip(p, before[0]))   # (the call did something)


# ---- 1. the operator, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [15, 24, 0])
@pytest.mark.parametrize("N", [1, 31, 33, 63, 65, 257, 5000])
def test_visible_rows_equal_the_dense_kernel_and_the_rest_is_untouched(lfs, N, R):
    for kind in MASKS:
        _check_case(N, R, kind)


def test_visible_rows_past_the_workgroup_cap(lfs):
    for kind in MASKS:
        _check_case(70001, 15, kind)


def test_wide_rows_past_the_workgroup_cap(lfs):
    for kind in ("blocks64", "iid"):
        _check_case(450001, 15, kind)


@pytest.mark.parametrize("offset", [1, 3])
def test_visible_rows_on_unaligned_views_take_the_scalar_path(lfs, offset):
    for kind in ("all", "blocks64", "iid", "last"):
        _check_case(257, 15, kind, offset=offset)


# ---- 2. the visibility bits ------------------------------------------------------------------------------------------
def _view_scene(N, seed, shift=0.0):
    """test_oracle_fastgs._scene with a third of the Gaussians out of sight: every third one behind the camera, every sixth far outside the frustum"""
    from test_oracle_fastgs import _scene
    sc = _scene(N=N, W=80, H=64, seed=seed, deg=1)
    sc["means"][2::3, 2] *= -1.0
    sc["means"][5::6, 0] += 60.0
    sc["w2c"][0, 3] += shift       # the second view: the camera moved sideways, another subset leaves the image
    R, tt = sc["w2c"][:3, :3], sc["w2c"][:3, 3]
    sc["cam_pos"] = -R.T @ tt
    return sc


def _visibility_of_view(lib, sc, bits, accumulate):
    """preprocess -> lfs_fastgs_view_visibility into `bits` -> render + backward with a zeroed densification_info -> its visibility count [N]"""
    from fastgs_raw import preprocess_raw, render_and_backward_raw, view_of
    from gpu_util import t
    from lichtfeld_studio_amd.capi import ptr, stream
    from lichtfeld_studio_amd.fastgs import FastGSSettings
    s = FastGSSettings(t(sc["cam_pos"]), sc["active_sh_bases"], sc["W"], sc["H"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], 0.01, 1e10)
    a = [t(sc[k]) for k in ("means", "scales_raw", "rot_raw", "opac_raw", "sh0", "sh_rest", "w2c")]
    rc, pws, n_dev = preprocess_raw(lib, a, s, 0)
    assert rc == 0
    assert lib.lfs_fastgs_view_visibility(C.byref(view_of(a, s, pws)), ptr(bits), C.c_int(accumulate), stream()) == 0
    rng = np.random.default_rng(3)
    gi, ga = t(rng.standard_normal((3, sc["H"], sc["W"]))), t(np.zeros((1, sc["H"], sc["W"])))
    dens = render_and_backward_raw(lib, a, s, pws, n_dev, gi, ga)[4]
    count = dens[0].detach().cpu().numpy()
    assert set(np.unique(count)) <= {0.0, 1.0}
    return count == 1.0


@pytest.mark.parametrize("N", [1, 33, 65, 1000])
def test_bits_are_the_backwards_visibility_count(lfs, N):
    lib = lfs.load_library()
    words = (N + 31) // 32
    assert int(lib.lfs_visibility_words(C.c_uint32(N))) == words
    bits = torch.full((words + 1,), -1, dtype=torch.int32, device=DEV)       # pre-filled with 0xFFFFFFFF; one guard word behind
    seen_a = _visibility_of_view(lib, _view_scene(N, 40 + N), bits, 0)
    got, tail = _unpack(bits[:words], N)
    assert np.array_equal(got, seen_a), (N, np.flatnonzero(got != seen_a)[:10])
    assert not tail.any()                                                      # accumulate == 0 overwrote the buffer: bits >= N are 0
    assert int(bits[words]) == -1                                              # ... and nothing behind the last word was written
    if N >= 33:
        assert seen_a.any() and not seen_a.all() and not seen_a[2::3].any()
    seen_b = _visibility_of_view(lib, _view_scene(N, 40 + N, shift=1.5), bits, 1)
    got, tail = _unpack(bits[:words], N)
    assert np.array_equal(got, seen_a | seen_b), N
    assert not tail.any() and int(bits[words]) == -1
    if N == 1000:
        assert (seen_a != seen_b).any()


# ---- 3. refusals -----------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_any_launch(lfs):
    from lichtfeld_studio_amd.capi import AdamTensor, FastgsView, ptr, stream
    lib = lfs.load_library()
    N = 8
    bufs = [torch.arange(24, dtype=torch.float32).to(DEV) + k for k in range(4)]
    keep = [b.clone() for b in bufs]
    bits = torch.full((1,), 0xFF, dtype=torch.int32, device=DEV)

    def tensor(n_elements, null=None):
        pts = [None if k == null else b.data_ptr() for k, b in enumerate(bufs)]
        return AdamTensor(pts[0], pts[1], pts[2], pts[3], n_elements, 1e-3, 0.9, 0.999, 1e-15, *BC)

    def call(tensors, bits_, n):
        arr = (AdamTensor * max(len(tensors), 1))(*tensors)
        return lib.lfs_adam_step_multi_visible(arr, C.c_int32(len(tensors)), ptr(bits_), C.c_uint32(n), stream())

    assert call([tensor(20)], bits, N) == -1                       # 20 % 8 != 0
    assert call([tensor(24), tensor(20)], bits, N) == -1           # ... in a later tensor: nothing of the first one is launched either
    assert call([tensor(24)], None, N) == -1                       # no bits
    for k in range(4):
        assert call([tensor(24, null=k)], bits, N) == -1           # a NULL tensor pointer
    assert call([tensor(24)] * 9, bits, N) == -1                   # more than LFS_ADAM_MAX_TENSORS
    assert lib.lfs_adam_step_multi_visible(None, C.c_int32(1), ptr(bits), C.c_uint32(N), stream()) == -1
    assert call([tensor(24)], bits, 0) == -1                       # rows of no Gaussian
    assert call([tensor(0), tensor(0)], None, 0) == 0              # N == 0 with an all-empty list
    assert call([tensor(0, null=0)], bits, N) == 0                 # an all-empty list
    assert call([], bits, N) == 0

    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    view = FastgsView()
    view.N, view.width, view.height, view.primitive_workspace, view.primitive_workspace_bytes = N, 16, 16, ws.data_ptr(), ws.numel()
    assert lib.lfs_fastgs_view_visibility(None, ptr(bits), 0, stream()) == -1
    assert lib.lfs_fastgs_view_visibility(C.byref(view), None, 0, stream()) == -1
    no_ws = FastgsView()
    no_ws.N, no_ws.width, no_ws.height = N, 16, 16
    assert lib.lfs_fastgs_view_visibility(C.byref(no_ws), ptr(bits), 0, stream()) == -1
    short = FastgsView()
    short.N, short.width, short.height, short.primitive_workspace, short.primitive_workspace_bytes = N, 16, 16, ws.data_ptr(), 64
    assert lib.lfs_fastgs_view_visibility(C.byref(short), ptr(bits), 0, stream()) == -3   # LFS_E_WORKSPACE
    empty = FastgsView()
    assert lib.lfs_fastgs_view_visibility(C.byref(empty), None, 0, stream()) == 0          # N == 0
    torch.cuda.synchronize()
    for b, k in zip(bufs, keep):
        assert torch.equal(b, k)
    assert int(bits[0]) == 0xFF


# ---- 4. the trainer --------------------------------------------------------------------------------------------------
N_SCENE, FAR = 600, 20


def _two_halves_scene(size=64):
    """SYN-A-sized Gaussians in two clusters 40 units apart, one camera in front of each: a view sees its own cluster and nothing of the other. The first FAR
    Gaussians sit between the two, far enough away for both cameras."""
    import dataclasses
    from lichtfeld_studio_amd import scenes
    sc = scenes.syn_a(n=N_SCENE, sh_degree=1)
    means = sc.means.clone()
    means[N_SCENE // 2:, 0] += 40.0
    means[:FAR, 0], means[:FAR, 2] = means[:FAR, 0] + 20.0, means[:FAR, 2] + 60.0
    viewmats = torch.eye(4).repeat(2, 1, 1)
    viewmats[1, 0, 3] = -40.0
    f = 60.0 * size / 64
    Ks = torch.tensor([[f, 0, size / 2], [0, f, size / 2], [0, 0, 1]]).repeat(2, 1, 1)
    return dataclasses.replace(sc, means=means, width=size, height=size, viewmats=viewmats, Ks=Ks)


def _targets(size=64):
    g = torch.Generator().manual_seed(5)
    return [(torch.rand(3, size, size, generator=g) * 0.7).to(DEV) for _ in range(2)]


def _trainer(strategy=None, **kw):
    from lichtfeld_studio_amd import strategies
    from lichtfeld_studio_amd.trainer import GutTrainer
    op = strategies.OptimizationParameters.for_strategy(strategy, iterations=3000) if strategy is not None else None
    tr = GutTrainer(_two_halves_scene(), torch.device(DEV), iterations=3000, rasterizer="fastgs", strategy=strategy, opt_params=op, **kw)
    tr.iteration = 1500        # Adam reads shN (iteration > 1000); far from any refinement or SH-degree step
    return tr


def _state(tr):
    out = []
    for p in tr.model.parameters():
        st = tr.optimizer.state[id(p)]
        out += [p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
    return out


def _seen(tr):
    got, tail = _unpack(tr._vis_bits, tr.model.means.shape[0])
    assert not tail.any()
    return torch.from_numpy(got).to(DEV)


def test_trainer_updates_only_the_rows_the_steps_views_saw(lfs):
    lib = lfs.load_library()
    targets = _targets()
    try:
        lib.lfs_set_debug_flags(16)          # deterministic accumulation: two trainers built alike take the same steps, bit for bit
        vis, dense = _trainer(visible_adam=True), _trainer()
        dense.inline_shN_adam = False        # the twin's shN goes through the separate optimizer as well (the fused form is held to it in tests/test_gpu_fastgs.py)
        for tr in (vis, dense):
            tr.train_step([targets[0]], views=[0])
        seen_a = _seen(vis)
        assert seen_a[FAR:N_SCENE // 2].any() and not seen_a[N_SCENE // 2:].any()
        after_1, dense_1 = _state(vis), _state(dense)
        for a, b in zip(after_1, dense_1):   # the moments start at zero: an invisible row (zero gradient) does not move in either trainer
            assert torch.equal(a, b)
        for tr in (vis, dense):
            tr.train_step([targets[1]], views=[1])
        seen_b = _seen(vis)
        assert seen_b[N_SCENE // 2:].any() and not seen_b[FAR:N_SCENE // 2].any()
        only_a, both = seen_a & ~seen_b, seen_a & seen_b
        assert only_a.any() and both.any()
        after_2, dense_2 = _state(vis), _state(dense)
        moved_in_dense = False
        for a2, a1, d2 in zip(after_2, after_1, dense_2):
            assert torch.equal(a2[only_a], a1[only_a])           # kept: parameters and moments of step 1
            moved_in_dense = moved_in_dense or not torch.equal(d2[only_a], a1[only_a])
            assert torch.equal(a2[both], d2[both])
            assert torch.equal(a2[seen_b], d2[seen_b])           # (the rows of view B were untouched before in both trainers: the same update)
        assert moved_in_dense                                   # the dense twin decays the moments and drifts along the stale momentum
    finally:
        lib.lfs_set_debug_flags(0)


def test_trainer_with_mcmc_leaves_unseen_rows_alone(lfs):
    lib = lfs.load_library()
    targets = _targets()
    try:
        lib.lfs_set_debug_flags(16)
        tr = _trainer(strategy="mcmc", visible_adam=True)
        assert not tr.strategy.is_refining(1501)
        before = [p.detach().clone() for p in tr.model.parameters()]
        tr.train_step([targets[0]], views=[0])
        seen = _seen(tr)
        assert seen.any() and not seen[N_SCENE // 2:].any() and not seen.all()
        for name, p, b in zip(NAMES, tr.model.parameters(), before):
            st = tr.optimizer.state[id(p)]
            if name != "means":      # (MCMC's noise is added to every mean by post_backward, outside the optimizer)
                assert torch.equal(p.detach()[~seen], b[~seen]), name
            assert not st["exp_avg"][~seen].any() and not st["exp_avg_sq"][~seen].any(), name   # the regularisers' gradients did not reach the unseen rows
            assert st["exp_avg"][seen].any(), name
        assert any(not torch.equal(p.detach()[seen], b[seen]) for p, b in zip(tr.model.parameters(), before))
    finally:
        lib.lfs_set_debug_flags(0)


def test_trainer_refuses_what_visible_adam_does_not_cover(lfs):
    from lichtfeld_studio_amd.trainer import GutTrainer
    sc, dev = _two_halves_scene(), torch.device(DEV)
    for kw, word in ((dict(rasterizer="gut"), "fastgs"), (dict(rasterizer="fastgs", world=2), "world"), (dict(rasterizer="fastgs", enable_sparsity=True), "sparsity"),
                     (dict(rasterizer="fastgs", one_call=True), "one_call"), (dict(rasterizer="fastgs", fused_adam=False), "fused_adam")):
        with pytest.raises(ValueError, match=word):
            GutTrainer(sc, dev, iterations=100, visible_adam=True, **kw)


def test_visible_adam_off_is_the_trainer_without_the_argument(lfs):
    """Bit for bit, loss_acc included: the image is 16 x 16, ONE workgroup of the loss kernel, whose float atomic on loss_acc then has one operand (at 64 x 64 the
    sixteen workgroups add in the order they finish, and two trainers built alike - with or without the argument - differ in the last bit of the loss)."""
    from lichtfeld_studio_amd.trainer import GutTrainer
    lib = lfs.load_library()
    targets = _targets(16)
    try:
        lib.lfs_set_debug_flags(16)
        trs = [GutTrainer(_two_halves_scene(16), torch.device(DEV), iterations=3000, rasterizer="fastgs", **kw) for kw in ({}, {"visible_adam": False})]
        losses = []
        for tr in trs:
            tr.iteration = 1500
            losses.append([tr.train_step([targets[k % 2]], views=[k % 2]).clone() for k in range(3)])
        assert trs[0].last_plan == trs[1].last_plan and trs[1]._vis_bits is None
        same_loss = [torch.equal(a, b) for a, b in zip(losses[0], losses[1])]
        same_param = [torch.equal(a.detach(), b.detach()) for a, b in zip(trs[0].model.parameters(), trs[1].model.parameters())]
        print("losses", [float(x) for x in losses[0]], [float(x) for x in losses[1]], same_loss, "parameters", same_param)
        assert all(float(x) > 0 for x in losses[0])
        assert all(same_loss) and all(same_param)
    finally:
        lib.lfs_set_debug_flags(0)


# ---- 5. a short run --------------------------------------------------------------------------------------------------
def test_short_run_trains(lfs):
    """150 steps alternating the two views: the loss of the visible-only trainer ends below its first. The dense twin's final loss is printed beside it; the gap is
    recorded in profiles/r17/visible_adam.json, not bounded here."""
    targets = _targets()
    vis, dense = _trainer(visible_adam=True), _trainer()
    first, last = {}, {}
    for name, tr in (("visible", vis), ("dense", dense)):
        for k in range(150):
            loss = float(tr.train_step([targets[k % 2]], views=[k % 2]))
            if k < 2:
                first[name, k] = loss
            if k >= 148:
                last[name, k % 2] = loss
    for v in (0, 1):
        print(f"view {v}: visible-only Adam loss {first['visible', v]:.6f} -> {last['visible', v]:.6f}; dense twin {first['dense', v]:.6f} -> {last['dense', v]:.6f}")
        assert math.isfinite(last["visible", v]) and last["visible", v] < first["visible", v]
