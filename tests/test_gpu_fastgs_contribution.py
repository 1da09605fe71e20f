"""GPU: the contribution statistic of the fastgs rasterizer (csrc/fastgs_contrib.hip, lfs_fastgs_view_contribution) and contribution.compute_contribution.

The independent check is the TWIN RENDER, which uses nothing but the existing, verified render: the same geometry with SH degree 0, the Gaussian under test given a
colour c~ ~ 1 in one channel and every other Gaussian sh0 = -10 (the colour clamps to exactly 0). That channel of the twin's image is then the per-pixel map c w of the
Gaussian, from which its pixel count (exactly), its maximum weight and its weight sum follow. Bounds (all from the number formats, none from the code under test):
  max:  2^-22 max_w                      one rounding of c (the SH evaluation: three float operations, 2.75 x 2^-24 in all) and one of the product c w
  sum:  2^-17 sum_w + n_pix 2^-24        any order of summing 64 non-negative floats (63 roundings of 2^-24) + the twin's 2^-22; one fixed-point rounding (2^-25) per
                                         wavefront, counted as 2^-24 per PIXEL (more than one per wavefront)
  view: sum_i sum_w_i against sum_p alpha_p: 2^-17 sum_p alpha_p + n_pairs 2^-22 (three roundings of 2^-24 on values <= 1 per blended instance, plus the above)
Scenes (tests/test_oracle_fastgs._scene): N = 1 at 50 x 35 (no size a multiple of 8: partial cells, lanes outside the image), N = 65 at 64 x 48, N = 257 at 96 x 80 (a fifth
of it behind the camera), and a deep stack at 48 x 40 - 300 Gaussians of opacity 0.3 centred on one pixel (a cell list longer than the walker's staging groups; the centre
pixels terminate inside it) with six small ones behind them. The N = 65 scene also runs antialiased with a 3D filter tensor. Everything a scene needs - the statistic, the
render, the twin renders - is computed once per scene and shared. The same bodies run on the emulated library (tests/test_emulated_fastgs_contribution.py); GPU and emulator
are not compared with each other (v_exp_f32 differs)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SH_C0 = 0.28209479177387814
N_STACK, N_BEHIND = 300, 6
SENTINEL = 0x5A5A5A5A


# ---- scenes ----------------------------------------------------------------------------------------------------------
def _stack_scene():
    """300 Gaussians (scale 0.2, opacity 0.3) centred on pixel (23, 15) of a 48 x 40 image at depths 4 .. 4.3, in index order; behind them (depth 6) six small ones
    (scale 0.02, opacity 0.9) whose 1/255 extent (2 px) stays inside the disc (7 px) in which every pixel terminates inside the stack: 0.3 exp(-r^2 / 2 sigma^2) > 0.0302,
    i.e. (1 - alpha)^300 < 1e-4, holds for r < 2.14 sigma = 2.14 x 3.5 px."""
    W, H, fx, fy, cx, cy = 48, 40, 70.0, 70.0, 24.0, 20.0
    N = N_STACK + N_BEHIND
    z = np.concatenate([4.0 + 0.001 * np.arange(N_STACK), 6.0 + 0.01 * np.arange(N_BEHIND)])
    px, py = 23.5, 15.5
    means = np.stack([(px - cx) / fx * z, (py - cy) / fy * z, z], 1)
    scales = np.concatenate([np.full(N_STACK, 0.2), np.full(N_BEHIND, 0.02)])
    opac = np.concatenate([np.full(N_STACK, 0.3), np.full(N_BEHIND, 0.9)])
    rng = np.random.default_rng(5)
    rot = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (N, 1))
    return dict(means=means, scales_raw=np.log(np.repeat(scales[:, None], 3, 1)), rot_raw=rot, opac_raw=np.log(opac / (1 - opac)), sh0=rng.standard_normal((N, 1, 3)) * 0.5,
                sh_rest=np.zeros((N, 15, 3)), w2c=np.eye(4), cam_pos=np.zeros(3), active_sh_bases=1, W=W, H=H, fx=fx, fy=fy, cx=cx, cy=cy)


def _named_scene(name):
    from test_oracle_fastgs import _scene
    if name == "stack":
        return _stack_scene()
    if name == "n1":      # one large Gaussian near the lower right corner of 50 x 35: it covers partial cells on both borders
        sc = _scene(N=1, W=50, H=35, seed=11, deg=1)
        sc["means"][0] = [0.9, 0.55, 4.0]
        sc["scales_raw"][0] = np.log(0.25)
        sc["opac_raw"][0] = 2.0
        return sc
    if name in ("n65", "n65_aa_f3d"):
        return _scene(N=65, W=64, H=48, seed=12, deg=1)
    if name == "n257":
        sc = _scene(N=257, W=96, H=80, seed=13, deg=1)
        sc["means"][4::5, 2] *= -1.0          # every fifth one behind the camera
        return sc
    raise ValueError(name)


SCENES = ["n1", "n65", "n257", "stack", "n65_aa_f3d"]


def _settings(sc, name, active_sh_bases=None):
    from gpu_util import t
    from lichtfeld_studio_amd.fastgs import FastGSSettings
    N = sc["means"].shape[0]
    special = name.endswith("_aa_f3d")
    f3d = t(0.002 * (1.0 + (np.arange(N) % 3))) if special else None
    return FastGSSettings(t(sc["cam_pos"]), sc["active_sh_bases"] if active_sh_bases is None else active_sh_bases, sc["W"], sc["H"], sc["fx"], sc["fy"], sc["cx"], sc["cy"],
                          0.01, 1e10, antialiased=special, filter3d=f3d)


def _tensors(sc):
    from gpu_util import t
    return [t(sc[k]) for k in ("means", "scales_raw", "rot_raw", "opac_raw", "sh0", "sh_rest", "w2c")]


def _forward_and_add(a, s, stats):
    """the forward of the view (fastgs._forward: preprocess + render through the C ABI), then lfs_fastgs_view_contribution ADDS into stats -> (image, alpha, pws, iws, n_instances)"""
    from lichtfeld_studio_amd import fastgs, ops
    image, alpha, pws, iws, n_inst = fastgs._forward(*a, s, False)
    ops.fastgs_view_contribution(pws, iws, n_inst, a[0].shape[0], s.width, s.height, stats)
    return image, alpha, pws, iws, n_inst


def _backend():
    from lichtfeld_studio_amd import ops
    return ops.load_library().lfs_version().decode()


def _unpack(stats):
    from lichtfeld_studio_amd.contribution import unpack_stats
    m, c, s = unpack_stats(stats)
    return m.cpu().numpy(), c.cpu().numpy(), s.cpu().numpy()


def _chosen(name, N):
    if name == "stack":   # the first of the stack, the ones around the instance that terminates the centre pixel (0.7^26 < 1e-4: index 25), the last ones, the six behind
        return sorted(set([0, 1, 2] + list(range(20, 32)) + [150, 298, 299] + list(range(N_STACK, N_STACK + N_BEHIND))))
    return sorted(set(np.linspace(0, N - 1, min(N, 24)).round().astype(int).tolist()))


@functools.lru_cache(maxsize=None)
def _case_cached(name, backend):
    sc = _named_scene(name)
    a, s = _tensors(sc), _settings(sc, name)
    N = a[0].shape[0]
    stats = torch.zeros((N, 4), dtype=torch.int32, device=DEV)
    image, alpha, pws, iws, n_inst = _forward_and_add(a, s, stats)
    # the twin renders: SH degree 0, three Gaussians under test per render (one per channel), sh0 = -10 for all the others
    s0 = _settings(sc, name, active_sh_bases=1)
    chosen = _chosen(name, N)
    bright = np.float32(0.5 / SH_C0)
    c_tilde = SH_C0 * float(bright) + 0.5
    twin = {}
    for k in range(0, len(chosen), 3):
        group = chosen[k:k + 3]
        sh0 = torch.full((N, 1, 3), -10.0, device=DEV)
        for ch, g in enumerate(group):
            sh0[g, 0, ch] = float(bright)
        b = list(a)
        b[4] = sh0
        from lichtfeld_studio_amd import fastgs
        img = fastgs._forward(*b, s0, False)[0].cpu().numpy().astype(np.float64)
        for ch, g in enumerate(group):
            twin[g] = img[ch]
            for other in range(len(group), 3):
                assert not img[other].any()      # (a channel nobody was given stays black: sh0 = -10 clamps to exactly 0)
    return dict(sc=sc, a=a, s=s, N=N, stats=stats, image=image, alpha=alpha, pws=pws, iws=iws, n_inst=n_inst, twin=twin, c_tilde=c_tilde)


def _case(name):
    return _case_cached(name, _backend())


# ---- 1. the twin render ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_statistic_equals_the_per_pixel_weight_map_of_the_twin_render(lfs, name):
    c = _case(name)
    max_w, n_pix, sum_fixed = _unpack(c["stats"])
    sum_w = sum_fixed.astype(np.float64) * 2.0 ** -24
    seen = 0
    for g, ch in c["twin"].items():
        wmap = ch / c["c_tilde"]
        n_ref, max_ref, sum_ref = int((ch > 0).sum()), float(wmap.max()), float(wmap.sum())
        print(f"{name} gaussian {g}: n_pix {n_pix[g]} / {n_ref}, max_w {max_w[g]:.9g} / {max_ref:.9g} (rel {abs(max_w[g] - max_ref) / max(max_ref, 1e-30):.2e}), "
              f"sum_w {sum_w[g]:.9g} / {sum_ref:.9g} (diff {abs(sum_w[g] - sum_ref):.2e}, bound {2.0 ** -17 * sum_w[g] + n_pix[g] * 2.0 ** -24:.2e})")
        assert n_pix[g] == n_ref, (name, g, n_pix[g], n_ref)
        assert abs(float(max_w[g]) - max_ref) <= 2.0 ** -22 * float(max_w[g]), (name, g, max_w[g], max_ref)
        assert abs(sum_w[g] - sum_ref) <= 2.0 ** -17 * sum_w[g] + n_pix[g] * 2.0 ** -24, (name, g, sum_w[g], sum_ref)
        seen += n_ref > 0
    assert seen >= min(c["N"], 12), (name, seen)      # (the check looked at Gaussians that are in the image)


# ---- 2. the view identity --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_weights_of_a_view_sum_to_its_alpha_map(lfs, name):
    c = _case(name)
    _, n_pix, sum_fixed = _unpack(c["stats"])
    total = float(sum_fixed.astype(np.float64).sum() * 2.0 ** -24)
    alpha_sum = float(c["alpha"].cpu().numpy().astype(np.float64).sum())
    bound = 2.0 ** -17 * alpha_sum + float(n_pix.sum()) * 2.0 ** -22
    print(f"{name}: sum_i sum_w {total:.9g}, sum_p alpha {alpha_sum:.9g}, diff {abs(total - alpha_sum):.3e}, bound {bound:.3e}, pairs {int(n_pix.sum())}")
    assert alpha_sum > 0
    assert abs(total - alpha_sum) <= bound


# ---- 3. range and reach ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_weights_stay_below_the_alpha_clamp(lfs, name):
    max_w, n_pix, sum_fixed = _unpack(_case(name)["stats"])
    assert (max_w <= np.float32(0.999)).all() and (max_w >= 0).all()
    assert ((n_pix == 0) == (max_w == 0)).all() and ((n_pix == 0) == (sum_fixed == 0)).all()


def test_gaussians_behind_the_point_of_termination_have_an_empty_row(lfs):
    from lichtfeld_studio_amd import ops
    c = _case("stack")
    N = c["N"]
    bits = torch.zeros((N + 31) // 32, dtype=torch.int32, device=DEV)
    ops.fastgs_view_visibility(c["pws"], N, c["s"].width, c["s"].height, bits)
    touched = np.unpackbits(bits.cpu().numpy().view(np.uint8), bitorder="little")[:N].astype(bool)
    assert touched[N_STACK:].all()                     # the preprocess projected the six onto tiles ...
    rows = c["stats"].cpu().numpy()
    assert not rows[N_STACK:].any()                    # ... and no pixel blends them: all of theirs terminated inside the stack
    max_w, n_pix, _ = _unpack(c["stats"])
    assert (n_pix[:N_STACK] > 0).all()                 # every Gaussian of the stack is blended somewhere (the outer pixels never terminate)
    assert n_pix[0] > n_pix[30] > 0                    # ... the later ones into fewer pixels: index 25 terminates the centre pixel
    assert float(max_w[0]) == pytest.approx(0.3, rel=1e-3)


def test_gaussians_outside_the_frustum_have_an_empty_row(lfs):
    c = _case("n257")
    rows = c["stats"].cpu().numpy()
    assert not rows[4::5].any()
    assert rows[:, 1].astype(np.int64).sum() > 0


# ---- 4. determinism --------------------------------------------------------------------------------------------------
def _second_view(sc):
    sc2 = dict(sc)
    sc2["w2c"] = sc["w2c"].copy()
    sc2["w2c"][0, 3] += 0.4
    R, tt = sc2["w2c"][:3, :3], sc2["w2c"][:3, 3]
    sc2["cam_pos"] = -R.T @ tt
    return sc2


@pytest.mark.parametrize("name", ["n65", "stack"])
def test_rows_are_bit_reproducible_and_independent_of_the_order_of_views(lfs, name):
    c = _case(name)
    N = c["N"]
    again = torch.zeros((N, 4), dtype=torch.int32, device=DEV)
    _forward_and_add(c["a"], c["s"], again)
    assert torch.equal(again, c["stats"])              # two calls on fresh buffers: the same bits
    _forward_and_add(c["a"], c["s"], again)            # a second accumulating call: count and fixed-point sum double exactly, the maximum stays
    one, two = c["stats"].cpu().numpy(), again.cpu().numpy()
    assert np.array_equal(two[:, 0], one[:, 0])
    assert np.array_equal(two[:, 1].astype(np.int64), 2 * one[:, 1].astype(np.int64))
    assert np.array_equal(two.view(np.int64)[:, 1], 2 * one.view(np.int64)[:, 1])
    views = [(c["a"], c["s"])]
    sc2 = _second_view(c["sc"])
    views.append((_tensors(sc2), _settings(sc2, name)))
    ab, ba = torch.zeros((N, 4), dtype=torch.int32, device=DEV), torch.zeros((N, 4), dtype=torch.int32, device=DEV)
    for k in (0, 1):
        _forward_and_add(*views[k], ab)
    for k in (1, 0):
        _forward_and_add(*views[k], ba)
    assert torch.equal(ab, ba)
    assert not torch.equal(ab, again)                  # (the second view is another view)


# ---- 5. the entry ----------------------------------------------------------------------------------------------------
def test_entry_refuses_before_any_launch_and_leaves_the_rows_untouched(lfs):
    from fastgs_raw import view_of
    from lichtfeld_studio_amd.capi import FastgsView, ptr, stream
    lib = lfs.load_library()
    c = _case("n65")
    a, s, pws, iws, n_inst, N = c["a"], c["s"], c["pws"], c["iws"], c["n_inst"], c["N"]
    assert n_inst > 0
    stats = torch.full((N, 4), SENTINEL, dtype=torch.int32, device=DEV)

    def call(view, n, iws_ptr, iws_bytes, st):
        return lib.lfs_fastgs_view_contribution(view, C.c_int64(n), iws_ptr, C.c_size_t(iws_bytes), st, stream())

    good = view_of(a, s, pws)
    assert call(C.byref(good), n_inst, ptr(iws), iws.numel(), None) == -1              # stats == NULL
    assert call(None, n_inst, ptr(iws), iws.numel(), ptr(stats)) == -1                  # view == NULL
    no_ws = view_of(a, s, pws)
    no_ws.primitive_workspace = None
    assert call(C.byref(no_ws), n_inst, ptr(iws), iws.numel(), ptr(stats)) == -1        # no primitive workspace
    need = lib.lfs_fastgs_instance_workspace_bytes(C.c_uint32(s.width), C.c_uint32(s.height), C.c_int64(n_inst))
    assert call(C.byref(good), n_inst, ptr(iws), need - 1, ptr(stats)) == -3            # instance workspace one byte short: LFS_E_WORKSPACE
    assert call(C.byref(good), n_inst, None, need, ptr(stats)) == -3
    short = view_of(a, s, pws)
    short.primitive_workspace_bytes = 64
    assert call(C.byref(short), n_inst, ptr(iws), iws.numel(), ptr(stats)) == -3
    assert call(C.byref(good), 0, ptr(iws), iws.numel(), ptr(stats)) == 0               # n_instances == 0: LFS_OK, nothing launched
    empty = FastgsView()
    empty.width, empty.height, empty.primitive_workspace, empty.primitive_workspace_bytes = s.width, s.height, pws.data_ptr(), pws.numel()
    assert call(C.byref(empty), 0, ptr(iws), iws.numel(), ptr(stats)) == 0              # N == 0
    torch.cuda.synchronize()
    assert bool((stats == SENTINEL).all())
    assert call(C.byref(good), n_inst, ptr(iws), iws.numel(), ptr(stats)) == 0          # (and the accepted call does write)
    torch.cuda.synchronize()
    assert not bool((stats == SENTINEL).all())


def test_a_camera_that_looks_away_has_no_instances_and_changes_nothing(lfs):
    sc = dict(_named_scene("n65"))
    sc["w2c"] = np.diag([-1.0, 1.0, -1.0, 1.0])      # turned by 180 degrees about y: every Gaussian is behind it
    sc["cam_pos"] = np.zeros(3)
    a, s = _tensors(sc), _settings(sc, "n65")
    stats = torch.full((65, 4), SENTINEL, dtype=torch.int32, device=DEV)
    image, alpha, _, _, n_inst = _forward_and_add(a, s, stats)
    assert n_inst == 0 and not bool(alpha.any())
    assert bool((stats == SENTINEL).all())


def test_the_call_leaves_image_and_alpha_of_the_render_as_they_were(lfs):
    from lichtfeld_studio_amd import fastgs
    c = _case("n257")
    image, alpha = fastgs._forward(*c["a"], c["s"], False)[:2]
    assert torch.equal(image, c["image"]) and torch.equal(alpha, c["alpha"])


# ---- 6. compute_contribution -----------------------------------------------------------------------------------------
def _model_and_cameras(sc_views):
    from gpu_util import t
    from lichtfeld_studio_amd.rasterizer import Camera, SplatModel
    sc = sc_views[0]
    model = SplatModel(t(sc["means"]), t(sc["sh0"]), t(sc["sh_rest"]), t(sc["scales_raw"]), t(sc["rot_raw"]), t(sc["opac_raw"]), 3, active_sh_degree=1)
    cams = []
    for v in sc_views:
        K = np.array([[v["fx"], 0, v["cx"]], [0, v["fy"], v["cy"]], [0, 0, 1.0]])
        cams.append(Camera(t(v["w2c"]).reshape(1, 4, 4), t(K).reshape(1, 3, 3), v["W"], v["H"]))
    return model, cams


def test_compute_contribution_folds_without_changing_a_bit(lfs, monkeypatch):
    from lichtfeld_studio_amd import contribution
    c = _case("n65")
    sc = c["sc"]
    views = [sc, _second_view(sc), sc]
    model, cams = _model_and_cameras(views)
    assert contribution.fold_interval(1920, 1080) == (2 ** 32 - 1) // (1920 * 1080) == 2071 and contribution.fold_interval(1 << 17, 1 << 17) == 1
    whole = contribution.compute_contribution(model, cams)
    monkeypatch.setattr(contribution, "FOLD_VIEWS", 1)
    folded = contribution.compute_contribution(model, cams)
    assert whole.views == folded.views == 3
    assert whole.max_w.dtype == torch.float32 and whole.sum_w.dtype == torch.float64 and whole.n_pix.dtype == torch.int64
    for x, y in zip(whole[:3], folded[:3]):
        assert torch.equal(x, y)
    # ... and it is the kernel's statistic of the three views: view 0 twice and the second view once, added into one buffer by hand
    buf = torch.zeros((65, 4), dtype=torch.int32, device=DEV)
    for v in views:
        _forward_and_add(_tensors(v), _settings(v, "n65"), buf)
    m, n, f = _unpack(buf)
    assert np.array_equal(whole.max_w.cpu().numpy(), m) and np.array_equal(whole.n_pix.cpu().numpy(), n)
    assert np.array_equal(whole.sum_w.cpu().numpy(), f.astype(np.float64) * 2.0 ** -24)
    # the modes reach the kernel: antialiased + filter3d give another statistic, the one of the special scene's single view
    sp = _case("n65_aa_f3d")
    one = contribution.compute_contribution(model, cams[:1], antialiased=True, filter3d=sp["s"].filter3d)
    m1, n1, f1 = _unpack(sp["stats"])
    assert np.array_equal(one.max_w.cpu().numpy(), m1) and np.array_equal(one.n_pix.cpu().numpy(), n1)
    assert not np.array_equal(m1, _unpack(c["stats"])[0])
