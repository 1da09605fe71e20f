"""Bodies of the background-colour tests, shared by tests/test_emulated_background.py (the wavefront emulator, no GPU) and
tests/test_gpu_background.py. `dev` is "cuda:0" in both: the emulated run serves it with CPU tensors.

The kernel model is numpy float32, one rounding per operation in the order include/lfs_gsplat.h states; the kernels must repeat it bit for bit."""
import ctypes as C
import functools

import numpy as np

F = np.float32
# scalar only | tail only | full lanes + ragged end | vector exact | scalar, ragged | vector, exactly one block | scalar, more than one block | vector, more than one block
SIZES = [(1, 1), (1, 3), (3, 5), (2, 6), (7, 67), (16, 64), (33, 130), (32, 66)]
COLOURS = [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.3, 0.6, 0.9)]
GUARD = 8          # floats (bytes for the uint8 plane) of NaN (0xAB) before and after every buffer
U = 2.0 ** -24


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- the float32 model ---------------------------------------------------------------------------------------------------------------------------------------------------
def model_compose(image, alpha, bg):
    return np.stack([image[c] + (F(1.0) - alpha.reshape(image.shape[1:])) * F(bg[c]) for c in range(3)]).astype(F)


def model_target(t, u8, bg):
    a = u8.astype(F) / F(255.0)
    return np.stack([a * t[c] + (F(1.0) - a) * F(bg[c]) for c in range(3)]).astype(F)


def model_bwd(v, bg, v_in=None):
    d = (v[0] * F(bg[0]) + v[1] * F(bg[1])) + v[2] * F(bg[2])
    return (-d if v_in is None else v_in.reshape(d.shape) - d).astype(F)


@functools.lru_cache(maxsize=None)
def inputs(H, W, seed=0):
    """image (negative and > 1 values: the fastgs image is unclamped), alpha with exact 0 and exact 1, target, uint8 alpha with 0 and 255, upstream gradients"""
    rng = np.random.default_rng(1000 * H + W + seed)
    n = H * W
    image = (rng.random((3, H, W)) * 2.0 - 0.5).astype(F)
    alpha = rng.random((1, H, W)).astype(F)
    alpha.reshape(-1)[0::5] = 0.0
    alpha.reshape(-1)[2::5] = 1.0
    target = rng.random((3, H, W)).astype(F)
    u8 = rng.integers(0, 256, (H, W)).astype(np.uint8)
    u8.reshape(-1)[0::4] = 255
    u8.reshape(-1)[1::4] = 0
    if n == 1:
        u8.reshape(-1)[0] = 255 if seed % 2 == 0 else 0
    v = rng.standard_normal((3, H, W)).astype(F)
    v_in = rng.standard_normal((1, H, W)).astype(F)
    return image, alpha, target, u8, v, v_in


def _guarded(torch, dev, arr, misalign):
    """a device view of `arr` inside a guard-filled buffer; misalign: the view starts one element of 4 bytes past a 16-byte boundary -> (buffer, view, front)"""
    n = arr.size
    if arr.dtype == np.uint8:
        front = GUARD + (4 if misalign else 0)
        buf = torch.full((front + n + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    else:
        front = GUARD + (1 if misalign else 0)
        buf = torch.full((front + n + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    view = buf[front:front + n].view(arr.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    assert view.data_ptr() % 16 == (4 if misalign else 0) or arr.dtype == np.uint8
    return buf, view, front


def _intact(torch, buf, front, n):
    if buf.dtype == torch.uint8:
        return bool((buf[:front] == 0xAB).all()) and bool((buf[front + n:] == 0xAB).all())
    return bool(torch.isnan(buf[:front]).all()) and bool(torch.isnan(buf[front + n:]).all())


def _np(t):
    return t.detach().cpu().numpy().copy()


def check_kernels(dev, bg):
    """Both entries at every size, on 16-byte- and 4-byte-aligned buffers with guards: each group alone and both together, shown in and out of place, v_alpha aliased
    and not - against the float32 model bit for bit, against torch (forward bit for bit, backward within 4 u sum |bg_c v_c|), and the a == 0 / a == 255 identities."""
    import torch
    from lichtfeld_studio_amd import ops
    bg_t = torch.tensor(bg, dtype=torch.float32, device=dev)
    for (H, W) in SIZES:
        image, alpha, target, u8, v, v_in = inputs(H, W)
        n = H * W
        want_s, want_t = model_compose(image, alpha, bg), model_target(target, u8, bg)
        want_b0, want_b1 = model_bwd(v, bg), model_bwd(v, bg, v_in)
        # the identities of the target group
        assert np.array_equal(bits(want_t[:, u8 == 0]), bits(np.broadcast_to(np.array(bg, F)[:, None], (3, int((u8 == 0).sum())))))
        assert np.array_equal(bits(want_t[:, u8 == 255]), bits(target[:, u8 == 255]))
        # torch's own expressions (on the device under test)
        ti, ta = torch.from_numpy(image).to(dev), torch.from_numpy(alpha).to(dev).requires_grad_(True)
        t_shown = ti + (1.0 - ta) * bg_t.view(3, 1, 1)
        assert np.array_equal(bits(_np(t_shown)), bits(want_s)), (H, W, "torch forward vs model")
        (g_alpha,) = torch.autograd.grad(t_shown, ta, torch.from_numpy(v).to(dev))
        bound = 4 * U * sum(abs(float(bg[c])) * np.abs(v[c].astype(np.float64)) for c in range(3))
        assert (np.abs(want_b0.astype(np.float64) - _np(g_alpha)[0].astype(np.float64)) <= bound).all(), (H, W, "backward vs autograd")
        for misalign in (False, True):
            for render, tgt, inplace in ((True, False, False), (True, False, True), (False, True, False), (True, True, False), (True, True, True)):
                held = []
                b_img = _guarded(torch, dev, image, misalign); b_al = _guarded(torch, dev, alpha, misalign)
                b_t = _guarded(torch, dev, target, misalign); b_u8 = _guarded(torch, dev, u8, misalign)
                b_sh = b_img if inplace else _guarded(torch, dev, np.full_like(image, 7.0), misalign)
                b_to = _guarded(torch, dev, np.full_like(target, 7.0), misalign)
                held = [(b_img, 3 * n), (b_al, n), (b_t, 3 * n), (b_u8, n), (b_sh, 3 * n), (b_to, 3 * n)]
                shown, t_out = ops.background_compose(bg, b_img[1] if render else None, b_al[1] if render else None, b_sh[1] if render else None,
                                                      b_t[1] if tgt else None, b_u8[1] if tgt else None, b_to[1] if tgt else None)
                tag = (H, W, misalign, render, tgt, inplace)
                if render:
                    assert shown.data_ptr() == b_sh[1].data_ptr()
                    assert np.array_equal(bits(_np(shown)), bits(want_s)), tag
                    if not inplace:
                        assert np.array_equal(bits(_np(b_img[1])), bits(image)), tag
                else:
                    assert shown is None and bool((b_sh[1] == 7.0).all()), tag
                if tgt:
                    got = _np(t_out)
                    assert np.array_equal(bits(got), bits(want_t)), tag
                    assert np.array_equal(bits(_np(b_t[1])), bits(target)) and np.array_equal(_np(b_u8[1]), u8), tag
                else:
                    assert t_out is None and bool((b_to[1] == 7.0).all()), tag
                assert np.array_equal(bits(_np(b_al[1])), bits(alpha)), tag
                for (buf, _, front), size in held:
                    assert _intact(torch, buf, front, size), ("a guard element was written", tag)
            for with_in, aliased in ((False, False), (True, False), (True, True)):
                b_v = _guarded(torch, dev, v, misalign); b_in = _guarded(torch, dev, v_in, misalign)
                b_o = b_in if aliased else _guarded(torch, dev, np.full_like(v_in, 7.0), misalign)
                out = ops.background_compose_bwd(bg, b_v[1], b_in[1] if with_in else None, b_o[1])
                tag = (H, W, misalign, with_in, aliased)
                assert out.data_ptr() == b_o[1].data_ptr()
                assert np.array_equal(bits(_np(out)[0]), bits(want_b1 if with_in else want_b0)), tag
                assert np.array_equal(bits(_np(b_v[1])), bits(v)), tag
                if not aliased:
                    assert np.array_equal(bits(_np(b_in[1])), bits(v_in)), tag
                for (buf, _, front), size in ((b_v, 3 * n), (b_in, n), (b_o, n)):
                    assert _intact(torch, buf, front, size), ("a guard element was written", tag)
        # allocation by the wrapper, [H,W] alpha
        shown, t_out = ops.background_compose(bg, torch.from_numpy(image).to(dev), torch.from_numpy(alpha[0]).to(dev), None, torch.from_numpy(target).to(dev),
                                              torch.from_numpy(u8).to(dev))
        assert np.array_equal(bits(_np(shown)), bits(want_s)) and np.array_equal(bits(_np(t_out)), bits(want_t))


def check_wrapper_refusals(dev):
    import pytest
    import torch
    from lichtfeld_studio_amd import ops
    from lichtfeld_studio_amd.capi import LfsError
    image, alpha, target, u8, v, v_in = [torch.from_numpy(a).to(dev) for a in inputs(3, 5)]
    before = dict(ops.background_launches)
    with pytest.raises(LfsError):
        ops.background_compose((0.3, 0.6, 0.9))                                           # no group
    with pytest.raises(LfsError):
        ops.background_compose((0.3, 0.6, 0.9), image)                                    # half a group
    with pytest.raises(LfsError):
        ops.background_compose((0.3, 0.6, 0.9), target_rgb=target, target_alpha=u8, target_out=target)    # the alias
    with pytest.raises(LfsError):
        ops.background_compose((0.3, 0.6, 0.9), target_rgb=target, target_alpha=u8.float())               # not a uint8 plane
    with pytest.raises(LfsError):
        ops.background_compose((0.3, float("nan"), 0.9), image, alpha)
    with pytest.raises(LfsError):
        ops.background_compose((0.3, 0.6), image, alpha)
    with pytest.raises(LfsError):
        ops.background_compose_bwd((0.3, 0.6, 0.9), v, v_in[:, :2])
    assert ops.background_launches == before


def check_entry_refusals(lfs):
    """LFS_E_INVALID before any launch: the pointers are host memory no kernel could read, and a launch without a device would not come back as -1"""
    from lichtfeld_studio_amd.capi import BackgroundComposeArgs, BackgroundComposeBwdArgs
    lib = lfs.load_library()
    assert C.sizeof(BackgroundComposeArgs) == 72 and C.sizeof(BackgroundComposeBwdArgs) == 48
    buf = (C.c_float * 4096)()
    p = lambda k: C.c_void_p(C.addressof(buf) + 1024 * k)
    col = lambda *c: (C.c_float * 3)(*c)
    good = col(0.3, 0.6, 0.9)
    fwd = lambda *a: lib.lfs_background_compose(C.byref(BackgroundComposeArgs(*a)), None)
    bwd = lambda *a: lib.lfs_background_compose_bwd(C.byref(BackgroundComposeBwdArgs(*a)), None)
    assert lib.lfs_background_compose(None, None) == -1 and lib.lfs_background_compose_bwd(None, None) == -1       # NULL struct
    assert fwd(4, 4, good, None, None, None, None, None, None) == -1                                                 # both groups NULL
    for k in range(3):                                                                                                # half a group, either group
        part = [p(j) if j != k else None for j in range(3)]
        assert fwd(4, 4, good, *part, None, None, None) == -1 and fwd(4, 4, good, None, None, None, *part) == -1
        assert fwd(4, 4, good, *part, p(3), p(4), p(5)) == -1 and fwd(4, 4, good, p(0), p(1), p(2), *part) == -1
        only = [p(j) if j == k else None for j in range(3)]
        assert fwd(4, 4, good, *only, None, None, None) == -1 and fwd(4, 4, good, None, None, None, *only) == -1
    assert fwd(0, 4, good, p(0), p(1), p(2), None, None, None) == -1 and fwd(4, 0, good, p(0), p(1), p(2), None, None, None) == -1       # zero extent
    assert fwd(1 << 16, 1 << 15, good, p(0), p(1), p(2), None, None, None) == -1                                     # H * W == 2^31
    assert fwd(4, 4, good, None, None, None, p(0), p(1), p(0)) == -1                                                 # target_out == target_rgb
    assert fwd(4, 4, good, p(0), p(1), p(2), p(3), p(4), p(3)) == -1
    for bad in (col(float("nan"), 0, 0), col(0, float("inf"), 0), col(0, 0, float("-inf"))):                          # a non-finite colour
        assert fwd(4, 4, bad, p(0), p(1), p(2), None, None, None) == -1 and bwd(4, 4, bad, p(0), None, p(1)) == -1
    assert bwd(4, 4, good, None, None, p(1)) == -1 and bwd(4, 4, good, p(0), None, None) == -1 and bwd(4, 4, good, None, p(0), None) == -1
    assert bwd(0, 4, good, p(0), None, p(1)) == -1 and bwd(4, 0, good, p(0), None, p(1)) == -1 and bwd(1 << 16, 1 << 15, good, p(0), None, p(1)) == -1
    assert not any(buf)


# ---- the policy (host only) ------------------------------------------------------------------------------------------------------------------------------------------------
def check_policy_table():
    from lichtfeld_studio_amd import background as B
    table = [(10000, 1, (0.5845004, 0.8897756, 0.0352015)), (10000, 37, (0.5, 0.9980035, 0.4151752)), (30000, 7000, (0.9639446, 0.6986914, 0.6323472))]
    for iterations, it, want in table:
        got = B.background_for_step(it, iterations, (0.0, 0.0, 0.0), "modulated", jitter=False)
        assert all(isinstance(x, float) for x in got) and max(abs(a - b) for a, b in zip(got, want)) <= 1e-6, (iterations, it, got)
    for it, w in ((1, 1.0), (2500, 1.0), (3750, 0.75), (5000, 0.5), (6250, 0.25), (7500, 0.0)):
        assert abs(B.inv_weight_piecewise(it, 10000) - w) <= 1e-6, (it, B.inv_weight_piecewise(it, 10000))
    for it in (7501, 8000, 9999, 10000, 12000):
        assert B.inv_weight_piecewise(it, 10000) <= 0.0
        assert B.background_for_step(it, 10000, (0.2, 0.4, 0.6), "modulated", jitter=False) == (0.2, 0.4, 0.6)       # the base colour, no draw
    # the mix: (1 - w) base + w sine
    base = (1.0, 1.0, 1.0)
    s = B.sine_background(5000)
    got = B.background_for_step(5000, 10000, base, "modulated", jitter=False)
    assert max(abs(g - (0.5 + 0.5 * float(x))) for g, x in zip(got, s)) <= 1e-6
    assert B.background_for_step(3, 10, "white", "constant") == (1.0, 1.0, 1.0) and B.parse_background("black") == (0.0, 0.0, 0.0)
    import pytest
    for bad in ("grey", (0.1, 0.2), (0.1, 0.2, 1.5), (0.1, float("nan"), 0.2), (-0.1, 0.0, 0.0), 3):
        with pytest.raises(ValueError):
            B.parse_background(bad)
    with pytest.raises(ValueError):
        B.background_for_step(1, 10, mode="sometimes")


def check_policy_random_and_jitter():
    import torch
    from lichtfeld_studio_amd import background as B
    def seq(seed, mode, n=40, **kw):
        g = torch.Generator().manual_seed(seed)
        return [B.background_for_step(i + 1, 100, (0.0, 0.0, 0.0), mode, g, **kw) for i in range(n)]

    a, b, c = seq(7, "random"), seq(7, "random"), seq(8, "random")
    assert a == b and a != c
    assert all(x != y for x, y in zip(a, a[1:]))
    assert all(0.0 <= v < 1.0 for col in a for v in col)
    # the jitter: reproducible, within +-0.03 of the unjittered colour where the clamp is not met, inside the clamp everywhere
    j1, j2 = seq(3, "modulated", 70), seq(3, "modulated", 70)
    plain = seq(3, "modulated", 70, jitter=False)
    assert j1 == j2 and j1 != plain
    lo, hi = float(np.float32(1e-4)), float(np.float32(1) - np.float32(1e-4))
    for i, (cj, cp) in enumerate(zip(j1, plain)):
        w = B.inv_weight_piecewise(i + 1, 100)
        for vj, vp in zip(cj, cp):
            if w > 0:
                assert w * lo - 1e-7 <= vj <= w * hi + 1e-7 and abs(vj - vp) <= w * 0.03 + 1e-6, (i, vj, vp)
            else:
                assert vj == vp == 0.0
    with np.errstate(all="ignore"):
        for it in range(1, 200):
            for jit in (np.array([0.03, -0.03, 0.03], F), np.array([-0.03, 0.03, -0.03], F)):
                s = B.sine_background(it, jit)
                assert s.dtype == F and (s >= F(1e-4)).all() and (s <= F(1) - F(1e-4)).all()
    import pytest
    with pytest.raises(ValueError):
        B.background_for_step(1, 10, mode="random", generator=None)


def check_trainer_policy(dev):
    """GutTrainer's side of the policy, without a step: validation, the generator's seed, last_background"""
    import pytest
    from lichtfeld_studio_amd import scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    sc = scenes.syn_a(n=64, sh_degree=0)
    mk = lambda **kw: GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", **kw)
    for bad in ({"background": (0.1, 0.2, 1.5)}, {"background": "grey"}, {"background": (0.1, float("nan"), 0.2)}, {"background_mode": "sometimes"}):
        with pytest.raises(ValueError):
            mk(**bad)
    a, b, c = mk(background_mode="random", seed=5), mk(background_mode="random", seed=5), mk(background_mode="random", seed=6)
    sa, sb, sc_ = ([t.background_for_step(i + 1) for i in range(10)] for t in (a, b, c))
    assert sa == sb and sa != sc_ and all(x != y for x, y in zip(sa, sa[1:])) and all(0.0 <= v < 1.0 for col in sa for v in col)
    w = mk(background="white")
    assert w.background == (1.0, 1.0, 1.0) and w.background_for_step(3) == (1.0, 1.0, 1.0)
    m = mk(background_mode="modulated", background_jitter=False)
    assert max(abs(x - y) for x, y in zip(m.background_for_step(1), (0.5845004, 0.8897756, 0.0352015))) <= 1e-6     # w = 1 in the first quarter of any run
    from lichtfeld_studio_amd.background import sine_background
    assert max(abs(x - 0.7 * float(y)) for x, y in zip(m.background_for_step(40), sine_background(40))) <= 1e-6     # 40 of 100: w = 0.7, base black
    assert m.background_for_step(80) == (0.0, 0.0, 0.0)


# ---- the trainer on the fastgs route -----------------------------------------------------------------------------------------------------------------------------------------
BG = (0.3, 0.6, 0.9)
NAMES = ["means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opacities"]


def n64(t):
    return t.detach().cpu().double().numpy()


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def half_mask(dev, H, W):
    import torch
    from lichtfeld_studio_amd import losses
    m = torch.zeros(H, W, dtype=torch.uint8)
    m[:, :W // 2] = 255
    return losses.prepare_mask(m.to(dev), W, H)


def check_fastgs_step_matches_autograd(dev, loss, segment=False, n=4000, sh_degree=2):
    """One step of GutTrainer(rasterizer="fastgs", background=BG) against fast_rasterize(cam, model, bg) + the loss + autograd: |dloss| < 1e-6, rel_l2 < 1e-4 for each
    of the six groups (the bounds of test_fastgs_trainer_step_matches_autograd)."""
    import torch
    from lichtfeld_studio_amd import fastgs, losses, ops, scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(dev)
    sc = scenes.syn_a(n=n, sh_degree=sh_degree)
    w_a = 0.5
    kw = dict(mask_mode="segment", mask_alpha_weight=w_a) if segment else {}
    tr = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", background=BG, loss=loss, **kw)
    target = scenes.target_image(sc.height, sc.width).to(dev)
    ref = fastgs.fast_rasterize(tr.camera(0), tr.model, torch.tensor(BG, device=dev))
    mask = half_mask(dev, sc.height, sc.width) if segment else None
    if segment:
        m = mask.mask_u8.float()
        loss_ref = losses.masked_photometric_loss(ref.image, target, mask, tr.lambda_dssim) + w_a * ((255.0 - m) * ref.alpha.reshape(m.shape)).sum() / (255.0 * m.numel())
    elif loss == "l1_ssim":
        loss_ref = losses.photometric_loss(ref.image, target, tr.lambda_dssim)
    else:
        loss_ref = torch.nn.functional.mse_loss(ref.image, target)
    loss_ref.backward()
    ref_grads = [p.grad.clone() for p in tr.model.parameters()]
    for p in tr.model.parameters():
        p.grad = None
    before = dict(ops.background_launches)
    got = tr.train_step([target], views=[0], masks=[mask] if segment else None)
    assert tr.last_plan.path == "fastgs" and tr.last_background == BG
    assert ops.background_launches["compose"] == before["compose"] + 1 and ops.background_launches["compose_bwd"] == before["compose_bwd"] + 1
    print(f"loss {float(got):.8f} autograd {float(loss_ref):.8f}")
    assert abs(float(got) - float(loss_ref)) < 1e-6
    for name, g, r in zip(NAMES, tr.bucket.views, ref_grads):
        e = rel_l2(n64(g), n64(r).reshape(n64(g).shape))
        print(name, e)
        assert e < 1e-4, (name, e)
    # the colour matters: the black-background gradient of the opacities is another one
    tb = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", loss=loss, **kw)
    tb.train_step([target], views=[0], masks=[mask] if segment else None)
    assert rel_l2(n64(tb.bucket.views[5]), n64(ref_grads[5]).reshape(-1, *tb.bucket.views[5].shape[1:])) > 1e-2


def check_defaults_are_the_parents(lfs, dev, n=4000, sh_degree=2):
    """deterministic mode: GutTrainer(rasterizer="fastgs") and the same with background="black", background_mode="constant" - 3 steps, bit-identical parameters, and
    neither launched a compose entry"""
    import torch
    from lichtfeld_studio_amd import ops, scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    lib = lfs.load_library()
    sc = scenes.syn_a(n=n, sh_degree=sh_degree)
    target = scenes.target_image(sc.height, sc.width).to(dev)
    before = dict(ops.background_launches)
    lib.lfs_set_debug_flags(16)
    try:
        a = GutTrainer(sc, torch.device(dev), iterations=100, rasterizer="fastgs")
        b = GutTrainer(sc, torch.device(dev), iterations=100, rasterizer="fastgs", background="black", background_mode="constant")
        for _ in range(3):
            # (the loss scalar is a float-atomic sum over the loss kernel's blocks, outside debug bit 4: printed, the parameters are what is compared)
            la, lb = a.train_step([target], views=[0]), b.train_step([target], views=[0], alphas=[None])
            print(f"loss {float(la):.9f} / {float(lb):.9f}")
    finally:
        lib.lfs_set_debug_flags(0)
    for pa, pb in zip(a.model.parameters(), b.model.parameters()):
        assert torch.equal(pa.detach(), pb.detach())
    assert ops.background_launches == before
    assert a.last_background == (0.0, 0.0, 0.0) == b.last_background and a._step_bg is None and b._step_bg is None
    assert bool((a.bg == 0).all()) and bool((b.bg == 0).all())


def disc_alpha(H, W):
    """a uint8 plane: 255 inside a disc, 0 far outside, a soft ramp between"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    r = np.hypot(y - H / 2.0, x - W / 2.0) / (min(H, W) / 2.0)
    return np.clip(np.rint((0.8 - r) / 0.3 * 255.0), 0, 255).astype(np.uint8)


def alpha_of(plane):
    """u8.float() / 255 as a DIVISION. torch divides a device tensor by a Python scalar by multiplying with the scalar's reciprocal (its true-divide kernel for a host
    scalar), which is another float for many bytes; divided by a 0-dim device tensor it is the correctly rounded quotient - on the CPU both are."""
    import torch
    return plane.float() / torch.tensor(255.0, dtype=torch.float32, device=plane.device)


def check_rgba_step(dev, bg=BG, n=4000, sh_degree=2):
    """A fastgs step with alphas=[plane] against a step on the target composited in torch: the composited targets bit-identical, loss and gradients within the
    bounds of check_fastgs_step_matches_autograd. bg black: the render is not composited, the target still is."""
    import torch
    from lichtfeld_studio_amd import fastgs, ops, scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(dev)
    sc = scenes.syn_a(n=n, sh_degree=sh_degree)
    target = scenes.target_image(sc.height, sc.width).to(dev)
    plane = torch.from_numpy(disc_alpha(sc.height, sc.width)).to(dev)
    a = alpha_of(plane)
    composited = a * target + (1.0 - a) * torch.tensor(bg, device=dev).view(3, 1, 1)
    t1 = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", background=bg)
    t2 = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", background=bg)
    keep = target.clone()
    before = dict(ops.background_launches)
    l1 = t1.train_step([target], views=[0], alphas=[plane])
    assert ops.background_launches["compose"] == before["compose"] + 1                      # ONE launch composes the render and the target
    assert ops.background_launches["compose_bwd"] == before["compose_bwd"] + (0 if bg == (0.0, 0.0, 0.0) else 1)
    assert torch.equal(target, keep)                                                       # the resident image is left alone
    seen = fastgs.render_and_backward._target
    assert np.array_equal(bits(seen.cpu().numpy()), bits(composited.cpu().numpy()))
    l2 = t2.train_step([composited], views=[0])
    print(f"loss with alphas {float(l1):.8f}, on the torch composite {float(l2):.8f}")
    assert abs(float(l1) - float(l2)) < 1e-6
    for name, g, r in zip(NAMES, t1.bucket.views, t2.bucket.views):
        e = rel_l2(n64(g), n64(r))
        assert e < 1e-4, (name, e)
    # the plane is checked
    import pytest
    for bad in (plane[:-1], plane.float(), plane.cpu().numpy()):
        with pytest.raises(ValueError):
            t1.train_step([target], views=[0], alphas=[bad])
    with pytest.raises(ValueError):
        t1.train_step([target], views=[0], alphas=[plane, plane])


def check_preload_alphas(dev, tmp_path):
    """preload_alphas on an RGBA PNG and an RGB PNG written here: the RGBA view's plane is prepare_mask's (threshold -1) of the file's alpha, the RGB view's is None;
    evaluate(alphas=) composites the ground truth"""
    import torch
    from PIL import Image
    from lichtfeld_studio_amd import loader, losses
    H, W = 24, 36
    rng = np.random.default_rng(4)
    rgba = rng.integers(0, 256, (H, W, 4)).astype(np.uint8)
    rgba[..., 3] = disc_alpha(H, W)
    Image.fromarray(rgba, "RGBA").save(str(tmp_path / "a.png"))
    Image.fromarray(rgba[..., :3].copy(), "RGB").save(str(tmp_path / "b.png"))
    assert loader.get_image_info(str(tmp_path / "a.png"))[2] == 4 and loader.get_image_info(str(tmp_path / "b.png"))[2] == 3
    cams = []
    for name in ("a.png", "b.png"):
        cams.append(loader.CameraData(0, 1, 0, W, H, 30.0, 30.0, W / 2.0, H / 2.0, np.eye(3, dtype=np.float32), np.zeros(3, np.float32), np.zeros(0, np.float32),
                                      np.zeros(0, np.float32), np.zeros(4, np.float32), name, str(tmp_path / name)))
    for factor, size in ((-1, (H, W)), (2, (H // 2, W // 2))):
        ds = loader.CameraDataset(cams, "all", resize_factor=factor, masks_folder=None)
        planes = loader.preload_alphas(ds, dev)
        assert len(planes) == 2 and planes[1] is None
        assert planes[0].dtype == torch.uint8 and tuple(planes[0].shape) == size
        want = losses.prepare_mask(torch.from_numpy(np.ascontiguousarray(rgba[..., 3])).to(dev), size[1], size[0], False, -1).mask_u8
        assert torch.equal(planes[0], want)
        if factor == -1:
            assert np.array_equal(planes[0].cpu().numpy(), rgba[..., 3])
        images = loader.preload(ds, dev, workers=1)
        assert tuple(images[0].shape) == (3, *size)


# ---- the 3DGUT route ---------------------------------------------------------------------------------------------------------------------------------------------------------
def check_gut_route(dev, one_call=False, background=BG, mode="constant"):
    """One-view scene, GutTrainer(rasterizer="gut", background=BG) in the default fused form (one_call: the one-call form) against its autograd twin (fused_l2=False) -
    the scene, the step count and the tolerances of the black-background comparison of the two forms (tests/test_gpu_fused.py:
    test_fused_and_autograd_trainers_take_the_same_steps). The colour matters: the black twin's first loss is another number."""
    import torch
    from lichtfeld_studio_amd import scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    sc = scenes.syn_a(n=3000, sh_degree=1)
    a = GutTrainer(sc, dev, iterations=200, fused_l2=True, one_call=one_call, background=background, background_mode=mode, seed=3)
    b = GutTrainer(sc, dev, iterations=200, fused_l2=False, background=background, background_mode=mode, seed=3)
    target = torch.rand(3, sc.height, sc.width, generator=torch.Generator().manual_seed(1)).to(dev) * 0.5
    first = None
    for _ in range(5):
        la, lb = float(a.train_step([target], views=[0])), float(b.train_step([target], views=[0]))
        first = la if first is None else first
        assert a.last_background == b.last_background and (mode != "constant" or a.last_background == background)
        assert a.last_plan.path == ("cxx_all" if one_call else "cxx_views") and b.last_plan.path == "autograd"
        print(f"fused {la:.8f} autograd {lb:.8f} |d| {abs(la - lb):.3e} bar {1e-4 * max(1.0, abs(lb)):.3e}")
        assert abs(la - lb) < 1e-4 * max(1.0, abs(lb))
    assert tuple(float(v) for v in a.bg.cpu()) == tuple(float(np.float32(v)) for v in a.last_background)
    for pa, pb in zip(a.model.parameters(), b.model.parameters()):
        assert float((pa - pb).abs().max()) < 5e-3 and rel_l2(n64(pa), n64(pb)) < 1e-4
    black = GutTrainer(sc, dev, iterations=200, fused_l2=True, one_call=one_call)
    assert abs(float(black.train_step([target], views=[0])) - first) > 1e-4
    assert bool((black.bg == 0).all())


def check_gut_route_rgba(dev):
    """alphas on a route other than fastgs: the target is composited by a target-only launch before the step form sees it - the step equals the one on the torch composite"""
    import torch
    from lichtfeld_studio_amd import ops, scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    sc = scenes.syn_a(n=3000, sh_degree=1)
    target = torch.rand(3, sc.height, sc.width, generator=torch.Generator().manual_seed(1)).to(dev) * 0.5
    plane = torch.from_numpy(disc_alpha(sc.height, sc.width)).to(dev)
    al = alpha_of(plane)
    composited = al * target + (1.0 - al) * torch.tensor(BG, device=dev).view(3, 1, 1)
    a = GutTrainer(sc, dev, iterations=200, background=BG)
    b = GutTrainer(sc, dev, iterations=200, background=BG)
    before = dict(ops.background_launches)
    la, lb = float(a.train_step([target], views=[0], alphas=[plane])), float(b.train_step([composited], views=[0]))
    assert ops.background_launches["compose"] == before["compose"] + 1 and ops.background_launches["compose_bwd"] == before["compose_bwd"]
    assert abs(la - lb) < 1e-4 * max(1.0, abs(lb))
