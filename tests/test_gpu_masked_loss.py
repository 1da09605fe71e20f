"""GPU parity of the masked losses (lfs_photometric_loss_masked_fwd_bwd, lfs_mse_loss_masked_fwd_bwd) and of lfs_mask_prepare against the float64 model of
tests/masked_loss_reference.py (the formulas of DESIGN.md §8 "Masked training"; there is no reference implementation of masks to compare with).
Bounds: the project's own for the unmasked loss (tests/test_gpu_loss.py) - loss 2e-6 absolute, gradient 1e-5 of the tensor's max.
The same bodies run on the wavefront emulator in tests/test_emulated_masked_loss.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import masked_loss_reference as mref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WEIGHT = 0.5
LOSS0 = 0.25   # the accumulator's value before the call: the entry ADDS to it

SHAPES = [(64, 64), (37, 53), (117, 203), (9, 40), (11, 11)]
MASKS = ["soft", "blob", "border", "full", "empty"]
LAMBDAS = [0.2, 0.0, 1.0]


def _mask(kind, H, W, seed=0):
    """uint8 [H,W] numpy"""
    rng = np.random.RandomState(1000 + seed)
    if kind == "soft":
        return rng.randint(0, 256, size=(H, W)).astype(np.uint8)
    if kind == "blob":
        m = np.zeros((H, W), np.uint8)
        m[H // 4:(3 * H) // 4 + 1, W // 5:(2 * W) // 3 + 1] = 255
        return m
    if kind == "border":   # nonzero only on the 5-pixel border: S_crop == 0 and S_img > 0 wherever the image can be cropped
        m = rng.randint(1, 256, size=(H, W)).astype(np.uint8)
        m[5:H - 5, 5:W - 5] = 0
        return m
    if kind == "full":
        return np.full((H, W), 255, np.uint8)
    assert kind == "empty"
    return np.zeros((H, W), np.uint8)


def _prepared(m_np):
    """PreparedMask from numpy, the sums by numpy's integer arithmetic and the crop rule written out here (independent of lfs_mask_prepare)"""
    from lichtfeld_studio_amd import losses
    H, W = m_np.shape
    mc = m_np[5:H - 5, 5:W - 5] if (H > 10 and W > 10) else m_np
    sums = torch.tensor([int(m_np.astype(np.int64).sum()), int(mc.astype(np.int64).sum())], dtype=torch.int64)
    return losses.PreparedMask(torch.from_numpy(m_np.copy()).to(DEV), sums.to(DEV))


def _render_target(H, W, chw, seed):
    g = torch.Generator().manual_seed(seed)
    render = torch.rand((3, H, W) if chw else (H, W, 3), generator=g) * 1.4 - 0.2   # values outside [0,1]: the clamp of the HWC case matters
    target = torch.rand(3, H, W, generator=g)
    return render, target


def _model_terms(render, target, M, chw, fn):
    """-> (value, gradient in the render's layout) of fn(r_chw, t, M) in float64; HWC is the clamped case, CHW the un-clamped one"""
    r = render.double().requires_grad_(True)
    img = r if chw else torch.clamp(r.permute(2, 0, 1), 0, 1)
    v = fn(img, target.double(), M)
    if v.requires_grad:
        v.backward()
    return float(v), (r.grad if r.grad is not None else torch.zeros_like(r))


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_masked_l1_ssim_value_and_gradient_match_the_f64_model(lfs, shape, kind):
    """Both layouts (HWC clamped with values in [-0.2, 1.2]; CHW un-clamped) and lambda in {0.2, 0, 1}: the loss is linear in its two terms, so the float64 model
    evaluates each term and its gradient once per layout and the three lambdas combine them."""
    from lichtfeld_studio_amd import losses
    H, W = shape
    m_np = _mask(kind, H, W, seed=H * 7 + W)
    pm = _prepared(m_np)
    M = torch.from_numpy(m_np).double()
    for chw in (False, True):
        render, target = _render_target(H, W, chw, H * 1000 + W + int(chw))
        l1, g_l1 = _model_terms(render, target, M, chw, mref.masked_l1)
        ss, g_ss = _model_terms(render, target, M, chw, mref.masked_ssim_term)
        for lam in LAMBDAS:
            loss = torch.full((1,), LOSS0, device=DEV)
            v = losses.loss_fwd_bwd("l1_ssim", render.to(DEV), target.to(DEV), WEIGHT, loss, chw=chw, clamp=not chw, lambda_dssim=lam, mask=pm)
            want = WEIGHT * ((1 - lam) * l1 + lam * ss)
            g_want = WEIGHT * ((1 - lam) * g_l1 + lam * g_ss)
            err_l = abs(float(loss) - LOSS0 - want)
            err_g, scale = float((v.cpu().double() - g_want).abs().max()), float(g_want.abs().max())
            print(f"{shape} {kind} chw={chw} lam={lam}: loss {want:.7f} err {err_l:.2e}; grad max {scale:.3e} err {err_g:.2e}")
            assert err_l < 2e-6, (chw, lam)
            assert err_g < 1e-5 * scale + 1e-12, (chw, lam)
            assert bool(torch.isfinite(v).all())
            if kind == "empty":   # the loss is untouched, the gradient all zeros
                assert float(loss) == LOSS0 and float(v.abs().max()) == 0.0


@pytest.mark.parametrize("chw", [False, True])
def test_full_mask_agrees_with_the_unmasked_entry(lfs, chw):
    from lichtfeld_studio_amd import losses
    H, W = 37, 53
    render, target = _render_target(H, W, chw, 11)
    pm = _prepared(_mask("full", H, W))
    for kind in ("l1_ssim", "mse"):
        a, b = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        va = losses.loss_fwd_bwd(kind, render.to(DEV), target.to(DEV), WEIGHT, a, chw=chw, clamp=not chw, lambda_dssim=0.2, mask=pm)
        vb = losses.loss_fwd_bwd(kind, render.to(DEV), target.to(DEV), WEIGHT, b, chw=chw, clamp=not chw, lambda_dssim=0.2)
        assert abs(float(a) - float(b)) < 2e-6
        assert float((va - vb).abs().max()) < 1e-5 * float(vb.abs().max()) + 1e-12


def _chebyshev_further_than(support, d):
    """bool [H,W]: pixels whose Chebyshev distance to every True pixel of `support` exceeds d"""
    near = torch.nn.functional.max_pool2d(support[None, None].float(), 2 * d + 1, stride=1, padding=d)[0, 0] > 0
    return ~near


def test_gradient_is_local_to_the_mask(lfs):
    """(64,80), M > 0 only inside rows 8-23 and columns 8-29: v_render is exactly 0 further than 5 pixels from the mask's support (the 11x11 window's reach),
    and what render and target hold further than 10 pixels away (the window of a pixel within the window's reach) does not reach v_render at all."""
    from lichtfeld_studio_amd import losses
    H, W = 64, 80
    m_np = np.zeros((H, W), np.uint8)
    m_np[8:24, 8:30] = np.random.RandomState(3).randint(1, 256, size=(16, 22)).astype(np.uint8)
    pm = _prepared(m_np)
    support = torch.from_numpy(m_np > 0)
    far5, far10 = _chebyshev_further_than(support, 5), _chebyshev_further_than(support, 10)
    assert bool(far5.any()) and bool(far10.any())
    for chw in (False, True):
        render, target = _render_target(H, W, chw, 21 + int(chw))
        loss = torch.zeros(1, device=DEV)
        v = losses.loss_fwd_bwd("l1_ssim", render.to(DEV), target.to(DEV), WEIGHT, loss, chw=chw, clamp=not chw, lambda_dssim=0.2, mask=pm).cpu()
        v_chw = v if chw else v.permute(2, 0, 1)
        assert float(v_chw[:, ~far5].abs().max()) > 0
        assert float(v_chw[:, far5].abs().max()) == 0.0
        g = torch.Generator().manual_seed(99)
        render2, target2 = render.clone(), target.clone()
        r2_chw = render2 if chw else render2.permute(2, 0, 1)
        r2_chw[:, far10] = torch.rand(3, int(far10.sum()), generator=g) * 1.4 - 0.2
        target2[:, far10] = torch.rand(3, int(far10.sum()), generator=g)
        loss2 = torch.zeros(1, device=DEV)
        v2 = losses.loss_fwd_bwd("l1_ssim", render2.contiguous().to(DEV), target2.to(DEV), WEIGHT, loss2, chw=chw, clamp=not chw, lambda_dssim=0.2, mask=pm).cpu()
        assert torch.equal(v.view(torch.int32), v2.view(torch.int32))
        assert abs(float(loss) - float(loss2)) < 2e-6   # (the blocks' float atomics arrive in any order: the value, not its bits)


def test_alpha_penalty_outside_the_mask(lfs):
    from lichtfeld_studio_amd import losses
    H, W, w_a = 37, 53, 0.7
    m_np = _mask("soft", H, W, seed=5)
    m_np[10:20, 10:30] = 255
    pm = _prepared(m_np)
    render, target = _render_target(H, W, True, 31)
    alpha = torch.rand(H, W, generator=torch.Generator().manual_seed(32))
    a, b = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    v0 = losses.loss_fwd_bwd("l1_ssim", render.to(DEV), target.to(DEV), WEIGHT, a, chw=True, clamp=False, lambda_dssim=0.2, mask=pm)
    v1, v_alpha = losses.loss_fwd_bwd("l1_ssim", render.to(DEV), target.to(DEV), WEIGHT, b, chw=True, clamp=False, lambda_dssim=0.2, mask=pm,
                                      alpha=alpha.to(DEV), alpha_weight=w_a)
    assert torch.equal(v0, v1)   # the penalty does not touch the image's gradient
    val, g = mref.alpha_penalty(alpha.double(), torch.from_numpy(m_np).double(), w_a)
    val, g = WEIGHT * float(val), WEIGHT * g
    # the photometric part is a float32 sum of its own, so the difference of the two calls holds the penalty only within the loss bound; a call with lambda 0
    # and the render as its own target has a photometric part of exactly 0 and leaves the penalty alone: 1e-6 relative
    assert abs((float(b) - float(a)) - val) < 2e-6
    c = torch.zeros(1, device=DEV)
    same = render.clamp(0, 1)
    _, v_alpha2 = losses.loss_fwd_bwd("l1_ssim", same.to(DEV), same.to(DEV), WEIGHT, c, chw=True, clamp=False, lambda_dssim=0.0, mask=pm, alpha=alpha.to(DEV), alpha_weight=w_a)
    assert abs(float(c) - val) < 1e-6 * abs(val)
    assert torch.equal(v_alpha, v_alpha2)
    assert float((v_alpha.cpu().double() - g).abs().max()) < 1e-6 * float(g.abs().max())
    assert float(v_alpha.cpu()[torch.from_numpy(m_np == 255)].abs().max()) == 0.0
    with pytest.raises(ValueError):
        losses.loss_fwd_bwd("l1_ssim", render.to(DEV), target.to(DEV), WEIGHT, c, chw=True, clamp=False, alpha=alpha.to(DEV), alpha_weight=w_a)


@pytest.mark.parametrize("kind", ["soft", "blob", "empty"])
@pytest.mark.parametrize("shape", [(37, 53), (9, 40)])
def test_masked_mse_matches_the_f64_model(lfs, shape, kind):
    from lichtfeld_studio_amd import losses
    H, W = shape
    m_np = _mask(kind, H, W, seed=H + W)
    pm = _prepared(m_np)
    M = torch.from_numpy(m_np).double()
    for chw in (False, True):
        for clamp in (True, False):
            render, target = _render_target(H, W, chw, 41 + int(chw))
            r = render.double().requires_grad_(True)
            img = r if chw else r.permute(2, 0, 1)
            img = torch.clamp(img, 0, 1) if clamp else img
            want = WEIGHT * mref.masked_mse(img, target.double(), M)
            if want.requires_grad:
                want.backward()
            g_want = r.grad if r.grad is not None else torch.zeros_like(r)
            loss = torch.full((1,), LOSS0, device=DEV)
            v = losses.loss_fwd_bwd("mse", render.to(DEV), target.to(DEV), WEIGHT, loss, chw=chw, clamp=clamp, mask=pm)
            assert abs(float(loss) - LOSS0 - float(want)) < 2e-6, (chw, clamp)
            assert float((v.cpu().double() - g_want).abs().max()) < 1e-5 * float(g_want.abs().max()) + 1e-12, (chw, clamp)
            if kind == "empty":
                assert float(loss) == LOSS0 and float(v.abs().max()) == 0.0


def _np_sums(m):
    H, W = m.shape
    mc = m[5:H - 5, 5:W - 5] if (H > 10 and W > 10) else m
    return [int(m.astype(np.int64).sum()), int(mc.astype(np.int64).sum())]


def test_mask_prepare_sums_copy_threshold_and_invert(lfs):
    from lichtfeld_studio_amd import losses
    for (H, W) in ((37, 300), (9, 40), (11, 11)):   # (37,300): 5 x 10 blocks of 64 x 4 pixels, ragged on both axes
        m_np = _mask("soft", H, W, seed=H)
        src = torch.from_numpy(m_np).to(DEV)
        a = losses.prepare_mask(src, W, H)
        b = losses.prepare_mask(src, W, H)
        assert np.array_equal(a.mask_u8.cpu().numpy(), m_np)   # a same-size call copies the bytes
        assert a.sums.cpu().tolist() == _np_sums(m_np) and b.sums.cpu().tolist() == a.sums.cpu().tolist()
        # threshold first, then invert
        t = losses.prepare_mask(src, W, H, invert=False, threshold=100)
        want = np.where(m_np >= 100, 255, 0).astype(np.uint8)
        assert np.array_equal(t.mask_u8.cpu().numpy(), want) and t.sums.cpu().tolist() == _np_sums(want)
        ti = losses.prepare_mask(src, W, H, invert=True, threshold=100)
        assert np.array_equal(ti.mask_u8.cpu().numpy(), 255 - want) and ti.sums.cpu().tolist() == _np_sums(255 - want)
        i = losses.prepare_mask(src, W, H, invert=True)
        assert np.array_equal(i.mask_u8.cpu().numpy(), 255 - m_np) and i.sums.cpu().tolist() == _np_sums(255 - m_np)
    # the sums are written, not accumulated: a PreparedMask's sums tensor is fresh, so call the entry twice on the same one
    lib = losses.load_library()
    sums = torch.full((2,), 12345, dtype=torch.int64, device=DEV)
    dst = torch.empty(H, W, dtype=torch.uint8, device=DEV)
    for _ in range(2):
        assert lib.lfs_mask_prepare(losses.ptr(src), C.c_uint32(W), C.c_uint32(H), losses.ptr(dst), C.c_uint32(W), C.c_uint32(H), C.c_uint32(0), C.c_int32(-1),
                                    losses.ptr(sums), losses.stream()) == 0
    assert sums.cpu().tolist() == _np_sums(m_np)


@pytest.mark.parametrize("src_hw,dst_hw", [((36, 48), (18, 24)), ((37, 50), (18, 25))])
def test_mask_prepare_resamples_as_the_image_path_does(lfs, src_hw, dst_hw):
    """byte for byte round(255 x) of u8_to_chw_f32 applied to the same plane replicated to 3 channels: mask and image stay registered"""
    from lichtfeld_studio_amd import loader, losses
    (sh, sw), (dh, dw) = src_hw, dst_hw
    m_np = _mask("soft", sh, sw, seed=sw)
    src = torch.from_numpy(m_np).to(DEV)
    pm = losses.prepare_mask(src, dw, dh)
    img = loader.u8_to_chw_f32(src[:, :, None].expand(sh, sw, 3).contiguous(), dw, dh)
    want = torch.round(img * 255.0).to(torch.uint8).cpu().numpy()
    assert np.array_equal(want[0], want[1]) and np.array_equal(want[0], want[2])
    got = pm.mask_u8.cpu().numpy()
    assert got.shape == (dh, dw) and np.array_equal(got, want[0])
    assert pm.sums.cpu().tolist() == _np_sums(got)
    t = losses.prepare_mask(src, dw, dh, invert=True, threshold=128)
    assert np.array_equal(t.mask_u8.cpu().numpy(), 255 - np.where(got >= 128, 255, 0).astype(np.uint8))


def test_masked_entry_points_refuse_bad_arguments_before_any_launch(lfs):
    from lichtfeld_studio_amd import losses
    lib = losses.load_library()
    H, W = 20, 24
    render, target = _render_target(H, W, True, 51)
    render, target = render.to(DEV), target.to(DEV)
    pm = _prepared(_mask("soft", H, W))
    alpha = torch.rand(H, W).to(DEV)
    nbytes = 3 * 3 * H * W * 4
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    v = torch.full((3, H, W), 7.0, device=DEV)
    v_alpha = torch.full((H, W), 7.0, device=DEV)
    loss = torch.full((1,), 3.0, device=DEV)
    p, u32, f32 = losses.ptr, C.c_uint32, C.c_float

    def photometric(h=H, w=W, mask=pm.mask_u8, sums=pm.sums, a=None, va=None, ws_bytes=nbytes):
        return lib.lfs_photometric_loss_masked_fwd_bwd(u32(h), u32(w), p(render), u32(1), u32(0), p(target), p(mask), p(sums), f32(0.2), f32(1.0), p(a), f32(1.0), p(va),
                                                       p(v), p(loss), p(ws), C.c_size_t(ws_bytes), losses.stream())

    def mse(h=H, w=W, mask=pm.mask_u8, sums=pm.sums):
        return lib.lfs_mse_loss_masked_fwd_bwd(u32(h), u32(w), p(render), u32(1), u32(0), p(target), p(mask), p(sums), f32(1.0), p(v), p(loss), losses.stream())

    INVALID, WORKSPACE = -1, -3
    assert photometric(mask=None) == INVALID and photometric(sums=None) == INVALID
    assert photometric(a=alpha) == INVALID and photometric(va=v_alpha) == INVALID   # alpha and v_alpha: both or neither
    assert photometric(ws_bytes=nbytes - 1) == WORKSPACE
    assert photometric(h=0) == 0 and photometric(w=0) == 0
    assert mse(mask=None) == INVALID and mse(sums=None) == INVALID
    assert mse(h=0) == 0 and mse(w=0) == 0
    src = torch.zeros(H, W, dtype=torch.uint8, device=DEV)
    dst = torch.full((H, W), 9, dtype=torch.uint8, device=DEV)
    sums = torch.full((2,), 5, dtype=torch.int64, device=DEV)

    def prepare(s=src, d=dst, sm=sums, sw=W, sh=H):
        return lib.lfs_mask_prepare(p(s), u32(sw), u32(sh), p(d), u32(W), u32(H), u32(0), C.c_int32(-1), p(sm), losses.stream())

    assert prepare(s=None) == INVALID and prepare(d=None) == INVALID and prepare(sm=None) == INVALID and prepare(sw=0) == INVALID and prepare(sh=0) == INVALID
    torch.cuda.synchronize()
    # nothing was launched: every output still holds its sentinel
    assert float(loss) == 3.0 and bool((v == 7.0).all()) and bool((v_alpha == 7.0).all()) and bool((dst == 9).all()) and sums.cpu().tolist() == [5, 5]
    assert photometric(a=alpha, va=v_alpha) == 0 and mse() == 0 and prepare() == 0
    torch.cuda.synchronize()
    assert float(loss) != 3.0 and sums.cpu().tolist() == [0, 0]
