"""float64 host model of the per-primitive depth value of the fastgs depth modes (LFS_FASTGS_DEPTH / LFS_FASTGS_INVDEPTH), independent of the code
under test: z_i = w2c[2,:3] . mean_i + w2c[2,3] on the float32 inputs the device sees, d_i = z_i ("depth") or 1 / z_i ("invdepth"), dd/dz = 1 or -1 / z^2.

A depth render is a colour render whose colour is d_i: twin() builds the degree-0 scene whose red channel is d_i / s (s = max d_i), which every value test of
tests/test_gpu_fastgs_depth.py compares the depth kernels against."""
import numpy as np

C0 = 0.28209479177387814


def z64(means, w2c):
    m = np.asarray(means, np.float32).astype(np.float64)
    w = np.asarray(w2c, np.float32).astype(np.float64)
    return m @ w[2, :3] + w[2, 3]


def d64(means, w2c, kind):
    """-> (d_i, dd_i/dz_i) in float64"""
    z = z64(means, w2c)
    if kind == "depth":
        return z, np.ones_like(z)
    assert kind == "invdepth"
    return 1.0 / z, -1.0 / (z * z)


def twin(sc, kind):
    """-> (twin scene, s): the same geometry and opacities, SH degree 0, colour (d_i / s, 0, 0) - sh0 = (colour - 0.5) / C0 (the rasterizer's colour is
    max(C0 sh0 + 0.5, 0)); green and blue get sh0 = -1 / C0 (colour -0.5, clamped to 0)."""
    d, _ = d64(sc["means"], sc["w2c"], kind)
    s = float(d.max())
    N = len(d)
    sh0 = np.full((N, 1, 3), -1.0 / C0)
    sh0[:, 0, 0] = (d / s - 0.5) / C0
    return dict(sc, sh0=sh0, sh_rest=np.zeros_like(np.asarray(sc["sh_rest"], np.float64)), active_sh_bases=1), s
