"""Scene transform over csrc/splat_transform.hip: move a trained splat by a similarity x' = s R x + t - turn it upright, centre it, bring it back to
the data's frame, merge two captures - and cut it to a box.

    xf = similarity(rotation=R, scale=s, translation=t)        # or similarity(M4x4); LfsError where the C function refuses (shear, reflection, ...)
    moved = transform_model(model, xf)                          # means, orientations, log-scales AND the SH bands (all bands the model holds)
    cams  = transform_cameras(viewmats, xf)                     # the rigid cameras that see the moved scene as before
    part  = crop(moved, box_min, box_max)                       # the Gaussians whose mean lies in the box

The reference's SplatData::transform (src/core/splat_data.cpp:288) leaves shN alone: after a rotation every view-dependent colour points the wrong way.
`transform_model(..., rotate_sh=False)` reproduces that, for comparison only. sh0 and the opacities are invariant under a similarity. Not covered: moving a model
DURING training (Adam's second moments do not transform linearly), non-uniform scale, shear, reflections."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from .capi import LfsError, SplatTransformStruct, check, load_library, ptr, require_gpu, stream

MAX_SH_DEGREE = 4


def sh_rotation_matrices(R, degree: int = MAX_SH_DEGREE):
    """[M_1, ..., M_degree] in float64 (lfs_sh_rotation_matrices): a'_l = M_l a_l rotates band l of one colour channel by the proper rotation R [3,3]."""
    R = np.ascontiguousarray(np.asarray(R, np.float64).reshape(3, 3))
    degree = int(degree)
    out = np.zeros(max(sum((2 * l + 1) ** 2 for l in range(1, min(degree, MAX_SH_DEGREE) + 1)), 1), np.float64)
    check(load_library().lfs_sh_rotation_matrices(R.ctypes.data_as(C.c_void_p), C.c_uint32(degree & 0xFFFFFFFF), out.ctypes.data_as(C.c_void_p)), "sh_rotation_matrices")
    mats, o = [], 0
    for l in range(1, degree + 1):
        n = 2 * l + 1
        mats.append(out[o:o + n * n].reshape(n, n).copy())
        o += n * n
    return mats


def _quat_to_rotmat(q) -> np.ndarray:
    q = np.asarray(q, np.float64).reshape(4)
    n = np.linalg.norm(q)
    if not np.isfinite(n) or n == 0:
        raise LfsError("similarity: the rotation quaternion must be finite and non-zero")
    w, x, y, z = q / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


class SplatTransform:
    """A similarity: the float64 4x4 (`matrix`) and the float32 record of the C library built from it (`record(sh_degree)`). `a @ b` applies b first;
    `inverse()`; both in float64. Constructed by `similarity`."""

    def __init__(self, matrix):
        m = np.ascontiguousarray(np.asarray(matrix, np.float64))
        if m.shape != (4, 4):
            raise LfsError("SplatTransform: a 4x4 matrix is needed")
        self.matrix = m
        self._records = {}
        self.record(0)   # refuses here what the C function refuses

    def record(self, sh_degree: int = 0) -> SplatTransformStruct:
        sh_degree = int(sh_degree)
        rec = self._records.get(sh_degree)
        if rec is None:
            rec = SplatTransformStruct()
            check(load_library().lfs_splat_transform_from_matrix(self.matrix.ctypes.data_as(C.c_void_p), C.c_uint32(sh_degree & 0xFFFFFFFF), C.byref(rec)),
                  "splat_transform_from_matrix")
            self._records[sh_degree] = rec
        return rec

    @property
    def scale(self) -> float:
        return float(np.cbrt(np.linalg.det(self.matrix[:3, :3])))

    @property
    def rotation(self) -> np.ndarray:
        """R in float64, re-orthonormalised (the polar factor of the linear part)"""
        u, _, vt = np.linalg.svd(self.matrix[:3, :3])
        return u @ vt

    @property
    def translation(self) -> np.ndarray:
        return self.matrix[:3, 3].copy()

    def inverse(self) -> "SplatTransform":
        s, R, t = self.scale, self.rotation, self.translation
        m = np.eye(4)
        m[:3, :3] = R.T / s
        m[:3, 3] = -(R.T @ t) / s
        return SplatTransform(m)

    def __matmul__(self, other: "SplatTransform") -> "SplatTransform":
        if not isinstance(other, SplatTransform):
            return NotImplemented
        return SplatTransform(self.matrix @ other.matrix)

    def __repr__(self) -> str:
        return f"SplatTransform(scale={self.scale:.6g}, translation={self.translation.tolist()})"


def similarity(matrix=None, *, rotation=None, scale: float = 1.0, translation=None) -> SplatTransform:
    """matrix: a 4x4 (x' = s R x + t in its upper rows, last row (0,0,0,1)); or rotation (a 3x3 or a wxyz quaternion; default none) + scale + translation.
    Raises LfsError exactly where lfs_splat_transform_from_matrix refuses."""
    if matrix is not None:
        if rotation is not None or translation is not None or scale != 1.0:
            raise LfsError("similarity: give a matrix OR rotation / scale / translation")
        return SplatTransform(matrix)
    R = np.eye(3)
    if rotation is not None:
        r = np.asarray(rotation, np.float64)
        if r.shape == (3, 3):
            R = r
        elif r.size == 4:
            R = _quat_to_rotmat(r)
        else:
            raise LfsError("similarity: rotation is a 3x3 matrix or a wxyz quaternion")
    m = np.eye(4)
    m[:3, :3] = float(scale) * R
    if translation is not None:
        m[:3, 3] = np.asarray(translation, np.float64).reshape(3)
    return SplatTransform(m)


def apply(xf: SplatTransform, sh_degree: int, means=None, quats=None, raw_scales=None, shN=None, *, out=None):
    """lfs_splat_transform_apply on float32 device tensors; any of the four may be None (skipped). out: None (new tensors), "inplace", or a 4-tuple of output tensors
    (None where the input is None). Bands 1..sh_degree of shN [N,K,3] are rotated, further rows copied. -> (means', quats', raw_scales', shN')."""
    ins = [means, quats, raw_scales, shN]
    widths = [(3,), (4,), (3,), None]
    N = next((int(t.shape[0]) for t in ins if t is not None), 0)
    for t, w in zip(ins, widths):
        if t is None:
            continue
        if t.dtype != torch.float32 or t.shape[0] != N or (w is not None and tuple(t.shape[1:]) != w) or (w is None and (t.dim() != 3 or t.shape[2] != 3)):
            raise LfsError("splat_transform: float32 means [N,3], quats [N,4], raw_scales [N,3], shN [N,K,3] are needed")
    require_gpu(*ins)
    rows = int(shN.shape[1]) if shN is not None else 0
    if shN is not None and rows == 0:
        ins[3] = None   # nothing to rotate, nothing to copy
    if out is None:
        outs = [None if t is None else torch.empty_like(t) for t in ins]
    elif isinstance(out, str) and out == "inplace":
        outs = list(ins)
    else:
        outs = list(out)
        if ins[3] is None:
            outs[3] = None
        require_gpu(*outs)
        for t, o in zip(ins, outs):
            if (t is None) != (o is None) or (t is not None and (o.shape != t.shape or o.dtype != t.dtype or o.device != t.device)):
                raise LfsError("splat_transform: every output must match its input in shape, dtype and device")
    rec = xf.record(sh_degree)
    check(load_library().lfs_splat_transform_apply(C.c_uint32(N), C.byref(rec), ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), ptr(ins[3]), C.c_uint32(rows),
                                                   ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), stream()), "splat_transform_apply")
    if shN is not None and rows == 0:
        outs[3] = shN if out is not None else shN.clone()
    return tuple(outs)


def transform_model(model, xf: SplatTransform, *, inplace: bool = False, rotate_sh: bool = True):
    """The model moved by xf: a new SplatModel (inplace=False) or the same object with its tensors overwritten. All bands the model holds are carried (max_sh_degree,
    not the active degree). rotate_sh=False leaves shN as it is - the reference's behaviour, kept for comparison. No host read."""
    from .rasterizer import SplatModel
    if not isinstance(xf, SplatTransform):
        raise LfsError("transform_model: xf is a SplatTransform (similarity(...))")
    if int(model.max_sh_degree) > MAX_SH_DEGREE:
        raise LfsError(f"transform_model: SH degree {model.max_sh_degree} > {MAX_SH_DEGREE}")
    with torch.no_grad():
        means, quats, scales, shN = (t.detach() for t in (model.means, model.raw_quats, model.raw_scales, model.shN))
        if not all(t.is_contiguous() for t in (means, quats, scales, shN)):
            if inplace:
                raise LfsError("transform_model: in place needs contiguous parameters")
            means, quats, scales, shN = (t.contiguous() for t in (means, quats, scales, shN))
        sh_in = shN if rotate_sh else None
        m2, q2, s2, h2 = apply(xf, int(model.max_sh_degree), means, quats, scales, sh_in, out="inplace" if inplace else None)
        if inplace:
            return model
        if not rotate_sh:
            h2 = shN.clone()
        return SplatModel(m2, model.sh0.detach().clone(), h2, s2, q2, model.raw_opacities.detach().clone(), model.max_sh_degree, model.active_sh_degree)


def transform_cameras(viewmats, xf: SplatTransform):
    """World-to-camera matrices [..., 4, 4] of the rigid cameras that see the scene moved by xf as the given ones saw it before: R_c' = R_c R^T,
    t_c' = s t_c - R_c R^T t. Camera-space points scale by s, so a pinhole image is unchanged. Computed in float64; a tensor comes back as a tensor of the same dtype
    and device, anything else as a float64 array."""
    is_tensor = isinstance(viewmats, torch.Tensor)
    v = viewmats.detach().to("cpu", torch.float64).numpy() if is_tensor else np.asarray(viewmats, np.float64)
    if v.shape[-2:] != (4, 4):
        raise LfsError("transform_cameras: [..., 4, 4] world-to-camera matrices are needed")
    s, R, t = xf.scale, xf.rotation, xf.translation
    out = np.zeros_like(v)
    Rc = v[..., :3, :3] @ R.T
    out[..., :3, :3] = Rc
    out[..., :3, 3] = s * v[..., :3, 3] - Rc @ t
    out[..., 3, 3] = 1.0
    if is_tensor:
        return torch.from_numpy(out).to(device=viewmats.device, dtype=viewmats.dtype)
    return out


def crop(model, box_min, box_max, *, world_to_box=None, invert: bool = False):
    """The Gaussians whose mean lies in the box box_min <= p <= box_max (invert: outside it), as a new SplatModel; order is preserved, an empty result is a valid model
    of N = 0. world_to_box: an optional 4x4 (or 3x4) taking world points into the box's frame (an oriented box); the test is evaluated in float32 on the model's device,
    on p = A mean + b. Plain tensor operations (the companion of the reference's SplatData::crop_by_cropbox, src/core/splat_data.cpp:615)."""
    from .rasterizer import SplatModel
    with torch.no_grad():
        means = model.means.detach()
        dev = means.device
        p = means
        if world_to_box is not None:
            w = torch.as_tensor(np.asarray(world_to_box, np.float64)[:3, :4], dtype=torch.float32).to(dev)
            p = means @ w[:, :3].T + w[:, 3]
        lo = torch.as_tensor(np.asarray(box_min, np.float64).reshape(3), dtype=torch.float32).to(dev)
        hi = torch.as_tensor(np.asarray(box_max, np.float64).reshape(3), dtype=torch.float32).to(dev)
        inside = ((p >= lo) & (p <= hi)).all(dim=1)
        keep = (inside.logical_not() if invert else inside).nonzero().squeeze(-1)
        return SplatModel(*[t.detach().index_select(0, keep).contiguous() for t in model.parameters()], model.max_sh_degree, model.active_sh_degree)
