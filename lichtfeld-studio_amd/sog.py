"""SOG export: the compressed `.sog` bundle web viewers load (the reference's --save-sog: src/core/sogs.cpp:335-744 writer,
src/loader/formats/sogs.cpp reader, kernels/kmeans.cu, kernels/morton_encoding.cu).

  morton_encode / morton_sort_indices   kernels/morton_encoding.cu:57-105    -> int64 [N] / the Morton order (stable: ties by index)
  kmeans_1d                             kernels/kmeans.cu:226-304            -> (centroids [k,1] ascending, labels int32 [n])
  kmeans                                kernels/kmeans.cu:162-224            -> (centroids [k,D], labels int32 [N])
  write_sog / read_sog                  the container, version 2

The four GPU operators (Morton codes; dense, 1-D assignment and centroid update of Lloyd's iteration) are HIP kernels behind the C ABI (csrc/sog.hip);
this module owns the host loops around them and the container. Quantisation is numpy f32 on the host in the reference's operation order: export runs
once per save. Images are lossless WebP through Pillow (`lossless=True, exact=True`; the reference links libwebp's lossless encoder); a `.sog` path
is a ZIP bundle, any other path gets the files loose beside it.

Deliberate differences from the reference writer:
  * palette size: `palette_size=None` reproduces sogs.cpp:630-632 as written - min(64, ...*1024), i.e. 64 for N >= 1024 and 1 below (a misplaced parenthesis
    relative to the original min(64, ...) * 1024); an explicit palette_size up to min(65536, N) is what the 16-bit labels are for.
  * shN centroid texture: channel c of pixel i * coeffs + j is coefficient j of colour c (row index j * 3 + c of the clustered rows), which is what the
    reference's own reader and the format expect; the reference writer reads index j + c * coeffs there (sogs.cpp:666-667) and scrambles its own round trip.
  * a 1-D codebook of a model so small that it has no more values than codebook entries (3 N <= 256) labels every value with the rank of that value, so
    the codebook decodes it exactly; the reference's kmeans_1d returns `arange` labels against SORTED data there (kept in kmeans_1d itself, kmeans.cu:237-241).
  * quaternion bytes: each of the three stored bytes is the reference's truncated value or the next one up, chosen so that the decoded quaternion - the
    reconstructed fourth component included - stays within one step, sqrt(2) / 255, of the original (_pack_quats). Any reader decodes it unchanged.
"""
from __future__ import annotations

import ctypes as C
import io
import json
import math
import os
import zipfile
from typing import Optional, Tuple

import numpy as np
import torch

from .capi import LfsError, check, load_library, ptr, require_gpu, stream, workspace

Tensor = torch.Tensor

K_MAX, D_MAX = 65536, 64          # csrc/sog.hip
KMEANSPP_MAX_K = 256


def _size_t(fn):
    fn.restype = C.c_size_t
    return fn


# ---------------------------------------------------------------------------------------------------------------------
# Morton order
# ---------------------------------------------------------------------------------------------------------------------
def morton_encode(means: Tensor) -> Tensor:
    """means f32 [N,3] -> int64 [N]: 21 bits per axis of (p - min) / cube, interleaved x | y << 1 | z << 2, plus INT64_MIN (morton_encoding.cu:21-97).
    The bounding cube is computed inside the call, on the device."""
    if means.dim() != 2 or means.shape[1] != 3:
        raise LfsError("Positions must have shape [N, 3]")
    if means.dtype != torch.float32:
        raise LfsError("Positions must be float32")
    means = means.detach().contiguous()
    require_gpu(means)
    lib = load_library()
    N = means.shape[0]
    codes = torch.empty(N, dtype=torch.int64, device=means.device)
    ws = workspace(_size_t(lib.lfs_morton_workspace_bytes)(C.c_int64(N)), means.device, "sog_morton")
    check(lib.lfs_morton_encode(C.c_int64(N), ptr(means), ptr(codes), ptr(ws), C.c_size_t(ws.numel()), stream()), "morton_encode")
    return codes


def morton_sort_indices(codes: Tensor) -> Tensor:
    """int64 [N] -> int64 [N], ascending. The reference's argsort leaves the order of equal codes unspecified; here it is a STABLE sort: ties by index."""
    if codes.dim() != 1:
        raise LfsError("Morton codes must be 1D tensor")
    return torch.sort(codes, stable=True)[1]


# ---------------------------------------------------------------------------------------------------------------------
# k-means
# ---------------------------------------------------------------------------------------------------------------------
def kmeans_assign(data: Tensor, centroids: Tensor) -> Tensor:
    """data [N,D], centroids [k,D] -> int32 [N]: the centroid maximising x.c - |c|^2/2 (= the nearest), lowest index among exactly equal scores."""
    require_gpu(data, centroids)
    if data.dim() != 2 or centroids.dim() != 2 or data.shape[1] != centroids.shape[1] or data.dtype != torch.float32 or centroids.dtype != torch.float32:
        raise LfsError("kmeans_assign: data [N,D] and centroids [k,D] must be float32 with the same D")
    lib = load_library()
    N, D = data.shape
    k = centroids.shape[0]
    labels = torch.empty(N, dtype=torch.int32, device=data.device)
    nbytes = _size_t(lib.lfs_kmeans_assign_workspace_bytes)(C.c_uint32(k), C.c_uint32(D))
    if nbytes == 0:
        raise LfsError(f"kmeans_assign: unsupported k = {k} (1..{K_MAX}) or D = {D} (1..{D_MAX})")
    ws = workspace(nbytes, data.device, "sog_kmeans")
    check(lib.lfs_kmeans_assign(C.c_int64(N), C.c_uint32(k), C.c_uint32(D), ptr(data), ptr(centroids), ptr(labels), ptr(ws), C.c_size_t(ws.numel()), stream()),
          "kmeans_assign")
    return labels


def kmeans_assign_1d(data: Tensor, sorted_centroids: Tensor) -> Tensor:
    """data [n], ascending centroids [k] -> int32 [n]: the first index that minimises |p - c| under a strict < (kmeans.cu:58-83)."""
    require_gpu(data, sorted_centroids)
    if data.dim() != 1 or sorted_centroids.dim() != 1 or data.dtype != torch.float32 or sorted_centroids.dtype != torch.float32:
        raise LfsError("kmeans_assign_1d: data [n] and centroids [k] must be 1-D float32")
    labels = torch.empty(data.shape[0], dtype=torch.int32, device=data.device)
    check(load_library().lfs_kmeans_assign_1d(C.c_int64(data.shape[0]), C.c_uint32(sorted_centroids.shape[0]), ptr(data), ptr(sorted_centroids), ptr(labels),
                                              stream()), "kmeans_assign_1d")
    return labels


def kmeans_update(data: Tensor, labels: Tensor, centroids: Tensor) -> None:
    """centroids [k,D], in place: the mean of the rows of data [N,D] that carry each label; a label nobody carries keeps its centroid (kmeans.cu:119-121).
    The grouping (stable sort of the labels, searchsorted for the segment bounds) is torch's; the sums are the kernel's."""
    require_gpu(data, labels, centroids)
    k, D = centroids.shape
    sorted_labels, order = torch.sort(labels, stable=True)
    order = order.to(torch.int32)
    seg_start = torch.searchsorted(sorted_labels, torch.arange(k + 1, dtype=labels.dtype, device=labels.device)).to(torch.int32)
    check(load_library().lfs_kmeans_update(C.c_int64(data.shape[0]), C.c_uint32(k), C.c_uint32(D), ptr(data), ptr(order), ptr(seg_start), ptr(centroids), stream()),
          "kmeans_update")


def kmeans_1d(data: Tensor, k: int, iterations: int = 10) -> Tuple[Tensor, Tensor]:
    """kmeans.cu:226-304. data [n] or [n,1] -> (centroids [k,1] ascending, labels int32 [n]).
    n <= k: the sorted data and `arange` labels (as the reference). Otherwise: centroids start as linspace(min, max, k); every iteration sorts them,
    assigns, and replaces the centroid of every non-empty cluster by its mean; after the last iteration the centroids are sorted once more and the labels
    remapped. The labels returned are therefore the assignment to the centroids BEFORE the last update."""
    flat = data.detach().reshape(-1).contiguous()
    if data.dim() == 2 and data.shape[1] != 1:
        raise LfsError("kmeans_1d expects 1D data")
    if flat.dtype != torch.float32:
        raise LfsError("Data must be float32")
    n = flat.shape[0]
    if n <= k:
        return torch.sort(flat)[0].unsqueeze(1), torch.arange(n, dtype=torch.int32, device=flat.device)
    lo, hi = float(flat.min()), float(flat.max())
    centroids = torch.linspace(lo, hi, k, dtype=torch.float32, device=flat.device)
    labels = torch.zeros(n, dtype=torch.int32, device=flat.device)
    points = flat.unsqueeze(1)
    for _ in range(iterations):
        centroids = torch.sort(centroids, stable=True)[0].contiguous()
        labels = kmeans_assign_1d(flat, centroids)
        kmeans_update(points, labels, centroids.unsqueeze(1))
    centroids, final_idx = torch.sort(centroids, stable=True)
    inv_map = torch.empty(k, dtype=torch.int32, device=flat.device)
    inv_map[final_idx] = torch.arange(k, dtype=torch.int32, device=flat.device)
    return centroids.unsqueeze(1).contiguous(), inv_map[labels.long()]


def _rand_device(generator):
    return generator.device if generator is not None else torch.device("cpu")


def _kmeanspp(data: Tensor, k: int, generator) -> Tensor:
    """k-means++ seeding with ONE running minimum-distance vector (O(k N D); the reference recomputes cdist against all chosen centroids for every new one:
    kmeans.cu:125-158, O(k^2 N D)). One host read per centroid for the draw."""
    n = data.shape[0]
    rdev = _rand_device(generator)
    first = int(torch.randint(n, (1,), generator=generator, device=rdev))
    chosen = [first]
    d2 = (data - data[first]).double().pow(2).sum(1)
    for _ in range(1, k):
        cum = torch.cumsum(d2, 0)
        total = float(cum[-1])
        u = float(torch.rand(1, generator=generator, device=rdev, dtype=torch.float64))
        nxt = int(torch.searchsorted(cum, torch.tensor([u * total], dtype=torch.float64, device=data.device), right=True)) if total > 0 else 0
        nxt = min(nxt, n - 1)
        chosen.append(nxt)
        d2 = torch.minimum(d2, (data - data[nxt]).double().pow(2).sum(1))
    return data[torch.tensor(chosen, device=data.device)].clone()


def kmeans(data: Tensor, k: int, iterations: int = 10, tolerance: float = 1e-4, init: Optional[Tensor] = None, generator=None) -> Tuple[Tensor, Tensor]:
    """kmeans.cu:162-224. data f32 [N,D] (D <= 64), k <= 65536 -> (centroids [k,D], labels int32 [N]).
    n <= k: a clone of the data and `arange` labels. Otherwise up to `iterations` rounds of assign + update, stopping once max|centroid movement| <
    tolerance (one host read per iteration, as in the reference; this is off the training path). The labels belong to the last assignment, i.e. to the
    centroids before the last update.

    Initialisation (the reference's k-means++ depends on torch's global RNG state and costs O(k^2 N D)):
      * `init` [k,D]: used as given (cloned);
      * otherwise k <= 256: k-means++ with a running minimum-distance vector, draws from `generator`;
      * otherwise (k > 256): k distinct points, the first k entries of torch.randperm(N, generator=generator).
    `generator` is a torch.Generator (CPU or the data's device); None uses torch's default CPU generator."""
    if data.dim() != 2:
        raise LfsError("Data must be 2D tensor [N, D]")
    if data.dtype != torch.float32:
        raise LfsError("Data must be float32")
    data = data.detach().contiguous()
    require_gpu(data)
    n, D = data.shape
    if n <= k:
        return data.clone(), torch.arange(n, dtype=torch.int32, device=data.device)
    if not 1 <= k <= K_MAX or not 1 <= D <= D_MAX:
        raise LfsError(f"kmeans: unsupported k = {k} (1..{K_MAX}) or D = {D} (1..{D_MAX})")
    if init is not None:
        if tuple(init.shape) != (k, D) or init.dtype != torch.float32:
            raise LfsError("kmeans: init must be float32 [k, D]")
        centroids = init.detach().to(data.device).clone().contiguous()
    elif k <= KMEANSPP_MAX_K:
        centroids = _kmeanspp(data, k, generator).contiguous()
    else:
        perm = torch.randperm(n, generator=generator, device=_rand_device(generator))[:k]
        centroids = data[perm.to(data.device)].clone().contiguous()
    labels = torch.zeros(n, dtype=torch.int32, device=data.device)
    for _ in range(iterations):
        old = centroids.clone()
        labels = kmeans_assign(data, centroids)
        kmeans_update(data, labels, centroids)
        if float((centroids - old).abs().max()) < tolerance:
            break
    return centroids, labels


# ---------------------------------------------------------------------------------------------------------------------
# the container
# ---------------------------------------------------------------------------------------------------------------------
SH_COEFFS = {0: 0, 1: 3, 2: 8, 3: 15}


def texture_size(n: int) -> Tuple[int, int]:
    """sogs.cpp:348-349: width = ceil(sqrt(N) / 4) * 4, height = ceil(N / width / 4) * 4 (the quotient in f32)."""
    width = int(math.ceil(math.sqrt(n) / 4.0)) * 4
    height = int(math.ceil(float(np.float32(n) / np.float32(width)) / 4.0)) * 4
    return width, height


def default_palette_size(n: int) -> int:
    """sogs.cpp:630-632 as written: min(64, max(1, int(2^floor(log2(N / 1024))) * 1024)), then min(., N): 64 for N >= 1024, 1 below."""
    p = min(64, max(1, int(2.0 ** math.floor(math.log2(n / 1024.0))) * 1024))
    return min(p, n)


def _codebook_1d(values: np.ndarray, device, iterations: int) -> Tuple[np.ndarray, np.ndarray]:
    """f32 [n] -> (codebook f32 [<= 256] ascending, labels uint8 [n]) through kmeans_1d(k = 256)."""
    n = values.shape[0]
    if n <= 256:          # every value gets its own entry: label = rank, so the codebook decodes it exactly (module docstring, third difference)
        order = np.argsort(values, kind="stable")
        labels = np.empty(n, np.uint8)
        labels[order] = np.arange(n, dtype=np.uint8)
        return values[order].astype(np.float32), labels
    cen, lab = kmeans_1d(torch.from_numpy(np.ascontiguousarray(values, np.float32)).to(device), 256, iterations)
    return cen.reshape(-1).cpu().numpy().astype(np.float32), lab.cpu().numpy().astype(np.uint8)


def _image(n: int, width: int, height: int, alpha: int) -> np.ndarray:
    img = np.zeros((width * height, 4), np.uint8)
    img[:, 3] = alpha
    if alpha == 255:
        img[:, :3] = 255      # the reference initialises these buffers to 255 throughout (sogs.cpp:425-426, :485, :526)
    return img


def _webp(img: np.ndarray, width: int, height: int) -> bytes:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img.reshape(height, width, 4), "RGBA").save(buf, format="WEBP", lossless=True, exact=True)
    return buf.getvalue()


_QUAT_OFFSETS = np.array([[i >> 2 & 1, i >> 1 & 1, i & 1] for i in range(8)], np.int32)     # row 0 = the reference's plain truncation


def _pack_quats(q: np.ndarray) -> np.ndarray:
    """pack_quaternion (sogs.cpp:60-140) on f32 [n,4] wxyz -> uint8 [n,4]: normalise (a zero quaternion becomes the identity), make the largest-magnitude
    component positive, scale by sqrt(2), store the other three in index order as bytes of (v / 2 + 1 / 2) * 255, alpha = 252 + argmax.
    Rounding of the three bytes (module docstring, fourth difference): the reference truncates all three, which keeps each STORED component within one step
    (sqrt(2) / 255) but lets the component the decoder reconstructs as sqrt(1 - v0^2 - v1^2 - v2^2) collect up to three one-sided steps. Each byte here is the
    truncated value or the next one up - still within one step of the true component - and of the eight combinations the one is kept whose decode (the
    reference reader's arithmetic, loader/formats/sogs.cpp:43-100) has the smallest largest error over all four components; ties keep the truncation."""
    f32 = np.float32
    q = q.astype(f32).copy()
    length = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    ok = length > 0
    q[ok] = q[ok] / length[ok, None]
    q[~ok] = np.array([1, 0, 0, 0], f32)
    largest = np.argmax(np.abs(q), axis=1)                       # first maximum, as the chain of strict > comparisons
    rows = np.arange(q.shape[0])
    q[q[rows, largest] < 0] *= f32(-1)
    sqrt2 = f32(1.41421356237)
    others = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])[largest]
    u = np.take_along_axis(q, others, axis=1)                    # the three stored components of the unit quaternion
    big = q[rows, largest]
    low = np.clip((u * sqrt2 * f32(0.5) + f32(0.5)) * f32(255.0), f32(0), f32(255)).astype(np.int32)
    out = np.empty((q.shape[0], 4), np.uint8)
    for s in range(0, q.shape[0], 1 << 16):
        e = slice(s, s + (1 << 16))
        cand = np.minimum(low[e, None, :] + _QUAT_OFFSETS[None], 255)                            # [m, 8, 3]
        v = (cand.astype(f32) / f32(255) - f32(0.5)) * sqrt2
        w = np.sqrt(np.clip(f32(1) - (v * v).sum(-1), f32(0), f32(1)))                           # the decoder's largest component
        norm = np.sqrt((v * v).sum(-1) + w * w)
        norm = np.where(norm > 0, norm, f32(1))
        err = np.maximum(np.abs(v / norm[..., None] - u[e, None, :]).max(-1), np.abs(w / norm - big[e, None]))
        pick = err.argmin(1)
        out[e, :3] = cand[np.arange(cand.shape[0]), pick].astype(np.uint8)
    out[:, 3] = 252 + largest
    return out


def write_sog(model, path: str, iterations: int = 10, palette_size: Optional[int] = None) -> dict:
    """Write `model` (a SplatModel) as SOG version 2; a path ending in .sog is one ZIP bundle, any other path writes the images loose beside it, with
    meta.json. iterations: Lloyd iterations of every clustering. palette_size: entries of the shN palette (None: the reference's value, see
    default_palette_size; explicit: up to min(65536, N)). Returns the meta dictionary."""
    means, sh0, shN, raw_scales, raw_quats, raw_opac = [p.detach() for p in model.parameters()]
    device = means.device
    N = int(means.shape[0])
    if N == 0:
        raise LfsError("No splats to write")
    width, height = texture_size(N)
    order = morton_sort_indices(morton_encode(means.float().contiguous())).cpu().numpy()
    files = {}

    # 1. means: sign(v) log(|v| + 1), per-axis range, 16 bits split over two images (sogs.cpp:424-480)
    m = means.float().cpu().numpy()
    mlog = np.copysign(np.log(np.abs(m) + np.float32(1.0)), m).astype(np.float32)
    mins, maxs = mlog.min(0), mlog.max(0)
    t = (mlog[order] - mins) / (maxs - mins + np.float32(1e-10))
    q16 = (np.float32(65535) * np.clip(t, np.float32(0), np.float32(1))).astype(np.uint16)
    img_l, img_u = _image(N, width, height, 255), _image(N, width, height, 255)
    img_l[:N, :3] = (q16 & 0xff).astype(np.uint8)
    img_u[:N, :3] = (q16 >> 8).astype(np.uint8)
    files["means_l.webp"], files["means_u.webp"] = _webp(img_l, width, height), _webp(img_u, width, height)

    # 2. quaternions: smallest three (sogs.cpp:484-508)
    img = _image(N, width, height, 255)
    img[:N] = _pack_quats(raw_quats.float().cpu().numpy()[order])
    files["quats.webp"] = _webp(img, width, height)

    # 3. raw (log) scales, column-major, 256-entry codebook (sogs.cpp:510-541)
    scale_codebook, lab = _codebook_1d(np.ascontiguousarray(raw_scales.float().cpu().numpy().T).reshape(-1), device, iterations)
    img = _image(N, width, height, 255)
    img[:N, :3] = lab.reshape(3, N).T[order]
    files["scales.webp"] = _webp(img, width, height)

    # 4. sh0 the same way; alpha = uint8(255 sigmoid(raw opacity)) (sogs.cpp:543-580)
    sh0_codebook, lab = _codebook_1d(np.ascontiguousarray(sh0.float().reshape(N, 3).cpu().numpy().T).reshape(-1), device, iterations)
    img = _image(N, width, height, 0)
    img[:N, :3] = lab.reshape(3, N).T[order]
    opacity = torch.sigmoid(raw_opac.float().reshape(N)).cpu().numpy()
    img[:N, 3] = (np.float32(255) * opacity[order]).astype(np.uint8)
    files["sh0.webp"] = _webp(img, width, height)

    meta = {"version": 2, "count": N, "width": width, "height": height,
            "means": {"mins": [float(v) for v in mins], "maxs": [float(v) for v in maxs], "files": ["means_l.webp", "means_u.webp"]},
            "scales": {"codebook": [float(v) for v in scale_codebook], "files": ["scales.webp"]},
            "quats": {"files": ["quats.webp"]},
            "sh0": {"codebook": [float(v) for v in sh0_codebook], "files": ["sh0.webp"]}}

    # 5. shN: palette of whole coefficient rows, then a 256-entry codebook over the palette's values (sogs.cpp:620-721)
    coeffs = int(shN.shape[1]) if shN.dim() == 3 else 0
    if coeffs > 0:
        bands = {3: 1, 8: 2, 15: 3}.get(coeffs)
        if bands is None:
            raise LfsError(f"write_sog: {coeffs} higher-order SH coefficients are not a whole number of bands")
        if palette_size is None:
            palette_size = default_palette_size(N)
        if not 1 <= palette_size <= min(K_MAX, N):
            raise LfsError(f"write_sog: palette_size must be in 1..min(65536, N) = {min(K_MAX, N)}")
        rows = shN.float().reshape(N, coeffs * 3).contiguous()            # row layout j * 3 + c
        centroids, labels = kmeans(rows, palette_size, iterations, generator=torch.Generator().manual_seed(0))   # a save is reproducible
        palette = int(centroids.shape[0])
        cb, cl = _codebook_1d(centroids.reshape(-1).cpu().numpy(), device, iterations)
        cw, chh = 64 * coeffs, (palette + 63) // 64
        cimg = _image(0, cw, chh, 255)
        cimg[:palette * coeffs, :3] = cl.reshape(palette * coeffs, 3)      # pixel i * coeffs + j, channel c = label of centroid i, element j * 3 + c
        files["shN_centroids.webp"] = _webp(cimg, cw, chh)
        lab = labels.cpu().numpy().astype(np.int64)[order]
        img = _image(N, width, height, 255)
        img[:N, 0], img[:N, 1], img[:N, 2] = lab & 0xff, (lab >> 8) & 0xff, 0
        files["shN_labels.webp"] = _webp(img, width, height)
        meta["shN"] = {"codebook": [float(v) for v in cb[:256]], "palette_size": palette, "bands": bands, "coeffs": coeffs,
                       "files": ["shN_centroids.webp", "shN_labels.webp"]}

    meta_json = json.dumps(meta, indent=2).encode()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if path.endswith(".sog"):
        with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:      # the images are compressed already
            for name, blob in files.items():
                z.writestr(name, blob)
            z.writestr("meta.json", meta_json)
    else:
        base = os.path.dirname(os.path.abspath(path))
        for name, blob in files.items():
            with open(os.path.join(base, name), "wb") as fh:
                fh.write(blob)
        with open(path if path.endswith(".json") else os.path.join(base, "meta.json"), "wb") as fh:
            fh.write(meta_json)
    return meta


def _read_files(path: str) -> dict:
    if zipfile.is_zipfile(path):
        with zipfile.ZipFile(path) as z:
            return {n: z.read(n) for n in z.namelist()}
    base = path if os.path.isdir(path) else os.path.dirname(os.path.abspath(path))
    out = {}
    for n in os.listdir(base):
        if n == "meta.json" or n.endswith(".webp"):
            with open(os.path.join(base, n), "rb") as fh:
                out[n] = fh.read()
    if os.path.isfile(path) and path.endswith(".json"):
        with open(path, "rb") as fh:
            out["meta.json"] = fh.read()
    return out


def _decode(blob: bytes) -> np.ndarray:
    from PIL import Image
    with Image.open(io.BytesIO(blob)) as im:
        return np.asarray(im.convert("RGBA")).reshape(-1, 4)


def read_sog(path: str, device="cuda:0"):
    """A .sog bundle, a meta.json or the directory that holds one -> SplatModel (src/loader/formats/sogs.cpp:230-480): raw scales / sh0 / shN from the
    codebooks, means through the inverse log transform, normalised wxyz quaternions, raw opacity = logit(clamp(alpha / 255, 1e-5, 1 - 1e-5))."""
    from .rasterizer import SplatModel
    files = _read_files(path)
    if "meta.json" not in files:
        raise LfsError(f"{path}: no meta.json")
    meta = json.loads(files["meta.json"])
    if meta.get("version") != 2:
        raise LfsError(f"{path}: SOG version {meta.get('version')} is not supported")
    N = int(meta["count"])
    f32 = np.float32

    def image(name):
        if name not in files:
            raise LfsError(f"{path}: missing {name}")
        img = _decode(files[name])
        if img.shape[0] < N:
            raise LfsError(f"{path}: {name} holds fewer than {N} pixels")
        return img

    lo, hi = image("means_l.webp")[:N, :3].astype(np.uint16), image("means_u.webp")[:N, :3].astype(np.uint16)
    mins, maxs = np.array(meta["means"]["mins"], f32), np.array(meta["means"]["maxs"], f32)
    mlog = (lo | (hi << 8)).astype(f32) / f32(65535) * (maxs - mins) + mins
    means = (np.where(mlog >= 0, f32(1), f32(-1)) * (np.exp(np.abs(mlog)) - f32(1))).astype(f32)

    qi = image("quats.webp")[:N]
    largest = qi[:, 3].astype(np.int64) - 252
    largest[(largest < 0) | (largest > 3)] = 0
    v = (qi[:, :3].astype(f32) / f32(255) - f32(0.5)) * f32(1.41421356237)
    big = np.sqrt(np.clip(f32(1) - (v * v).sum(1), f32(0), f32(1)))
    quats = np.empty((N, 4), f32)
    others = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])[largest]
    np.put_along_axis(quats, others, v, axis=1)
    quats[np.arange(N), largest] = big
    length = np.sqrt((quats * quats).sum(1, keepdims=True))
    quats = np.where(length > 0, quats / np.where(length > 0, length, f32(1)), quats).astype(f32)

    def lookup(codebook, idx, what):
        codebook = np.array(codebook, f32)
        if idx.size and int(idx.max()) >= codebook.shape[0]:
            raise LfsError(f"{path}: {what} codebook index out of bounds")
        return codebook[idx]

    scales = lookup(meta["scales"]["codebook"], image("scales.webp")[:N, :3], "scale")
    ci = image("sh0.webp")[:N]
    sh0 = lookup(meta["sh0"]["codebook"], ci[:, :3], "color").reshape(N, 1, 3)
    a = np.clip(ci[:, 3].astype(f32) / f32(255), f32(1e-5), f32(1) - f32(1e-5))
    opac = np.log(a / (f32(1) - a)).astype(f32)

    sh_degree, shN = 0, np.zeros((N, 0, 3), f32)
    if "shN" in meta:
        sm = meta["shN"]
        sh_degree = int(sm.get("bands") or {3: 1, 8: 2, 15: 3}[int(sm["coeffs"])])
        coeffs = SH_COEFFS[sh_degree]
        cimg = image_any = _decode(files["shN_centroids.webp"]) if "shN_centroids.webp" in files else None
        if image_any is None:
            raise LfsError(f"{path}: missing shN_centroids.webp")
        palette = int(sm.get("palette_size") or cimg.shape[0] // (64 * coeffs))
        if cimg.shape[0] < palette * coeffs:
            raise LfsError(f"{path}: shN_centroids.webp holds fewer than {palette} centroids")
        centroids = lookup(sm["codebook"], cimg[:palette * coeffs, :3], "SH").reshape(palette, coeffs, 3)   # [i][j][c] = channel c of pixel i * coeffs + j
        li = image("shN_labels.webp")[:N]
        labels = li[:, 0].astype(np.int64) | (li[:, 1].astype(np.int64) << 8)
        shN = np.zeros((N, coeffs, 3), f32)
        ok = labels < palette                                       # (a label past the palette leaves zeros, sogs.cpp:453)
        shN[ok] = centroids[labels[ok]]

    mk = lambda x: torch.from_numpy(np.ascontiguousarray(x, f32)).to(device).requires_grad_(True)
    return SplatModel(mk(means), mk(sh0), mk(shN), mk(scales), mk(quats), mk(opac), sh_degree)
