"""Independent numpy models of the SOG export operators (lichtfeld_studio_amd/sog.py, csrc/sog.hip), written from the reference's semantics
(kernels/morton_encoding.cu, kernels/kmeans.cu, src/core/sogs.cpp, src/loader/formats/sogs.cpp) without sharing code with the product. The reference's CUDA
and libwebp sources have no CPU build, so these models are what the tests hold the kernels to."""
import io
import json
import zipfile

import numpy as np

U = 2.0 ** -24      # unit roundoff of f32


def _split_by_3(a):
    x = a.astype(np.uint64) & np.uint64(0x1fffff)
    for shift, mask in ((32, 0x1f00000000ffff), (16, 0x1f0000ff0000ff), (8, 0x100f00f00f00f00f), (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(shift))) & np.uint64(mask)
    return x


def morton_codes(means):
    """f32 [N,3] -> int64 [N] (morton_encoding.cu:21-87)"""
    means = np.asarray(means, np.float32)
    mins, maxs = means.min(0), means.max(0)
    cube = np.maximum((maxs - mins).max(), np.float32(1e-7)).astype(np.float32)
    rel = (means - mins).astype(np.float32)
    q = (rel.astype(np.float64) / np.float64(cube) * 2097151.0).astype(np.uint32)
    code = _split_by_3(q[:, 0]) | (_split_by_3(q[:, 1]) << np.uint64(1)) | (_split_by_3(q[:, 2]) << np.uint64(2))
    return (code ^ np.uint64(1 << 63)).view(np.int64)


def squared_distances(data, centroids, chunk=4096):
    """fp64 [N,k] of |x - c|^2, difference form"""
    data, centroids = np.asarray(data, np.float64), np.asarray(centroids, np.float64)
    out = np.empty((data.shape[0], centroids.shape[0]))
    for s in range(0, data.shape[0], chunk):
        diff = data[s:s + chunk, None, :] - centroids[None, :, :]
        out[s:s + chunk] = (diff * diff).sum(-1)
    return out


def assignment_excess_and_bound(data, centroids, labels):
    """-> (d2(x, c_label) - min_c d2(x, c), 8 (D + 2) u (|x|^2 + max_c |c|^2)), both fp64 [N]"""
    d2 = squared_distances(data, centroids)
    D = np.asarray(data).shape[1]
    x2 = (np.asarray(data, np.float64) ** 2).sum(1)
    c2 = (np.asarray(centroids, np.float64) ** 2).sum(1).max()
    excess = d2[np.arange(d2.shape[0]), np.asarray(labels, np.int64)] - d2.min(1)
    return excess, 8.0 * (D + 2) * U * (x2 + c2)


def assign_1d(data, sorted_centroids):
    """first strict minimum of |p - c| in f32 (kmeans.cu:58-83)"""
    p, c = np.asarray(data, np.float32), np.asarray(sorted_centroids, np.float32)
    dist = np.abs(p[:, None] - c[None, :])
    assert dist.dtype == np.float32
    return dist.argmin(1).astype(np.int32)      # numpy's argmin returns the first occurrence


def segment_means(data, labels, k):
    """fp64 means per label -> ([k,D], counts [k])"""
    data, labels = np.asarray(data, np.float64), np.asarray(labels, np.int64)
    sums = np.zeros((k, data.shape[1]))
    np.add.at(sums, labels, data)
    counts = np.bincount(labels, minlength=k)
    return sums / np.maximum(counts, 1)[:, None], counts


def inertia(data, centroids, labels):
    diff = np.asarray(data, np.float64) - np.asarray(centroids, np.float64)[np.asarray(labels, np.int64)]
    return float((diff * diff).sum())


# ---- the container, decoded from the format description alone --------------------------------------------------------
def texture_size(n):
    width = int(np.ceil(np.sqrt(n) / 4.0)) * 4
    height = int(np.ceil(np.float32(n) / np.float32(width) / 4.0)) * 4
    return width, height


def open_bundle(path):
    """-> (meta dict, {name: uint8 [h,w,4]}, list of names)"""
    from PIL import Image
    with zipfile.ZipFile(path) as z:
        names = z.namelist()
        meta = json.loads(z.read("meta.json"))
        images = {}
        for nme in names:
            if nme.endswith(".webp"):
                with Image.open(io.BytesIO(z.read(nme))) as im:
                    assert im.format == "WEBP" and im.mode in ("RGBA", "RGB"), (nme, im.format, im.mode)   # (an all-opaque image carries no alpha plane: it decodes to 255)
                    images[nme] = np.asarray(im.convert("RGBA")).copy()
    return meta, images, names


def log_transform(v):
    v = np.asarray(v, np.float64)
    return np.sign(v) * np.log(np.abs(v) + 1.0)
