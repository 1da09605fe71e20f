"""The three fastgs entry points of the C ABI (lfs_fastgs_view_preprocess / _render / _backward) called directly through ctypes, for the tests that look at return
codes, at what a refused call left untouched, and at one stage on a workspace another call prepared. `a` is the device tensor list in the order
(means, scales_raw, rot_raw, opac_raw, sh0, sh_rest, w2c), `s` a FastGSSettings. Nothing here checks a return code unless it says so: the callers assert on them."""
import ctypes as C

import torch

DEV = "cuda:0"


def view_of(a, s, pws):
    """lfs_fastgs_view of the scene, the camera and a primitive workspace (the temporaries it points to stay alive with it)"""
    from lichtfeld_studio_amd import fastgs
    cam, w2c = s.cam_position.reshape(-1)[:3].contiguous(), a[6].reshape(-1, 4, 4)[0].contiguous()
    v = fastgs.view_struct(s, a[0], a[1], a[2], a[3].reshape(-1), a[4], a[5], w2c, cam, pws)
    v.keep = (cam, w2c)
    return v


def instance_workspace(lib, s, n_inst):
    return torch.empty(max(256, lib.lfs_fastgs_instance_workspace_bytes(C.c_uint32(s.width), C.c_uint32(s.height), C.c_int64(n_inst))), dtype=torch.uint8, device=DEV)


def preprocess_raw(lib, a, s, flags, pws=None, n_dev=None):
    """lfs_fastgs_view_preprocess -> (return code, primitive workspace, device n_instances)"""
    from lichtfeld_studio_amd.capi import ptr, stream
    if pws is None:
        pws = torch.zeros(max(256, lib.lfs_fastgs_primitive_workspace_bytes(C.c_uint32(a[0].shape[0]), C.c_uint32(s.width), C.c_uint32(s.height))), dtype=torch.uint8, device=DEV)
    if n_dev is None:
        n_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
    rc = lib.lfs_fastgs_view_preprocess(C.byref(view_of(a, s, pws)), C.c_uint32(flags), ptr(n_dev), stream())
    return rc, pws, n_dev


def render_raw(lib, a, s, pws, n_inst, iws, image, alpha, depth=None):
    """lfs_fastgs_view_render -> return code"""
    from lichtfeld_studio_amd.capi import ptr, stream
    return lib.lfs_fastgs_view_render(C.byref(view_of(a, s, pws)), C.c_int64(n_inst), ptr(iws), C.c_size_t(iws.numel()), ptr(image), ptr(alpha), ptr(depth), stream())


def backward_raw(lib, a, s, pws, iws, n_inst, gi, ga, alpha, dens, grads, gd=None, w2c_tail=None, adam=None):
    """lfs_fastgs_view_backward -> return code. grads: the six gradient buffers; gd: grad_depth; w2c_tail = (grad_w2c pointer, workspace pointer, workspace bytes), each
    as given (None: NULL); adam = (parameter, exp_avg, exp_avg_sq) with the hyper-parameters of a first Adam step."""
    from lichtfeld_studio_amd.capi import FastgsBackwardArgs, FastgsShRestAdam, ptr, stream
    tail = w2c_tail if w2c_tail is not None else (None, None, 0)
    fused = None
    if adam is not None:
        fused = FastgsShRestAdam(ptr(adam[0]), ptr(adam[1]), ptr(adam[2]), 1e-3, 0.9, 0.999, 1e-15, 1.0 / (1.0 - 0.9), 1.0 / (1.0 - 0.999) ** 0.5)
    args = FastgsBackwardArgs(n_inst, ptr(iws), iws.numel(), ptr(gi), ptr(ga), ptr(alpha), ptr(gd), ptr(dens), *[ptr(g) for g in grads], tail[0], tail[1], tail[2],
                              C.pointer(fused) if fused is not None else None)
    return lib.lfs_fastgs_view_backward(C.byref(view_of(a, s, pws)), C.byref(args), stream())


def render_and_backward_raw(lib, a, s, pws, n_dev, gi, ga):
    """the rest of the forward and the backward on a preprocessed workspace -> (image, alpha, n_instances, gradients, densification_info)"""
    from lichtfeld_studio_amd import fastgs
    from lichtfeld_studio_amd.capi import check
    N = a[0].shape[0]
    n_inst = int(n_dev.item())
    iws = instance_workspace(lib, s, n_inst)
    image, alpha = torch.empty((3, s.height, s.width), device=DEV), torch.empty((1, s.height, s.width), device=DEV)
    check(render_raw(lib, a, s, pws, n_inst, iws, image, alpha), "render")
    dens = torch.zeros(2, N, device=DEV)
    g = fastgs.backward_wrapper(dens, gi, ga, image, alpha, a[0], a[1], a[2], a[4], a[5], pws, iws, a[6], s, n_inst)
    return image, alpha, n_inst, g, dens
