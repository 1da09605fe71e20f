"""Shared by tests/test_gpu_lean_step.py (the device) and tests/test_emulated_lean_step.py (the wavefront emulator): scenes, one driver of the one-call training step
through the C ABI over either backend, and the bitwise comparisons. The lean fused-tail step (csrc/gut_step.hip: FwdLean) leaves out work whose result it never reads -
the activated quaternions / scales / opacities are recomputed by the tail kernel instead of stored and read back, the per-tile sort writes no keys, the count no
tiles_per_gauss - and none of that may change a bit of what the step computes. (The backward's accumulator clear as a rider of the scan launch was built with these,
measured and taken out again - profiles/r20/lean_step; its cases stay, and hold the memset that stayed: whatever clears the rows, no step may see the sums of the one before.)

Every comparison is on the bytes (integer views): a NaN a crafted row produces has to be the same NaN on both sides."""
import ctypes as C
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opac")
W, H, TILE = 40, 24, 16            # partial tiles in both directions
FOCAL = 32.0


def _structs():
    src = open(os.path.join(ROOT, "lichtfeld-studio_amd", "gut_step.py")).read()
    ns = {}
    exec("import ctypes as C\n" + src[src.index("class StepArgs"):src.index("class GutStep")], ns)   # (the module itself imports the GPU library loader)
    return ns["StepArgs"], ns["StepLayout"], ns["StepOptions"]


StepArgs, StepLayout, StepOptions = _structs()


def kmat(w=W, h=H, f=FOCAL):
    return np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]], np.float32)


def viewmat(shift=(0.0, 0.0, 0.0), angle=0.0):
    """world -> camera: a rotation by `angle` about y, then a translation"""
    m = np.eye(4, dtype=np.float64)
    c, s = np.cos(angle), np.sin(angle)
    m[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    m[:3, 3] = shift
    return m.astype(np.float32)


def scene(seed, N, K, degree, crafted=False, w=W, h=H):
    """N Gaussians inside the frustum of the identity view (all of them seen by it), depths 2 .. 6. crafted (N >= 6): rows at the places where the activations and
    their backward branch - an all-zero quaternion, one of norm 1e-20 (both below the 1e-12 clamp of the normalisation), raw scales of -104 (exp underflows to a
    denormal) and +60 (1e26), raw opacities of +90 (sigmoid rounds to 1: o (1 - o) = 0) and -90 (sigmoid 8e-40, a denormal)."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(2.0, 6.0, N)
    means = np.stack([rng.uniform(-1, 1, N) * z * 0.5 * (w / 2) / FOCAL, rng.uniform(-1, 1, N) * z * 0.5 * (h / 2) / FOCAL, z], 1).astype(np.float32)
    quats = rng.standard_normal((N, 4)).astype(np.float32)
    raw_scales = np.log(rng.uniform(0.05, 0.3, (N, 3))).astype(np.float32)
    opac = rng.uniform(0.3, 0.9, N)
    raw_opac = np.log(opac / (1 - opac)).astype(np.float32)
    if crafted:
        assert N >= 6
        quats[0] = 0.0
        quats[1] = (1e-20, 0.0, 0.0, 0.0)
        raw_scales[2] = (-104.0, raw_scales[2, 1], raw_scales[2, 2])
        raw_scales[3] = (60.0, raw_scales[3, 1], raw_scales[3, 2])
        raw_opac[4], raw_opac[5] = 90.0, -90.0
    return dict(means=means, raw_quats=quats, raw_scales=raw_scales, raw_opac=raw_opac, sh0=(rng.standard_normal((N, 1, 3)) * 0.5).astype(np.float32),
                shN=(rng.standard_normal((N, K - 1, 3)) * 0.2).astype(np.float32), K=K, degree=degree, N=N, W=w, H=h,
                target=rng.random((3, h, w)).astype(np.float32), bg=rng.random(3).astype(np.float32), noise=rng.standard_normal((N, 3)).astype(np.float32))


def stacked_scene(n_stack, equal_depths, seed=3):
    """A 32 x 16 image = two tiles. n_stack small Gaussians sit on the centre of tile 0 (footprints of ~2 pixels: tile 0 only), one on tile 1: tile 0's list has exactly
    n_stack entries. equal_depths: one depth for all of them - every key of the tile ties on the depth bits (the order is the tie-break by id) and falls into one bin
    of the counting sort, which then goes through the bitonic network (BIN_LIMIT)."""
    sc = scene(seed, n_stack + 1, 4, 1, w=32, h=16)
    N = n_stack + 1
    rng = np.random.default_rng(seed + 1)
    z = np.full(N, 4.0) if equal_depths else rng.permutation(N) * 1e-4 + 3.0   # distinct, unordered (a narrow range: far away, these small Gaussians fall below the 1/255 opacity cut)
    px = np.where(np.arange(N) < n_stack, 8.0, 24.0) + rng.uniform(-0.5, 0.5, N)
    py = 8.0 + rng.uniform(-0.5, 0.5, N)
    sc["means"] = np.stack([(px - 16.0) / FOCAL * z, (py - 8.0) / FOCAL * z, z], 1).astype(np.float32)
    sc["raw_scales"][:] = np.log(0.01)
    sc["raw_opac"][:] = 0.0
    return sc


class Backend:
    """numpy + the emulated library, or torch on the device + the shipped one: allocation, pointers, the way back to numpy"""

    def __init__(self, lib, torch=None, device=None, stream=None):
        self.lib, self.torch, self.device, self._stream = lib, torch, device, stream

    def put(self, a):
        a = np.ascontiguousarray(a)
        return a.copy() if self.torch is None else self.torch.from_numpy(a.copy()).to(self.device).contiguous()

    def full_bytes(self, n, value):
        return np.full(n, value, np.uint8) if self.torch is None else self.torch.full((n,), value, dtype=self.torch.uint8, device=self.device)

    def ptr(self, x):
        return C.c_void_p(None if x is None else x.ctypes.data if self.torch is None else x.data_ptr())

    def get(self, x):
        if self.torch is None:
            return x.copy()
        self.torch.cuda.synchronize()
        return x.cpu().numpy().copy()

    def stream(self):
        return None if self._stream is None else self._stream()


class Run:
    """the six parameters, their moments and one step workspace: what a caller of the C ABI keeps"""

    def __init__(self, be, sc, capacity=None, assumed_longest=1 << 20, fill=0xFF):
        self.be, self.sc, self.lib = be, sc, be.lib
        self.N = sc["N"]
        self.params = [be.put(sc[k]) for k in NAMES]
        self.m = [be.put(np.zeros_like(sc[k])) for k in NAMES]
        self.v = [be.put(np.zeros_like(sc[k])) for k in NAMES]
        self.K, self.bg, self.target, self.noise = be.put(kmat(sc["W"], sc["H"])), be.put(sc["bg"]), be.put(sc["target"]), be.put(sc["noise"])
        self.loss = be.put(np.zeros(1, np.float32))
        self.capacity = capacity if capacity is not None else 64 * self.N + 1024
        self.assumed_longest = assumed_longest
        self.fill = fill
        self.ws, self.lay, self.ws_capacity = None, None, None
        self.stamp = 0
        self.vm_keep = []

    def workspace(self, capacity):
        """(re)allocated when the capacity changes; filled with 0xFF bytes (NaN as float): the step must not rely on what a workspace holds"""
        if self.ws_capacity != capacity:
            lay = StepLayout()
            sc = self.sc
            assert self.lib.lfs_gut_step_layout_for(C.c_uint32(self.N), C.c_uint32(sc["W"]), C.c_uint32(sc["H"]), C.c_uint32(TILE), C.c_int64(capacity), C.byref(lay)) == 0
            self.ws, self.lay, self.ws_capacity = self.be.full_bytes(int(lay.bytes) + 64, self.fill), lay, capacity
        return self.ws, self.lay

    def state(self):
        g = self.be.get
        return dict(params=[g(p) for p in self.params], m=[g(x) for x in self.m], v=[g(x) for x in self.v])

    def load(self, st):
        for k in range(6):
            for dst, src in ((self.params[k], st["params"][k]), (self.m[k], st["m"][k]), (self.v[k], st["v"][k])):
                if self.be.torch is None:
                    dst[...] = src
                else:
                    dst.copy_(self.be.torch.from_numpy(src))

    def step(self, it, vm, form, next_vm=None, colors_ready=False, freeze=False, noise=False, capacity=None):
        """one call of lfs_gut_train_step (form "three"), lfs_gut_train_step_ex ("fused") or lfs_gut_train_step_opt ("opt": freeze / noise) -> (fitted, loss, counts)"""
        sc, be, lib = self.sc, self.be, self.lib
        cap = capacity if capacity is not None else self.capacity
        ws, lay = self.workspace(cap)
        vm_d = be.put(vm)
        nxt_d = None if next_vm is None else be.put(next_vm)
        self.vm_keep = [vm_d, nxt_d]
        a = StepArgs()
        a.N, a.K, a.sh_degree, a.image_width, a.image_height, a.tile_size = self.N, sc["K"], sc["degree"], sc["W"], sc["H"], TILE
        a.means, a.sh0, a.shN, a.raw_scales, a.raw_quats, a.raw_opacities = [be.ptr(p).value for p in self.params]
        for k in range(6):
            if not (freeze and k == 2):
                a.exp_avg[k], a.exp_avg_sq[k] = be.ptr(self.m[k]).value, be.ptr(self.v[k]).value
            t = it + 1
            for j, val in enumerate((1e-2 if k else 1e-3, 0.9, 0.999, 1e-15, 1.0 / (1.0 - 0.9 ** t), 1.0 / np.sqrt(1.0 - 0.999 ** t))):
                a.adam[k][j] = val
        a.viewmat, a.Kmat, a.background, a.target_chw = be.ptr(vm_d).value, be.ptr(self.K).value, be.ptr(self.bg).value, be.ptr(self.target).value
        a.loss_weight, a.scale_reg, a.opacity_reg, a.loss = 1.0, 0.01, 0.01, be.ptr(self.loss).value
        self.stamp += 1
        tail = (C.c_int64(cap), C.c_int64(self.assumed_longest), be.ptr(ws), C.c_size_t(int(lay.bytes)), None, C.c_int64(self.stamp), be.stream())   # (counts: the workspace's own)
        if form == "three":
            rc = lib.lfs_gut_train_step(C.byref(a), *tail)
        elif form == "fused":
            rc = lib.lfs_gut_train_step_ex(C.byref(a), be.ptr(nxt_d), C.c_int(int(colors_ready)), *tail)
        else:
            o = StepOptions()
            o.freeze_shN = int(freeze)
            if noise:
                o.noise, o.noise_lr = be.ptr(self.noise).value, NOISE_LR
            rc = lib.lfs_gut_train_step_opt(C.byref(a), C.byref(o), be.ptr(nxt_d), C.c_int(int(colors_ready)), *tail)
        assert rc == 0, rc
        counts = self.view("counts", np.int64, (3,))
        assert counts[2] == self.stamp
        fitted = bool(lib.lfs_gut_step_fits(C.c_int64(int(counts[0])), C.c_int64(int(counts[1])), C.c_int64(cap), C.c_int64(self.assumed_longest)))
        return fitted, self.be.get(self.loss)[0], counts

    def view(self, name, dtype, shape):
        off, n = getattr(self.lay, name), int(np.prod(shape)) * np.dtype(dtype).itemsize
        return self.be.get(self.ws[off:off + n]).view(dtype).reshape(shape)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def assert_same_state(a, b, what, skip=()):
    for k, name in enumerate(NAMES):
        for part in ("params", "m", "v"):
            if (name, part) in skip:
                continue
            x, y = bits(a[part][k]), bits(b[part][k])
            assert np.array_equal(x, y), (what, name, part, int((x != y).sum()), np.argwhere(x != y)[:4].tolist())


def assert_same_loss(la, lb, what):
    """The loss VALUE, on its bits - on the device as on the emulator. The backward adds one partial sum per wavefront into slot (4 x workgroup + wavefront) & 255 with a
    float atomic, and both tails fold the 256 slots in one fixed order. The images of these tests have 6 tiles (40 x 24) or 2 (32 x 16): fewer wavefronts than slots, so
    every slot receives at most one add onto the zero the clear left and no sum depends on an arrival order (at 320 x 192, tests/test_gpu_gut_step.py, slots are shared
    and the value is held to 1e-5 instead). A stale slot of the step before shows in the last bit."""
    assert bits(np.float32(la)) == bits(np.float32(lb)), (what, la, lb)


def assert_lean_blocks(run, lean, what):
    """The workspace started as 0xFF bytes. After a lean step (fused tail, K <= 16) the blocks of the activated quaternions / scales / opacities still hold them: the
    projection kernel stored nothing there. After any other form they are written (a quiet fall-back of the lean step to the storing path shows here, not only in a
    byte counter)."""
    N = run.N
    for name, width in (("quats", 16), ("scales", 12), ("opacities", 4)):
        block = run.view(name, np.uint8, (N * width,))
        if lean:
            assert (block == 0xFF).all(), (what, name, "written by a lean step")
        else:
            assert not (block == 0xFF).all(), (what, name, "not written")


NOISE_LR = 0.05


def noise_displacement(st, noise, lr):
    """float64: what lfs_add_noise adds to the means (csrc/lfs_mcmc_noise.cuh) - lr * sigmoid(-100 (opacity - 0.005)) * (R diag(exp(2 raw_scale)) R^T) noise"""
    with np.errstate(all="ignore"):
        q = st["params"][4].astype(np.float64)
        q = q / np.sqrt((q * q).sum(1, keepdims=True))
        w, x, y, z = q.T
        R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
                      np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1),
                      np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)
        s2 = np.exp(2.0 * st["params"][3].astype(np.float64))
        cov = np.einsum("nij,nj,nkj->nik", R, s2, R)
        op = 1.0 / (1.0 + np.exp(-st["params"][5].astype(np.float64)))
        nf = lr / (1.0 + np.exp(100.0 * op - 0.5))
        return nf[:, None] * np.einsum("nij,nj->ni", cov, noise.astype(np.float64))


# ---- 1. activations recomputed by the tail ------------------------------------------------------------------------------------------------------------------------
VIEWS = (viewmat(), viewmat(shift=(0.15, -0.05, 0.3), angle=0.06))


def check_activations(be, N, degree, mode="plain", seed=0):
    """Two steps over two views, the fused-tail step (the second one on the colours the first one's tail handed over: colors_ready) against lfs_gut_train_step, whose
    three passes read the activated values the projection kernel stored. mode "freeze" / "noise" (lfs_gut_train_step_opt; the three-pass form has neither): the
    reference is taken step by step from the fused run's state before the step, and what it cannot show is compared for what it must be - freeze: shN and its moments
    keep their bytes, everything else is the three-pass step's; noise: the noise moves the means only (it is added in front of their Adam update, the gradient is that
    of the mean the forward rendered), so every moment and the other five parameters are the three-pass step's bit for bit, and the means are its means plus the
    displacement of the noise up to the rounding of adding three floats in another order. (The means under noise are the one comparison of these tests that is not on
    the bits: the library has no second form of the noised update to take them from - the three-pass step has no noise, and Adam after the noise is not the noise after
    Adam in floating point. They are held to a float64 model of lfs_add_noise within the bar derived below; the gradient that moves them is held bitwise through the
    means' two moments.)"""
    K = (degree + 1) ** 2
    sc = scene(1000 * N + 10 * degree + seed, N, K, degree, crafted=True)
    f, r = Run(be, sc), Run(be, sc)
    ready = False
    moved = 0
    for it in range(2):
        vm, nxt = VIEWS[it % 2], VIEWS[(it + 1) % 2]
        before = f.state()
        if mode == "plain":
            fit_f, loss_f, cnt_f = f.step(it, vm, "fused", next_vm=nxt, colors_ready=ready)
        else:
            r.load(before)
            fit_f, loss_f, cnt_f = f.step(it, vm, "opt", next_vm=nxt, colors_ready=ready, freeze=mode == "freeze", noise=mode == "noise")
        fit_r, loss_r, cnt_r = r.step(it, vm, "three")
        assert fit_f and fit_r and int(cnt_f[0]) == int(cnt_r[0]) > 0
        ready = True
        sf, sr = f.state(), r.state()
        what = f"N={N} degree={degree} {mode} step {it}"
        if mode == "plain":
            assert_same_state(sf, sr, what)
        elif mode == "freeze":
            assert_same_state(sf, sr, what, skip=[("shN", "params"), ("shN", "m"), ("shN", "v")])
            assert_same_state(sf, before, what + " frozen shN", skip=[(n, p) for n in NAMES if n != "shN" for p in ("params", "m", "v")])
        else:
            assert_same_state(sf, sr, what, skip=[("means", "params")])
            delta = noise_displacement(before, sc["noise"], NOISE_LR)
            mf, mr = sf["params"][0].astype(np.float64), sr["params"][0].astype(np.float64)
            ok = np.isfinite(delta) & np.isfinite(mf) & np.isfinite(mr)
            assert ok[6:].all(), "a random row is not finite"
            assert np.abs(delta[ok]).max() > 1e-4, "the noise moved nothing"
            # (mean + noise) - update against (mean - update) + noise: one rounding of each intermediate, eps32 x (|mean| + |noise| + |update|, the update at most a
            # few lr = 1e-3), twice over; the displacement itself is evaluated here in float64 from fp32 operands the kernel rounds ~20 times on the way: 1e-5 of it
            bar = 4 * 2.0 ** -24 * (np.abs(mr) + np.abs(delta) + 1e-2) + 1e-5 * np.abs(delta)
            err = np.abs(mf - (mr + delta))
            assert (err[ok] <= bar[ok]).all(), (what, float((err[ok] / bar[ok]).max()))
        assert_same_loss(loss_f, loss_r, what)
        assert_lean_blocks(f, True, what + " fused")
        assert_lean_blocks(r, False, what + " three-pass")
        # the next view's colours, as the tail wrote them (what step it + 1 renders with) against the SH colour kernel of a fresh three-pass forward: compared through
        # the next step's results above; here directly for the last step
        moved += int((bits(sf["m"][3]) != 0).sum())
    assert moved > N, "no gradient reached the scales"
    return f, r


def check_next_colours(be, N, degree):
    """the colours the fused tail leaves for the next view = the SH colour kernel's for that view on the updated parameters (lfs_gut_view_forward on another workspace)"""
    K = (degree + 1) ** 2
    sc = scene(77 + N, N, K, degree, crafted=True)
    f = Run(be, sc)
    fit, _, _ = f.step(0, VIEWS[0], "fused", next_vm=VIEWS[1])
    assert fit
    tail_colours = f.view("colors", np.float32, (N, 3))
    g = Run(be, sc)
    g.load(f.state())
    a = StepArgs()
    a.N, a.K, a.sh_degree, a.image_width, a.image_height, a.tile_size = N, K, degree, sc["W"], sc["H"], TILE
    a.means, a.sh0, a.shN, a.raw_scales, a.raw_quats, a.raw_opacities = [be.ptr(p).value for p in g.params]
    vm_d = be.put(VIEWS[1])
    a.viewmat, a.Kmat, a.background = be.ptr(vm_d).value, be.ptr(g.K).value, be.ptr(g.bg).value
    ws, lay = g.workspace(g.capacity)
    rc = be.lib.lfs_gut_view_forward(C.byref(a), C.c_int64(g.capacity), C.c_int64(1 << 20), be.ptr(ws), C.c_size_t(int(lay.bytes)), None, C.c_int64(1), be.stream())
    assert rc == 0
    assert np.array_equal(bits(tail_colours), bits(g.view("colors", np.float32, (N, 3))))


# ---- 2. the accumulator clear between two steps -------------------------------------------------------------------------------------------------------------------
ALL_SEEN, HALF_BEHIND = viewmat(), viewmat(shift=(0.0, 0.0, -4.0))   # the second camera stands at depth 4: the Gaussians in front of it (2 .. 4) are behind its image plane


def check_clear(be, N, overflow=False):
    """Step k on a view that sees every Gaussian (every accumulator row and the loss slots are written), step k + 1 on a view that has half of them behind the camera:
    a row the clear missed would feed the stale sums of step k into step k + 1's update of a Gaussian nothing touched, a missed loss slot into its loss. The
    workspace starts as 0xFF bytes (NaN), so the first step shows a missed clear as well. Against lfs_gut_train_step on a workspace of its own.
    overflow: step k + 1 is first attempted with a capacity of 8 - nothing may be updated - and then run again."""
    sc = scene(500 + N, N, 4, 1)
    f, r = Run(be, sc), Run(be, sc)
    for it, vm in enumerate((ALL_SEEN, HALF_BEHIND)):
        if overflow and it == 1:
            before = f.state()
            fit, _, cnt = f.step(it, vm, "fused", capacity=8)
            assert not fit and int(cnt[0]) > 8
            assert_same_state(f.state(), before, f"N={N} overflowing attempt")
        fit_f, loss_f, cnt_f = f.step(it, vm, "fused")
        fit_r, loss_r, cnt_r = r.step(it, vm, "three")
        assert fit_f and fit_r and int(cnt_f[0]) == int(cnt_r[0]) > 0
        radii = f.view("radii", np.int32, (N, 2))
        seen = int(((radii > 0).all(1)).sum())
        if it == 0:
            assert seen == N, (seen, N)
        elif N > 1:
            assert 0 < seen < N, (seen, N)
        sf, sr = f.state(), r.state()
        assert_same_state(sf, sr, f"N={N} step {it}")
        assert all(np.isfinite(x).all() for part in ("params", "m", "v") for x in sf[part]), "NaN: a part of the workspace the step read before it wrote it"
        assert np.isfinite(loss_f) and loss_f > 0
        assert_same_loss(loss_f, loss_r, f"N={N} step {it}")


def check_clear_with_float_atomics(be, N):
    """The same without the deterministic mode (whose backward clears a second array and runs other kernels): float atomics and all. Two runs of a step then
    differ in the last bits of every row that received a sum - but not in the rows that received none: a Gaussian behind the camera of step k + 1 takes an update from
    the regularisers and its moments alone, the same bits in every run, unless its accumulator row still holds step k's sums (or the 0xFF the workspace started with).
    Step k + 1 of the three-pass form starts from the fused run's state after step k."""
    sc = scene(900 + N, N, 4, 1)
    f, r = Run(be, sc), Run(be, sc)
    fit, loss0, _ = f.step(0, ALL_SEEN, "fused")
    assert fit and np.isfinite(loss0) and loss0 > 0
    r.step(0, ALL_SEEN, "three")           # (its workspace has been through a step as well)
    r.load(f.state())
    fit_f, loss_f, _ = f.step(1, HALF_BEHIND, "fused")
    fit_r, loss_r, _ = r.step(1, HALF_BEHIND, "three")
    assert fit_f and fit_r
    unseen = ~(f.view("radii", np.int32, (N, 2)) > 0).all(1)
    assert np.array_equal(unseen, ~(r.view("radii", np.int32, (N, 2)) > 0).all(1))
    if N > 1:
        assert 0 < int(unseen.sum()) < N
    sf, sr = f.state(), r.state()
    for part in ("params", "m", "v"):
        for k, name in enumerate(NAMES):
            assert np.isfinite(sf[part][k]).all(), (name, part)
            assert np.array_equal(bits(sf[part][k])[unseen], bits(sr[part][k])[unseen]), (name, part)
    assert np.isfinite(loss_f)
    assert_same_loss(loss_f, loss_r, f"N={N} float atomics")   # (the render both backwards take their loss from is the forward's: no atomics in it)


# ---- 3. the per-tile sort without the key write-back ---------------------------------------------------------------------------------------------------------------
def check_sort(be, n_stack, equal_depths):
    """flatten_ids and tile_offsets the step left in its workspace against lfs_intersect_tile_count / _emit (which write the keys) on the projection outputs of the
    same workspace."""
    sc = stacked_scene(n_stack, equal_depths)
    N, lib = sc["N"], be.lib
    f = Run(be, sc, capacity=2 * N + 64, assumed_longest=max(n_stack, 8))
    fit, _, cnt = f.step(0, viewmat(), "fused")
    assert fit and int(cnt[1]) == n_stack, (cnt, n_stack)
    n_isects = int(cnt[0])
    T = 2
    offs = f.view("tile_offsets", np.int32, (T + 1,))
    assert offs.tolist() == [0, n_stack, n_stack + 1] and n_isects == n_stack + 1
    flat = f.view("flatten_ids", np.int32, (n_isects,))
    radii, means2d, depths = f.view("radii", np.int32, (N, 2)), f.view("means2d", np.float32, (N, 2)), f.view("depths", np.float32, (N,))
    d_radii, d_m2, d_depths = be.put(radii), be.put(means2d), be.put(depths)
    lib.lfs_intersect_tile_workspace_bytes.restype = C.c_size_t
    wsb = int(lib.lfs_intersect_tile_workspace_bytes(C.c_uint32(1), C.c_uint32(N), C.c_uint32(2), C.c_uint32(1)))
    iws = be.full_bytes(wsb, 0)
    tpg, n_dev = be.put(np.zeros(N, np.int32)), be.put(np.zeros(1, np.int64))
    rc = lib.lfs_intersect_tile_count(C.c_uint32(1), C.c_uint32(N), be.ptr(d_m2), be.ptr(d_radii), C.c_uint32(TILE), C.c_uint32(2), C.c_uint32(1), be.ptr(tpg), be.ptr(n_dev),
                                      be.ptr(iws), C.c_size_t(wsb), be.stream())
    assert rc == 0 and int(be.get(n_dev)[0]) == n_isects
    ids, flat_ref, offs_ref = be.put(np.zeros(n_isects, np.int64)), be.put(np.zeros(n_isects, np.int32)), be.put(np.zeros(T, np.int32))
    rc = lib.lfs_intersect_tile_emit(C.c_uint32(1), C.c_uint32(N), be.ptr(d_m2), be.ptr(d_radii), be.ptr(d_depths), C.c_uint32(TILE), C.c_uint32(2), C.c_uint32(1), C.c_int(1),
                                     C.c_int64(n_isects), be.ptr(tpg), be.ptr(ids), be.ptr(flat_ref), be.ptr(offs_ref), be.ptr(iws), C.c_size_t(wsb), be.stream())
    assert rc == 0
    flat_ref, ids, offs_ref = be.get(flat_ref), be.get(ids), be.get(offs_ref)
    assert np.array_equal(offs[:T], offs_ref)
    assert (np.diff(ids) >= 0).all(), "the operator's keys are not sorted"
    assert np.array_equal(flat, flat_ref), np.argwhere(flat != flat_ref)[:4].tolist()
    if equal_depths:   # the tie-break: ascending id
        assert np.array_equal(flat[:n_stack], np.arange(n_stack))
    # and the lean path was taken: isect_ids still holds what the scatter parked there, (depth bits << 32 | id) per tile bucket in some order - not the reference's
    # (tile << 32 | depth bits) keys, whose upper word would be the tile index 0 or 1
    parked = f.view("isect_ids", np.uint64, (n_isects,))
    dbits = bits(depths)
    for t in range(T):
        b = parked[offs[t]:offs[t + 1]]
        ids_t = (b & np.uint64(0xFFFFFFFF)).astype(np.int64)
        assert np.array_equal(np.sort(ids_t), np.sort(flat[offs[t]:offs[t + 1]])), t
        assert np.array_equal((b >> np.uint64(32)).astype(np.uint32), dbits[ids_t]), t
    assert not np.array_equal(parked.view(np.int64), ids), "the step wrote the keys"
