"""CPU: the camera pose optimisation modules (lichtfeld-studio_amd/poseopt.py, mirror of the reference's src/training/components/poseopt.cpp).
Plain torch modules: nothing here needs the HIP library."""
import numpy as np
import pytest
import torch


def _poseopt():
    import lichtfeld_studio_amd  # noqa: F401
    from lichtfeld_studio_amd import poseopt
    return poseopt


def _rot6d_f64(r):
    """float64 restatement: Gram-Schmidt, rows b1, b2, b1 x b2"""
    r = np.asarray(r, np.float64)
    a1, a2 = r[..., :3], r[..., 3:]
    b1 = a1 / np.linalg.norm(a1, axis=-1, keepdims=True)
    b2 = a2 - (b1 * a2).sum(-1, keepdims=True) * b1
    b2 = b2 / np.linalg.norm(b2, axis=-1, keepdims=True)
    return np.stack([b1, b2, np.cross(b1, b2)], axis=-2)


def _transforms(b, seed=0):
    g = torch.Generator().manual_seed(seed)
    T = torch.zeros(b, 4, 4)
    T[:, :3, :3] = torch.from_numpy(_rot6d_f64(torch.randn(b, 6, generator=g).numpy())).float()
    T[:, :3, 3] = torch.randn(b, 3, generator=g)
    T[:, 3, 3] = 1.0
    return T


def test_rotation_6d_to_matrix_is_a_rotation_and_matches_float64():
    p = _poseopt()
    g = torch.Generator().manual_seed(1)
    r = torch.randn(64, 6, generator=g)
    r[:8] = torch.tensor([1.0, 0, 0, 0, 1, 0]) + 1e-2 * torch.randn(8, 6, generator=g)   # near the identity: where training lives
    R = p.rotation_6d_to_matrix(r)
    assert R.shape == (64, 3, 3)
    Rd = R.double().numpy()
    assert np.abs(Rd @ Rd.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6
    assert np.abs(np.linalg.det(Rd) - 1.0).max() < 1e-6
    assert np.abs(Rd - _rot6d_f64(r.numpy())).max() < 1e-6
    assert torch.equal(p.rotation_6d_to_matrix(torch.tensor([1.0, 0, 0, 0, 1, 0])), torch.eye(3))
    assert p.rotation_6d_to_matrix(torch.randn(2, 5, 6, generator=g)).shape == (2, 5, 3, 3)      # leading dimensions pass through


@pytest.mark.parametrize("kind", ["direct", "mlp"])
def test_zero_initialised_modules_return_the_camera_transforms_exactly(kind):
    p = _poseopt()
    torch.manual_seed(3)
    mod = p.make_pose_module(kind, 5)
    T = _transforms(3)
    out = mod(T, [4, 0, 2])
    assert out.shape == (3, 4, 4) and torch.equal(out, T)
    assert torch.equal(mod(T[1:2], torch.tensor([3])), T[1:2])          # ids as a tensor, as the reference passes them
    assert float(mod.camera_embeddings.weight.detach().abs().max()) == 0
    if kind == "mlp":
        assert tuple(mod.camera_embeddings.weight.shape) == (5, 64)
        lin = [m for m in mod.mlp if isinstance(m, torch.nn.Linear)]
        assert [(l.in_features, l.out_features) for l in lin] == [(64, 64), (64, 64), (64, 9)]
        assert float(lin[-1].weight.detach().abs().max()) == 0 and float(lin[-1].bias.detach().abs().max()) == 0
        assert float(lin[0].weight.detach().abs().max()) > 0
    else:
        assert tuple(mod.camera_embeddings.weight.shape) == (5, 9)


def test_direct_module_composes_on_the_right():
    """delta = [t | rot6d offset]: result = camera_transforms @ [[R(rot6d + identity), t], [0, 1]]"""
    p = _poseopt()
    mod = p.DirectPoseOptimization(3)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        mod.camera_embeddings.weight.copy_(0.1 * torch.randn(3, 9, generator=g))
    T = _transforms(2, seed=7)
    out = mod(T, [2, 1]).detach().double().numpy()
    w = mod.camera_embeddings.weight.detach().double().numpy()
    for b, cam in enumerate([2, 1]):
        D = np.eye(4)
        D[:3, :3] = _rot6d_f64(w[cam, 3:] + np.array([1.0, 0, 0, 0, 1, 0]))
        D[:3, 3] = w[cam, :3]
        assert np.abs(out[b] - T[b].double().numpy() @ D).max() < 1e-6
    assert np.abs(out[:, 3] - np.array([0, 0, 0, 1.0])).max() == 0


@pytest.mark.parametrize("kind", ["direct", "mlp"])
def test_gradients_reach_only_the_indexed_embedding_row(kind):
    p = _poseopt()
    torch.manual_seed(11)
    mod = p.make_pose_module(kind, 6)
    if kind == "mlp":   # (behind the zero last layer nothing reaches the embedding yet: give it a weight)
        with torch.no_grad():
            mod.mlp[-1].weight.normal_(0, 0.1)
    T = _transforms(1, seed=2)
    out = mod(T, [4])
    g = torch.Generator().manual_seed(13)
    out.backward(torch.randn(1, 4, 4, generator=g))
    grad = mod.camera_embeddings.weight.grad
    assert float(grad[4].abs().max()) > 0
    assert float(grad[[0, 1, 2, 3, 5]].abs().max()) == 0
    # ... and an Adam step moves that row alone
    opt = torch.optim.Adam(mod.parameters(), lr=1e-5)
    opt.step()
    w = mod.camera_embeddings.weight.detach()
    assert float(w[4].abs().max()) > 0 and float(w[[0, 1, 2, 3, 5]].abs().max()) == 0


def test_make_pose_module_kinds():
    p = _poseopt()
    assert p.make_pose_module("none", 3) is None
    assert isinstance(p.make_pose_module("direct", 3), p.DirectPoseOptimization)
    assert isinstance(p.make_pose_module("mlp", 3), p.MLPPoseOptimization)
    with pytest.raises(ValueError):
        p.make_pose_module("sideways", 3)
