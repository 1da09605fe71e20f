"""Mirror of the reference's camera pose optimisation modules (src/training/components/poseopt.{hpp,cpp}): a learned rigid
correction per training camera, composed on the right of the stored world-to-camera transform. Plain torch modules - a handful of
parameters per camera, nothing here is a hot path; the gradient they are trained with (grad_w2c) comes out of the fastgs backward
(csrc/fastgs_prep.hip, fastgs.backward_wrapper(grad_w2c=...)).

Both modules start as the identity: the embeddings are zero and, in the MLP form, so are the last layer's weight and bias."""
from __future__ import annotations

import torch
import torch.nn.functional as F


def rotation_6d_to_matrix(rot_6d: torch.Tensor) -> torch.Tensor:
    """[..., 6] -> [..., 3, 3] (poseopt.cpp:12-20): Gram-Schmidt on the two 3-vectors, the third ROW is their cross product."""
    a1, a2 = rot_6d[..., :3], rot_6d[..., 3:]
    b1 = F.normalize(a1, dim=-1)
    b2 = F.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    b3 = torch.cross(b1, b2, dim=-1)
    return torch.stack((b1, b2, b3), dim=-2)


def _ids(embedding_ids, device) -> torch.Tensor:
    return torch.as_tensor(embedding_ids, dtype=torch.long, device=device).reshape(-1)


def _compose(camera_transforms: torch.Tensor, delta: torch.Tensor, rot_identity: torch.Tensor) -> torch.Tensor:
    """delta [B,9] = [translation(3) | rot6d(6) offset from the identity] -> camera_transforms @ [[R_delta, t], [0, 1]]"""
    bs = camera_transforms.shape[0]
    rot = rotation_6d_to_matrix(delta[..., 3:] + rot_identity.expand(bs, -1))
    top = torch.cat((rot, delta[..., :3].unsqueeze(-1)), dim=-1)                                   # [B,3,4]
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=top.dtype, device=top.device).expand(bs, 1, 4)
    return torch.matmul(camera_transforms, torch.cat((top, bottom), dim=-2))


class DirectPoseOptimization(torch.nn.Module):
    """poseopt.cpp:22-44: Embedding(n_cameras, 9), zero-initialised; one row IS the camera's delta."""

    def __init__(self, n_cameras: int):
        super().__init__()
        self.camera_embeddings = torch.nn.Embedding(n_cameras, 9)
        torch.nn.init.zeros_(self.camera_embeddings.weight)
        self.register_buffer("rot_identity", torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]))

    def forward(self, camera_transforms: torch.Tensor, embedding_ids) -> torch.Tensor:
        return _compose(camera_transforms, self.camera_embeddings(_ids(embedding_ids, camera_transforms.device)), self.rot_identity)


class MLPPoseOptimization(torch.nn.Module):
    """poseopt.cpp:45-75: Embedding(n_cameras, width) zeros -> depth x (Linear(width, width) + ReLU) -> Linear(width, 9) with zero weight and bias."""

    def __init__(self, n_cameras: int, width: int = 64, depth: int = 2):
        super().__init__()
        self.camera_embeddings = torch.nn.Embedding(n_cameras, width)
        torch.nn.init.zeros_(self.camera_embeddings.weight)
        self.register_buffer("rot_identity", torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]))
        layers = []
        for _ in range(depth):
            layers += [torch.nn.Linear(width, width), torch.nn.ReLU()]
        last = torch.nn.Linear(width, 9)
        torch.nn.init.zeros_(last.weight)
        torch.nn.init.zeros_(last.bias)
        self.mlp = torch.nn.Sequential(*layers, last)

    def forward(self, camera_transforms: torch.Tensor, embedding_ids) -> torch.Tensor:
        return _compose(camera_transforms, self.mlp(self.camera_embeddings(_ids(embedding_ids, camera_transforms.device))), self.rot_identity)


def make_pose_module(kind: str, n_cameras: int):
    """"none" -> None; "direct" | "mlp" -> the module (trainer.cpp:366-389)."""
    if kind == "none":
        return None
    if kind == "direct":
        return DirectPoseOptimization(n_cameras)
    if kind == "mlp":
        return MLPPoseOptimization(n_cameras)
    raise ValueError(f"Invalid pose optimization type: {kind}")
