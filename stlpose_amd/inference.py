"""Forward wrapper (mirror of reference ``src/lib/inference.py``), flip-test kept on device."""
from __future__ import annotations

import torch

from . import capi, ops  # noqa: F401  (ops registers the stlpose:: custom ops)

FLIP_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]  # CONSTANTS.py:65


def _perm(j: int, device) -> torch.Tensor:
    p = list(range(j))
    for a, b in FLIP_PAIRS:
        if a < j and b < j:
            p[a], p[b] = b, a
    return torch.tensor(p, dtype=torch.int32, device=device)


def forward_pass(model, img, model_name="HRNet", device=None, flip=False):
    """reference lib/inference.py:11-32.  flip=True: second forward on img.flip(3); flip_back
    (lib/transforms.py:147-164: reverse W, swap L/R joints), 1-px right shift with column 0 kept,
    average -- done by one HIP kernel instead of a device->numpy->device round trip.  Differentiable with respect to `img` in eval
    mode (one batch of 2B, see below); in training mode with flip=True, backward raises the stale-forward error."""
    if model_name != "HRNet":
        raise NotImplementedError("Wrong model name. Only ['HRNet'] supported")
    if flip is True and img.requires_grad and torch.is_grad_enabled() and not model.training:
        # Differentiable flip test (eval mode): a plan keeps ONE set of activations, so the image and its mirror run as one batch
        # -- eval-mode BatchNorm is per sample, the heat maps are those of the two calls -- and flip_merge's autograd formula
        # (stl_flip_merge_backward) carries the gradient back to both halves.  (In training mode the two forwards below share a
        # plan and backward through the first raises the stale-forward error of PoseHighResolutionNet.)
        both = model(torch.cat([img, img.flip(3)]))
        b = img.shape[0]
        return torch.ops.stlpose.flip_merge(both[:b], both[b:], _perm(both.shape[1], both.device))
    output = model(img)
    if flip is True:
        of = model(img.flip(3))
        output = torch.ops.stlpose.flip_merge(output, of, _perm(output.shape[1], output.device))   # custom op -> stl_flip_merge
    return output
