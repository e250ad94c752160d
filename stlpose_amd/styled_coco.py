"""Styled-COCO producer: COCO images through ``AdaINStylizer`` with a set of style images (vase paintings in the paper), written
where the reference reads them -- ``<data_path>/images_style_{styles}_alpha_{alpha}/{split}/<file name>``
(``src/data/data_loaders.py:83-100``) -- and, in the same pass, the per-image perceptual losses of
``perceptual_offline.create_offline_perceptual_loss`` (``lib/loss.py:153-198``).

No reference counterpart: the reference reads these files, the code that makes them is not in its tree.  PARITY UNPINNED.
Image file decoding is the caller's: images come in as arrays or tensors.
"""
from __future__ import annotations

import os
import random
from typing import Callable, Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch

from . import capi
from .perceptual_offline import create_offline_perceptual_loss


def styled_dir(data_path: str, styles_tag, alpha, split: str = "train") -> str:
    """Directory ``data_loaders.py:84`` reads the stylised images from."""
    return os.path.join(data_path, f"images_style_{styles_tag}_alpha_{alpha}", split)


def pil_writer(path: str, image: np.ndarray) -> None:
    """Default writer: ``image`` uint8 HWC -> file at `path`, format by its extension."""
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("create_styled_dataset: the default writer needs PIL (Pillow) to encode image files; "
                           "install it or pass writer=callable(path, uint8 HWC array)") from e
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(image).save(path)


def to_chw_float(image) -> torch.Tensor:
    """uint8 HWC (array or tensor) or float CHW in [0, 1] -> float32 CHW in [0, 1] (on the image's device)."""
    t = torch.as_tensor(image)
    if t.dtype == torch.uint8:
        if t.dim() != 3 or t.shape[2] != 3:
            raise ValueError(f"uint8 images must be HWC with 3 channels, got {tuple(t.shape)}")
        return t.permute(2, 0, 1).float() / 255.0
    if t.dim() != 3 or t.shape[0] != 3:
        raise ValueError(f"float images must be CHW with 3 channels, got {tuple(t.shape)}")
    return t.float()


def to_hwc_uint8(image: torch.Tensor) -> np.ndarray:
    """float CHW in [0, 1] -> uint8 HWC, rounded to nearest."""
    return (image.clamp(0.0, 1.0) * 255.0 + 0.5).floor().to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy()


def fit_size(H: int, W: int) -> Tuple[int, int]:
    """The next multiple of 8 below (or at) each side: the size an image is stylised at."""
    return H - H % 8, W - W % 8


def _resize(x: torch.Tensor, Ho: int, Wo: int) -> torch.Tensor:
    """[B,3,H,W] on the GPU -> [B,3,Ho,Wo], bilinear (align_corners=False) by stl_bilinear_nchw."""
    B, _, H, W = x.shape
    if (H, W) == (Ho, Wo):
        return x
    x = x.contiguous()
    out = torch.empty(B, 3, Ho, Wo, device=x.device)
    capi.call("stl_bilinear_nchw", x.data_ptr(), out.data_ptr(), B, 3, H, W, Ho, Wo, torch.cuda.current_stream().cuda_stream)
    return out


@torch.no_grad()
def create_styled_dataset(stylizer, images: Iterable[Tuple[str, object]], styles: List[torch.Tensor], data_path: str, styles_tag, alpha,
                          seed: int = 0, batch: int = 16, split: str = "train", vgg=None, dict_path: Optional[str] = None,
                          writer: Optional[Callable[[str, np.ndarray], None]] = None, device="cuda") -> Dict[str, dict]:
    """Stylise `images` and write them as the reference's Styled-COCO directory.

    images: iterable of (file_name, uint8 HWC or float CHW image in [0, 1]).  styles: list of style images ([3,h,w] or [1,3,h,w],
    sizes multiples of 8), prepared once (``stylizer.prepare_style``).  Each image gets ONE style, drawn by
    ``random.Random(seed)`` in iteration order.  Consecutive images of equal size are stylised as one batch of up to `batch`.
    An image whose height or width is not a multiple of 8 is resized DOWN to the next multiple (bilinear, align_corners=False,
    ``stl_bilinear_nchw``) before it is stylised and is written at that size; sides below 16 raise ValueError.

    Output: ``writer(path, uint8 HWC array)`` with path = ``data_path/images_style_{styles_tag}_alpha_{alpha}/{split}/{file_name}``;
    the default writer encodes with PIL.  With `vgg` (a ``VGGPerceptualLoss``) and `dict_path`, the (stylised, original) pairs --
    the original at the stylised size -- also go through ``create_offline_perceptual_loss``, which writes
    ``dict_path/perceptual_loss_dict_alpha_{alpha}_styles_{styles_tag}.json``.  Returns {file_name: {"style": index, "path": path}}.
    """
    if (vgg is None) != (dict_path is None):
        raise ValueError("create_styled_dataset: vgg and dict_path go together")
    if not styles:
        raise ValueError("create_styled_dataset: no style images")
    if batch < 1:
        raise ValueError(f"create_styled_dataset: batch must be at least 1, got {batch}")
    writer = writer or pil_writer
    dev = torch.device(device)
    out_dir = styled_dir(data_path, styles_tag, alpha, split)
    rng = random.Random(seed)
    prepared = [stylizer.prepare_style((s if s.dim() == 4 else s.unsqueeze(0)).to(dev, torch.float32)) for s in styles]
    mean_s = torch.cat([p[0] for p in prepared])   # [S, C]
    sigma_s = torch.cat([p[1] for p in prepared])
    manifest: Dict[str, dict] = {}

    def flush(group):
        names, idxs, imgs = zip(*group)
        x = torch.stack([im.to(dev) for im in imgs])
        x = _resize(x, *fit_size(x.shape[2], x.shape[3]))
        sel = torch.tensor(idxs, device=mean_s.device)
        out = stylizer.stylise(x, (mean_s[sel], sigma_s[sel]), alpha=float(alpha), clamp=True)
        for name, k, styled, orig in zip(names, idxs, out, x):
            path = os.path.join(out_dir, name)
            writer(path, to_hwc_uint8(styled))
            manifest[name] = {"style": k, "path": path}
            yield name, styled, orig

    def produce():
        """(file name, stylised CHW, original CHW at the stylised size), batch by batch."""
        group, size = [], None
        for name, image in images:
            im = to_chw_float(image)
            if min(im.shape[1:]) < 16:
                raise ValueError(f"create_styled_dataset: image {name!r} is {im.shape[1]}x{im.shape[2]}; sides of at least 16 are needed")
            if group and (tuple(im.shape) != size or len(group) >= batch):
                yield from flush(group)
                group = []
            size = tuple(im.shape)
            group.append((name, rng.randrange(len(styles)), im))
        if group:
            yield from flush(group)

    if vgg is not None:
        create_offline_perceptual_loss(produce(), vgg, dict_path, alpha, styles_tag, device=dev)
    else:
        for _ in produce():
            pass
    return manifest
