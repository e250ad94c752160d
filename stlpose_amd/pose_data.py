"""HRNet training / validation batches built on the GPU from COCO person annotations (reference ``data/HRNet_Coco.py`` +
``data/JointsDataset.py`` + the ``DataLoader`` of ``data/data_loaders.py``).

Three parts:

  * ``coco_person_db``: a COCO keypoint file -> one table row per kept person (``HRNet_Coco.py:156-248``), host numpy.  pycocotools
    is not a dependency: the JSON is read directly, so the reading order and the filters are this module's reading of
    ``pycocotools.coco.COCO`` (images in file order, an image's annotations in file order).  Parity with pycocotools is UNPINNED in
    the same sense as the AP code's: nothing here was compared with it.
  * ``ResidentImages`` / ``StreamedImages``: where the decoded uint8 images live.  Resident: all of them packed once into one
    device buffer (COCO train2017's person images are tens of GB, which fits in HBM), so a batch copies nothing.  Streamed: one
    batch's distinct images are uploaded per call, which waits for the copy.
  * ``PoseBatchLoader``: per batch three launches -- ``pose_augment`` (the per-person augmentation arithmetic, csrc/pose_batch.hip),
    ``affine_crop`` (the warp) and ``gaussian_targets`` (the heat maps) -- and no per-person Python.  With ``ResidentImages`` the
    host never waits for the device between the first and the last batch of an epoch.

Decoding image files stays the caller's (``ResidentImages.from_files`` takes a ``decode`` callable), and so do the detection-result
boxes of ``HRNet_Coco._load_coco_person_detection_results``.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import capi, ops  # noqa: F401  (ops registers the stlpose:: custom ops)
from .augment import IMAGENET_MEAN, IMAGENET_STD

NUM_JOINTS = capi.POSE_JOINTS
JOINTS_WEIGHT = (1., 1., 1., 1., 1., 1., 1., 1.2, 1.2, 1.5, 1.5, 1., 1., 1.2, 1.2, 1.5, 1.5)   # HRNet_Coco.py:101-104
PIXEL_STD = 200


# ---------------------------------------------------------------------------------------------------------------- person tables
@dataclass
class PersonDB:
    """One row per person.  ``images[k]`` = {"id", "file_name", "width", "height"} of the k-th distinct image that has a person."""
    joints: np.ndarray            # (N, 17, 3) float64, z = 0
    joints_vis: np.ndarray        # (N, 17, 3) float64: visibility clipped to 1 in columns 0 and 1, column 2 = 0
    center: np.ndarray            # (N, 2) float32
    scale: np.ndarray             # (N, 2) float32, in units of 200 px
    image_index: np.ndarray       # (N,) int64 into `images`
    image_id: np.ndarray          # (N,) int64
    width: np.ndarray             # (N,) int32: the source image's
    height: np.ndarray            # (N,) int32
    score: np.ndarray             # (N,) float64, 1 for ground-truth boxes
    alpha: np.ndarray             # (N,) float64 (HRNet_Coco.py:203-208)
    perceptual_loss: np.ndarray   # (N,) float64, 0 without a dictionary
    images: List[dict] = field(default_factory=list)
    image_size: Tuple[int, int] = (192, 256)   # (W, H) of the crop

    def __len__(self) -> int:
        return int(self.joints.shape[0])

    def image_sizes(self) -> List[Tuple[int, int]]:
        """(height, width) of every distinct image, for ``ResidentImages.from_files``."""
        return [(int(im["height"]), int(im["width"])) for im in self.images]


def xywh2cs(x, y, w, h, aspect_ratio: float) -> Tuple[np.ndarray, np.ndarray]:
    """HRNet_Coco.py:233-248: the centre in float32, the box widened to the crop's aspect ratio in Python floats, / 200 rounded to
    float32, times 1.25 in float32."""
    center = np.zeros(2, dtype=np.float32)
    center[0] = x + w * 0.5
    center[1] = y + h * 0.5
    if w > aspect_ratio * h:
        h = w * 1.0 / aspect_ratio
    elif w < aspect_ratio * h:
        w = h * aspect_ratio
    scale = np.array([w * 1.0 / PIXEL_STD, h * 1.0 / PIXEL_STD], dtype=np.float32)
    if center[0] != -1:
        scale = scale * np.float32(1.25)
    return center, scale


def coco_person_db(annotations, image_size: Sequence[int], alpha=None, perceptual_loss: Optional[Dict[str, float]] = None) -> PersonDB:
    """``annotations``: the parsed COCO keypoint JSON (a dict with "images", "annotations" and optionally "categories") or its
    path.  ``image_size`` = (W, H) of the crop.  ``alpha``: a number stored with every row, or "random" to read it from file names
    that carry ``alpha_<value>.jpg`` (HRNet_Coco.py:203-208).  ``perceptual_loss``: file name -> precomputed loss
    (JointsDataset.py:146-148; a missing name is a KeyError, as there)."""
    if isinstance(annotations, (str, os.PathLike)):
        with open(annotations) as f:
            annotations = json.load(f)
    w_out, h_out = int(image_size[0]), int(image_size[1])
    aspect_ratio = w_out * 1.0 / h_out
    person_ids = {c["id"] for c in annotations.get("categories", []) if c.get("name") == "person"} or {1}
    by_image: Dict[int, list] = {}
    for ann in annotations["annotations"]:
        by_image.setdefault(ann["image_id"], []).append(ann)
    cols: Dict[str, list] = {k: [] for k in ("joints", "vis", "center", "scale", "image_index", "image_id", "width", "height", "alpha", "perc")}
    images: List[dict] = []
    for im in annotations["images"]:
        width, height = im["width"], im["height"]
        name = os.path.basename(im.get("file_name", ""))
        slot = None
        for obj in by_image.get(im["id"], []):
            if obj.get("iscrowd", 0):
                continue
            x, y, w, h = obj["bbox"]
            x1, y1 = max(0, x), max(0, y)                                    # :167-170
            x2 = min(width - 1, x1 + max(0, w - 1))
            y2 = min(height - 1, y1 + max(0, h - 1))
            if not (obj["area"] > 0 and x2 >= x1 and y2 >= y1):
                continue
            if obj["category_id"] not in person_ids:
                continue
            kp = obj["keypoints"]
            if len(kp) != 3 * NUM_JOINTS:
                raise ValueError(f"coco_person_db: annotation {obj.get('id')} has {len(kp) // 3} keypoints; the pipeline is built for {NUM_JOINTS}")
            if max(kp) == 0:
                continue
            k = np.asarray(kp, np.float64).reshape(NUM_JOINTS, 3)
            joints = np.zeros((NUM_JOINTS, 3), np.float64)
            joints[:, :2] = k[:, :2]
            vis = np.zeros((NUM_JOINTS, 3), np.float64)
            vis[:, 0] = vis[:, 1] = np.minimum(k[:, 2], 1.0)
            c, s = xywh2cs(x1, y1, x2 - x1, y2 - y1, aspect_ratio)
            if slot is None:
                slot = len(images)
                images.append({"id": int(im["id"]), "file_name": im.get("file_name", ""), "width": int(width), "height": int(height)})
            if alpha == "random" and "alpha" in name:
                a = float(name.split("alpha_")[-1].split(".jpg")[0])
            else:
                a = float(alpha) if alpha is not None and alpha != "random" else 0.0
            for key, v in (("joints", joints), ("vis", vis), ("center", c), ("scale", s), ("image_index", slot), ("image_id", int(im["id"])),
                           ("width", int(width)), ("height", int(height)), ("alpha", a),
                           ("perc", float(perceptual_loss[name]) if perceptual_loss else 0.0)):
                cols[key].append(v)
    n = len(cols["joints"])

    def arr(key, dtype, tail):
        return np.asarray(cols[key], dtype).reshape((n,) + tail)
    return PersonDB(joints=arr("joints", np.float64, (NUM_JOINTS, 3)), joints_vis=arr("vis", np.float64, (NUM_JOINTS, 3)),
                    center=arr("center", np.float32, (2,)), scale=arr("scale", np.float32, (2,)),
                    image_index=arr("image_index", np.int64, ()), image_id=arr("image_id", np.int64, ()),
                    width=arr("width", np.int32, ()), height=arr("height", np.int32, ()), score=np.ones(n, np.float64),
                    alpha=arr("alpha", np.float64, ()), perceptual_loss=arr("perc", np.float64, ()), images=images,
                    image_size=(w_out, h_out))


def epoch_indices(n: int, batch: int, seed: int, epoch: int, rank: int = 0, world: int = 1, drop_last: bool = True,
                  shuffle: bool = True) -> List[np.ndarray]:
    """The batches of one epoch for one rank, a pure function of its arguments: the permutation of ``(seed, epoch)`` (the identity
    without ``shuffle``) cut into batches of ``batch``; ``drop_last`` drops a ragged tail.  Rank r gets batches r, r + world, ...
    Every rank gets the same number of batches -- each training step holds a collective -- so the last ``batches % world`` batches
    of the epoch are left out."""
    if batch < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"epoch_indices: batch {batch}, rank {rank} of {world}")
    order = np.random.default_rng([int(seed), int(epoch)]).permutation(n) if shuffle else np.arange(n)
    order = order.astype(np.int64)
    nb = n // batch if drop_last else -(-n // batch)
    nb -= nb % world
    return [order[i * batch:min((i + 1) * batch, n)] for i in range(rank, nb, world)]


# ---------------------------------------------------------------------------------------------------------------- image stores
def _check_image(im: np.ndarray, where) -> np.ndarray:
    im = np.asarray(im)
    if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
        raise ValueError(f"image {where}: must be uint8 HWC RGB, got {im.dtype} {im.shape}")
    return np.ascontiguousarray(im)


class ResidentImages:
    """Every decoded image packed into ONE uint8 device buffer, with the (offset, height / width) tables stl_affine_crop reads.
    ``rows`` gathers the two small tables on the device: no image byte moves and the host does not wait."""
    device_resident = True

    def __init__(self, sizes: Sequence[Tuple[int, int]], device="cuda", mem_info: Optional[Tuple[int, int]] = None):
        """Allocates the buffer for images of the given (height, width); ``put`` fills it.  ``mem_info`` = (free, total) bytes
        instead of asking the device (for tests)."""
        self.device = torch.device(device)
        self.offsets_host, self.hw_host, self.nbytes = self.layout(sizes)
        self.check_capacity(self.nbytes, mem_info if mem_info is not None else torch.cuda.mem_get_info(self.device))
        self.buffer = torch.empty(max(self.nbytes, 1), dtype=torch.uint8, device=self.device)
        self.offsets = torch.from_numpy(self.offsets_host).to(self.device)
        self.hw = torch.from_numpy(self.hw_host).to(self.device)

    @staticmethod
    def layout(sizes: Sequence[Tuple[int, int]]) -> Tuple[np.ndarray, np.ndarray, int]:
        """(byte offset int64 [K], (height, width) int32 [K, 2], total bytes) of images packed back to back, 3 bytes per pixel."""
        hw = np.asarray(sizes, np.int64).reshape(-1, 2)
        if (hw < 1).any() or (hw >= 1 << 31).any():
            raise ValueError("ResidentImages: every image side must be in 1 .. 2^31 - 1")
        nbytes = hw[:, 0] * hw[:, 1] * 3
        offsets = (np.cumsum(nbytes) - nbytes).astype(np.int64)
        return offsets, hw.astype(np.int32), int(nbytes.sum())

    @staticmethod
    def check_capacity(nbytes: int, mem_info: Tuple[int, int]) -> None:
        free, total = int(mem_info[0]), int(mem_info[1])
        if nbytes > free:
            raise MemoryError(f"ResidentImages: the decoded images take {nbytes} bytes, the device has {free} bytes free (of {total}); "
                              "use StreamedImages, which uploads one batch's images at a time")

    def __len__(self) -> int:
        return int(self.hw_host.shape[0])

    def put(self, k: int, image: np.ndarray) -> None:
        im = _check_image(image, k)
        if tuple(im.shape[:2]) != tuple(int(v) for v in self.hw_host[k]):
            raise ValueError(f"image {k}: decoded to {im.shape[:2]}, the store was sized for {tuple(int(v) for v in self.hw_host[k])}")
        a = int(self.offsets_host[k])
        self.buffer[a:a + im.size].copy_(torch.from_numpy(im.reshape(-1)))

    @classmethod
    def from_arrays(cls, arrays: Sequence[np.ndarray], device="cuda", mem_info=None) -> "ResidentImages":
        arrays = [_check_image(a, k) for k, a in enumerate(arrays)]
        self = cls([a.shape[:2] for a in arrays], device, mem_info)
        for k, a in enumerate(arrays):
            self.put(k, a)
        return self

    @classmethod
    def from_files(cls, paths: Sequence[str], decode: Callable[[str], np.ndarray], sizes: Optional[Sequence[Tuple[int, int]]] = None,
                   device="cuda", mem_info=None) -> "ResidentImages":
        """``decode(path)`` -> HWC uint8 RGB array.  With ``sizes`` ((height, width) per path, e.g. ``PersonDB.image_sizes()``) the
        buffer is allocated first and each image goes to the device as soon as it is decoded; without, every image is decoded
        first and held on the host until the buffer is filled."""
        if sizes is None:
            return cls.from_arrays([decode(p) for p in paths], device, mem_info)
        if len(sizes) != len(paths):
            raise ValueError(f"ResidentImages.from_files: {len(paths)} paths, {len(sizes)} sizes")
        self = cls(sizes, device, mem_info)
        for k, p in enumerate(paths):
            self.put(k, decode(p))
        return self

    def rows(self, image_indices: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """image_indices: int64 device tensor.  (buffer, offsets int64 [B], hw int32 [B, 2])."""
        return self.buffer, self.offsets.index_select(0, image_indices), self.hw.index_select(0, image_indices)


class StreamedImages:
    """For datasets that do not fit on the device: the images stay on the host (arrays, or paths with a ``decode`` callable) and
    ``rows`` uploads the distinct images of one batch.  That copy SYNCHRONISES the host with the device on every call."""
    device_resident = False

    def __init__(self, get: Callable[[int], np.ndarray], count: int, device="cuda"):
        self._get, self._count, self.device = get, int(count), torch.device(device)

    @classmethod
    def from_arrays(cls, arrays: Sequence[np.ndarray], device="cuda") -> "StreamedImages":
        arrays = [_check_image(a, k) for k, a in enumerate(arrays)]
        return cls(lambda k: arrays[k], len(arrays), device)

    @classmethod
    def from_files(cls, paths: Sequence[str], decode: Callable[[str], np.ndarray], device="cuda") -> "StreamedImages":
        paths = list(paths)
        return cls(lambda k: _check_image(decode(paths[k]), paths[k]), len(paths), device)

    def __len__(self) -> int:
        return self._count

    def rows(self, image_indices) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """image_indices: host integers.  (buffer of this batch's distinct images, offsets int64 [B], hw int32 [B, 2])."""
        idx = np.asarray(image_indices, np.int64).reshape(-1)
        distinct, inverse = np.unique(idx, return_inverse=True)
        ims = [self._get(int(k)) for k in distinct]
        sizes = np.asarray([im.size for im in ims], np.int64)
        starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        hw = np.asarray([im.shape[:2] for im in ims], np.int32).reshape(-1, 2)
        flat = np.concatenate([im.reshape(-1) for im in ims]) if ims else np.zeros(1, np.uint8)
        return (torch.from_numpy(flat).to(self.device), torch.from_numpy(starts[inverse]).to(self.device),
                torch.from_numpy(np.ascontiguousarray(hw[inverse])).to(self.device))


# ---------------------------------------------------------------------------------------------------------------- the loader
class PoseBatchLoader:
    """An iterable of ``(imgs (B, 3, H, W) f32, target (B, 17, H/4, W/4) f32, target_weight (B, 17, 1) f32, meta)`` on the device,
    what ``Trainer.train_epoch`` and ``Evaluator.evaluate_model`` consume.  The crop size is ``db.image_size``; the heat maps are
    a quarter of it (HRNet's output stride).  ``exp_data["dataset"]`` gives ``scale_factor``, ``rot_factor``, ``flip``,
    ``num_joints_half_body`` and ``prob_half_body`` (JointsDataset.py:51-55).

    Every ``iter()`` is a new epoch (``set_epoch`` chooses it): its permutation (``epoch_indices``) and its random draws (a device
    generator seeded from ``(seed, epoch, rank)``) are made before the first batch, so the same ``(seed, epoch)`` gives the same
    batches bit for bit.  The training loader shuffles and drops the ragged last batch (``TrainStep`` has a fixed batch); the
    validation loader does neither.

    ``meta``: ``image_id``, ``score``, ``index`` (host arrays), ``perceptual_loss`` (CPU tensor), ``batch_index`` (the batch's
    number in the whole epoch, over all ranks); validation adds ``center`` / ``scale`` as host float64 arrays from the table
    (nothing is copied back); training adds ``center`` / ``scale`` / ``rotation`` / ``joints`` / ``joints_vis`` as device tensors.
    ``loader.last`` holds the augmentation kernel's inputs and outputs of the batch just made (its ``index``, ``draws``, ``minv``,
    ``flip``, ...), so that a batch can be replayed."""

    def __init__(self, db: PersonDB, images, exp_data: dict, batch_size: int, is_train: bool, seed: int = 0, rank: int = 0,
                 world: int = 1, sigma: float = 2.0, joints_weight: Sequence[float] = JOINTS_WEIGHT, device="cuda"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("PoseBatchLoader (HIP) needs a GPU device; there is no CPU path")
        if db.joints.shape[1:] != (NUM_JOINTS, 3) or len(joints_weight) != NUM_JOINTS:
            raise ValueError(f"PoseBatchLoader: the augmentation kernel is built for {NUM_JOINTS} joints, got tables of {db.joints.shape[1]} "
                             f"and {len(joints_weight)} joint weights")
        if len(db) == 0:
            raise ValueError("PoseBatchLoader: the person table is empty")
        if len(images) <= int(db.image_index.max()):
            raise ValueError(f"PoseBatchLoader: the table refers to image {int(db.image_index.max())}, the store holds {len(images)}")
        self.db, self.images, self.device = db, images, dev
        self.batch_size, self.is_train = int(batch_size), bool(is_train)
        self.seed, self.rank, self.world, self.sigma, self.epoch = int(seed), int(rank), int(world), float(sigma), 0
        ds = exp_data["dataset"]
        self.scale_factor, self.rot_factor = float(ds["scale_factor"]), float(ds["rot_factor"])
        self.flip = bool(ds["flip"])
        self.num_joints_half_body, self.prob_half_body = int(ds["num_joints_half_body"]), float(ds["prob_half_body"])
        self.image_size = (int(db.image_size[0]), int(db.image_size[1]))           # (W, H)
        if self.image_size[0] % 4 or self.image_size[1] % 4:
            raise ValueError(f"PoseBatchLoader: crop {self.image_size} is no multiple of the output stride 4")
        if "image_size" in ds and tuple(int(v) for v in ds["image_size"]) != (self.image_size[1], self.image_size[0]):
            raise ValueError(f"PoseBatchLoader: exp_data's image_size (H, W) = {tuple(ds['image_size'])}, the table was built for "
                             f"(W, H) = {self.image_size}")
        self.heatmap_size = (self.image_size[0] // 4, self.image_size[1] // 4)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)           # noqa: E731
        self._tables = (up(db.joints), up(db.joints_vis), up(db.center), up(db.scale), up(db.width))
        self._image_index = up(db.image_index)
        self._joints_weight = torch.tensor([float(v) for v in joints_weight], dtype=torch.float32, device=dev).view(1, NUM_JOINTS, 1)
        self._mean, self._std = torch.tensor(IMAGENET_MEAN, device=dev), torch.tensor(IMAGENET_STD, device=dev)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def _batches(self, epoch: int) -> List[np.ndarray]:
        return epoch_indices(len(self.db), self.batch_size, self.seed, epoch, self.rank, self.world, drop_last=self.is_train,
                             shuffle=self.is_train)

    def __len__(self) -> int:
        n, b = len(self.db), self.batch_size
        nb = n // b if self.is_train else -(-n // b)
        nb -= nb % self.world
        return len(range(self.rank, nb, self.world))

    def __iter__(self):
        """Everything the epoch needs from the host goes up here, before the first batch: the indices, and the draws' seed."""
        epoch, self.epoch = self.epoch, self.epoch + 1
        batches = self._batches(epoch)
        total = int(sum(len(b) for b in batches))
        index = torch.from_numpy(np.concatenate(batches) if batches else np.zeros(0, np.int64)).to(self.device)
        if self.is_train:
            gen = torch.Generator(device=self.device)
            gen.manual_seed(int(np.random.SeedSequence([self.seed, epoch, self.rank]).generate_state(1, np.uint64)[0] >> np.uint64(1)))
            u = torch.rand(total, 3, dtype=torch.float64, device=self.device, generator=gen)
            g = torch.randn(total, 3, dtype=torch.float64, device=self.device, generator=gen)
            draws = torch.stack([u[:, 0], g[:, 0], g[:, 1], u[:, 1], g[:, 2], u[:, 2]], 1).contiguous()   # u_half n_half n_scale u_rot n_rot u_flip
        else:
            draws = torch.zeros(total, 6, dtype=torch.float64, device=self.device)
        image_index = self._image_index.index_select(0, index) if self.images.device_resident else None
        return self._produce(batches, index, draws, image_index)

    def _produce(self, batches, index, draws, image_index):
        db, (w, h) = self.db, self.image_size
        pos = 0
        for i, rows in enumerate(batches):
            a, pos = pos, pos + len(rows)
            idx = index[a:pos]
            with torch.cuda.device(self.device):
                center, scale, rot, flip, trans, minv, joints, joints_vis, joints_xy, vis0 = torch.ops.stlpose.pose_augment(
                    *self._tables, idx, draws[a:pos], self.is_train, self.flip, self.scale_factor, self.rot_factor,
                    self.num_joints_half_body, self.prob_half_body, w, h)
                # what the kernel read and wrote for the batch just made (device tensors, a few hundred bytes per person)
                self.last = dict(index=idx, draws=draws[a:pos], center=center, scale=scale, rot=rot, flip=flip, trans=trans, minv=minv,
                                 joints=joints, joints_vis=joints_vis, joints_xy=joints_xy, vis0=vis0)
                src, off, hw = self.images.rows(image_index[a:pos] if image_index is not None else db.image_index[rows])
                imgs = torch.ops.stlpose.affine_crop(src, off, hw, minv, flip, h, w, self._mean, self._std)
                target, tw = torch.ops.stlpose.gaussian_targets(joints_xy, vis0, self.heatmap_size[1], self.heatmap_size[0],
                                                                float(w) / self.heatmap_size[0], float(h) / self.heatmap_size[1],
                                                                self.sigma)
            target_weight = tw.view(-1, NUM_JOINTS, 1) * self._joints_weight       # JointsDataset.py:283-284
            meta = {"image_id": db.image_id[rows], "score": db.score[rows], "index": rows,
                    "perceptual_loss": torch.from_numpy(db.perceptual_loss[rows]), "batch_index": self.rank + self.world * i}
            if self.is_train:
                meta.update(center=center, scale=scale, rotation=rot, joints=joints, joints_vis=joints_vis)
            else:
                meta.update(center=db.center[rows].astype(np.float64), scale=db.scale[rows].astype(np.float64))
            yield imgs, target, target_weight, meta
