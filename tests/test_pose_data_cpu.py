"""CPU: the host half of stlpose_amd/pose_data.py -- person tables from a COCO keypoint dict, the epoch's batches, the resident
store's capacity arithmetic -- and the yardstick's own consistency (tests/pose_batch_ref.py)."""
import json

import numpy as np
import pytest

from stlpose_amd.pose_data import PersonDB, ResidentImages, coco_person_db, epoch_indices
from tests import pose_batch_ref as R


def _kp(vis=2, zero=False):
    out = []
    for j in range(17):
        out += [0, 0, 0] if zero else [10 + j, 20 + 2 * j, vis if j % 3 else 1]
    return out


def _annotations():
    """Image 1 is 100 x 80 (w x h), image 2 is 64 x 48 and holds only rejected annotations, image 3 is 200 x 300."""
    images = [dict(id=1, file_name="a.jpg", width=100, height=80), dict(id=2, file_name="b.jpg", width=64, height=48),
              dict(id=3, file_name="c_alpha_0.5.jpg", width=200, height=300)]
    a = lambda i, im, bbox, **kw: dict(dict(id=i, image_id=im, category_id=1, iscrowd=0, area=100.0, bbox=bbox, keypoints=_kp()), **kw)  # noqa: E731
    anns = [
        a(1, 1, [10, 20, 61, 21]),                            # wider than 3:4 -> kept, row 0
        a(2, 1, [5, 5, 30, 30], iscrowd=1),                   # crowd
        a(3, 1, [5, 5, 30, 30], category_id=2),               # not a person
        a(4, 2, [5, 5, 30, 30], keypoints=_kp(zero=True)),    # no keypoints
        a(5, 1, [-4, 70, 200, 50]),                           # leaves the image: clipped to x 0 .. 99, y 70 .. 79 -> kept, row 1
        a(6, 2, [5, 5, 30, 30], area=0),                      # zero area
        a(7, 2, [70, 5, 10, 10]),                             # x1 = 70 beyond width - 1 = 63: x2 < x1
        a(8, 3, [20.5, 30.25, 31, 101]),                      # taller than 3:4 -> kept, row 2
    ]
    return dict(images=images, annotations=anns, categories=[dict(id=1, name="person"), dict(id=2, name="dog")])


def test_coco_person_db_keeps_and_converts_as_the_reference():
    db = coco_person_db(_annotations(), (192, 256), alpha="random", perceptual_loss={"a.jpg": 0.25, "c_alpha_0.5.jpg": 0.75})
    assert isinstance(db, PersonDB) and len(db) == 3
    assert [im["id"] for im in db.images] == [1, 3] and db.image_sizes() == [(80, 100), (300, 200)]
    assert db.image_index.tolist() == [0, 0, 1] and db.image_id.tolist() == [1, 1, 3]
    assert db.width.tolist() == [100, 100, 200] and db.height.tolist() == [80, 80, 300]
    assert db.score.tolist() == [1, 1, 1] and db.alpha.tolist() == [0, 0, 0.5] and db.perceptual_loss.tolist() == [0.25, 0.25, 0.75]
    assert db.joints.dtype == np.float64 and db.joints.shape == (3, 17, 3) and db.center.dtype == np.float32 and db.scale.dtype == np.float32
    assert db.joints[0, 4].tolist() == [14, 28, 0]
    # visibility 2 is clipped to 1, copied into columns 0 and 1, column 2 stays 0
    assert db.joints_vis[0, :, 0].tolist() == [1.0] * 17 and np.array_equal(db.joints_vis[..., 0], db.joints_vis[..., 1])
    assert not db.joints_vis[..., 2].any()
    # row 0: clean box (10, 20, 60, 20): centre (40, 30); 60 > 0.75 * 20, so h = 60 / 0.75 = 80; scale = (60, 80) / 200 * 1.25
    assert db.center[0].tolist() == [40.0, 30.0]
    assert np.array_equal(db.scale[0], np.array([60 / 200, 80 / 200], np.float32) * np.float32(1.25))
    # row 1: x1 = 0, x2 = min(99, 0 + 199) = 99, y1 = 70, y2 = min(79, 70 + 49) = 79: box (0, 70, 99, 9): centre (49.5, 74.5);
    # 99 > 0.75 * 9, h = 132
    assert db.center[1].tolist() == [49.5, 74.5]
    assert np.array_equal(db.scale[1], np.array([99 / 200, 99 / 0.75 / 200], np.float32) * np.float32(1.25))
    # row 2: box (20.5, 30.25, 30, 100): centre (35.5, 80.25); 30 < 0.75 * 100, so w = 75
    assert db.center[2].tolist() == [35.5, 80.25]
    assert np.array_equal(db.scale[2], np.array([75 / 200, 100 / 200], np.float32) * np.float32(1.25))


def test_coco_person_db_reads_a_file_and_defaults(tmp_path):
    path = tmp_path / "person_keypoints.json"
    path.write_text(json.dumps(_annotations()))
    a, b = coco_person_db(str(path), (192, 256)), coco_person_db(_annotations(), (192, 256), alpha=0.3)
    assert np.array_equal(a.center, b.center) and np.array_equal(a.joints, b.joints)
    assert a.alpha.tolist() == [0, 0, 0] and b.alpha.tolist() == [0.3] * 3 and not a.perceptual_loss.any()
    wide = coco_person_db(_annotations(), (256, 192))      # another aspect ratio: 4:3.  Row 2: 30 < 4/3 * 100 -> w = 133.33
    assert np.array_equal(wide.scale[2], np.array([100 * (256 / 192) / 200, 100 / 200], np.float32) * np.float32(1.25))
    bad = _annotations()
    bad["annotations"][0]["keypoints"] = [1, 1, 1] * 16
    with pytest.raises(ValueError, match="17"):
        coco_person_db(bad, (192, 256))
    with pytest.raises(KeyError):
        coco_person_db(_annotations(), (192, 256), perceptual_loss={"a.jpg": 1.0})


def test_epoch_indices_permutes_shards_and_drops_only_the_training_tail():
    n, batch = 45, 4
    one = epoch_indices(n, batch, seed=3, epoch=0)
    again = epoch_indices(n, batch, seed=3, epoch=0)
    other = epoch_indices(n, batch, seed=3, epoch=1)
    assert len(one) == 11 and all(len(b) == batch and b.dtype == np.int64 for b in one)
    assert all(np.array_equal(a, b) for a, b in zip(one, again))
    flat, flat_other = np.concatenate(one), np.concatenate(other)
    assert len(set(flat.tolist())) == 44 and set(flat.tolist()) <= set(range(n))
    assert not np.array_equal(flat, flat_other) and not np.array_equal(flat, np.concatenate(epoch_indices(n, batch, seed=4, epoch=0)))
    # validation: in order, the ragged tail stays
    val = epoch_indices(n, batch, seed=3, epoch=5, drop_last=False, shuffle=False)
    assert len(val) == 12 and np.array_equal(np.concatenate(val), np.arange(n)) and len(val[-1]) == 1
    # ranks: batches r, r + world, ...; disjoint, equal in count, together the permutation's batches
    whole = epoch_indices(48, batch, seed=3, epoch=2)                      # 12 batches
    parts = [epoch_indices(48, batch, seed=3, epoch=2, rank=r, world=3) for r in range(3)]
    assert [len(p) for p in parts] == [4, 4, 4]
    for r, p in enumerate(parts):
        assert all(np.array_equal(b, whole[r + 3 * i]) for i, b in enumerate(p))
    assert sorted(np.concatenate([np.concatenate(p) for p in parts]).tolist()) == list(range(48))
    # 11 batches over 3 ranks: every rank takes 3, the last two batches of the epoch are left out
    parts = [epoch_indices(n, batch, seed=3, epoch=0, rank=r, world=3) for r in range(3)]
    assert [len(p) for p in parts] == [3, 3, 3]
    assert np.array_equal(np.concatenate([parts[i % 3][i // 3] for i in range(9)]), flat[:36])
    with pytest.raises(ValueError):
        epoch_indices(n, batch, 0, 0, rank=3, world=3)


def test_resident_images_layout_and_capacity_message():
    sizes = [(4, 5), (1, 1), (480, 640)]
    offsets, hw, nbytes = ResidentImages.layout(sizes)
    assert offsets.tolist() == [0, 60, 63] and offsets.dtype == np.int64 and hw.dtype == np.int32 and hw.tolist() == [[4, 5], [1, 1], [480, 640]]
    assert nbytes == 60 + 3 + 480 * 640 * 3
    # 64 k images of 640 x 480: offsets beyond 2^31 stay exact
    big, _, total = ResidentImages.layout([(480, 640)] * 64000)
    assert total == 64000 * 921600 and int(big[-1]) == 63999 * 921600 > 2 ** 31
    ResidentImages.check_capacity(nbytes, (nbytes, 2 * nbytes))            # fits exactly
    with pytest.raises(MemoryError) as e:
        ResidentImages.check_capacity(total, (40_000_000_000, 300_000_000_000))
    msg = str(e.value)
    assert str(total) in msg and "40000000000" in msg and "StreamedImages" in msg
    with pytest.raises(MemoryError):                                        # the constructor asks before it allocates
        ResidentImages(sizes, device="cpu", mem_info=(100, 1000))
    with pytest.raises(ValueError):
        ResidentImages.layout([(0, 5)])


def test_the_yardstick_agrees_with_itself():
    """The exact rational fit reproduces the control points, the host's LU solve is within a few ulps of it, and the fixed test set
    holds every branch the GPU test asserts."""
    tables, _, _, draws = R.make_cases()
    out = R.replay(tables, np.arange(R.N_PERSONS), draws, True, R.PARAMS, (48, 64))
    for o in out:
        exact = R.exact_fit(o["img"], o["crop"])
        for p, q in zip(o["img"], o["crop"]):
            for k in range(2):
                assert exact[k][0] * R.Fraction(float(p[0])) + exact[k][1] * R.Fraction(float(p[1])) + exact[k][2] == R.Fraction(float(q[k]))
        assert R.fit_error(o["trans"], exact) <= 64 * np.spacing(np.abs(o["trans"]).max())
    assert {o["half"] for o in out} == {"off", "upper", "lower", "none"} and {o["flip"] for o in out} == {0, 1}
    quiet = R.replay(tables, np.arange(R.N_PERSONS), draws, False, R.PARAMS, (48, 64))
    assert all(o["flip"] == 0 and o["rot"] == 0.0 and np.array_equal(o["center"], tables[2][i].astype(np.float64))
               and np.array_equal(o["scale"], tables[3][i].astype(np.float64)) for i, o in enumerate(quiet))
