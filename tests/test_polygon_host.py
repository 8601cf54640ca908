"""myolo.polygon (skimage.draw.polygon restated) against outputs of the real function (tests/golden/polygon_fixture.npz, written by
tests/golden/make_polygon_fixture.py with scikit-image 0.18.3), the sampled form against resize_mask, and myolo.via.VIADataset."""
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_FX = {}


def fixture_cases():
    """-> dict(names, verts (list of [k,2]), frames, masks (list of bool [h,w]), fx): read once, shared, left unchanged."""
    if not _FX:
        fx = np.load(os.path.join(GOLDEN, "polygon_fixture.npz"), allow_pickle=False)
        bits = np.unpackbits(fx["bits"])
        off, frames = fx["off"], fx["frames"]
        masks, verts, o = [], [], 0
        for k in range(len(fx["names"])):
            h, w = int(frames[k][0]), int(frames[k][1])
            m = bits[o:o + h * w].reshape(h, w).astype(bool)
            m.setflags(write=False)
            masks.append(m)
            verts.append(fx["verts"][off[k]:off[k + 1]])
            o += h * w
        _FX.update(names=[str(n) for n in fx["names"]], verts=verts, frames=frames, masks=masks, fx=fx)
    return _FX


def test_fixture_holds_what_it_should():
    c = fixture_cases()
    fx = c["fx"]
    assert str(fx["skimage_version"]) == "0.18.3"
    assert int(fx["n_real"]) == 228 and len(c["names"]) >= 228 + 190
    chunk = int(fx["lds_chunk"])
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "mask-yolo_amd", "csrc", "segment_kernels.hip")).read()
    assert "#define SEG_CHUNK %d " % chunk in src                 # the chunk the long outlines were cut for is the kernel's
    lens = {n: len(v) for n, v in zip(c["names"], c["verts"])}
    for d in (-1, 0, 1):
        assert lens["syn/chunk%+d/0" % d] == chunk + d
    assert lens["syn/long1500/0"] == 1500 and lens["syn/one_int/0"] == 1 and lens["syn/two/0"] == 2
    assert not c["masks"][c["names"].index("syn/outside/0")].any()
    assert c["masks"][c["names"].index("syn/one_int/0")].sum() == 1 and not c["masks"][c["names"].index("syn/one_float/0")].any()
    assert os.path.getsize(os.path.join(GOLDEN, "polygon_fixture.npz")) < 1 << 20


def test_polygon_mask_equals_scikit_image_bit_for_bit():
    from myolo.polygon import polygon, polygon_mask
    c = fixture_cases()
    for name, v, frame, want in zip(c["names"], c["verts"], c["frames"], c["masks"]):
        got = polygon_mask(v[:, 0], v[:, 1], frame)
        assert got.dtype == bool and got.shape == want.shape
        assert np.array_equal(got, want), (name, int((got != want).sum()))
    # (rr, cc) in scikit-image's order: the cases whose index lists were stored as the real function returned them
    fx = c["fx"]
    first, rc_off = int(fx["order_first"]), fx["rc_off"]
    assert len(rc_off) - 1 >= 30
    nonempty = 0
    for j in range(len(rc_off) - 1):
        k = first + j
        rr, cc = polygon(c["verts"][k][:, 0], c["verts"][k][:, 1], c["frames"][k])
        assert rr.dtype == np.intp and cc.dtype == np.intp
        assert np.array_equal(rr, fx["rr"][rc_off[j]:rc_off[j + 1]]) and np.array_equal(cc, fx["cc"][rc_off[j]:rc_off[j + 1]]), c["names"][k]
        nonempty += len(rr) > 1
    assert nonempty >= 20
    # integer lists are taken as they are, like the reference passes them
    k = c["names"].index("real/food/val/0/0")
    v = c["verts"][k]
    assert np.array_equal(polygon_mask([int(a) for a in v[:, 0]], [int(a) for a in v[:, 1]], c["frames"][k]), c["masks"][k])
    assert not polygon_mask([], [], (4, 5)).any()
    with pytest.raises(ValueError):
        polygon_mask([1, 2], [1], (4, 5))
    with pytest.raises(ValueError):
        polygon_mask([1, np.nan, 3], [1, 2, 3], (4, 5))


@pytest.mark.parametrize("net", [(40, 56), (224, 224), (97, 131), (150, 300)])
def test_sampled_fill_equals_resize_mask_of_the_full_mask(net):
    """a downscale, an upscale (both axes or one), and the identity: the frame of the synthetic cases below is 97 x 131."""
    from myolo.myolo_utils import mask_index_tables, resize_mask
    from myolo.polygon import polygon_mask_sampled
    c = fixture_cases()
    picks = [k for k, n in enumerate(c["names"]) if tuple(c["frames"][k]) == (97, 131) and n.startswith("syn/")]
    assert len(picks) >= 50
    hit = 0
    for k in picks:
        h, w = 97, 131
        scale = [net[0] / h, net[1] / w]
        rows, cols = mask_index_tables(h, w, scale)
        want = resize_mask(c["masks"][k], scale)
        assert want.shape == net == (len(rows), len(cols))
        got = polygon_mask_sampled(c["verts"][k][:, 0], c["verts"][k][:, 1], rows, cols)
        assert np.array_equal(got, want), c["names"][k]
        hit += bool(want.any())
    assert hit >= 30
    if net == (97, 131):
        assert np.array_equal(rows, np.arange(97)) and np.array_equal(cols, np.arange(131))


def test_resize_mask_is_unchanged_by_the_shared_index_rule():
    """the reference's own resize_mask outputs stay pinned by test_ref_host_pins; here the rule itself, against the formula spelled out."""
    from myolo.myolo_utils import resize_mask, zoom_index
    rs = np.random.RandomState(3)
    m = rs.rand(23, 31, 2) > .5
    for oh, ow in ((23, 31), (10, 77), (1, 5), (64, 2)):
        scale = [oh / 23., ow / 31.]
        got = resize_mask(m, scale)
        ri = [int(np.floor(o * (22 / float(oh - 1)) + .5)) if oh > 1 else 0 for o in range(oh)]
        ci = [int(np.floor(o * (30 / float(ow - 1)) + .5)) if ow > 1 else 0 for o in range(ow)]
        assert np.array_equal(got, m[ri][:, ci])
    assert zoom_index(9, 0).shape == (0,)


# ---------------------------------------------------------------- VIADataset
def _write_dataset(tmp_path, subset="val", layout="list", with_attr=None, n_images=3):
    """the first images of golden/via/food/val with PNGs of the fixture's frame; -> (dir, the entries kept)"""
    from PIL import Image
    src = json.load(open(os.path.join(GOLDEN, "via", "food", subset, "via_food_annotation.json")))
    c = fixture_cases()
    folder = tmp_path / "data" / subset
    folder.mkdir(parents=True)
    out, kept = {}, []
    entries = [a for a in src.values() if a["regions"]][:n_images]
    for i, a in enumerate(entries):
        a = json.loads(json.dumps(a))
        a["filename"] = "img_%d.png" % i
        h, w = [int(v) for v in c["frames"][c["names"].index("real/food/%s/%d/0" % (subset, i))]]
        rs = np.random.RandomState(i)
        Image.fromarray(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(str(folder / a["filename"]))
        if with_attr:
            for j, reg in enumerate(a["regions"]):
                reg["region_attributes"] = {with_attr: ["rice", "soup"][j % 2]}
        if layout == "dict":
            a["regions"] = {str(j): reg for j, reg in enumerate(a["regions"])}
        out["%s%d" % (a["filename"], a.get("size", 0))] = a
        kept.append(a)
    out["empty.png0"] = {"filename": "empty.png", "size": 0, "regions": [] if layout == "list" else {}, "file_attributes": {}}
    with open(str(folder / "via_food_annotation.json"), "w") as f:
        json.dump(out, f)
    return str(tmp_path / "data"), kept


@pytest.mark.parametrize("layout", ["list", "dict"])
def test_via_dataset_reads_both_region_layouts(tmp_path, layout):
    from myolo.config import RiceConfig, make_config
    from myolo.myolo_utils import extract_bboxes, load_image_gt, resize_mask
    from myolo.via import VIADataset, load_via
    root, kept = _write_dataset(tmp_path, layout=layout)
    ds = load_via(root, "val")
    assert isinstance(ds, VIADataset) and len(ds.image_ids) == len(kept) == 3          # the image without regions is skipped
    assert ds.class_names == ["BG", "object"]
    c = fixture_cases()
    cfg = make_config(RiceConfig, IMAGE_SHAPE=[64, 64, 3])
    for i in ds.image_ids:
        n = len(kept[i]["regions"])
        names = ["real/food/val/%d/%d" % (i, j) for j in range(n)]
        want = np.stack([c["masks"][c["names"].index(nm)] for nm in names], axis=-1)
        info = ds.image_info[i]
        assert (info["height"], info["width"]) == want.shape[:2] and ds.image_reference(i).endswith("img_%d.png" % i)
        image = ds.load_image(i)
        assert image.dtype == np.uint8 and image.shape == want.shape[:2] + (3,)
        mask, ids = ds.load_mask(i)
        assert mask.dtype == bool and ids.dtype == np.int32 and list(ids) == [1] * n
        assert np.array_equal(mask, want)
        polys, pids = ds.load_polygons(i)
        assert len(polys) == n and all(p.dtype == np.float64 and p.shape[1] == 2 for p in polys) and pids.dtype == np.int32
        assert np.array_equal(polys[0], c["verts"][c["names"].index(names[0])])
        img, cls, bbox, m = load_image_gt(ds, cfg, i)
        small = resize_mask(want, [64 / want.shape[0], 64 / want.shape[1]])
        assert img.shape == (64, 64, 3) and np.array_equal(m, small) and np.array_equal(bbox, extract_bboxes(small)) and len(cls) == n
        assert (bbox[:, 2] > bbox[:, 0]).all()


def test_via_class_mapping_and_errors(tmp_path):
    from myolo.via import load_via
    root, kept = _write_dataset(tmp_path, with_attr="dish")
    ds = load_via(root, "val", class_attribute="dish", class_names=["soup", "rice"])
    assert ds.class_names == ["BG", "soup", "rice"]
    for i in ds.image_ids:
        want = [2 if j % 2 == 0 else 1 for j in range(len(kept[i]["regions"]))]
        assert list(ds.load_mask(i)[1]) == want and list(ds.load_polygons(i)[1]) == want
    # without a class attribute everything is class 1, whatever the regions carry
    assert all(list(load_via(root, "val").load_polygons(i)[1]) == [1] * len(kept[i]["regions"]) for i in range(3))
    with pytest.raises(ValueError, match="not one of class_names"):
        load_via(root, "val", class_attribute="dish", class_names=["soup"])
    with pytest.raises(ValueError, match="needs class_names"):
        load_via(root, "val", class_attribute="dish")
    # a shape that is not a polygon: the error names the file and the region
    path = os.path.join(root, "val", "via_food_annotation.json")
    d = json.load(open(path))
    key = [k for k in d if d[k]["regions"]][1]
    d[key]["regions"][1]["shape_attributes"] = {"name": "circle", "cx": 10, "cy": 10, "r": 4}
    other = os.path.join(root, "val", "other.json")
    json.dump(d, open(other, "w"))
    with pytest.raises(ValueError) as e:
        load_via(root, "val", annotation="other.json")
    msg = str(e.value)
    assert "other.json" in msg and "region 1" in msg and "circle" in msg and "img_1.png" in msg
    with pytest.raises(ValueError, match="expected one via_"):
        load_via(root, "train")


def test_polygon_batch_packs_what_the_kernel_reads():
    """BatchGenerator.segment_batch on outlines as one-part segments: offsets, empty slots, the sub-sampling to T outlines and the capacity check
    -- no GPU."""
    from myolo.config import RiceConfig, make_config
    from myolo.myolo_utils import BatchGenerator
    cfg = make_config(RiceConfig, IMAGE_SHAPE=[64, 64, 3], BATCH_SIZE=2, TRUE_BOX_BUFFER=3, MAX_GT_INSTANCES=3)
    T = 3
    tables = (np.arange(64, dtype=np.int32), np.arange(64, dtype=np.int32)[::-1].copy())
    tri = [np.array([[1., 2.], [9., 3.], [4., 12.]]) + k for k in range(5)]
    info = [[np.full((64, 64, 3), 7, np.uint8), np.array([1, 2], np.int32), [[p] for p in tri[:2]], tables, 0, 64],
            [np.full((64, 64, 3), 9, np.uint8), np.array([1, 1, 2, 1, 2], np.int32), [[p] for p in tri], tables, 1, 80]]
    gen = BatchGenerator(info, cfg, 'training', shuffle=False, norm=True)
    np.random.seed(4)
    fill, n_verts, n_parts, n_bounds = gen.segment_batch(0, lambda inst: np.arange(8.) + inst[4])
    assert n_verts == 3 * (2 + T) == 15 and n_parts == 2 + T == 5 and n_bounds == 0
    out = [np.zeros((2, 64, 64, 3), np.uint8), np.full((32, 2), -1.), np.full(8 + 1, -1, np.int32), np.full(2 * T + 1, -1, np.int32),
           np.full(4, -1, np.int32), np.full(2 * T + 1, -1, np.int32), np.full(2, -1, np.int32), np.full((2, T), -1, np.int32),
           np.zeros((2, 64), np.int32), np.zeros((2, 64), np.int32), np.zeros((2, 8))]
    fill(out)
    images, verts, part_off, slot_part, bounds, slot_bound, src_h, ids_b, rows_t, cols_t, rows = out
    # the vertex offset of every slot, as the kernel derives it: one part per live slot, none for the empty one
    assert list(part_off[slot_part]) == [0, 3, 6, 6, 9, 12, 15] and list(slot_part) == [0, 1, 2, 2, 3, 4, 5] and (verts[15:] == -1).all()
    assert list(part_off[:6]) == [0, 3, 6, 9, 12, 15] and not slot_bound.any() and (bounds == -1).all() and list(src_h) == [64, 80]
    assert list(ids_b[0]) == [1, 2, 0] and (ids_b[1] != 0).all()
    assert np.array_equal(verts[0:3], tri[0]) and np.array_equal(verts[3:6], tri[1])
    np.random.seed(4)
    ids = np.random.choice(np.arange(5), T, replace=False)
    assert np.array_equal(verts[6:15], np.concatenate([tri[j] for j in ids])) and list(ids_b[1]) == [[1, 1, 2, 1, 2][j] for j in ids]
    assert images[1, 0, 0, 0] == 9 and np.array_equal(cols_t[0], tables[1]) and np.array_equal(rows_t[1], tables[0])
    assert np.array_equal(rows[1], np.arange(8.) + 1)
    with pytest.raises(ValueError, match="do not fit"):
        fill([images, np.zeros((8, 2))] + out[2:])
