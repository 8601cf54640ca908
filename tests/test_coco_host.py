"""myolo.coco on the host: the COCO loader, load_mask (union of parts, run-length codes), segment_mask_sampled against resize_mask of the full
mask, BatchGenerator.segment_batch's tables, and the binding of myolo_segment_masks -- no GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- shared with test_gpu_segments.py
def hand_rles(h, w):
    """name -> counts (lists that sum to h * w): the hand-made run-length codes both test files use"""
    n = h * w
    a, b, c = n // 5, n // 4, n // 7
    return {"zero": [n], "one": [0, n], "lead0": [0, max(1, n // 3), n - max(1, n // 3)],
            "midzero": [a, 0, 0, b, 0, c, n - a - b - c], "alternate": [1] * n}


def rle_segment(h, w, counts):
    return {"size": [h, w], "counts": np.asarray(counts, np.int64)}


def scaled_parts(h, w):
    """a three-part instance with overlaps, in fractions of an h x w frame: float64 [k,2] (row, col) arrays"""
    f = np.array([h, w], np.float64)
    tri = np.array([[.1, .1], [.8, .2], [.3, .75]]) * f
    quad = np.array([[.2, .3], [.2, .9], [.7, .9], [.7, .3]]) * f + .25
    star = np.array([[.5, .05], [.62, .4], [.95, .5], [.62, .6], [.5, .95], [.38, .6], [.05, .5], [.38, .4]]) * f
    return [tri, quad, star]


def flat_xy(part):
    """(row, col) [k,2] -> COCO's flat [x0, y0, x1, y1, ...]"""
    return [float(v) for v in np.asarray(part)[:, ::-1].reshape(-1)]


def write_coco(folder, images, annotations, categories, name="instances.json"):
    """images: (id, file name, h, w); a PNG of random bytes is written for each.  -> the annotation file's path"""
    from PIL import Image
    os.makedirs(str(folder), exist_ok=True)
    for i, (_, fn, h, w) in enumerate(images):
        Image.fromarray(np.random.RandomState(i).randint(0, 256, (h, w, 3)).astype(np.uint8)).save(os.path.join(str(folder), fn))
    path = os.path.join(str(folder), name)
    with open(path, "w") as f:
        json.dump({"images": [{"id": i, "file_name": fn, "height": h, "width": w} for i, fn, h, w in images],
                   "annotations": annotations, "categories": [{"id": i, "name": n} for i, n in categories]}, f)
    return path


CATS = [(7, "rice"), (3, "soup"), (12, "bowl")]


def _small_dataset(tmp_path):
    from myolo import rle
    h, w = 20, 30
    parts = scaled_parts(h, w)
    square = rle.encode(np.pad(np.ones((6, 8), bool), ((3, 11), (5, 17))))
    images = [(101, "a.png", h, w), (102, "b.png", h, w), (103, "c.png", h, w), (104, "d.png", 12, 9)]
    anns = [
        {"id": 1, "image_id": 101, "category_id": 7, "iscrowd": 0, "segmentation": [flat_xy(parts[0])]},
        {"id": 2, "image_id": 101, "category_id": 12, "iscrowd": 0, "segmentation": [flat_xy(parts[1]), flat_xy(parts[2])]},
        {"id": 3, "image_id": 101, "category_id": 3, "iscrowd": 1,
         "segmentation": {"size": [h, w], "counts": rle.to_string(square["counts"])}},
        {"id": 4, "image_id": 101, "category_id": 3, "iscrowd": 0, "segmentation": []},                     # empty: skipped
        {"id": 5, "image_id": 102, "category_id": 3, "iscrowd": 0,
         "segmentation": {"size": [h, w], "counts": [int(v) for v in square["counts"]]}},
        {"id": 6, "image_id": 103, "category_id": 3, "iscrowd": 1, "segmentation": {"size": [h, w], "counts": [h * w]}},   # crowd only
        # image 104 has no annotation at all
    ]
    return write_coco(tmp_path / "coco", images, anns, CATS), str(tmp_path / "coco"), parts, square


# ---------------------------------------------------------------- the loader
def test_loader_maps_categories_and_skips(tmp_path):
    from myolo import rle
    from myolo.coco import COCODataset, load_coco
    path, folder, parts, square = _small_dataset(tmp_path)
    ds = load_coco(path, folder)
    assert isinstance(ds, COCODataset) and not hasattr(ds, "load_polygons")
    assert ds.class_names == ["BG", "soup", "rice", "bowl"] and ds.category_ids == [0, 3, 7, 12]
    # crowd="skip": annotation 3 and image 103 (crowd only) go, as do the empty annotation 4 and the image without annotations
    assert [ds.image_info[i]["id"] for i in ds.image_ids] == [101, 102]
    segs, ids = ds.load_segments(0)
    assert ids.dtype == np.int32 and list(ids) == [2, 3] and ds.image_info[0]["annotation_ids"] == [1, 2]
    assert len(segs[0]) == 1 and len(segs[1]) == 2 and all(p.dtype == np.float64 and p.shape[1] == 2 for s in segs for p in s)
    assert np.array_equal(segs[0][0], parts[0]) and np.array_equal(segs[1][1], parts[2])                    # (row, col) from x, y
    info = ds.image_info[0]
    assert (info["height"], info["width"]) == (20, 30) and ds.image_reference(0).endswith("a.png")
    assert ds.load_image(0).shape == (20, 30, 3) and ds.load_image(0).dtype == np.uint8
    # crowd="keep": ordinary instances
    dk = load_coco(path, folder, crowd="keep")
    assert [dk.image_info[i]["id"] for i in dk.image_ids] == [101, 102, 103]
    assert list(dk.load_segments(0)[1]) == [2, 3, 1] and list(dk.load_segments(2)[1]) == [1]
    # string counts and list counts give the same segment and the same mask
    s_str, s_list = dk.load_segments(0)[0][2], dk.load_segments(1)[0][0]
    assert s_str["size"] == [20, 30] and s_str["counts"].dtype == np.int64 and np.array_equal(s_str["counts"], s_list["counts"])
    assert np.array_equal(dk.load_mask(0)[0][:, :, 2], dk.load_mask(1)[0][:, :, 0]) and dk.load_mask(1)[0].sum() == 48
    # category_ids restricts AND orders; the annotations of other categories are dropped
    dc = load_coco(path, folder, category_ids=[12, 3], crowd="keep")
    assert dc.class_names == ["BG", "bowl", "soup"] and dc.category_ids == [0, 12, 3]
    assert list(dc.load_segments(0)[1]) == [1, 2] and dc.image_info[0]["annotation_ids"] == [2, 3]
    d7 = load_coco(path, folder, category_ids=[7])
    assert len(d7.image_ids) == 1 and list(d7.load_segments(0)[1]) == [1]
    # the round trip through rle.coco_results
    res = {"class_ids": np.array([1, 2]), "rle_masks": [square, square], "bboxes": np.array([[5, 3, 13, 9]] * 2), "confidence_scores": [.9, .8]}
    out = rle.coco_results([res], [dc.image_info[0]["id"]], category_ids=dc.category_ids)
    assert [o["category_id"] for o in out] == [12, 3] and out[0]["image_id"] == 101
    with pytest.raises(ValueError, match="crowd"):
        load_coco(path, folder, crowd="ignore")
    with pytest.raises(ValueError, match="category_ids"):
        load_coco(path, folder, category_ids=[3, 99])


def test_loader_rejects_what_it_cannot_read(tmp_path):
    from myolo.coco import load_coco
    h, w = 10, 12
    images = [(1, "a.png", h, w)]

    def load(seg, name):
        anns = [{"id": 77, "image_id": 1, "category_id": 3, "iscrowd": 0, "segmentation": seg}]
        return load_coco(write_coco(tmp_path / "bad", images, anns, CATS, name=name), str(tmp_path / "bad"))
    with pytest.raises(ValueError, match="77.*size"):
        load({"size": [w, h], "counts": [h * w]}, "size.json")                          # the code's size is not the image's
    with pytest.raises(ValueError, match="77"):
        load({"size": [h, w], "counts": [h * w - 1]}, "short.json")                     # the counts do not sum to h * w
    with pytest.raises(ValueError, match="77"):
        load({"size": [h, w], "counts": [5, -2, h * w - 3]}, "negative.json")
    with pytest.raises(ValueError, match="77"):
        load({"size": [h, w], "counts": "0~"}, "string.json")                           # no character of a compressed code
    with pytest.raises(ValueError, match="77.*part 1"):
        load([[1, 1, 5, 1, 5, 5], [1, 2, 3]], "odd.json")                                # an odd number of coordinates
    with pytest.raises(ValueError, match="part 0"):
        load([[]], "novertex.json")
    with pytest.raises(ValueError, match="finite"):
        load([[1, 1, float("nan"), 2]], "nan.json")
    ok = load([[3, 4]], "one.json")                                                      # one vertex is a part
    assert ok.load_mask(0)[0][4, 3, 0] and ok.load_mask(0)[0].sum() == 1


# ---------------------------------------------------------------- load_mask
def test_load_mask_is_the_union_of_the_parts_and_decodes_codes(tmp_path):
    from myolo import rle
    from myolo.coco import load_coco, segment_mask
    from myolo.polygon import polygon_mask
    h, w = 24, 24
    a = np.array([[2., 2.], [2., 12.], [12., 12.], [12., 2.]])
    b = a + 5.0
    code = rle.encode(np.random.RandomState(0).rand(h, w) > .6)
    anns = [{"id": 1, "image_id": 1, "category_id": 3, "iscrowd": 0, "segmentation": [flat_xy(a), flat_xy(b)]},
            {"id": 2, "image_id": 1, "category_id": 7, "iscrowd": 0, "segmentation": [flat_xy(p) for p in scaled_parts(h, w)]},
            {"id": 3, "image_id": 1, "category_id": 7, "iscrowd": 0, "segmentation": {"size": [h, w], "counts": rle.to_string(code["counts"])}}]
    ds = load_coco(write_coco(tmp_path / "u", [(1, "a.png", h, w)], anns, CATS), str(tmp_path / "u"))
    mask, ids = ds.load_mask(0)
    assert mask.dtype == bool and mask.shape == (h, w, 3) and list(ids) == [1, 2, 2] and ids.dtype == np.int32
    fa, fb = polygon_mask(a[:, 0], a[:, 1], (h, w)), polygon_mask(b[:, 0], b[:, 1], (h, w))
    assert np.array_equal(mask[:, :, 0], fa | fb) and (fa & fb).sum() > 20
    both = np.concatenate([a, b])
    evenodd = polygon_mask(both[:, 0], both[:, 1], (h, w))                                # the two outlines read as ONE outline
    assert (mask[:, :, 0] & ~evenodd).any(), "the union keeps the overlap that even-odd over the concatenated outline clears"
    want = np.zeros((h, w), bool)
    for p in scaled_parts(h, w):
        want |= polygon_mask(p[:, 0], p[:, 1], (h, w))
    assert np.array_equal(mask[:, :, 1], want) and np.array_equal(segment_mask(ds.load_segments(0)[0][1], (h, w)), want)
    assert np.array_equal(mask[:, :, 2], rle.decode(code))
    again = rle.encode(mask[:, :, 2])
    assert np.array_equal(again["counts"], code["counts"]) and again["size"] == [h, w]


# ---------------------------------------------------------------- segment_mask_sampled
@pytest.mark.parametrize("src", [(1, 1), (7, 300), (300, 7), (37, 53), (40, 56)])
def test_sampled_segment_equals_resize_mask_of_the_full_mask(src):
    from myolo import rle
    from myolo.coco import rle_bounds, segment_mask, segment_mask_sampled
    from myolo.myolo_utils import mask_index_tables, resize_mask
    h, w = src
    H, W = 40, 56
    scale = [H / h, W / w]
    rows, cols = mask_index_tables(h, w, scale)
    assert (len(rows), len(cols)) == (H, W)
    if src == (H, W):
        assert np.array_equal(rows, np.arange(H)) and np.array_equal(cols, np.arange(W))
    segments = [rle_segment(h, w, c) for c in hand_rles(h, w).values()]
    segments.append(rle.encode(np.random.RandomState(1).rand(h, w) > .5))
    segments += [scaled_parts(h, w), scaled_parts(h, w)[:1], []]
    set_somewhere = 0
    for s in segments:
        full = segment_mask(s, (h, w))
        got = segment_mask_sampled(s, rows, cols)
        assert got.dtype == bool and got.shape == (H, W)
        assert np.array_equal(got, resize_mask(full, scale))
        set_somewhere += bool(got.any())
    assert set_somewhere >= (2 if h * w == 1 else 5)                 # (one pixel: only the codes that set it)
    hr = hand_rles(h, w)
    assert not segment_mask_sampled(rle_segment(h, w, hr["zero"]), rows, cols).any()
    assert segment_mask_sampled(rle_segment(h, w, hr["one"]), rows, cols).all()
    assert len(rle_bounds(rle_segment(h, w, hr["zero"]))) == 0 and list(rle_bounds(rle_segment(h, w, hr["one"]))) == [0]
    if src == (37, 53):
        alt = segment_mask(rle_segment(h, w, hr["alternate"]), (h, w))
        assert alt.sum() == (h * w) // 2 and not alt[0, 0] and alt[1, 0]


# ---------------------------------------------------------------- BatchGenerator.segment_batch
def test_segment_batch_packs_what_the_kernel_reads():
    from myolo.config import RiceConfig, make_config
    from myolo.myolo_utils import BatchGenerator
    cfg = make_config(RiceConfig, IMAGE_SHAPE=[64, 64, 3], BATCH_SIZE=2, TRUE_BOX_BUFFER=3, MAX_GT_INSTANCES=3)
    T = 3
    tables = (np.arange(64, dtype=np.int32), np.arange(64, dtype=np.int32)[::-1].copy())
    tri = [np.array([[1., 2.], [9., 3.], [4., 12.]]) + k for k in range(6)]
    quad = np.array([[1., 1.], [1., 5.], [5., 5.], [5., 1.]])
    code = rle_segment(64, 64, [10, 5, 0, 7, 64 * 64 - 22])
    segs1 = [[tri[k]] for k in range(5)]
    info = [[np.full((64, 64, 3), 7, np.uint8), np.array([1, 2], np.int32), [[tri[0], quad], code], tables, 0, 64],
            [np.full((64, 64, 3), 9, np.uint8), np.array([1, 1, 2, 1, 2], np.int32), segs1, tables, 1, 80]]
    gen = BatchGenerator(info, cfg, 'training', shuffle=False, norm=True)
    np.random.seed(4)
    fill, n_verts, n_parts, n_bounds = gen.segment_batch(0, lambda inst: np.arange(8.) + inst[4])
    assert (n_verts, n_parts, n_bounds) == (7 + 3 * T, 2 + T, 4)

    def buffers(nv=32, npart=8, nb=8):
        return [np.zeros((2, 64, 64, 3), np.uint8), np.full((nv, 2), -1.), np.full(npart + 1, -1, np.int32), np.full(2 * T + 1, -1, np.int32),
                np.full(nb, -1, np.int32), np.full(2 * T + 1, -1, np.int32), np.full(2, -1, np.int32), np.full((2, T), -1, np.int32),
                np.zeros((2, 64), np.int32), np.zeros((2, 64), np.int32), np.zeros((2, 8))]
    out = fill(buffers())
    images, verts, part_off, slot_part, bounds, slot_bound, src_h, ids_b, rows_t, cols_t, rows = out
    # image 0: slot 0 = two parts, slot 1 = a code, slot 2 empty; image 1: three one-part slots
    assert list(slot_part) == [0, 2, 2, 2, 3, 4, 5] and list(part_off[:6]) == [0, 3, 7, 10, 13, 16] and (verts[16:] == -1).all()
    assert list(slot_bound) == [0, 0, 4, 4, 4, 4, 4] and list(bounds[:4]) == [10, 15, 15, 22] and (bounds[4:] == -1).all()
    assert list(src_h) == [64, 80] and list(ids_b[0]) == [1, 2, 0] and (ids_b[1] != 0).all()
    assert np.array_equal(verts[0:3], tri[0]) and np.array_equal(verts[3:7], quad)
    np.random.seed(4)
    ids = np.random.choice(np.arange(5), T, replace=False)                                # the one draw, as fill_raw makes it
    assert np.array_equal(verts[7:16], np.concatenate([tri[j] for j in ids])) and list(ids_b[1]) == [[1, 1, 2, 1, 2][j] for j in ids]
    assert images[1, 0, 0, 0] == 9 and np.array_equal(cols_t[0], tables[1]) and np.array_equal(rows[1], np.arange(8.) + 1)
    for short in (dict(nv=15), dict(npart=4), dict(nb=3)):
        with pytest.raises(ValueError, match="do not fit"):
            fill(buffers(**short))


def test_segment_tables_builds_what_dataset_boxes_and_evaluate_hand_the_kernel():
    """a group of 2 images in B = 3 rows (one padding row), T = 3: a two-part segment, a code and an empty slot; then a group without a part or a
    code -- the arrays anchors.dataset_boxes and MaskYOLO._evaluate_segments used to build each for itself"""
    from myolo.myolo_utils import segment_tables
    B, T, H, W = 3, 3, 5, 7
    tri = np.array([[1., 2.], [9., 3.], [4., 12.]])
    quad = np.array([[1., 1.], [1., 5.], [5., 5.], [5., 1.]])
    code = rle_segment(40, 30, [10, 5, 0, 7, 40 * 30 - 22])
    t0 = (np.arange(H, dtype=np.int32) * 3, np.arange(W, dtype=np.int32)[::-1] * 2)
    t1 = (np.arange(H, dtype=np.int32) + 30, np.arange(W, dtype=np.int32) + 4)
    group = [([[tri, quad], code], t0, 40), ([[tri + 1]], t1, 57)]
    verts, part_off, slot_part, bounds, slot_bound, src_h, rows, cols = segment_tables(group, B, T, H, W)
    assert verts.dtype == np.float64 and all(a.dtype == np.int32 for a in (part_off, slot_part, bounds, slot_bound, src_h, rows, cols))
    assert verts.shape == (10, 2) and np.array_equal(verts, np.concatenate([tri, quad, tri + 1])) and list(part_off) == [0, 3, 7, 10]
    assert list(bounds) == [10, 15, 15, 22]
    # image 0: two parts, a code, an empty slot; image 1: one part and two empty slots; constant past the last image
    assert list(slot_part) == [0, 2, 2, 2, 3, 3] + [3] * (T + 1) and list(slot_bound) == [0, 0, 4, 4, 4, 4] + [4] * (T + 1)
    assert list(src_h) == [40, 57, 1]
    assert np.array_equal(rows[0], t0[0]) and np.array_equal(cols[0], t0[1]) and np.array_equal(rows[1], t1[0]) and np.array_equal(cols[1], t1[1])
    assert rows.shape == (B, H) and cols.shape == (B, W) and not rows[2].any() and not cols[2].any()
    # no part and no code: at least one element everywhere, every slot empty
    verts, part_off, slot_part, bounds, slot_bound, src_h, rows, cols = segment_tables([([], t1, 57)], B, T, H, W)
    assert verts.shape == (1, 2) and not verts.any() and list(part_off) == [0] and list(bounds) == [0]
    assert slot_part.shape == slot_bound.shape == (B * T + 1,) and not slot_part.any() and not slot_bound.any()
    assert list(src_h) == [57, 1, 1] and np.array_equal(rows[0], t1[0]) and not rows[1:].any() and not cols[1:].any()
    with pytest.raises(ValueError, match="for 3 slots"):
        segment_tables([([[tri]] * 4, t1, 57)], B, T, H, W)


# ---------------------------------------------------------------- the binding
def test_binding_declares_segment_masks_with_the_headers_arity():
    from myolo import _ext as X
    txt = open(os.path.join(ROOT, "include", "myolo_hip_internal.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = dict(re.findall(r"\b(?:int|size_t)\s+(myolo_segment_\w+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S))
    assert sorted(decl) == ["myolo_segment_masks"]
    assert len(X.SIGS["myolo_segment_masks"]) == decl["myolo_segment_masks"].count(",") + 1 == 15
    assert "myolo_segment_masks" in X.exported_symbols()
    assert "myolo_segment_masks" not in open(os.path.join(ROOT, "include", "myolo_hip.h")).read()          # the operator API stays as it is
    import __graft_entry__ as G
    assert ("segment_kernels.hip", ["-ffp-contract=off"]) in G.UNITS
    assert "#pragma clang fp contract(off)" in open(os.path.join(G.CSRC, "segment_kernels.hip")).read()


def test_segment_masks_refuses_null_arguments_without_a_gpu():
    from myolo import _ext as X
    lib = X.load()
    rc = lib.myolo_segment_masks(None, None, None, None, None, None, None, None, None, None, 1, 1, 1, 1, None)
    assert rc == -1 and b"segment_masks: null" in lib.myolo_last_error_string()
    buf = (ctypes.c_int32 * 16)()                                   # host memory: the sizes are refused before anything is launched
    p = ctypes.addressof(buf)
    assert lib.myolo_segment_masks(None, p, p, None, p, p, p, p, p, None, 1, 1, 1, 0, None) == -1 and b"T=0" in lib.myolo_last_error_string()
    assert lib.myolo_segment_masks(None, p, p, None, p, p, p, p, p, None, 0, 1, 1, 1, None) == -1 and b"B=0" in lib.myolo_last_error_string()
    assert lib.myolo_segment_masks(p, p, p, p, p, p, p, p, None, p, 1, 1, 1, 1, None) == -1 and b"null" in lib.myolo_last_error_string()
