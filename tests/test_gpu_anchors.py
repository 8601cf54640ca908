"""myolo.anchors on the device: myolo_anchor_kmeans against a float64 numpy restatement of its contract -- assignments,
counts, iterations, convergence and the centroids bit for bit; the mean IoU to n * 2^-52 --, the fit against the reference's published anchors,
and dataset_boxes' device route against its host route."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


# ---------------------------------------------------------------- the yardstick: the contract restated in numpy float64 (NOT myolo.anchors)
def iou_matrix(wh, cent):
    w, h = wh[:, 0].astype(np.float64)[:, None], wh[:, 1].astype(np.float64)[:, None]
    cw, ch = cent[:, 0][None, :], cent[:, 1][None, :]
    inter = np.minimum(w, cw) * np.minimum(h, ch)
    return inter / ((w * h + cw * ch) - inter)


def restate(wh, start, max_iter=300):
    """-> centroids, assign, counts, iterations, converged, mean_iou"""
    cent, k = np.array(start, np.float64), len(start)
    prev, passes, converged = None, 0, False
    while passes < max_iter:
        assign = np.argmin(1.0 - iou_matrix(wh, cent), axis=1)          # the lowest index of the smallest d
        passes += 1
        counts = np.bincount(assign, minlength=k).astype(np.int64)
        if prev is not None and np.array_equal(assign, prev):
            converged = True
            break
        sums = np.zeros((k, 2), np.int64)
        np.add.at(sums, assign, wh.astype(np.int64))
        full = counts > 0                                               # an empty cluster keeps its centroid
        cent[full] = sums[full] / counts[full][:, None]
        prev = assign
    return cent, assign, counts, passes, converged, float(iou_matrix(wh, cent).max(axis=1).mean())


def mean_best_iou(wh, cent):
    return float(iou_matrix(wh, np.asarray(cent, np.float64)).max(axis=1).mean())


def sizes(n, lo=1, hi=224):
    return np.random.RandomState(n).randint(lo, hi + 1, (n, 2)).astype(np.int32)


def distinct(wh):
    return len(np.unique(wh, axis=0))


def check_run(res, r, wh, start, max_iter=300):
    """run r of an AnchorResult (asked with assign=True) against the restatement of the same start: everything EQUAL, the mean IoU to n * 2^-52"""
    cent, assign, counts, passes, converged, miou = restate(wh, start, max_iter)
    assert np.array_equal(res.assign[r], assign)
    assert np.array_equal(res.counts[r], counts)
    assert int(res.iterations[r]) == passes and bool(res.converged[r]) == converged
    assert res.centroids_px[r].tobytes() == cent.tobytes()              # bit for bit
    print("mean_iou: device %.17g restatement %.17g bound %.3g" % (res.mean_iou[r], miou, len(wh) * 2.0 ** -52))
    assert abs(float(res.mean_iou[r]) - miou) <= len(wh) * 2.0 ** -52
    return passes, converged


def fit_mixed(wh, starts, max_iter=300):
    """several runs of DIFFERENT k in one call of the kernel -> [(centroids [k,2], counts, iterations, converged, mean_iou, assign)]"""
    from myolo import anchors as A
    cent, counts, iters, conv, miou, assign = A._fit(wh, [np.asarray(s, np.float64) for s in starts], max_iter, DEV, True)
    return [(cent[r, :len(s)], counts[r, :len(s)], int(iters[r]), bool(conv[r]), float(miou[r]), assign[r]) for r, s in enumerate(starts)]


@pytest.fixture(scope="module")
def cfg():
    from myolo.config import Config, make_config
    return make_config(Config)


# ---------------------------------------------------------------- exact agreement
@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 257, 5000])
def test_single_runs_equal_the_restatement(cfg, n):
    from myolo.anchors import initial_centroids, kmeans_anchors
    wh = sizes(n)
    ks = [k for k in (1, 2, 5, 9, 32) if distinct(wh) >= k]
    assert ks and (n < 257 or ks == [1, 2, 5, 9, 32])
    for k in ks:
        res = kmeans_anchors(wh, k, cfg, restarts=1, seed=0, assign=True, device=DEV)
        assert res.centroids_px.shape == (1, k, 2) and res.assign.shape == (1, n) and res.assign.dtype == np.int32
        _, converged = check_run(res, 0, wh, initial_centroids(wh, k, 1, 0)[0])
        assert converged and res.best == 0


@pytest.mark.parametrize("n", [257, 5000])
def test_eight_runs_of_mixed_k_in_one_call(n):
    from myolo.anchors import initial_centroids
    wh = sizes(n)
    starts = [initial_centroids(wh, k, 1, seed=r)[0] for r, k in enumerate((1, 2, 5, 9, 32, 5, 5, 3))]
    got = fit_mixed(wh, starts)
    for (cent, counts, iters, conv, miou, assign), s in zip(got, starts):
        w_cent, w_assign, w_counts, w_passes, w_conv, w_miou = restate(wh, s)
        assert np.array_equal(assign, w_assign) and np.array_equal(counts, w_counts) and (iters, conv) == (w_passes, w_conv)
        assert cent.tobytes() == w_cent.tobytes()
        assert abs(miou - w_miou) <= n * 2.0 ** -52
    # the runs do not see one another: runs 3, 5 and 6 have k = 5 and different draws
    assert len({got[r][0].tobytes() for r in (2, 5, 6)}) == 3


def test_lattice_with_heavy_duplication(cfg):
    from myolo.anchors import initial_centroids, kmeans_anchors
    wh = np.random.RandomState(0).choice([8, 16, 32], (300, 2)).astype(np.int32)
    assert distinct(wh) == 9
    for k in (1, 2, 5, 9):
        res = kmeans_anchors(wh, k, cfg, restarts=3, seed=0, assign=True, device=DEV)
        starts = initial_centroids(wh, k, 3, 0)
        for r in range(3):
            check_run(res, r, wh, starts[r])


@pytest.mark.parametrize("lo, hi", [(500000, 1000000), (900000, 1000000)], ids=["issue", "past-2^32-at-k1"])
def test_sums_beyond_32_bits(cfg, lo, hi):
    """sizes of 5e5 .. 1e6: with k = 1 the 5000 widths sum to ~3.75e9 (past 2^31: a signed 32-bit accumulator shows); the second set, 9e5 .. 1e6,
    sums to ~4.75e9, past 2^32 as well"""
    from myolo.anchors import initial_centroids, kmeans_anchors
    wh = sizes(5000, lo, hi)
    assert int(wh[:, 0].astype(np.int64).sum()) > (1 << 31 if lo < 900000 else 1 << 32)
    for k in (1, 2, 5):
        res = kmeans_anchors(wh, k, cfg, restarts=1, seed=0, assign=True, device=DEV)
        check_run(res, 0, wh, initial_centroids(wh, k, 1, 0)[0])


def test_ties_go_to_the_lower_index_and_an_empty_cluster_keeps_its_centroid(cfg):
    from myolo.anchors import kmeans_anchors
    wh = sizes(257)
    init = [[50., 50.], [50., 50.]]
    # one pass: every point ties and the lower index takes them all.  (From the second pass on cluster 0 sits at the mean and cluster 1, still at
    # (50, 50), wins the small boxes back: the whole run is only held to the restatement.)
    res = kmeans_anchors(wh, 2, cfg, init=init, max_iter=1, assign=True, device=DEV)
    check_run(res, 0, wh, init, max_iter=1)
    assert (res.assign[0] == 0).all() and list(res.counts[0]) == [257, 0] and not bool(res.converged[0])
    assert res.centroids_px[0, 1].tolist() == [50., 50.] and res.centroids_px[0, 0].tolist() != [50., 50.]
    res = kmeans_anchors(wh, 2, cfg, init=init, assign=True, device=DEV)
    check_run(res, 0, wh, init)
    # two identical centroids that no box comes back to (all boxes are >= 100 x 100, the pair sits at 1 x 1): the other cluster ENDS empty
    big = sizes(257, 100, 224)
    init = [[1., 1.], [1., 1.]]
    res = kmeans_anchors(big, 2, cfg, init=init, assign=True, device=DEV)
    check_run(res, 0, big, init)
    assert (res.assign[0] == 0).all() and list(res.counts[0]) == [257, 0]
    assert res.centroids_px[0, 1].tolist() == [1., 1.] and bool(res.converged[0]) and int(res.iterations[0]) == 2
    small = sizes(300, 1, 40)                                            # no large box: the (200, 200) cluster never gets a point
    init = [[10., 10.], [10., 10.], [200., 200.]]
    res = kmeans_anchors(small, 3, cfg, init=init, assign=True, device=DEV)
    check_run(res, 0, small, init)
    assert int(res.counts[0, 2]) == 0 and int(res.counts[0].sum()) == 300 and res.centroids_px[0, 2].tolist() == [200., 200.]
    assert np.isfinite(res.centroids_px).all() and np.isfinite(res.mean_iou).all()


def test_max_iter_stops_an_unconverged_run(cfg):
    from myolo.anchors import initial_centroids, kmeans_anchors
    wh = sizes(5000)
    start = initial_centroids(wh, 9, 1, 0)[0]
    full = restate(wh, start)
    print("the restatement converges after %d passes" % full[3])
    assert full[4] and full[3] > 2
    res = kmeans_anchors(wh, 9, cfg, restarts=1, seed=0, max_iter=2, assign=True, device=DEV)
    assert int(res.iterations[0]) == 2 and not bool(res.converged[0])
    check_run(res, 0, wh, start, max_iter=2)


# ---------------------------------------------------------------- mean IoU, determinism, best
def test_two_calls_give_the_same_bits_and_best_is_the_argmax(cfg):
    from myolo.anchors import kmeans_anchors
    wh = sizes(5000)
    a = kmeans_anchors(wh, 9, cfg, restarts=8, seed=0, assign=True, device=DEV)
    b = kmeans_anchors(wh, 9, cfg, restarts=8, seed=0, assign=True, device=DEV)
    for name in ("centroids_px", "counts", "iterations", "converged", "mean_iou", "assign"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert a.best == int(np.argmax(a.mean_iou)) and a.anchors == b.anchors
    for r in range(8):
        assert abs(float(a.mean_iou[r]) - mean_best_iou(wh, a.centroids_px[r])) <= 5000 * 2.0 ** -52
    # a tie: the same start twice -> the same mean IoU twice, best is the lower index
    init = np.stack([a.centroids_px[3], a.centroids_px[3]])
    t = kmeans_anchors(wh, 9, cfg, init=init, device=DEV)
    assert t.mean_iou[0] == t.mean_iou[1] and t.best == 0 and t.assign is None


# ---------------------------------------------------------------- the reference's published anchors
def _golden_boxes(name):
    rows = [line.strip()[1:-1].split() for line in open(os.path.join(ROOT, "tests", "golden", name)) if line.strip()]
    return np.asarray(rows, dtype=np.int32)


@pytest.mark.parametrize("name, n_boxes, base", [("rice_boxes.txt", 53, "RiceConfig"), ("food_boxes.txt", 148, "Config")])
def test_fit_is_no_worse_than_the_published_anchors(name, n_boxes, base):
    from myolo import config as C
    from myolo.anchors import box_sizes, kmeans_anchors
    boxes = _golden_boxes(name)
    assert boxes.shape == (n_boxes, 4)
    cfg = C.make_config(getattr(C, base), IMAGE_SHAPE=[224, 224, 3])
    res = kmeans_anchors(boxes, 5, cfg, restarts=8, seed=0, device=DEV)
    published = np.asarray(getattr(C, base).ANCHORS, np.float64).reshape(-1, 2) * 32.0
    theirs = mean_best_iou(box_sizes(boxes), published)
    print("%s: fitted %.5f, published %.5f" % (name, res.mean_iou[res.best], theirs))
    assert res.converged.all()
    assert float(res.mean_iou[res.best]) >= theirs
    a = np.asarray(res.anchors).reshape(-1, 2)
    assert (np.diff(a[:, 0]) >= 0).all() and res.overrides()["N_BOX"] == 5
    assert np.allclose(np.sort(a[:, 0] * 32.0), np.sort(res.centroids_px[res.best][:, 0]), rtol=0, atol=1e-12)


def test_sweep_over_k_on_the_food_boxes(cfg):
    from myolo.anchors import box_sizes, initial_centroids, kmeans_anchors, sweep_anchors
    boxes = _golden_boxes("food_boxes.txt")
    wh = box_sizes(boxes)
    sweep = sweep_anchors(boxes, cfg, ks=range(1, 11), restarts=8, seed=0, device=DEV)
    assert list(sweep) == list(range(1, 11))
    for k, res in sweep.items():
        assert res.k == k and res.centroids_px.shape == (8, k, 2) and res.converged.all()
    one = restate(wh, initial_centroids(wh, 1, 1, 0)[0])
    assert abs(float(sweep[1].mean_iou[0]) - one[5]) <= len(wh) * 2.0 ** -52
    assert round(float(sweep[1].mean_iou[sweep[1].best]), 4) == 0.5529
    assert sweep[10].mean_iou[sweep[10].best] > sweep[1].mean_iou[sweep[1].best]
    # one call for all (k, restart) pairs gives what a call per k gives
    five = kmeans_anchors(boxes, 5, cfg, restarts=8, seed=0, device=DEV)
    assert five.centroids_px.tobytes() == sweep[5].centroids_px.tobytes() and five.mean_iou.tobytes() == sweep[5].mean_iou.tobytes()


# ---------------------------------------------------------------- the boxes of a dataset, on the device
def _rect(r0, c0, r1, c1):
    return np.array([[r0, c0], [r0, c1], [r1, c1], [r1, c0]], np.float64)


def _images():
    """(h, w, outlines float64 [k,2] (row, col)) of three images; the second has 9 instances; the third holds, as its second outline, a square around
    ONE source pixel that the 64 x 64 index tables do not sample (the construction of tests/test_gpu_polygon.py::_via_dataset)"""
    from myolo.myolo_utils import mask_index_tables
    a = [_rect(3.2, 4.1, 30.7, 40.3), np.array([[5., 50.], [35., 54.5], [20.5, 30.]]), _rect(-4., -3., 9.5, 12.5)]
    b = [_rect(2 + 20 * i + .3 * j, 3 + 20 * j + .2 * i, 2 + 20 * i + 9 + j, 3 + 20 * j + 7 + 2 * i) for i in range(3) for j in range(3)]
    h, w = 100, 70
    rows, cols = mask_index_tables(h, w, [64 / h, 64 / w])
    r = [v for v in range(10, h) if v not in rows][0]
    c = [v for v in range(10, w) if v not in cols][0]
    tiny = _rect(r - .4, c - .4, r + .4, c + .4)
    cc = [_rect(10.5, 8.5, 60.2, 33.3), tiny, np.array([[50., 20.], [95., 30.], [99., 66.], [70., 60.], [62., 35.]]), _rect(80., 50., 120., 90.)]
    return [(40, 56, a), (64, 64, b), (h, w, cc)], (r, c)


def _via(images):
    from myolo.via import VIADataset
    ds = VIADataset()
    ds.add_class(ds.SOURCE, 1, "object")
    for i, (h, w, polys) in enumerate(images):
        ds.add_image(ds.SOURCE, image_id=i, path=None, width=w, height=h, polygons=polys, polygon_class_ids=np.ones(len(polys), np.int32))
    ds.prepare()
    return ds


def _coco(images):
    """the same instances as segments: the first of image 0 as a run-length code, the last of image 0 joined to the first as a second part of a
    two-part instance in image 2"""
    from myolo import rle
    from myolo.coco import COCODataset
    from myolo.polygon import polygon_mask
    ds = COCODataset()
    ds.add_class(ds.SOURCE, 1, "object")
    for i, (h, w, polys) in enumerate(images):
        segs = [[p] for p in polys]
        if i == 0:
            segs[0] = rle.encode(polygon_mask(polys[0][:, 0], polys[0][:, 1], (h, w)))
        if i == 2:
            segs[0] = [polys[0], _rect(55., 30., 75., 60.)]
        ds.add_image(ds.SOURCE, image_id=i, path=None, width=w, height=h, segments=segs, segment_class_ids=np.ones(len(segs), np.int32))
    ds.prepare()
    return ds


@pytest.mark.parametrize("kind", ["via", "coco"])
def test_device_boxes_equal_the_host_route(kind):
    from myolo.anchors import dataset_boxes, fit_anchors, kmeans_anchors
    from myolo.config import Config, make_config
    cfg = make_config(Config, IMAGE_SHAPE=[64, 64, 3])
    images, (r, c) = _images()
    ds = _via(images) if kind == "via" else _coco(images)
    full = ds.load_mask(2)[0]
    assert full[:, :, 1].sum() == 1 and full[r, c, 1]                    # one pixel at full resolution ...
    host, host_index = dataset_boxes(ds, cfg, device=None)
    assert list(np.bincount(host_index)) == [3, 9, 3]                   # ... and nothing in the network frame: absent
    for slots in (4, 32):                                                # slots=4: the 9 instances of image 1 span three rows
        boxes, index = dataset_boxes(ds, cfg, device=DEV, slots=slots)
        assert boxes.dtype == np.int32 and index.dtype == np.int64
        assert np.array_equal(boxes, host) and np.array_equal(index, host_index)
    first, first_index = dataset_boxes(ds, cfg, device=DEV, max_samples=1, slots=4)
    assert np.array_equal(first, host[:3]) and np.array_equal(first_index, host_index[:3])
    a = fit_anchors(ds, cfg, 3, device=DEV, slots=4, restarts=4, seed=1)
    b = kmeans_anchors(host, 3, cfg, restarts=4, seed=1, device=DEV)
    assert a.centroids_px.tobytes() == b.centroids_px.tobytes() and a.anchors == b.anchors and a.mean_iou.tobytes() == b.mean_iou.tobytes()
