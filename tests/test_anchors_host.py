"""myolo.anchors on the host: the binding and the refusals of myolo_anchor_kmeans, the pinned initial draws, the errors raised before anything
reaches a device, AnchorResult's anchors / overrides / file, and dataset_boxes' host route against load_image_gt -- no GPU."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _lib():
    from myolo import _ext as X
    return X.load()


def test_library_exports_the_two_entry_points():
    import __graft_entry__ as G
    from myolo import _ext as X
    lib = _lib()
    assert hasattr(lib, "myolo_anchor_kmeans") and hasattr(lib, "myolo_anchor_kmeans_ws_bytes")
    assert len(X.SIGS["myolo_anchor_kmeans"]) == 14
    assert "myolo_anchor_kmeans" in X.exported_symbols() and "myolo_anchor_kmeans_ws_bytes" in X.exported_symbols()
    assert ("anchors_kernels.hip", ["-ffp-contract=off"]) in G.UNITS
    src = open(os.path.join(ROOT, "mask-yolo_amd", "csrc", "anchors_kernels.hip")).read()
    assert "fp contract(off)" in src


def _call(lib, n=100, runs=2, ks=(3, 5), max_iter=10, ws_short=0, null=None):
    """every pointer is a live host buffer (a refused call reads run_k and launches nothing) -> (status, message)"""
    from myolo import _ext as X
    need = X.anchor_kmeans_ws_bytes(max(n, 1), max(runs, 1))
    bufs = {name: ctypes.create_string_buffer(4096) for name in ("wh", "centroids", "counts", "iterations", "converged", "mean_iou", "assign", "ws")}
    run_k = (ctypes.c_int32 * max(len(ks), 1))(*ks)
    p = {name: ctypes.addressof(b) for name, b in bufs.items()}
    p["run_k"] = ctypes.addressof(run_k)
    if null is not None:
        p[null] = None
    rc = lib.myolo_anchor_kmeans(p["wh"], n, p["run_k"], p["centroids"], runs, max_iter, p["counts"], p["iterations"], p["converged"],
                                 p["mean_iou"], p["assign"], p["ws"], max(need - ws_short, 0), None)
    return rc, lib.myolo_last_error_string().decode()


@pytest.mark.parametrize("kw", [dict(null="wh"), dict(null="run_k"), dict(null="centroids"), dict(null="counts"), dict(null="iterations"),
                                dict(null="converged"), dict(null="mean_iou"), dict(null="ws"),
                                dict(n=0), dict(n=-5), dict(runs=0), dict(runs=-1), dict(ks=(3, 0)), dict(ks=(33, 5)), dict(ks=(-1, 5)),
                                dict(max_iter=0), dict(ws_short=1)],
                         ids=lambda kw: "-".join("%s=%s" % kv for kv in kw.items()))
def test_refusals_come_back_as_einval_with_the_prefix(kw):
    rc, msg = _call(_lib(), **kw)
    assert rc == EINVAL and msg.startswith("anchor_kmeans: "), (rc, msg)


def test_workspace_grows_with_n_and_with_runs():
    from myolo import _ext as X
    a, b, c = X.anchor_kmeans_ws_bytes(1000, 8), X.anchor_kmeans_ws_bytes(1000000, 8), X.anchor_kmeans_ws_bytes(1000, 80)
    assert 0 < a < b and a < c
    assert b >= 8 * 1000000                                       # one byte per point and run: the previous assignment
    assert X.anchor_kmeans_ws_bytes(1, 1) > 0


def test_initial_centroids_are_the_pinned_distinct_draws():
    from myolo.anchors import initial_centroids
    wh = np.random.RandomState(3).randint(1, 40, (200, 2)).astype(np.int32)
    wh[50:100] = wh[:50]                                          # duplicates: the draw is over the distinct sizes
    u = np.unique(wh, axis=0)
    got = initial_centroids(wh, 5, restarts=4, seed=7)
    assert got.shape == (4, 5, 2) and got.dtype == np.float64
    for r in range(4):
        want = u[np.random.RandomState(7 + r).permutation(len(u))[:5]]
        assert np.array_equal(got[r], want.astype(np.float64))
        assert len(np.unique(got[r], axis=0)) == 5
    assert np.array_equal(initial_centroids(wh, 5, restarts=2, seed=8)[0], got[1])


def test_errors_raised_before_anything_reaches_a_device():
    from myolo.anchors import box_sizes, kmeans_anchors, sweep_anchors
    from myolo.config import Config, make_config
    cfg = make_config(Config)
    lattice = np.array([[8, 8], [8, 16], [16, 8]] * 10, np.int32)
    with pytest.raises(ValueError, match="3 distinct sizes"):
        kmeans_anchors(lattice, 4, cfg)
    with pytest.raises(ValueError, match="3 distinct sizes"):
        sweep_anchors(lattice, cfg, ks=[1, 2, 3, 4])
    with pytest.raises(ValueError, match="width or height < 1"):
        kmeans_anchors(np.array([[4, 4], [0, 3], [5, 5]]), 1, cfg)
    with pytest.raises(ValueError, match="width or height < 1"):
        kmeans_anchors(np.array([[10, 10, 20, 20], [10, 10, 10, 30]]), 1, cfg)         # a box of width 0
    with pytest.raises(ValueError):
        kmeans_anchors(lattice, 33, cfg)
    with pytest.raises(ValueError):
        kmeans_anchors(lattice, 2, cfg, init=[[4., 4.], [0., 3.]])
    assert np.array_equal(box_sizes(np.array([[1, 2, 11, 32]])), [[10, 30]]) and box_sizes(np.array([[3., 4.]])).dtype == np.int32


def test_anchors_overrides_and_file_of_a_hand_built_result(tmp_path):
    from myolo.anchors import AnchorResult
    from myolo.config import Config, RiceConfig, make_config
    cent = np.array([[[100., 50.], [20., 30.], [64., 64.]],
                     [[96., 48.], [16., 24.], [72.5, 40.25]]])
    counts = np.array([[3, 4, 5], [2, 5, 5]])
    for base, size in ((Config, 224), (RiceConfig, 416)):
        cfg = make_config(base, IMAGE_SHAPE=[size, size, 3])
        assert cfg.GRID_W == size // 32
        res = AnchorResult(cent, counts, [4, 5], [1, 1], [0.5, 0.75], cfg)
        assert res.best == 1 and res.k == 3
        # the best run, pixels / 32, sorted by width
        assert res.anchors == [16 / 32., 24 / 32., 72.5 / 32., 40.25 / 32., 96 / 32., 48 / 32.]
        assert res.overrides() == {"ANCHORS": res.anchors, "N_BOX": 3}
        new = make_config(base, IMAGE_SHAPE=[size, size, 3], **res.overrides())
        assert new.N_BOX == 3 and new.TRAIN_ROIS_PER_IMAGE == new.GRID_H * new.GRID_W * 3 and list(new.ANCHORS) == res.anchors
        path = str(tmp_path / ("anchors_3_%d.txt" % size))
        res.save(path)
        assert open(path).read() == "0.50, 0.75\n2.27, 1.26\n3.00, 1.50\n"
    tie = AnchorResult(cent, counts, [4, 5], [1, 1], [0.75, 0.75], make_config(Config))
    assert tie.best == 0 and tie.anchors[:2] == [20 / 32., 30 / 32.]


def test_dataset_boxes_host_route_equals_load_image_gt():
    from myolo.anchors import dataset_boxes
    from myolo.config import ShapesConfig, make_config
    from myolo.myolo_utils import load_image_gt
    from myolo.shapes import ShapesDataset
    ds = ShapesDataset(seed=5)
    ds.load_shapes(6, 96, 128)                                    # not the network frame: the masks are resized
    ds.prepare()
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[64, 64, 3])
    want = [load_image_gt(ds, cfg, i)[2] for i in ds.image_ids]
    boxes, index = dataset_boxes(ds, cfg)                         # no load_segments / load_polygons: the host route, no device
    assert boxes.dtype == np.int32 and index.dtype == np.int64
    assert np.array_equal(boxes, np.concatenate(want))
    assert np.array_equal(index, np.concatenate([np.full(len(b), i) for i, b in zip(ds.image_ids, want)]))
    assert len(boxes) >= 6 and ((boxes[:, 2] > boxes[:, 0]) & (boxes[:, 3] > boxes[:, 1])).all()
    b2, i2 = dataset_boxes(ds, cfg, max_samples=2)
    assert np.array_equal(b2, boxes[index < 2]) and np.array_equal(i2, index[index < 2])
