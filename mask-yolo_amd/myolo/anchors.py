"""
Fit the YOLO anchors to a dataset: the working counterpart of the reference's example/*/03_anchor_generator.ipynb (k-means over the boxes' (w, h)
with 1 - IoU as the distance; its anchors_5.txt files are where Config.ANCHORS and RiceConfig.ANCHORS come from).  The first step of the
custom-dataset workflow: load_via / load_coco -> fit_anchors -> make_config(**result.overrides()) -> train -> evaluate.

    boxes, image_index = dataset_boxes(dataset, config)        # the boxes training sees, from the device rasteriser
    result = kmeans_anchors(boxes, 5, config)                   # 8 seeded restarts in one call of the kernel
    config = make_config(Config, IMAGE_SHAPE=config.IMAGE_SHAPE, **result.overrides())

The clustering runs on the device (myolo_anchor_kmeans, csrc/anchors_kernels.hip; the contract: DESIGN.md section 19): every restart and, in
sweep_anchors, every k is one run of ONE call.  Differences from the notebook: the sizes are pixels of the network frame (integers, so the
cluster sums are exact and a result is the same bits from run to run); the initial centroids are DISTINCT sizes drawn by a seeded generator (the
notebook draws with replacement from an unseeded one); a cluster that loses all its points keeps its centroid (the notebook divides by zero and
its centroids are NaN from then on: "Iter 105: distances: nan" in its recorded output); a point goes to the lowest index among equal distances.
"""
import numpy as np

from . import myolo_utils as mutils

KMAX = 32           # clusters of a run (ANCH_KMAX of csrc/anchors_kernels.hip)
CHUNK_ROWS = 32     # rows of slots that one myolo_segment_masks call of dataset_boxes fills


# ------------------------------------------------------------------ the boxes of a dataset
def _frame(config):
    return int(config.IMAGE_SHAPE[0]), int(config.IMAGE_SHAPE[1])


def _host_boxes(dataset, config, ids):
    H, W = _frame(config)
    boxes, index = [], []
    for i in ids:
        mask, _ = dataset.load_mask(i)
        h, w = mask.shape[:2]
        if [h, w] != [H, W]:
            mask = mutils.resize_mask(mask, [H / h, W / w])
            if list(mask.shape[:2]) != [H, W]:
                raise ValueError("image %r: %d x %d does not resize to the %d x %d network frame" % (i, h, w, H, W))
        mask = mask[:, :, np.sum(mask, axis=(0, 1)) > 0]
        b = mutils.extract_bboxes(mask)
        boxes.append(b)
        index.append(np.full(b.shape[0], int(i), np.int64))
    if not boxes:
        return np.zeros((0, 4), np.int32), np.zeros(0, np.int64)
    return np.concatenate(boxes).astype(np.int32), np.concatenate(index)


def dataset_boxes(dataset, config, device="cuda:0", max_samples=None, slots=32):
    """-> (boxes int32 [n,4] x1,y1,x2,y2 in the network frame (far corner exclusive), image_index int64 [n] = the dataset's image id of each box):
    the boxes training sees -- the tight box of every instance's mask after resize_mask's sampling, image by image, instances in order.  An instance
    that sets no sampled pixel is dropped, as load_image_gt drops it.  ALL instances of an image count, not the first MAX_GT_INSTANCES.

    A dataset with load_segments (myolo.coco) or load_polygons (myolo.via) goes the device route: the image size comes from image_info's height /
    width (no image file is opened), the segments and the index tables of CHUNK_ROWS rows of `slots` instances go up per chunk, and
    myolo_segment_masks leaves the boxes (its masks land in one reused scratch buffer).  An image with more than `slots` instances takes several
    rows with the same tables.  Any other dataset -- or any dataset with device=None -- goes the host route: load_mask, resize_mask,
    extract_bboxes; that one needs no device."""
    H, W = _frame(config)
    ids = [int(i) for i in dataset.image_ids]
    if max_samples is not None:
        ids = ids[:max_samples]
    if device is None or not (hasattr(dataset, "load_segments") or hasattr(dataset, "load_polygons")):
        return _host_boxes(dataset, config, ids)
    import torch
    from .engine import Net
    T = int(slots)
    if T < 1:
        raise ValueError("dataset_boxes: slots=%r; at least 1" % (slots,))
    rows_of = []                                             # (image id, its segments of this row, (row table, column table), source height)
    for i in ids:
        info = dataset.image_info[i]
        h, w = int(info["height"]), int(info["width"])
        segs, _ = mutils.segments_of(dataset, i)
        for s in segs:
            if isinstance(s, dict) and ([int(v) for v in s["size"]] != [h, w] or int(np.sum(s["counts"])) != h * w or h * w >= 1 << 31):
                raise ValueError("image %r: a run-length code does not cover its %d x %d image" % (i, h, w))
        r, c = mutils.mask_index_tables(h, w, [H / h, W / w])
        if r.shape[0] != H or c.shape[0] != W:
            raise ValueError("image %r: %d x %d does not resize to the %d x %d network frame" % (i, h, w, H, W))
        tables = (r.astype(np.int32), c.astype(np.int32))
        for lo in range(0, len(segs), T):
            rows_of.append((i, segs[lo:lo + T], tables, h))
    if not rows_of:
        return np.zeros((0, 4), np.int32), np.zeros(0, np.int64)
    dev = torch.device(device)
    B = min(CHUNK_ROWS, len(rows_of))
    scratch = torch.empty((B, H, W, T), dtype=torch.uint8, device=dev)
    boxes_d = torch.empty((B, T, 4), dtype=torch.int32, device=dev)
    boxes, index = [], []
    with torch.cuda.device(dev):
        for lo in range(0, len(rows_of), B):
            grp = rows_of[lo:lo + B]
            tables = [torch.from_numpy(a).to(dev) for a in mutils.segment_tables([g[1:] for g in grp], B, T, H, W)]
            Net.segment_masks(tables, scratch, boxes_d)
            got = boxes_d.cpu().numpy()                      # (synchronises: the tables are free to go)
            for k, g in enumerate(grp):
                b = got[k, :len(g[1])]
                b = b[b[:, 2] > 0]                           # a slot without a set pixel reads 0, 0, 0, 0
                boxes.append(b)
                index.append(np.full(b.shape[0], g[0], np.int64))
    return np.concatenate(boxes).astype(np.int32), np.concatenate(index)


# ------------------------------------------------------------------ the clustering
def box_sizes(boxes_or_wh):
    """[n,4] x1,y1,x2,y2 boxes or [n,2] (w, h) sizes of positive integers -> int32 [n,2] sizes.  ValueError for a row with w < 1 or h < 1."""
    a = np.asarray(boxes_or_wh)
    if a.ndim != 2 or a.shape[1] not in (2, 4) or a.shape[0] < 1:
        raise ValueError("anchors: [n,4] boxes or [n,2] sizes with n >= 1 are needed, got an array of shape %s" % (a.shape,))
    if not np.issubdtype(a.dtype, np.integer):
        if not (np.isfinite(a).all() and (a == np.rint(a)).all()):
            raise ValueError("anchors: box sizes are whole pixels of the network frame")
    a = a.astype(np.int64)
    wh = a if a.shape[1] == 2 else np.stack([a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]], axis=1)
    bad = np.where((wh < 1).any(axis=1))[0]
    if bad.shape[0]:
        raise ValueError("anchors: %d rows have a width or height < 1 (the first: row %d, %d x %d)" %
                         (bad.shape[0], bad[0], wh[bad[0], 0], wh[bad[0], 1]))
    if wh.max() >= 1 << 31:
        raise ValueError("anchors: a size beyond 2^31 - 1")
    return np.ascontiguousarray(wh, np.int32)


def initial_centroids(wh, k, restarts=8, seed=0):
    """-> float64 [restarts,k,2]: with u = np.unique(wh, axis=0), run r starts from u[np.random.RandomState(seed + r).permutation(len(u))[:k]] --
    DISTINCT sizes, so no cluster starts empty.  ValueError when there are fewer than k distinct sizes."""
    u = np.unique(np.asarray(wh), axis=0)
    if len(u) < k:
        raise ValueError("anchors: k = %d clusters but only %d distinct sizes" % (k, len(u)))
    return np.stack([u[np.random.RandomState(seed + r).permutation(len(u))[:k]] for r in range(restarts)]).astype(np.float64)


class AnchorResult(object):
    """The runs of one k.  Per run: centroids_px float64 [runs,k,2] (w, h in pixels), counts int64 [runs,k], iterations int32 [runs], converged
    bool [runs], mean_iou float64 [runs], assign int32 [runs,n] (None unless asked for).  best = the run with the largest mean_iou, the lowest
    index on a tie; anchors = its centroids in grid units, sorted by width, flattened like Config.ANCHORS."""

    def __init__(self, centroids_px, counts, iterations, converged, mean_iou, config, assign=None):
        if isinstance(config, type):
            config = config()
        self.centroids_px = np.asarray(centroids_px, np.float64)
        self.k = int(self.centroids_px.shape[1])
        self.counts = np.asarray(counts, np.int64)
        self.iterations = np.asarray(iterations, np.int32)
        self.converged = np.asarray(converged).astype(bool)
        self.mean_iou = np.asarray(mean_iou, np.float64)
        self.assign = assign
        H, W = _frame(config)
        self.cell = (W / float(config.GRID_W), H / float(config.GRID_H))          # pixels per grid cell (w, h)

    @property
    def best(self):
        return int(np.argmax(self.mean_iou))

    @property
    def anchors(self):
        c = self.centroids_px[self.best] / np.asarray(self.cell, np.float64)
        c = c[np.argsort(c[:, 0], kind="stable")]                                # as the reference's save_anchors sorts
        return [float(v) for v in c.reshape(-1)]

    def overrides(self):
        """-> the make_config overrides of the best run: make_config(Base, **result.overrides())"""
        return {"ANCHORS": self.anchors, "N_BOX": self.k}

    def save(self, path):
        """the reference's anchors_K.txt: one 'w, h' line per anchor, two decimals, sorted by width"""
        a = self.anchors
        with open(path, "w") as f:
            for j in range(self.k):
                f.write('%0.2f, %0.2f\n' % (a[2 * j], a[2 * j + 1]))


def _check_init(init, k):
    c = np.asarray(init, np.float64)
    if c.ndim == 2:
        c = c[None]
    if c.ndim != 3 or c.shape[1] != k or c.shape[2] != 2 or c.shape[0] < 1:
        raise ValueError("anchors: init is [k,2] or [runs,k,2] with k = %d, got shape %s" % (k, np.asarray(init).shape))
    if not (np.isfinite(c).all() and (c > 0).all()):
        raise ValueError("anchors: init holds a centroid that is not a positive size")
    return c


def _fit(wh, starts, max_iter, device, want_assign):
    """starts: a list of float64 [k_r,2] initial centroids, one per run -> the device's outputs as host arrays (padded to KMAX clusters)"""
    import torch
    from . import _ext as X
    runs, n = len(starts), int(wh.shape[0])
    run_k = np.asarray([s.shape[0] for s in starts], np.int32)
    if run_k.min() < 1 or run_k.max() > KMAX:
        raise ValueError("anchors: k = %d; 1 .. %d clusters" % (run_k.max() if run_k.max() > KMAX else run_k.min(), KMAX))
    cent = np.zeros((runs, KMAX, 2), np.float64)
    for r, s in enumerate(starts):
        cent[r, :s.shape[0]] = s
    dev = torch.device(device)
    with torch.cuda.device(dev):
        wh_d = torch.from_numpy(wh).to(dev)
        cent_d = torch.from_numpy(cent).to(dev)
        counts = torch.empty((runs, KMAX), dtype=torch.int64, device=dev)
        iters = torch.empty(runs, dtype=torch.int32, device=dev)
        conv = torch.empty(runs, dtype=torch.int32, device=dev)
        miou = torch.empty(runs, dtype=torch.float64, device=dev)
        assign = torch.empty((runs, n), dtype=torch.int32, device=dev) if want_assign else None
        ws = torch.empty(X.anchor_kmeans_ws_bytes(n, runs), dtype=torch.uint8, device=dev)
        # (the entry point synchronises the stream before it returns: run_k has been read and the outputs are final)
        X.call("myolo_anchor_kmeans", X.ptr(wh_d), n, run_k.ctypes.data, X.ptr(cent_d), runs, int(max_iter), X.ptr(counts), X.ptr(iters),
               X.ptr(conv), X.ptr(miou), X.ptr(assign), X.ptr(ws), ws.numel(), X.stream())
        return (cent_d.cpu().numpy(), counts.cpu().numpy(), iters.cpu().numpy(), conv.cpu().numpy(), miou.cpu().numpy(),
                None if assign is None else assign.cpu().numpy())


def _result(out, lo, hi, k, config):
    cent, counts, iters, conv, miou, assign = out
    return AnchorResult(cent[lo:hi, :k].copy(), counts[lo:hi, :k].copy(), iters[lo:hi].copy(), conv[lo:hi].copy(), miou[lo:hi].copy(), config,
                        None if assign is None else assign[lo:hi].copy())


def kmeans_anchors(boxes_or_wh, k, config, restarts=8, seed=0, max_iter=300, init=None, device="cuda:0", assign=False):
    """k anchors for [n,4] boxes or [n,2] sizes (positive integers: pixels of the network frame) -> AnchorResult of `restarts` runs, all in one call
    of myolo_anchor_kmeans.  Run r starts from initial_centroids(wh, k, restarts, seed)[r]; init (float [k,2], or [runs,k,2]; pixels) replaces the
    draw -- duplicates are allowed there (equal centroids tie, the lower index takes the points, the other cluster stays empty and keeps its
    centroid).  A run stops after the first pass that changes no assignment, or after max_iter passes (converged False).  assign=True also returns
    every run's assignment."""
    wh = box_sizes(boxes_or_wh)
    k = int(k)
    if not 1 <= k <= KMAX:
        raise ValueError("anchors: k = %d; 1 .. %d clusters" % (k, KMAX))
    if int(max_iter) < 1:
        raise ValueError("anchors: max_iter = %r; at least 1" % (max_iter,))
    starts = _check_init(init, k) if init is not None else initial_centroids(wh, k, restarts, seed)
    out = _fit(wh, list(starts), max_iter, device, assign)
    return _result(out, 0, len(starts), k, config)


def sweep_anchors(boxes_or_wh, config, ks=range(1, 11), restarts=8, seed=0, max_iter=300, device="cuda:0", assign=False):
    """The notebook's n_clusters = 0 mode: every k of ks with `restarts` runs each, ALL (k, restart) pairs through one call of the kernel ->
    {k: AnchorResult}, and so the curve of the mean IoU against k ([(k, r.mean_iou[r.best]) for k, r in result.items()]).  Restart r of every k
    draws with seed + r, as kmeans_anchors does."""
    wh = box_sizes(boxes_or_wh)
    ks = [int(k) for k in ks]
    if not ks or min(ks) < 1 or max(ks) > KMAX or len(set(ks)) != len(ks):
        raise ValueError("anchors: ks = %r; distinct values in 1 .. %d" % (ks, KMAX))
    if int(max_iter) < 1:
        raise ValueError("anchors: max_iter = %r; at least 1" % (max_iter,))
    starts = []
    for k in ks:
        starts += list(initial_centroids(wh, k, restarts, seed))
    out = _fit(wh, starts, max_iter, device, assign)
    return {k: _result(out, j * restarts, (j + 1) * restarts, k, config) for j, k in enumerate(ks)}


def fit_anchors(dataset, config, k, device="cuda:0", max_samples=None, slots=32, **kw):
    """kmeans_anchors on dataset_boxes(dataset, config): the anchors of a dataset in one call"""
    boxes, _ = dataset_boxes(dataset, config, device=device, max_samples=max_samples, slots=slots)
    return kmeans_anchors(boxes, k, config, device=device, **kw)
