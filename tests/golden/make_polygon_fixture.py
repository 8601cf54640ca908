#!/usr/bin/env python
"""Generates tests/golden/polygon_fixture.npz with the REAL skimage.draw.polygon (the reference's rasteriser of VIA outlines,
example/rice/rice_dataset.py:154).  scikit-image is not installed for the project interpreter; run this with a Python that has it, the
same one make_skimage_fixture.py is run with (scikit-image 0.18.3, numpy 1.26: both versions are recorded in the file).

Cases, in order (`names[k]`, vertices `verts[off[k]:off[k+1]]` as (row, col) float64, frame `frames[k]`):
  real/<set>/<subset>/<image>/<region>   every polygon of tests/golden/via/*/*/via_*_annotation.json (228).  The JSON carries no image size:
                                         the frame is (max y + 7, max x + 5) over the image's regions.
  syn/...                                about 200 synthetic outlines in frames of 40 x 56, 97 x 131 and 17 x 23: float vertices, vertices
                                         outside the frame on every side, vertices on pixel centres, horizontal edges through pixel rows,
                                         self-intersecting outlines, 1 / 2 / 3-collinear vertices, a closed ring (first vertex repeated), one
                                         outline of 1500 vertices, outlines of LDS_CHUNK - 1, LDS_CHUNK and LDS_CHUNK + 1 vertices (the vertex
                                         chunk of csrc/segment_kernels.hip), one polygon wholly outside its frame.
`bits` = np.packbits of all masks (row-major, case after case).  For every case the generator checks that skimage's (rr, cc) come in row-major
order, i.e. equal np.nonzero of the mask; the first cases' (rr, cc) are stored as they came (`rr`, `cc`, `rc_off`) so that a test can see it."""
import glob
import json
import os

import numpy as np
import skimage
import skimage.draw

HERE = os.path.dirname(os.path.abspath(__file__))
LDS_CHUNK = 256
FRAMES = [(40, 56), (97, 131), (17, 23)]
rng = np.random.default_rng(20261019)
names, polys, frames = [], [], []


def add(name, r, c, frame):
    names.append(name)
    polys.append(np.stack([np.asarray(r, np.float64), np.asarray(c, np.float64)], axis=1))
    frames.append((int(frame[0]), int(frame[1])))


# ---- the reference's own annotations
for path in sorted(glob.glob(os.path.join(HERE, "via", "*", "*", "via_*_annotation.json"))):
    tag = "/".join(path.split(os.sep)[-3:-1])
    entries = [a for a in json.load(open(path)).values() if a["regions"]]
    for i, a in enumerate(entries):
        regs = list(a["regions"].values()) if isinstance(a["regions"], dict) else a["regions"]
        shapes = [g["shape_attributes"] for g in regs]
        frame = (max(max(s["all_points_y"]) for s in shapes) + 7, max(max(s["all_points_x"]) for s in shapes) + 5)
        for j, s in enumerate(shapes):
            add("real/%s/%d/%d" % (tag, i, j), s["all_points_y"], s["all_points_x"], frame)
n_real = len(names)


# ---- synthetic outlines
def wobble(n, frame, phase=0.0):
    """a closed, wavy outline of n float vertices that fills most of the frame"""
    h, w = frame
    th = np.linspace(0, 2 * np.pi, n, endpoint=False) + phase
    rad = 1.0 + 0.15 * np.sin(17 * th) + 0.05 * np.cos(5 * th)
    return (h - 1) / 2.0 + 0.42 * h * rad * np.sin(th), (w - 1) / 2.0 + 0.42 * w * rad * np.cos(th)


k = 0
for i in range(60):                                  # float vertices, many of them outside the frame
    f = FRAMES[i % 3]
    n = int(rng.integers(3, 13))
    add("syn/float/%d" % i, rng.uniform(-0.3 * f[0], 1.3 * f[0], n), rng.uniform(-0.3 * f[1], 1.3 * f[1], n), f)
for i in range(30):                                  # integer vertices: vertices and edges ON pixel centres
    f = FRAMES[i % 3]
    n = int(rng.integers(3, 10))
    add("syn/int/%d" % i, rng.integers(-4, f[0] + 4, n), rng.integers(-4, f[1] + 4, n), f)
for i in range(24):                                  # horizontal (and vertical) edges through pixel rows: rectangles and staircases
    f = FRAMES[i % 3]
    r0, r1 = sorted(rng.integers(0, f[0], 2))
    c0, c1 = sorted(rng.uniform(-2, f[1] + 2, 2))
    if i % 2:
        add("syn/hrect/%d" % i, [r0, r0, r1, r1], [c0, c1, c1, c0], f)
    else:
        rm = (r0 + r1) // 2
        cm = (c0 + c1) / 2
        add("syn/stair/%d" % i, [r0, r0, rm, rm, r1, r1], [c0, cm, cm, c1, c1, c0], f)
for i in range(24):                                  # self-intersecting: star polygons and shuffled point sets
    f = FRAMES[i % 3]
    if i % 2:
        m = 5 + 2 * (i % 4)
        th = (np.arange(m) * (m // 2)) * 2 * np.pi / m + 0.1 * i
        add("syn/star/%d" % i, f[0] / 2 + 0.45 * f[0] * np.sin(th), f[1] / 2 + 0.45 * f[1] * np.cos(th), f)
    else:
        n = int(rng.integers(5, 11))
        add("syn/tangle/%d" % i, rng.uniform(0, f[0], n), rng.uniform(0, f[1], n), f)
for i, f in enumerate(FRAMES):                       # on every side of the frame at once, and wholly outside it
    add("syn/around/%d" % i, [-5, -5, f[0] + 5, f[0] + 5], [-7, f[1] + 7, f[1] + 7, -7], f)
    add("syn/outside/%d" % i, [-9.5, -3, -6], [f[1] + 2, f[1] + 9.5, f[1] + 20], f)
for i, f in enumerate(FRAMES):                       # degenerate inputs
    add("syn/one_int/%d" % i, [5], [7], f)
    add("syn/one_float/%d" % i, [5.5], [7.25], f)
    add("syn/two/%d" % i, [2, 12], [3, 18], f)
    add("syn/two_h/%d" % i, [6, 6], [3, 18], f)
    add("syn/col3_h/%d" % i, [4, 4, 4], [2, 9, 15], f)
    add("syn/col3_v/%d" % i, [2, 9, 15], [4, 4, 4], f)
    add("syn/col3_d/%d" % i, [1, 6, 11], [2, 7, 12], f)
    r, c = wobble(11, f)
    add("syn/ring/%d" % i, list(r) + [r[0]], list(c) + [c[0]], f)
for i, f in enumerate(FRAMES):                       # long outlines: the kernel stages vertices in chunks of LDS_CHUNK
    for n in (LDS_CHUNK - 1, LDS_CHUNK, LDS_CHUNK + 1):
        r, c = wobble(n, f, phase=0.3 * i)
        add("syn/chunk%+d/%d" % (n - LDS_CHUNK, i), r, c, f)
    r, c = wobble(1500, f, phase=0.7 * i)
    add("syn/long1500/%d" % i, r, c, f)
    r, c = wobble(2 * LDS_CHUNK + 3, f)              # integer vertices over three chunks
    add("syn/long_int/%d" % i, np.round(r), np.round(c), f)
for i in range(18):                                  # small float polygons: a few pixels, some none
    f = FRAMES[i % 3]
    cy, cx = rng.uniform(1, f[0] - 2), rng.uniform(1, f[1] - 2)
    n = int(rng.integers(3, 7))
    add("syn/small/%d" % i, cy + rng.uniform(-1.6, 1.6, n), cx + rng.uniform(-1.6, 1.6, n), f)

bits, rr_all, cc_all, rc_off, counts = [], [], [], [0], []
N_ORDER = 40
for k, (p, f) in enumerate(zip(polys, frames)):
    rr, cc = skimage.draw.polygon(p[:, 0], p[:, 1], shape=f)
    m = np.zeros(f, bool)
    m[rr, cc] = True
    assert len(rr) == int(m.sum())
    nz = np.nonzero(m)
    assert np.array_equal(rr, nz[0]) and np.array_equal(cc, nz[1]), "not row-major: %s" % names[k]
    bits.append(m.reshape(-1))
    counts.append(len(rr))
    if n_real <= k < n_real + N_ORDER:
        rr_all.append(rr)
        cc_all.append(cc)
        rc_off.append(rc_off[-1] + len(rr))
off = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.int64)
out = dict(skimage_version=np.array(skimage.__version__), numpy_version=np.array(np.__version__), lds_chunk=np.array(LDS_CHUNK),
           names=np.array(names), n_real=np.array(n_real), verts=np.concatenate(polys), off=off, frames=np.array(frames, np.int32),
           counts=np.array(counts, np.int64), bits=np.packbits(np.concatenate(bits)),
           order_first=np.array(n_real), rr=np.concatenate(rr_all).astype(np.int32), cc=np.concatenate(cc_all).astype(np.int32),
           rc_off=np.array(rc_off, np.int64))
path = os.path.join(HERE, "polygon_fixture.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes;", len(names), "cases,", n_real, "real; empty:", int((np.array(counts) == 0).sum()),
      "; scikit-image", skimage.__version__, "numpy", np.__version__)
