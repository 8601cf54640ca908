"""
Polygon fill on the host: ``skimage.draw.polygon`` (scikit-image 0.18.3) restated in numpy, bit for bit.

The reference's rice / food datasets fill VIA outlines with skimage.draw.polygon (example/rice/rice_dataset.py:154).  scikit-image does not
use the textbook even-odd ray test: its point_in_polygon counts crossings to the right AND to the left of the pixel and treats a pixel that
sits on a vertex or an edge as inside.  For pixel (y, x) and vertices (r[i], c[i]) taken cyclically, all in float64:

    x0 = c[prev]-x; y0 = r[prev]-y
    for each vertex i:
        x1 = c[i]-x; y1 = r[i]-y
        if |x1| < 1e-12 and |y1| < 1e-12: ON (vertex)
        q = (x1*y0 - x0*y1) / (y0 - y1)
        if (y1 > 0) != (y0 > 0) and q > 0: r_cross += 1
        if (y1 < 0) != (y0 < 0) and q < 0: l_cross += 1
        x0, y0 = x1, y1
    ON if r_cross and l_cross differ in parity (edge), or r_cross is odd (inside)  ==  either parity is odd

This is the arithmetic contract of the device rasteriser too (csrc/segment_kernels.hip): the two products, their
difference and the quotient are single binary64 operations in that order.  Pinned by tests/golden/polygon_fixture.npz (outputs of the real
function).
"""
import numpy as np

EPS = 1e-12


def _vertices(r, c):
    r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
    c = np.ascontiguousarray(c, dtype=np.float64).reshape(-1)
    if r.shape != c.shape:
        raise ValueError("polygon: r and c must have the same length, got %d and %d" % (r.shape[0], c.shape[0]))
    if not (np.isfinite(r).all() and np.isfinite(c).all()):
        raise ValueError("polygon: vertex coordinates must be finite")
    return r, c


def polygon_mask_sampled(r, c, src_row, src_col):
    """-> bool [H,W]: the fill evaluated ONLY at the source pixels (src_row[i], src_col[j]) -- polygon_mask(r, c, shape)[src_row][:, src_col]
    without the full-resolution mask.  With the index tables of myolo_utils.mask_index_tables this is what resize_mask makes of the filled
    mask.  Work is one [rows straddled, W] quotient per edge, so a long outline costs its perimeter, not its vertex count times the frame."""
    r, c = _vertices(r, c)
    ys = np.asarray(src_row, dtype=np.float64).reshape(-1)
    xs = np.asarray(src_col, dtype=np.float64).reshape(-1)
    H, W = ys.shape[0], xs.shape[0]
    rc = np.zeros((H, W), bool)              # parity of the crossings to the right
    lc = np.zeros((H, W), bool)              # ... to the left
    vt = np.zeros((H, W), bool)              # pixel on a vertex
    if r.shape[0] == 0:
        return vt
    y0, x0 = r[-1] - ys, c[-1] - xs
    for i in range(r.shape[0]):
        y1, x1 = r[i] - ys, c[i] - xs
        ny = np.abs(y1) < EPS
        if ny.any():
            nx = np.abs(x1) < EPS
            if nx.any():
                vt[np.ix_(ny, nx)] = True
        sr = (y1 > 0) != (y0 > 0)
        sl = (y1 < 0) != (y0 < 0)
        rows = np.nonzero(sr | sl)[0]
        if rows.shape[0]:
            a, b = y0[rows, None], y1[rows, None]
            q = (x1[None, :] * a - x0[None, :] * b) / (a - b)
            rc[rows] ^= sr[rows, None] & (q > 0)
            lc[rows] ^= sl[rows, None] & (q < 0)
        y0, x0 = y1, x1
    return vt | rc | lc


def polygon_mask(r, c, shape):
    """-> bool [h,w]: True where skimage.draw.polygon(r, c, shape) lists the pixel."""
    h, w = int(shape[0]), int(shape[1])
    return polygon_mask_sampled(r, c, np.arange(h), np.arange(w))


def polygon(r, c, shape):
    """-> (rr, cc): the pixels of the filled polygon inside the `shape` frame, in scikit-image's order (row-major)."""
    rr, cc = np.nonzero(polygon_mask(r, c, shape))
    return rr.astype(np.intp), cc.astype(np.intp)
