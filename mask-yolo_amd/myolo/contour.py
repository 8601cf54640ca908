"""Mask outlines on the host (numpy only): the form MaskYOLO.detect(..., mask_format="polygon") returns, restated edge by edge.

Coordinates are lattice CORNER coordinates, COCO's: pixel (y, x) is the square [x, x+1] x [y, y+1], X runs 0..w and Y 0..h, pixels outside the frame
are 0.  Every set pixel contributes one directed unit edge on each side whose neighbour is 0, the inside on the right of travel:

    top     (x, y)     -> (x+1, y)      E = 0          bottom  (x+1, y+1) -> (x, y+1)    W = 2
    right   (x+1, y)   -> (x+1, y+1)    S = 1          left    (x, y+1)   -> (x, y)      N = 3

An edge's key is (Y, X, dir) of its start corner.  The successor of an edge that arrives at corner c with direction d is the first existing edge
leaving c among (d+1)%4, d, (d+3)%4 -- right turn, straight, left turn -- so two pixels that touch only diagonally stay apart and every loop is
a simple polygon.  The successor is a permutation of the edges; its cycles are the loops.  A vertex is the start corner of an edge whose
predecessor has another direction.  Loops ascend by their smallest edge key; a loop's vertices run in traversal order from the start corner of
its smallest edge (always a vertex): an outer loop starts at its top-left corner heading east and runs clockwise on screen (signed_area > 0), a
hole starts heading south and runs the other way (signed_area < 0).  The XOR over the loops of polygon_mask(Y - 0.5, X - 0.5, (h, w)) is the mask.
"""
import numpy as np

DX = (1, 0, -1, 0)           # E S W N
DY = (0, 1, 0, -1)


def trace(mask):
    """bool [h,w] -> list of int32 [n,2] arrays (X, Y), one per closed loop, in the order stated above"""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError("trace: a [h,w] mask is expected (got shape %s)" % (tuple(m.shape),))
    m = m.astype(bool)
    h, w = m.shape
    p = np.zeros((h + 2, w + 2), bool)
    p[1:h + 1, 1:w + 1] = m
    # the four pixels round corner (X, Y): a b above (columns X-1, X of row Y-1), c d below
    a, b, c, d = p[0:h + 1, 0:w + 1], p[0:h + 1, 1:w + 2], p[1:h + 2, 0:w + 1], p[1:h + 2, 1:w + 2]
    leaves = np.stack([d & ~b, c & ~d, a & ~c, b & ~a], axis=2)          # [Y, X, dir]: the edge that starts here with this direction exists
    flat = leaves.reshape(-1)
    edges = np.flatnonzero(flat)                                           # edge ids = ((Y * (w+1)) + X) * 4 + dir, ascending = key order
    if edges.size == 0:
        return []
    index = np.full(flat.size, -1, np.int64)
    index[edges] = np.arange(edges.size)
    corner, dirs = edges // 4, edges % 4
    Y, X = corner // (w + 1), corner % (w + 1)
    eY, eX = Y + np.take(DY, dirs), X + np.take(DX, dirs)
    right, left = (dirs + 1) % 4, (dirs + 3) % 4
    nd = np.where(leaves[eY, eX, right], right, np.where(leaves[eY, eX, dirs], dirs, left))
    succ = index[(eY * (w + 1) + eX) * 4 + nd]
    assert (succ >= 0).all() and np.array_equal(np.sort(succ), np.arange(edges.size))      # a permutation
    is_vertex = np.zeros(edges.size, bool)
    is_vertex[succ] = nd != dirs
    # the next VERTEX edge behind every edge, by pointer doubling over the straight stretches
    nxt = succ.copy()
    while True:
        short = ~is_vertex[nxt]
        if not short.any():
            break
        nxt[short] = nxt[nxt[short]]
    loops, seen = [], np.zeros(edges.size, bool)
    for e in np.flatnonzero(is_vertex):
        if seen[e]:
            continue
        ring, k = [], e
        while not seen[k]:
            seen[k] = True
            ring.append(k)
            k = nxt[k]
        loops.append(np.stack([X[ring], Y[ring]], axis=1).astype(np.int32))
    return loops


def signed_area(loop):
    """the shoelace sum of a loop in pixels: > 0 for an outer loop (clockwise on screen, y down), < 0 for a hole"""
    q = np.asarray(loop, dtype=np.int64).reshape(-1, 2)
    x, y = q[:, 0], q[:, 1]
    twice = int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())
    return twice / 2.0


def outer_loops(loops):
    """the loops that bound a piece from outside (the holes dropped), order kept"""
    return [l for l in loops if signed_area(l) > 0]


def _distance(pts, p, q):
    """distance of every point of pts [n,2] from the segment p - q"""
    pts, p, q = np.asarray(pts, np.float64), np.asarray(p, np.float64), np.asarray(q, np.float64)
    pq = q - p
    L = float(pq @ pq)
    if L == 0.0:
        return np.hypot(pts[:, 0] - p[0], pts[:, 1] - p[1])
    t = np.clip(((pts - p) @ pq) / L, 0.0, 1.0)
    foot = p + t[:, None] * pq
    return np.hypot(pts[:, 0] - foot[:, 0], pts[:, 1] - foot[:, 1])


def simplify(loop, tolerance):
    """Douglas-Peucker on the closed loop, anchored at its first vertex and at the vertex farthest from it: every dropped vertex lies within
    `tolerance` of the simplified outline; tolerance 0 returns the input unchanged.  -> [m,2], the loop's dtype, a subsequence of the loop"""
    loop = np.asarray(loop)
    n = loop.shape[0]
    if tolerance < 0:
        raise ValueError("simplify: tolerance must be >= 0 (got %r)" % (tolerance,))
    if tolerance == 0 or n <= 3:
        return loop
    pts = loop.astype(np.float64)
    far = int(np.argmax(np.hypot(pts[:, 0] - pts[0, 0], pts[:, 1] - pts[0, 1])))
    keep = np.zeros(n + 1, bool)                       # index n stands for the first vertex again: the closing chain far .. n
    keep[[0, far, n]] = True
    ring = np.concatenate([pts, pts[:1]])
    stack = [(0, far), (far, n)]
    while stack:
        i, j = stack.pop()
        if j - i < 2:
            continue
        dist = _distance(ring[i + 1:j], ring[i], ring[j])
        k = int(np.argmax(dist))
        if dist[k] > tolerance:
            k += i + 1
            keep[k] = True
            stack += [(i, k), (k, j)]
    return loop[keep[:n]]
