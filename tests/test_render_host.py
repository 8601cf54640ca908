"""The host statement of the overlay (myolo/render.py): the blend and the palette against the reference's own apply_mask
and random_colors (tests/golden/ref_render.npz, made by tests/golden/make_render_fixture.py), the outline and box rules on hand-made masks,
and the PNG writer against its reader.  No GPU."""
import os
import struct
import zlib

import numpy as np
import pytest

from myolo import render

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_render.npz")


@pytest.fixture(scope="module")
def ref():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_blend_layer_is_the_reference_apply_mask_bit_for_bit(ref):
    image, masks, colors = ref["image"], ref["masks"], ref["colors"]
    assert image.shape == (12, 17, 3) and masks.shape == (12, 17, 3)
    assert sorted(set(masks.sum(axis=2).ravel().tolist())) == [0, 1, 2, 3]           # single, double and triple blends are all in the picture
    nowin = np.zeros((3, 4), np.int64)
    for alpha in ref["alphas"].tolist():
        want = ref["blend_%02d" % round(alpha * 10)]
        assert want.dtype == np.uint32 and want.max() <= 255
        got = render.render_instances(image, nowin, masks, colors, alpha=alpha, show_outline=False, show_bbox=False)
        assert got.dtype == np.uint8 and np.array_equal(got, want.astype(np.uint8)), alpha
        assert np.array_equal(render.render_instances(image, nowin, masks.astype(bool), colors, alpha=alpha, show_outline=False, show_bbox=False), got)
    # the order matters (a truncation between two blends): the fixture would tell a renderer that blends in another order apart
    swapped = render.render_instances(image, nowin, masks[:, :, ::-1], colors[::-1], alpha=0.5, show_outline=False, show_bbox=False)
    assert not np.array_equal(swapped, ref["blend_05"].astype(np.uint8))
    # nothing switched on, or no instance: the image
    assert np.array_equal(render.render_instances(image, nowin, masks, colors, show_mask=False, show_outline=False, show_bbox=False), image)
    assert np.array_equal(render.render_instances(image, np.zeros((0, 4)), np.zeros((12, 17, 0)), np.zeros((0, 3))), image)


def test_instance_colors_are_the_reference_palette_in_slot_order(ref):
    for n in (1, 3, 10):
        got = render.instance_colors(n)
        assert len(got) == n and all(isinstance(v, float) for c in got for v in c)
        assert np.array_equal(np.array(got, np.float64), ref["palette_%d" % n]), n           # bit for bit


def _draw(mask, window, color=(1.0, 0.5, 0.25), **kw):
    h, w = mask.shape
    image = np.full((h, w, 3), 100, np.uint8)
    return render.render_instances(image, [window], mask[:, :, None], [color], **kw)


def test_outline_rule_on_hand_made_masks():
    line = np.array([255, 127, 63], np.uint8)                       # uint32(colour * 255)
    # a single pixel is its own outline
    m = np.zeros((5, 7), bool)
    m[2, 3] = True
    got = _draw(m, [0, 0, 0, 0], show_mask=False, show_bbox=False)
    assert np.array_equal(got[2, 3], line) and (np.delete(got.reshape(-1, 3), 2 * 7 + 3, axis=0) == 100).all()
    assert np.array_equal(render.outline(m), m)
    # a full frame: the frame's border
    full = np.ones((6, 9), bool)
    want = np.zeros((6, 9), bool)
    want[0], want[-1], want[:, 0], want[:, -1] = True, True, True, True
    assert np.array_equal(render.outline(full), want)
    got = _draw(full, [0, 0, 0, 0], show_mask=False, show_bbox=False)
    assert (got[want] == line).all() and (got[~want] == 100).all()
    # a 4 x 5 block inside: its rim, not its two inner pixels; diagonal neighbours do not count
    m = np.zeros((8, 9), bool)
    m[2:6, 2:7] = True
    want = m.copy()
    want[3:5, 3:6] = False
    assert np.array_equal(render.outline(m), want)
    m[3, 3] = False                                                 # a hole makes its four neighbours outline
    assert render.outline(m)[3, 4] and render.outline(m)[4, 3] and not render.outline(m)[4, 4]
    # the outline goes over the blend, and the later instance over the earlier
    two = np.ones((3, 3, 2), bool)
    got = render.render_instances(np.zeros((3, 3, 3), np.uint8), np.zeros((2, 4), int), two, [(1, 0, 0), (0, 0, 1)], show_bbox=False)
    assert (got[[0, 0, 2, 2, 0, 1], [0, 2, 0, 2, 1, 0]] == [0, 0, 255]).all()
    assert np.array_equal(got[1, 1], [63, 0, 127])                  # blended twice: 0 -> 127 -> 63 in red, 0 -> 0 -> 127 in blue


def test_box_rule_on_hand_made_windows():
    blank = np.zeros((40, 50), bool)
    ring = render.box_ring(40, 50, [5, 4, 45, 30])
    y, x = np.mgrid[0:40, 0:50]
    inside = (x >= 5) & (x < 45) & (y >= 4) & (y < 30)
    assert not ring[~inside].any()
    assert not ring[6:28, 7:43].any()                               # more than 2 px from every edge
    # the top band: rows 4 and 5, dashes of 6 from the window's left edge
    for row in (4, 5, 28, 29):
        assert ring[row, 5:45].tolist() == [((c - 5) // 6) % 2 == 0 for c in range(5, 45)], row
    # the sides below the bands: columns 5, 6, 43, 44, dashed along y from the window's top
    for col in (5, 6, 43, 44):
        assert ring[6:28, col].tolist() == [((r - 4) // 6) % 2 == 0 for r in range(6, 28)], col
    # drawn pixels are blended with box_alpha, the rest is the image
    got = _draw(blank, [5, 4, 45, 30], show_mask=False, show_outline=False)
    assert (got[ring] == [int(100 * (1 - 0.7) + 0.7 * 1.0 * 255), int(100 * (1 - 0.7) + 0.7 * 0.5 * 255), int(100 * (1 - 0.7) + 0.7 * 0.25 * 255)]).all()
    assert (got[~ring] == 100).all()
    # a window 3 px wide: the ring is the whole window, every pixel in a band or a side
    ring = render.box_ring(40, 50, [10, 2, 13, 22])
    assert ring[2:4, 10:13].all() and ring[20:22, 10:13].all()      # bands: (x - x1) // 6 == 0 across all 3 columns
    assert ring[4:20, 10:13].tolist() == [[((r - 2) // 6) % 2 == 0] * 3 for r in range(4, 20)]
    assert ring.sum() == ring[2:22, 10:13].sum()
    # empty windows draw nothing
    for win in ([7, 7, 7, 20], [7, 7, 20, 7], [9, 3, 4, 30], [0, 0, 0, 0]):
        assert not render.box_ring(40, 50, win).any(), win
        assert (_draw(blank, win) == 100).all(), win
    # the box goes over the outline
    m = np.zeros((12, 12), bool)
    m[0:12, 0:12] = True
    got = _draw(m, [0, 0, 12, 12], show_mask=False, alpha=0.5, box_alpha=0.5)
    assert np.array_equal(got[0, 0], [255, int(127 * 0.5 + 0.5 * 0.5 * 255), int(63 * 0.5 + 0.5 * 0.25 * 255)])
    assert np.array_equal(got[0, 6], [255, 127, 63])                # in a gap of the dashes: the outline stays


def test_render_instances_checks_its_arguments():
    image = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(ValueError, match="uint8"):
        render.render_instances(image.astype(np.float32), np.zeros((0, 4)), np.zeros((4, 4, 0)), np.zeros((0, 3)))
    with pytest.raises(ValueError, match="expected"):
        render.render_instances(image, np.zeros((1, 4)), np.zeros((4, 5, 1)), np.zeros((1, 3)))
    with pytest.raises(ValueError, match="expected"):
        render.render_instances(image, np.zeros((2, 4)), np.zeros((4, 4, 1)), np.zeros((1, 3)))


def test_png_round_trip(tmp_path):
    rng = np.random.RandomState(3)
    for shape in ((1, 1, 3), (7, 13, 3), (64, 48, 3)):
        rgb = rng.randint(0, 256, size=shape).astype(np.uint8)
        p = str(tmp_path / ("a%d.png" % shape[0]))
        render.write_png(p, rgb)
        assert np.array_equal(render.read_png(p), rgb)
        data = open(p, "rb").read()
        assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR" and data[-8:-4] == b"IEND"
        assert struct.unpack(">IIBBBBB", data[16:29]) == (shape[1], shape[0], 8, 2, 0, 0, 0)
    render.write_png(p, rgb[:, ::2])                                 # a view that is not contiguous
    assert np.array_equal(render.read_png(p), rgb[:, ::2])
    with pytest.raises(ValueError):
        render.write_png(p, rgb.astype(np.float32))
    with pytest.raises(ValueError):
        render.write_png(p, rgb[:, :, :1])
    # the reader refuses what it does not read: other filters, a damaged chunk, another file
    rows = np.zeros((2, 1 + 3 * 2), np.uint8)
    rows[1, 0] = 1                                                   # a Sub-filtered row
    chunk = lambda kind, body: struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)   # noqa: E731
    with open(p, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 2, 2, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows.tobytes()))
                + chunk(b"IEND", b""))
    with pytest.raises(ValueError, match="filter"):
        render.read_png(p)
    render.write_png(p, rgb)
    data = bytearray(open(p, "rb").read())
    data[40] ^= 1
    open(p, "wb").write(bytes(data))
    with pytest.raises(ValueError, match="damaged"):
        render.read_png(p)
    open(p, "wb").write(b"not a png at all")
    with pytest.raises(ValueError, match="not a PNG"):
        render.read_png(p)
