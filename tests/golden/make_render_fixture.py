"""Generate tests/golden/ref_render.npz by EXECUTING THE REFERENCE'S OWN apply_mask and random_colors.

    python tests/golden/make_render_fixture.py <the reference checkout>

The reference's myolo/visualize.py cannot be imported as a module (its header imports matplotlib, skimage, IPython and mrcnn), but the two
functions need nothing except numpy, random and colorsys.  Their definitions are picked out of the parsed file (`ast`) and compiled from the
reference file where it lies, as make_ref_host_fixtures.py does with myolo_utils.py -- nothing of the reference's text is written anywhere.

Stored: a seeded 12 x 17 uint8 image, three overlapping masks, three colours; for each alpha of 0.5, 0.3 and 0.7 the uint32 canvas after
apply_mask of the three masks in turn (a pixel under two masks is blended twice, with a truncation in between); and random_colors(n) for
n = 1, 3, 10 with its shuffle taken back out (sorted on hue, which is how the n colours were made: hue i / n, full saturation and value).
Outputs are data (arrays).  The .npz file is the fixture; this script is its provenance."""
import ast
import colorsys
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
WANT = ["random_colors", "apply_mask"]
ALPHAS = [0.5, 0.3, 0.7]
PALETTES = [1, 3, 10]


def load_reference_functions(ref):
    with open(ref) as f:
        tree = ast.parse(f.read(), filename=ref)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANT]
    assert sorted(n.name for n in keep) == sorted(WANT), [n.name for n in keep]
    ns = {"np": np, "random": random, "colorsys": colorsys}
    exec(compile(ast.Module(body=keep, type_ignores=[]), ref, "exec"), ns)
    return ns


def main():
    ref = os.path.join(sys.argv[1], "myolo", "visualize.py")
    ns = load_reference_functions(ref)
    rng = np.random.RandomState(20)
    h, w = 12, 17
    image = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    masks = np.zeros((h, w, 3), dtype=np.uint8)
    masks[1:8, 2:11, 0] = 1                      # overlaps the second ...
    masks[4:12, 6:17, 1] = 1                     # ... which touches two frame borders and overlaps the third
    masks[:, :, 2] = (rng.rand(h, w) < 0.4)      # scattered pixels all over: every pixel count 0 .. 3 occurs
    colors = np.array([[1.0, 0.0, 0.0], [0.2, 1.0, 0.6], [0.123456789, 0.987654321, 0.5]], dtype=np.float64)
    out = {"image": image, "masks": masks, "colors": colors, "alphas": np.array(ALPHAS, dtype=np.float64)}
    for a in ALPHAS:
        canvas = image.astype(np.uint32).copy()
        for i in range(3):
            canvas = ns["apply_mask"](canvas, masks[:, :, i], tuple(float(v) for v in colors[i]), a)
        assert canvas.dtype == np.uint32
        out["blend_%02d" % round(a * 10)] = canvas
    random.seed(7)
    for n in PALETTES:
        got = ns["random_colors"](n)
        got.sort(key=lambda c: colorsys.rgb_to_hsv(*c)[0])
        out["palette_%d" % n] = np.array(got, dtype=np.float64).reshape(n, 3)
    np.savez_compressed(os.path.join(HERE, "ref_render.npz"), **out)
    print("ref_render.npz:", sorted(out))


if __name__ == "__main__":
    main()
