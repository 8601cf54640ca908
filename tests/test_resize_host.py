"""The host side of the device resize (csrc/resize_kernels.hip): every refusal of myolo_resize_images_u8 comes back as
MYOLO_EINVAL with a message naming the entry before anything is launched, engine.pack_images lays a batch of mixed sizes out the way the entry
reads it, and the binding declares the new symbols with the header's arity.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from myolo import _ext as X
from myolo.engine import pack_images, packed_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _call(src=True, src_bytes=300, desc=True, desc_host=((0, 10, 10),), out_u8=True, out_unit=True, B=1, H=8, W=8, ws=True, ws_bytes=None):
    """one call whose pointers are real host buffers (True) or NULL (False): a call that passed every check would launch, so every case here is
    one the entry must refuse -> (status, message)"""
    lib = X.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    dh = None
    if desc_host is not None:
        dh = np.ascontiguousarray(np.array(desc_host, np.int64).reshape(-1, 3))
    rc = lib.myolo_resize_images_u8(p if src else None, src_bytes, p if desc else None, None if dh is None else dh.ctypes.data,
                                    p if out_u8 else None, p if out_unit else None, B, H, W, p if ws else None,
                                    X.resize_ws_bytes(B) if ws_bytes is None else ws_bytes, None)
    return rc, lib.myolo_last_error_string()


REFUSED = {
    "src null": dict(src=False),
    "desc null": dict(desc=False),
    "desc_host null": dict(desc_host=None),
    "both outputs null": dict(out_u8=False, out_unit=False),
    "B = 0": dict(B=0),
    "B < 0": dict(B=-3),
    "H = 0": dict(H=0),
    "W = 0": dict(W=0),
    "H < 0": dict(H=-8),
    "W < 0": dict(W=-1),
    "h = 0": dict(desc_host=((0, 0, 10),)),
    "w = 0": dict(desc_host=((0, 10, 0),)),
    "h < 0": dict(desc_host=((0, -10, 10),)),
    "one byte short": dict(src_bytes=299),
    "offset pushes it out": dict(desc_host=((1, 10, 10),)),
    "negative offset": dict(desc_host=((-1, 10, 10),)),
    "second image out": dict(B=2, desc_host=((0, 5, 5), (75, 5, 16))),
    "3 h w overflows int64": dict(desc_host=((0, 1 << 40, 1 << 40),)),
    "h w overflows int64": dict(desc_host=((0, (1 << 62) + 1, 4),)),
    "workspace null": dict(ws=False),
    "workspace short": dict(B=2, desc_host=((0, 5, 5), (75, 5, 5)), ws_bytes=15),
    "workspace empty": dict(ws_bytes=0),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_bad_arguments_are_refused_with_a_message(case):
    rc, msg = _call(**REFUSED[case])
    assert rc == -1, (case, rc, msg)
    assert b"resize_images" in msg, (case, msg)


def test_refusal_messages_say_what_was_wrong():
    assert b"null" in _call(src=False)[1] and b"null" in _call(out_u8=False, out_unit=False)[1]
    assert b"B=0" in _call(B=0)[1] and b"H=-8" in _call(H=-8)[1]
    assert b"no pixels" in _call(desc_host=((0, 0, 10),))[1]
    assert b"image 1" in _call(B=2, desc_host=((0, 5, 5), (75, 5, 16)))[1] and b"does not fit" in _call(src_bytes=299)[1]
    assert b"workspace" in _call(ws_bytes=0)[1]
    # one output alone is enough: with either pointer given the refusal is about something else
    assert b"workspace" in _call(out_u8=False, ws_bytes=0)[1] and b"workspace" in _call(out_unit=False, ws_bytes=0)[1]


def test_workspace_query():
    assert X.resize_ws_bytes(1) == 8 and X.resize_ws_bytes(7) == 56
    assert X.resize_ws_bytes(0) == 0 and X.resize_ws_bytes(-1) == 0


def test_packer_descriptor_with_odd_offsets():
    """three images whose byte counts are odd: the second and third start on odd offsets, with no padding between them"""
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (5, 7, 3), dtype=np.uint8), rng.integers(0, 256, (3, 3, 3), dtype=np.uint8),
            rng.integers(0, 256, (1, 5, 3), dtype=np.uint8)]
    assert packed_bytes(imgs) == 3 * 24 + 105 + 27 + 15
    out = np.full(packed_bytes(imgs) + 5, 0xAB, np.uint8)
    desc = pack_images(imgs, out)
    assert desc.dtype == np.int64 and desc.tolist() == [[0, 5, 7], [105, 3, 3], [132, 1, 5]]
    assert desc[1, 0] % 2 == 1 and (72 + desc[1, 0]) % 2 == 1
    assert out[:72].view(np.int64).reshape(3, 3).tolist() == desc.tolist()               # the descriptor leads the buffer
    for im, (o, h, w) in zip(imgs, desc):
        assert np.array_equal(out[72 + o:72 + o + 3 * h * w].reshape(h, w, 3), im)
    assert (out[72 + 147:] == 0xAB).all()                                                 # nothing behind the last image is touched
    # more slots than images: the extra slots name the last image again, and no byte is added for them
    assert packed_bytes(imgs, 5) == 5 * 24 + 147
    out5 = np.zeros(packed_bytes(imgs, 5), np.uint8)
    d5 = pack_images(imgs, out5, 5)
    assert d5.tolist() == desc.tolist() + [[132, 1, 5]] * 2
    assert np.array_equal(out5[120:], out[72:72 + 147])
    # a strided view is packed densely
    big = rng.integers(0, 256, (8, 9, 3), dtype=np.uint8)
    view = big[1:7:2, ::3]
    o1 = np.zeros(packed_bytes([view]), np.uint8)
    assert pack_images([view], o1).tolist() == [[0, 3, 3]] and np.array_equal(o1[24:].reshape(3, 3, 3), view)


def test_packer_refuses_what_the_entry_cannot_read():
    ok = np.zeros((2, 2, 3), np.uint8)
    for bad in (np.zeros((2, 2, 3), np.float32), np.zeros((2, 2), np.uint8), np.zeros((2, 2, 4), np.uint8), np.zeros((0, 2, 3), np.uint8)):
        with pytest.raises(ValueError):
            pack_images([ok, bad], np.zeros(4096, np.uint8))
    with pytest.raises(ValueError):
        pack_images([ok], np.zeros(24 + 11, np.uint8))            # one byte short
    with pytest.raises(ValueError):
        pack_images([], np.zeros(64, np.uint8))
    with pytest.raises(ValueError):
        pack_images([ok, ok], np.zeros(4096, np.uint8), 1)        # fewer slots than images


def test_binding_declares_the_new_symbols_with_the_headers_arity():
    txt = open(os.path.join(ROOT, "include", "myolo_hip_internal.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = dict(re.findall(r"\b(?:int|size_t)\s+(myolo_resize_\w+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S))
    assert sorted(decl) == ["myolo_resize_images_u8", "myolo_resize_images_ws_bytes"]
    assert "myolo_resize_images_u8" in X.SIGS and len(X.SIGS["myolo_resize_images_u8"]) == decl["myolo_resize_images_u8"].count(",") + 1 == 12
    assert "myolo_resize_images_ws_bytes" in X.exported_symbols() and "myolo_resize_images_u8" in X.exported_symbols()
    lib = X.load()
    assert lib.myolo_resize_images_ws_bytes.argtypes == [ctypes.c_int] and decl["myolo_resize_images_ws_bytes"].count(",") == 0
    assert lib.myolo_resize_images_ws_bytes.restype is ctypes.c_size_t


def test_unit_is_built_without_contraction():
    import __graft_entry__ as G
    assert ("resize_kernels.hip", ["-ffp-contract=off"]) in G.UNITS
    src = open(os.path.join(G.CSRC, "resize_kernels.hip")).read()
    assert "#pragma clang fp contract(off)" in src
