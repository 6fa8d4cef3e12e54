"""Generates tests/golden/stb_written.hdr, stb_written.png, io_expected.npz and io_stb_checks.npz with the REFERENCE's own
vendored stb (oracle/_ref/libstbref.so, compiled by oracle/Makefile from /root/reference/dependencies/stb
where it lies).  The fixtures are data: files written by stb plus the pixels stb itself decodes from them, and
(io_stb_checks.npz) the same for tests/test_image_io.py's test images, with what stb decodes from the product's HDR file.
Run in the build container (needs /root/reference and a built tree):  python tests/golden/make_io_fixtures.py"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

if __name__ == "__main__":
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libstbref.so"))
    lib.stbi_loadf.restype = C.POINTER(C.c_float)
    lib.stbi_loadf.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    lib.stbi_write_png.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.stbi_write_hdr.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
    r = np.random.default_rng(2024)
    hdr = np.exp(r.uniform(-6, 4, (20, 48, 3))).astype(np.float32)
    hdr[3:6, 5:30] = 12.0
    hdr[15] = 0.0
    png = r.integers(0, 256, (19, 31, 3), dtype=np.uint8)
    png[4:9, :] = (png[4:9, :] // 32) * 32   # smooth-ish rows so stb picks non-zero filters
    hp, pp = os.path.join(HERE, "stb_written.hdr"), os.path.join(HERE, "stb_written.png")
    assert lib.stbi_write_hdr(hp.encode(), 48, 20, 3, hdr.ctypes.data_as(C.POINTER(C.c_float))) == 1
    assert lib.stbi_write_png(pp.encode(), 31, 19, 3, png.ctypes.data, 31 * 3) == 1
    w, h, ch = C.c_int(), C.c_int(), C.c_int()
    ptr = lib.stbi_loadf(hp.encode(), C.byref(w), C.byref(h), C.byref(ch), 0)
    dec = np.ctypeslib.as_array(ptr, shape=(h.value, w.value, 3)).copy()
    np.savez(os.path.join(HERE, "io_expected.npz"), hdr_decoded_by_stb=dec, png_pixels=png)
    print("wrote", hp, pp)

    # tests/test_image_io.py's HDR and PNG test images, so that those tests need no stb of their own
    import tempfile

    from hobbyraytracer_amd import api
    from tests.test_image_io import _test_image
    lib.stbi_load.restype = C.POINTER(C.c_uint8)
    lib.stbi_load.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]

    def stb_loadf(path):
        ptr = lib.stbi_loadf(path.encode(), C.byref(w), C.byref(h), C.byref(ch), 0)
        assert ptr and ch.value == 3
        return np.ctypeslib.as_array(ptr, shape=(h.value, w.value, 3)).copy()

    himg = _test_image()
    pimg = np.random.default_rng(4).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    with tempfile.TemporaryDirectory() as d:
        ours, theirs, ours_png, theirs_png = (os.path.join(d, n) for n in ("ours.hdr", "theirs.hdr", "ours.png", "theirs.png"))
        api.write_hdr(ours, himg)
        assert lib.stbi_write_hdr(theirs.encode(), himg.shape[1], himg.shape[0], 3, himg.ctypes.data_as(C.POINTER(C.c_float))) == 1
        api.write_image(ours_png, pimg)
        ptr = lib.stbi_load(ours_png.encode(), C.byref(w), C.byref(h), C.byref(ch), 3)
        assert ptr and np.array_equal(np.ctypeslib.as_array(ptr, shape=(h.value, w.value, 3)), pimg)
        assert lib.stbi_write_png(theirs_png.encode(), pimg.shape[1], pimg.shape[0], 3, pimg.ctypes.data, pimg.shape[1] * 3) == 1
        np.savez(os.path.join(HERE, "io_stb_checks.npz"), hdr_image=himg,
                 hdr_stb_written=np.fromfile(theirs, np.uint8), hdr_stb_written_decoded_by_stb=stb_loadf(theirs),
                 hdr_ours_decoded_by_stb=stb_loadf(ours), png_image=pimg, png_stb_written=np.fromfile(theirs_png, np.uint8))
    print("wrote", os.path.join(HERE, "io_stb_checks.npz"))
