"""The unique-correspondence oracle (tests/decode_unique_ref.py) against the reference's own output
(tests/golden/decode_unique.npz, tools/capture_decode_unique_fixture.py), the C-ABI's two new
symbols, and the host side of the three decode entry points (workspace sizes, the batch limit).  No GPU."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import decode_unique_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("two_tiles", "tail", "single_tile", "empty", "one_class", "distinct", "near7", "near3", "table_stress",
         "classes5", "classes6")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("decode_unique.npz")


def test_fixture_holds_the_cases(fx):
    cs = ref.cases()
    assert tuple(cs) == CASES
    for name, (mask, ids, bbox, size) in cs.items():
        np.testing.assert_array_equal(fx[f"{name}_mask"], np.asarray(mask).astype(np.uint8))
        np.testing.assert_array_equal(fx[f"{name}_ids"], ids)
        np.testing.assert_array_equal(fx[f"{name}_bbox"], bbox)
        assert int(fx[f"{name}_size"]) == size


@pytest.mark.parametrize("name", CASES)
def test_oracle_equals_reference(fx, name):
    """means (bitwise), mapped ints, 3D points and order"""
    lut = ref.make_lut(ref.LUT_CLASSES)
    u = ref.unique_crop(fx[f"{name}_mask"] > 0, fx[f"{name}_ids"], lut, fx[f"{name}_bbox"], int(fx[f"{name}_size"]))
    assert u.count == len(fx[f"{name}_p2d"])
    assert u.mean.tobytes() == fx[f"{name}_p2d"].tobytes()
    np.testing.assert_array_equal(u.xy, fx[f"{name}_orig"])
    assert u.xyz.tobytes() == fx[f"{name}_p3d"].tobytes()
    np.testing.assert_array_equal(u.xyz[:, 0], u.ids_order)  # make_lut: x = id, so this is the order
    assert int(u.mult.sum()) == int((fx[f"{name}_mask"] > 0).sum())


def test_host_builder_equals_reference(fx):
    """the drop-in's numpy build_unique_2D_3D_correspondence (same signature, f64 means)"""
    from zebrapose_amd.binary_code_helper.CNN_output_to_pose import build_unique_2D_3D_correspondence
    lut = ref.make_lut(ref.LUT_CLASSES)
    d = {float(i): lut[i] for i in range(len(lut))}
    for name in CASES:
        p2d, p3d = build_unique_2D_3D_correspondence((fx[f"{name}_mask"] > 0).nonzero(), fx[f"{name}_ids"], d)
        assert p2d.dtype == np.float64 and p2d.tobytes() == fx[f"{name}_p2d"].tobytes(), name
        assert p3d.tobytes() == fx[f"{name}_p3d"].tobytes(), name


def test_preconditions_of_the_cases():
    cs = ref.cases()
    lut = ref.make_lut(ref.LUT_CLASSES)
    u = {k: ref.unique_crop(m, i, lut, bb, s) for k, (m, i, bb, s) in cs.items()}
    assert u["empty"].count == 0 and u["one_class"].count == 1 and u["one_class"].mult[0] == 40 * 36
    assert u["distinct"].count == int(cs["distinct"][0].sum()) > 1024
    assert u["classes5"].count == 5 and u["classes6"].count == 6
    assert cs["classes5"][0].sum() > 100 and cs["classes6"][0].sum() > 100
    # a class whose first pixel lies in tile 0 and whose other pixels lie in tile 1
    m, i = cs["two_tiles"][0], cs["two_tiles"][1]
    px = np.flatnonzero((i == 5) & m)
    assert px[0] < 1024 and np.all(px[1:] >= 1024) and len(px) > 1
    # >= 16 ids that agree in their low 12 bits
    present = np.unique(cs["table_stress"][1][cs["table_stress"][0]])
    assert (present % 4096 == 0).sum() >= 16
    assert set(u["near7"].mult) >= {3, 7}
    # the near-integer groups: the two-step f64 value is within 1e-9 of an integer, and the exactly
    # computed product-plus-offset (what a contracted FMA rounds) truncates to another integer
    for spec, name, axes in ((ref.NEAR7, "near7", (0, 1)), (ref.NEAR3, "near3", (0,))):
        r = u[name]
        j = list(r.ids_order).index(spec["id"])
        assert r.mult[j] == len(spec["xs"])
        for ax in axes:
            ratio = np.float64(spec["bbox"][2 + ax]) / np.float64(spec["bbox_size"])
            two_step = float(ratio * r.mean[j, ax] + np.float64(spec["bbox"][ax]))
            assert abs(two_step - round(two_step)) < 1e-9 and math.trunc(two_step) == r.xy[j, ax]
            fused = float(Fraction(float(ratio)) * Fraction(float(r.mean[j, ax])) + spec["bbox"][ax])
            assert math.trunc(fused) != r.xy[j, ax]
    # 7-group: multiplying by the rounded reciprocal instead of dividing changes the result too
    s = np.float64(sum(ref.NEAR7["xs"]))
    recip = float(np.float64(119) / np.float64(36) * (s * (np.float64(1) / np.float64(7))) + np.float64(-100))
    assert math.trunc(recip) != u["near7"].xy[list(u["near7"].ids_order).index(ref.NEAR7["id"]), 0]


def test_header_and_binding_declare_the_symbols():
    with open(os.path.join(ROOT, "include", "zp.h")) as f:
        h = f.read()
    with open(os.path.join(ROOT, "zebrapose_amd", "_lib.py")) as f:
        lib = f.read()
    for sym in ("zp_decode_unique_ws_bytes", "zp_decode_unique"):
        assert re.search(r"\b" + sym + r"\s*\(", h), sym
        assert f'"{sym}"' in lib, sym


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 33, 31), (3, 128, 128)])
def test_workspace_bytes(B, H, W):
    """the sizes Python allocates from: ids [B][HW], one (unique: two) count per 1024-pixel tile, the
    unique form's two tables of T = 2^k >= 2 HW slots and three accumulators per pixel; 256 spare bytes"""
    from zebrapose_amd import _lib as L
    HW = H * W
    tiles = (HW + 1023) // 1024
    T = 2
    while T < 2 * HW:
        T *= 2
    assert L.lib.zp_decode_ws_bytes(B, H, W) == B * HW * 4 + B * tiles * 4 + 256
    assert L.lib.zp_decode_unique_ws_bytes(B, H, W) == (B * HW * 4 + 2 * B * tiles * 4 + 2 * B * T * 4
                                                         + 3 * B * HW * 4 + 256)


def test_batch_limit():
    """the grids are (tiles, B): B = 65536 is ZP_ERR_ARG from each entry point (valid pointers and
    sizes otherwise, never dereferenced: the checks reject before any launch), B = 0 likewise"""
    from zebrapose_amd import _lib as L
    p = [ctypes.c_void_p(0x1000 * k) for k in range(1, 12)]
    m, c, lut, bb, ids, cnt, xy, xyz, ws, mult, mean = p
    calls = {
        "zp_decode": lambda B: L.lib.zp_decode(m, c, B, 8, 8, 16, 16, lut, None, bb, 8, ids, cnt, xy, xyz, ws, None),
        "zp_decode_radix": lambda B: L.lib.zp_decode_radix(m, c, B, 8, 8, 4, 4, lut, None, bb, 8, ids, cnt, xy, xyz, ws,
                                                           None),
        "zp_decode_unique": lambda B: L.lib.zp_decode_unique(m, c, B, 8, 8, 16, 16, 2, lut, None, bb, 8, ids, cnt, xy,
                                                             xyz, mult, mean, ws, None)}
    for name, f in calls.items():
        for B in (65536, 0):
            assert f(B) == 1, (name, B)  # ZP_ERR_ARG (include/zp.h)
            assert L.lib.zp_last_error() == name.encode() + b": bad sizes"
