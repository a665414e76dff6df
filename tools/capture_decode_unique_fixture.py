#!/usr/bin/env python3
"""Records tests/golden/decode_unique.npz: the reference's own ``build_unique_2D_3D_correspondence``
and ``mapping_pixel_position_to_original_position`` (binary_code_helper/CNN_output_to_pose.py:34-50,
67-91) on the cases of tests/decode_unique_ref.py.  Needs the reference checkout that
oracle/capture_fixtures.py points at; runs on the CPU.

Per case <name>: <name>_mask u8 [H, W], <name>_ids u16 [H, W], <name>_bbox int64 [4], <name>_size,
<name>_p2d f64 [n, 2] (the crop-space means), <name>_p3d f64 [n, 3], <name>_orig int64 [n, 2] (the
mapped points).  The LUT is tests/decode_unique_ref.make_lut(65536) and is not stored.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from oracle import capture_fixtures
    from tests import decode_unique_ref as ref
    capture_fixtures.install_shim()
    from binary_code_helper.CNN_output_to_pose import (build_unique_2D_3D_correspondence,
                                                       mapping_pixel_position_to_original_position)
    lut = ref.make_lut(ref.LUT_CLASSES)
    lut_dict = {i: lut[i] for i in range(len(lut))}
    out = {}
    for name, (mask, ids, bbox, size) in ref.cases().items():
        mask8 = np.asarray(mask).astype(np.uint8)
        ids16 = np.asarray(ids).astype(np.uint16)
        assert np.array_equal(ids16, ids)
        p2d, p3d = build_unique_2D_3D_correspondence(mask8.nonzero(), ids16, lut_dict)
        orig = mapping_pixel_position_to_original_position(p2d, np.asarray(bbox), size)
        out[f"{name}_mask"], out[f"{name}_ids"] = mask8, ids16
        out[f"{name}_bbox"], out[f"{name}_size"] = np.asarray(bbox, np.int64), np.int64(size)
        out[f"{name}_p2d"] = np.asarray(p2d, np.float64).reshape(-1, 2)
        out[f"{name}_p3d"] = np.asarray(p3d, np.float64).reshape(-1, 3)
        out[f"{name}_orig"] = np.asarray(orig, np.int64).reshape(-1, 2)
        print(f"{name}: {int(mask8.sum())} pixels -> {len(p2d)} correspondences")
    path = os.path.join(capture_fixtures.GOLDEN, "decode_unique.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
