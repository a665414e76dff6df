"""Workspace sizes of the three mesh tools (no GPU).  The carves of zp_mesh_code, zp_mesh_code_radix and
zp_mesh_subdivide share one carver (csrc/zp_mesh.h); the byte counts below were taken from the library as
it stood before they did, each region being rounded to 256 bytes on its own, so that a change to the
carver, to a region or to the rocPRIM budget shows up here and not as a device fault."""
import pytest


@pytest.mark.parametrize("fn,args,want", [
    ("zp_mesh_code_ws_bytes", (642, 1280, 9), 16903168),
    ("zp_mesh_code_ws_bytes", (65536, 131068, 16), 30408960),
    ("zp_mesh_code_ws_bytes", (1 << 21, 1 << 22, 16), 306708736),
    ("zp_mesh_code_radix_ws_bytes", (642, 1280, 4, 3), 16874752),
    ("zp_mesh_code_radix_ws_bytes", (65536, 131068, 16, 4), 30802176),
    ("zp_mesh_code_radix_ws_bytes", (1 << 21, 1 << 22, 256, 2), 315105536),
    ("zp_mesh_subdivide_ws_bytes", (8, 12), 16782592),
    ("zp_mesh_subdivide_ws_bytes", (642, 1280), 17110272),
    ("zp_mesh_subdivide_ws_bytes", (1 << 21, 1 << 24), 4378853632),
])
def test_workspace_bytes_are_pinned(fn, args, want):
    from zebrapose_amd import _lib
    assert getattr(_lib.lib, fn)(*args) == want
