"""The three mesh entry points stay inside the workspace their *_ws_bytes functions report and read
nothing from it that they have not written: each runs through the C ABI once in a workspace of
ws_bytes + 4096 bytes filled with 0xA5, whose last 4096 bytes must come back untouched, and once in a
zero-filled workspace of exactly ws_bytes; the outputs of the two runs must agree bit for bit.  The
guard lies inside the test's own allocation, so a carve that outgrew its total fails an assert."""
import numpy as np
import pytest
import torch

from tests import meshcode_radix_ref as RR
from tests import meshcode_ref as MR
from tests import subdiv_ref as SR

pytestmark = pytest.mark.gpu

GUARD, FILL = 4096, 0xA5


def guarded_and_plain(ws_bytes, run):
    """run(ws) -> output tensors.  Returns the outputs under the 0xA5 workspace with a guard and under
    the zeroed workspace of exactly ws_bytes, after checking the guard."""
    assert ws_bytes > 0
    ws = torch.full((ws_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    a = run(ws)
    torch.cuda.synchronize()
    assert bool((ws[ws_bytes:] == FILL).all()), "the call wrote past the workspace it asked for"
    b = run(torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    return a, b


def assert_bitwise(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def coder(name, split_args, classes, draws):
    from zebrapose_amd import _lib as L
    from zebrapose_amd.meshcode import eps_to_grid, grid_log2
    v, f = MR.icosphere(3)
    v = np.ascontiguousarray(v * np.float32(40))
    assert len(v) == 642 and len(f) == 1280
    f = np.ascontiguousarray(f.astype(np.int32))
    k = grid_log2(v)
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    dd = torch.from_numpy(np.ascontiguousarray(draws).view(np.int32)).cuda()

    def run(ws):
        vid = torch.full((len(v),), -7, dtype=torch.int32, device="cuda")
        fid = torch.full((len(f),), -7, dtype=torch.int32, device="cuda")
        lut = torch.full((classes, 3), -7.0, dtype=torch.float64, device="cuda")
        L.call(name, vd.data_ptr(), len(v), fd.data_ptr(), len(f), *split_args, 3, 10, k, eps_to_grid(1.0, k),
               dd.data_ptr(), vid.data_ptr(), fid.data_ptr(), lut.data_ptr(), ws.data_ptr(), L.stream_ptr())
        return vid, fid, lut

    a, b = guarded_and_plain(getattr(L.lib, name + "_ws_bytes")(len(v), len(f), *split_args), run)
    assert_bitwise(a, b)
    vid = a[0].cpu().numpy()  # every vertex was coded (the comparison with the numpy definition is in the coders' own tests)
    assert vid.min() >= 0 and np.bincount(vid, minlength=classes).min() >= len(v) // classes


def test_binary_coder_icosphere_642_at_9_bits():
    coder("zp_mesh_code", (9,), 512, MR.sample_draws(0, 3, 9))


def test_radix_coder_icosphere_642_at_4_to_the_3():
    coder("zp_mesh_code_radix", (4, 3), 64, RR.sample_draws(0, 3, 4, 3))


def test_subdivider_box_full_split():
    from zebrapose_amd import _lib as L
    v, f = SR.box()
    v = np.ascontiguousarray(np.asarray(v, np.float32))
    f = np.ascontiguousarray(np.asarray(f, np.int32))
    nv, nf = len(v), len(f)
    assert (nv, nf) == (8, 12)
    cap_v, cap_f = nv + 3 * nf, 4 * nf
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()

    def run(ws):
        ov = torch.full((cap_v, 3), -7.0, dtype=torch.float32, device="cuda")
        of = torch.full((cap_f, 3), -7, dtype=torch.int32, device="cuda")
        par = torch.full((cap_v, 2), -7, dtype=torch.int32, device="cuda")
        counts = torch.full((4,), -7, dtype=torch.int64, device="cuda")
        mx = torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
        L.call("zp_mesh_subdivide", vd.data_ptr(), nv, fd.data_ptr(), nf, 0.0, 0.0, SR.NO_BUDGET, ov.data_ptr(), cap_v,
               of.data_ptr(), cap_f, par.data_ptr(), counts.data_ptr(), mx.data_ptr(), ws.data_ptr(), L.stream_ptr())
        return ov, of, par, counts, mx

    a, b = guarded_and_plain(L.lib.zp_mesh_subdivide_ws_bytes(nv, nf), run)
    assert_bitwise(a, b)
    assert a[3].cpu().tolist() == [18, 18, 26, 48]
