"""zp_mask_contour and zp_edge_refine_step at their edges, against tests/refine_ref.py: the sweep cap
and its off-by-one on the staircase serpentines of tests/test_refine_host.py (whose pass counts are
asserted there on the oracle alone), what the Python layer does with counts = -1, the largest image
the size check accepts, row-word and frame edges, borders of exactly 19 and 20 pixels, and observed
coordinates at the saturation boundary.  Comparisons are tests/test_gpu_refine.py's own: integers
exactly, H and b to 1e-12 of the largest entry, the pose to 64 cond(A) 2^-52."""
import numpy as np
import pytest

from tests import refine_ref as RF
from tests.test_gpu_refine import _check_contour, _check_step, _contour, _depth_of, _poses, _ring_points
from tests.test_refine_host import STAIR_S, border_of, embed, grid, scene, spiral, staircase_at_cap

pytestmark = pytest.mark.gpu


def _K(B, H, W):
    return np.tile(np.array([570.0, 575.0, W / 2 - 0.5, H / 2 + 0.25]), (B, 1))


def test_mask_contour_reports_the_sweep_cap(gpu):
    """-1 exactly where the oracle gives up, next to ordinary crops in the same launch; the serpentine
    one cell short of the cap comes back whole"""
    S = STAIR_S
    over, last, under = staircase_at_cap()
    block = embed(grid("block")[0], S, S, 3, 5, 4)
    ent = np.stack([over, block, last, under, spiral(S, S), over]).astype(np.uint8) * 255
    assert [RF.capped(e) for e in ent] == [True, False, True, False, False, True]
    bbox = np.array([[10 * b, 7 * b, S + b, S - b] for b in range(len(ent))], np.int32)
    counts, xy = _contour(gpu, ent, None, bbox)
    for b, e in enumerate(ent):
        if RF.capped(e):
            assert counts[b] == -1 and not xy[b].any()  # the list is left as the wrapper zeroed it
        else:
            want = RF.mask_contour(e, None, bbox[b])
            assert counts[b] == len(want) > 0 and np.array_equal(xy[b, :len(want)], want), b
    vis = (np.random.default_rng(0).random(ent.shape) < 0.3).astype(np.uint8)
    counts, _ = _contour(gpu, ent, vis, bbox)
    assert [int(c) for c in counts[[0, 2, 5]]] == [-1, -1, -1]
    _check_contour(gpu, ent[[1, 3, 4]], vis[[1, 3, 4]], bbox[[1, 3, 4]])


def test_step_reports_the_sweep_cap(gpu):
    """status 2, the pose bit for bit, cost 0, match -1 and Hb 0 where the fill's last changing pass is
    pass `cap` or later; status 0 and the exact border one pass earlier; both kinds in one launch"""
    S = STAIR_S
    rng = np.random.default_rng(1)
    over, last, under = staircase_at_cap()
    sils = [over, under, last, embed(grid("ring")[0], S, S, 2, 2, 4), under, over]
    depth = np.stack([_depth_of(s, rng) for s in sils])
    pts = [_ring_points(rng, S, S, 30 + b) for b in range(len(sils))]
    R, t = _poses(rng, len(sils))
    got, stats = _check_step(gpu, depth, pts, R, t, _K(len(sils), S, S))
    assert stats == [2, 0, 2, 0, 0, 2]
    assert (got["border_n"][[0, 2, 5]] == 0).all() and got["border_n"][1] == len(RF.border_list(under)) > 500


def test_refiner_takes_a_capped_contour_as_no_points(gpu):
    """counts = -1 from mask_contour goes into EdgeRefiner.refine as it is: the step clamps it to 0 and
    reports status 1, and the pose comes back bit for bit"""
    import torch
    from zebrapose_amd.refine import EdgeRefiner, mask_contour
    from zebrapose_amd.render import MeshRenderer
    H = W = 96
    verts, faces, K, Rg, tg, pts, _ = scene(H, W)
    rend = MeshRenderer(verts, faces, device=gpu)
    over = staircase_at_cap()[0]
    good = np.zeros_like(over)
    good[10:40, 10:40] = 1
    counts, xy = mask_contour(torch.from_numpy(np.stack([over, good])).to(gpu), None, np.array([[0, 0, 54, 54]] * 2))
    assert counts.cpu().tolist() == [-1, 116]
    ref = EdgeRefiner(rend, H, W)
    R0 = np.stack([Rg, Rg])
    t0 = np.stack([tg, tg + np.array([1.0, -1.0, 3.0])])
    Ro, to, status, cost = ref.refine(R0, t0, K, counts, xy)
    assert status.cpu().tolist() == [1, 0] and cost[:, 0].cpu().tolist() == [0] * 10
    assert np.array_equal(Ro[0].cpu().numpy().view(np.int64), R0[0].view(np.int64))
    assert np.array_equal(to[0].cpu().numpy().view(np.int64), t0[0].view(np.int64))
    assert not np.array_equal(to[1].cpu().numpy(), t0[1])  # the neighbour was refined


def test_largest_accepted_image(gpu):
    """512 x 1024 = 2^19 padded bits: 128 KB of dynamic LDS beside the static 20 KB.  The launch is
    accepted and the step matches the oracle; one more row is refused by the size check."""
    from zebrapose_amd import _lib as L
    H, W = 512, 1024
    assert L.lib.zp_edge_refine_ws_bytes(1, H, W) > 0 and L.lib.zp_edge_refine_ws_bytes(1, H + 1, W) == -1
    assert L.lib.zp_edge_refine_ws_bytes(1, H, W - 31) > 0 and L.lib.zp_edge_refine_ws_bytes(1, H, W + 1) == -1
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[:H, :W]
    sil = np.zeros((H, W), np.uint8)
    sil[((yy - 250) / 120.0) ** 2 + ((xx - 400) / 260.0) ** 2 < 1] = 1
    sil[220:280, 380:460] = 0            # a hole
    sil[H - 40:, W - 70:] = 1            # a block in the last rows and columns (the last word of a row)
    sil[0:3, 0:5] = 1                    # and one in the first
    depth = _depth_of(sil, rng)[None]
    pts = [np.stack([rng.integers(-20, W + 20, 300), rng.integers(-20, H + 20, 300)], 1)]
    R, t = _poses(rng, 1)
    got, stats = _check_step(gpu, depth, pts, R, t, np.array([[572.4, 573.6, W / 2 + 0.3, H / 2 - 0.2]]))
    assert stats == [0] and got["border_n"][0] > 1000


def test_largest_accepted_crop(gpu):
    """S = 704: 704 x 22 words, the largest square within 2^19 padded bits to a multiple of 32"""
    from scipy import ndimage
    from zebrapose_amd import _lib as L
    S = 704
    rng = np.random.default_rng(3)
    ent = (ndimage.gaussian_filter(rng.normal(size=(1, S, S)), (0, 6.0, 6.0)) > 0.01).astype(np.uint8) * 255
    ent[0, S - 9:, S - 40:] = 255
    counts, _ = _check_contour(gpu, ent, None, np.array([[30, 20, 500, 650]], np.int32))
    assert counts[0] > 1000
    big = np.zeros((1, 725, 725), np.uint8)  # 725 x 23 words is beyond the limit: refused before any launch
    with pytest.raises(L.ZPError, match="sizes out of range"):
        _contour(gpu, big, None, np.array([[0, 0, 725, 725]], np.int32))


def _edge_silhouettes(H, W, rng):
    """set pixels in the last column and the last row, in the first ones, both, and a full frame"""
    a = np.zeros((4, H, W), np.uint8)
    a[0, H // 3:, W - 1] = 1                   # the last column alone
    a[0, H - 1, :] = 1                         # and the last row
    a[1, :, 0] = 1
    a[1, 0, :] = 1
    a[2] = rng.random((H, W)) < 0.55           # noise up to every edge
    a[2, :, W - 1] = 1
    a[3] = 1
    return a


@pytest.mark.parametrize("H,W", [(37, 1), (37, 31), (37, 32), (37, 33), (37, 64), (37, 65), (1, 65), (1, 1), (2, 96)])
def test_step_row_word_edges(gpu, H, W):
    """W a multiple of 32 and one beyond (the ring's bit in the last word of a row), one word, H = 1"""
    rng = np.random.default_rng(100 * H + W)
    sils = _edge_silhouettes(H, W, rng)
    B = len(sils)
    depth = np.stack([_depth_of(s, rng) for s in sils])
    pts = [_ring_points(rng, H, W, 25 + b) for b in range(B)]
    R, t = _poses(rng, B)
    got, stats = _check_step(gpu, depth, pts, R, t, _K(B, H, W))
    assert 2 not in stats
    if H * W >= 64:
        assert stats.count(0) >= 3, stats
    for b in range(B):  # the last column's set pixels are border pixels (the ring lies beyond them)
        last = np.nonzero(sils[b][:, W - 1])[0]
        bxy = {tuple(p) for p in got["border_xy"][b, :got["border_n"][b]]}
        assert all((W - 1, int(y)) in bxy for y in last)


@pytest.mark.parametrize("S", [1, 31, 32, 33, 64, 65])
def test_contour_row_word_edges(gpu, S):
    rng = np.random.default_rng(S)
    ent = _edge_silhouettes(S, S, rng) * 255
    bbox = np.array([[5, 9, S, S], [0, 0, 2 * S, 3 * S], [100, 50, S + 7, S], [3, 3, S, S]], np.int32)
    counts, _ = _check_contour(gpu, ent, None, bbox)
    if S > 1:  # the second holds the first row and column alone, which the x > 0, y > 0 rule drops
        assert counts[1] == 0 and counts[[0, 2, 3]].min() > 0
    _check_contour(gpu, ent, (rng.random(ent.shape) < 0.2).astype(np.uint8), bbox)


def test_min_border_boundary(gpu):
    """19 border pixels: status 1; 20: a step (RF_MIN_BORDER)"""
    rng = np.random.default_rng(4)
    depth = np.stack([border_of(19), border_of(20), border_of(19), border_of(20)])
    pts = [_ring_points(rng, 16, 16, 12 + b) for b in range(4)]
    R, t = _poses(rng, 4)
    got, stats = _check_step(gpu, depth, pts, R, t, _K(4, 16, 16))
    assert stats == [1, 0, 1, 0] and got["border_n"].tolist() == [19, 20, 19, 20]


def test_observed_coordinates_saturate(gpu):
    """+-2^20 is kept, +-(2^20 + 1) and INT_MIN / INT_MAX land on +-2^20: the list that exceeds the
    range gives the bits of the clipped list, and matches, the integer cost, H and b are the oracle's.
    The step itself is thousands of radians long with residuals of a million pixels, so _check_step's
    pose tolerance (64 cond(A) 2^-52, made for steps below a radian) is scaled here by max(1, |theta_r|)
    for R: a relative error r of theta turns R exp([theta]x) by r |theta|."""
    from tests.test_gpu_refine import LR, LT, _step
    H, W = 45, 37
    rng = np.random.default_rng(5)
    sil = np.zeros((H, W), np.uint8)
    sil[8:30, 6:30] = 1
    depth = np.stack([_depth_of(sil, rng)] * 3)
    s, lo, hi = 1 << 20, -2 ** 31, 2 ** 31 - 1
    edge = [[s, 5], [-s, 5], [5, s], [5, -s], [s, s], [-s, -s], [s - 1, 1 - s]]
    over = [[s + 1, 5], [-s - 1, 5], [5, s + 1], [5, -s - 1], [hi, lo], [lo, hi], [hi, hi], [lo, lo], [lo, 5], [5, hi]]
    near = _ring_points(rng, H, W, 20).tolist()
    pts = [np.array(edge + near), np.array(over + near), np.array(edge + over + near)]
    R, t = _poses(rng, 3)
    K = _K(3, H, W)
    got = _step(gpu, depth, pts, R, t, K)
    again = _step(gpu, depth, [np.clip(p, -s, s) for p in pts], R, t, K)
    for k in got:
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), k
    for b in range(3):
        w = RF.step(depth[b], pts[b], R[b], t[b], K[b], LR, LT)
        assert w["status"] == 0 and got["status"][b] == 0 and got["cost"][b] == w["cost"] > 2 ** 40
        assert got["border_n"][b] == len(w["border"]) and np.array_equal(got["match"][b, :len(pts[b])], w["match"])
        assert np.abs(got["Hb"][b] - w["Hb"]).max() <= 1e-12 * np.abs(w["Hb"]).max()
        tol = 64 * np.linalg.cond(w["A"]) * 2.0 ** -52
        turn = max(1.0, np.linalg.norm(w["theta"][:3]))
        assert np.abs(got["R"][b].reshape(3, 3) - w["R"]).max() <= tol * turn, (b, tol, turn)
        assert np.abs(got["t"][b] - w["t"]).max() <= tol * turn * np.abs(w["t"]).max(), (b, tol)
