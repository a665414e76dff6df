"""Edge refinement on the device (zp_mask_contour, zp_edge_refine_step; zebrapose_amd/refine.py)
against the numpy restatement tests/refine_ref.py.

Integers (contours, border lists, matches, costs, statuses) are compared exactly.  H and b: f64 on
both sides and only the order of summation differs, 1e-12 of the largest entry.  The pose after a
step: 64 cond(A) 2^-52 relative, cond from the oracle's matrix.  End to end: equal integer costs per
iteration and poses within 1e-6; both renderers are bit-exact for equal pose bits, and the oracle-side
snap margin of every rendered pose is asserted, so a 1e-12 pose difference cannot move a vertex
across a 1/256-px snap."""
import numpy as np
import pytest

from tests import refine_ref as RF
from tests.test_refine_host import GRIDS, embed, grid, perturbed, scene, spiral

pytestmark = pytest.mark.gpu

K0 = np.array([570.0, 575.0, 31.5, 29.25])
LR, LT = 5000.0, 0.5


def _contour(gpu, entire, visible, bbox, cap=None):
    import torch
    from zebrapose_amd.refine import mask_contour
    counts, xy = mask_contour(torch.from_numpy(entire).to(gpu), None if visible is None else torch.from_numpy(visible).to(gpu),
                              bbox, cap=cap)
    return counts.cpu().numpy(), xy.cpu().numpy()


def _check_contour(gpu, entire, visible, bbox, cap=None):
    counts, xy = _contour(gpu, entire, visible, bbox, cap)
    for b in range(len(entire)):
        want = RF.mask_contour(entire[b], None if visible is None else visible[b], bbox[b])
        assert counts[b] == len(want), (b, counts[b], len(want))
        n = min(len(want), xy.shape[1])
        assert np.array_equal(xy[b, :n], want[:n]), b
    return counts, xy


def test_mask_contour_grids(gpu):
    """Every hand-written grid at S = 16, at the origin (frame pixels, x = 0 / y = 0 dropped) and
    inside; visible absent, all-zero and partial; a bbox with w < S."""
    names = sorted(GRIDS)
    ent = np.stack([embed(grid(n)[0], 16, 16, *o) for n in names for o in [(0, 0), (5, 3)]])
    B = len(ent)
    rng = np.random.default_rng(0)
    bbox = np.stack([rng.integers(0, 400, B), rng.integers(0, 300, B), rng.integers(5, 40, B), rng.integers(5, 40, B)],
                    1).astype(np.int32)
    bbox[:4, 2:] = 16
    counts, _ = _check_contour(gpu, ent, None, bbox)
    assert counts.max() > 0
    _check_contour(gpu, ent, np.zeros_like(ent), bbox)
    part = (rng.random(ent.shape) < 0.08).astype(np.uint8)
    c2, _ = _check_contour(gpu, ent, part, bbox)
    assert 0 < c2.sum() < counts.sum()
    _check_contour(gpu, ent, None, bbox, cap=5)  # cap below the count: the true count, the first five


def test_mask_contour_blobs(gpu):
    """B = 3 random blob fields at S = 128 (holes, islands, many components), a partial visible mask."""
    from scipy import ndimage
    rng = np.random.default_rng(3)
    ent = np.stack([(ndimage.gaussian_filter(rng.normal(size=(128, 128)), 3.0) > 0.02).astype(np.uint8) * 255
                    for _ in range(3)])
    vis = ent * (rng.random(ent.shape) < 0.5)
    vis[2] = 0
    bbox = np.array([[100, 50, 128, 128], [3, 7, 90, 200], [0, 0, 64, 64]], np.int32)
    counts, _ = _check_contour(gpu, ent, None, bbox)
    assert counts.min() > 100
    c2, _ = _check_contour(gpu, ent, vis.astype(np.uint8), bbox)
    assert c2[2] == 0 and 0 < c2[0] < counts[0]


def _step(gpu, depth, pts, R, t, K, cap=None, counts=None, optional=True, lr=LR, lt=LT):
    """zp_edge_refine_step on B depth images; pts: one int array [n, 2] per pose."""
    import torch
    from zebrapose_amd import _lib as L
    B, H, W = depth.shape
    cap = cap or max(1, max(len(p) for p in pts))
    xy = np.zeros((B, cap, 2), np.int32)
    for b, p in enumerate(pts):
        xy[b, :min(len(p), cap)] = np.asarray(p, np.int32).reshape(-1, 2)[:cap]
    cn = np.array([len(p) for p in pts] if counts is None else counts, np.int32)
    bcap = H * W
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for k, v in dict(
        depth=depth.astype(np.float32), counts=cn, xy=xy, R=np.asarray(R, np.float64).reshape(B, 9),
        t=np.asarray(t, np.float64).reshape(B, 3), K=np.asarray(K, np.float64).reshape(B, 4)).items()}
    o = dict(R=torch.full((B, 9), np.nan, dtype=torch.float64, device=gpu),
             t=torch.full((B, 3), np.nan, dtype=torch.float64, device=gpu),
             cost=torch.full((B,), -7, dtype=torch.int64, device=gpu),
             status=torch.full((B,), -7, dtype=torch.int32, device=gpu))
    if optional:
        o.update(border_n=torch.full((B,), -7, dtype=torch.int32, device=gpu),
                 border_xy=torch.full((B, bcap, 2), -7, dtype=torch.int32, device=gpu),
                 match=torch.full((B, cap), -7, dtype=torch.int32, device=gpu),
                 Hb=torch.full((B, 27), np.nan, dtype=torch.float64, device=gpu))
    ws = torch.empty(L.lib.zp_edge_refine_ws_bytes(B, H, W), dtype=torch.uint8, device=gpu)
    L.call("zp_edge_refine_step", B, H, W, d["depth"].data_ptr(), d["counts"].data_ptr(), d["xy"].data_ptr(), cap,
           d["R"].data_ptr(), d["t"].data_ptr(), d["K"].data_ptr(), lr, lt, o["R"].data_ptr(), o["t"].data_ptr(),
           o["cost"].data_ptr(), o["status"].data_ptr(), L.ptr(o.get("border_n")), L.ptr(o.get("border_xy")), bcap,
           L.ptr(o.get("match")), L.ptr(o.get("Hb")), ws.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _check_step(gpu, depth, pts, R, t, K, cap=None):
    got = _step(gpu, depth, pts, R, t, K, cap)
    again = _step(gpu, depth, pts, R, t, K, cap)
    for k in got:  # two runs: the same bits
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), k
    B = len(depth)
    capn = got["match"].shape[1]
    stats = []
    for b in range(B):
        p = np.asarray(pts[b]).reshape(-1, 2)[:capn]
        w = RF.step(depth[b], p, R[b], t[b], K[b], LR, LT)
        stats.append(w["status"])
        assert got["status"][b] == w["status"], (b, got["status"][b], w["status"])
        assert got["border_n"][b] == len(w["border"]), (b, got["border_n"][b], len(w["border"]))
        assert np.array_equal(got["border_xy"][b, :len(w["border"])], w["border"]), b
        assert got["cost"][b] == w["cost"], (b, got["cost"][b], w["cost"])
        if w["status"] != 0:  # copied through bit for bit
            assert np.array_equal(got["R"][b].view(np.int64), np.asarray(R[b], np.float64).reshape(9).view(np.int64))
            assert np.array_equal(got["t"][b].view(np.int64), np.asarray(t[b], np.float64).reshape(3).view(np.int64))
            assert np.all(got["match"][b] == -1) and np.all(got["Hb"][b] == 0)
            continue
        assert np.array_equal(got["match"][b, :len(p)], w["match"]), b
        assert np.all(got["match"][b, len(p):] == -1)
        assert np.abs(got["Hb"][b] - w["Hb"]).max() <= 1e-12 * np.abs(w["Hb"]).max(), b
        tol = 64 * np.linalg.cond(w["A"]) * 2.0 ** -52
        assert np.abs(got["R"][b].reshape(3, 3) - w["R"]).max() <= tol * np.abs(w["R"]).max(), (b, tol)
        assert np.abs(got["t"][b] - w["t"]).max() <= tol * np.abs(w["t"]).max(), (b, tol)
    return got, stats


def _depth_of(sil, rng):
    """A depth image over a silhouette: a smooth surface around 600 plus a little noise, f32."""
    H, W = sil.shape
    yy, xx = np.mgrid[:H, :W]
    d = 600.0 + 0.5 * xx - 0.3 * yy + rng.uniform(0, 2, sil.shape)
    return np.where(sil != 0, d, 0.0).astype(np.float32)


def _poses(rng, B):
    R = np.stack([RF.rodrigues(rng.normal(size=3), rng.uniform(0.2, 2.0)) for _ in range(B)])
    t = rng.uniform(-40, 40, (B, 3)) + np.array([0, 0, 600.0])
    return R, t


def _ring_points(rng, H, W, n):
    """Observed points around the image, some on it, some outside (negative and beyond the far corner)."""
    p = np.stack([rng.integers(-10, W + 10, n), rng.integers(-10, H + 10, n)], 1)
    p[0] = (-5, -7)
    p[1] = (W + 300, H + 200)
    return p


@pytest.mark.parametrize("H,W", [(45, 37), (64, 64)])
def test_step_on_hand_made_silhouettes(gpu, H, W):
    """Every grid scaled until its border has 20 pixels, the spiral, a frame-filling silhouette, a
    border shorter than 20 and an empty image, each with points on and off the image."""
    rng = np.random.default_rng(H)
    sils = []
    for n in sorted(GRIDS):
        g = grid(n)[0]
        s = max(1, min((H - 2) // g.shape[0], (W - 2) // g.shape[1], 4))
        sils.append(embed(g, H, W, 1 if n in ("block", "ring") else 0, 1 if n in ("block", "ring") else 0, s))
    sils.append(spiral(H, W))
    sils.append(np.ones((H, W), np.uint8))          # touches all four frame edges
    cross = np.zeros((H, W), np.uint8)
    cross[H // 2 - 2:H // 2 + 3, :] = 1
    cross[:, W // 2 - 2:W // 2 + 3] = 1
    sils.append(cross)                                # so does this, with four outside regions
    small = np.zeros((H, W), np.uint8)
    small[5:9, 33:37] = 1                             # 12 border pixels, across a word boundary
    sils.append(small)
    B = len(sils)
    depth = np.stack([_depth_of(s, rng) for s in sils])
    pts = [_ring_points(rng, H, W, 40 + 3 * b) for b in range(B)]
    pts[0] = np.zeros((0, 2), np.int64)               # counts = 0
    R, t = _poses(rng, B)
    K = np.tile(np.array([570.0, 575.0, W / 2 - 0.5, H / 2 + 0.25]), (B, 1))
    got, stats = _check_step(gpu, depth, pts, R, t, K)
    assert stats.count(0) >= 8 and stats.count(1) >= 3 and 2 not in stats, stats
    # capped observed list: the first cap points only
    _check_step(gpu, depth[1:4], pts[1:4], R[1:4], t[1:4], K[1:4], cap=17)


def test_step_ties_go_to_the_lowest_index(gpu):
    """A point midway between two border pixels, and the centre of a square: the lowest row-major index."""
    sil = np.zeros((64, 64), np.uint8)
    sil[10:30, 10:30] = 1
    sil[10:30, 41:61] = 1
    rng = np.random.default_rng(1)
    depth = _depth_of(sil, rng)[None]
    pts = [np.array([[35, 20], [19, 19], [50, 20], [35, 5], [35, 40]])]
    R, t = _poses(rng, 1)
    got, _ = _check_step(gpu, depth, pts, R, t, K0[None])
    bxy = got["border_xy"][0]
    m = got["match"][0]
    assert tuple(bxy[m[0]]) == (29, 20)  # (29, 20) and (41, 20) tie: the left one comes first in the row
    assert tuple(bxy[m[1]]) == (19, 10)  # (19, 10) and (10, 19) tie: the upper row comes first


def test_step_large_image_and_spill(gpu):
    """640 x 480 once: masks beyond 64 KB of LDS together, a comb whose border runs past the 4096
    entries kept on chip (the rest go through the workspace), matches in both parts."""
    H, W = 480, 640
    rng = np.random.default_rng(2)
    sil = np.zeros((H, W), np.uint8)
    sil[20:460, 30:600:3] = 1  # 190 teeth, 440 long: every pixel a border pixel
    sil[20:24, 30:600] = 1
    blob = np.zeros((H, W), np.uint8)
    yy, xx = np.mgrid[:H, :W]
    blob[((yy - 250) / 150.0) ** 2 + ((xx - 330) / 220.0) ** 2 < 1] = 1
    blob[200:300, 300:360] = 0  # a hole
    depth = np.stack([_depth_of(sil, rng), _depth_of(blob, rng)])
    assert len(RF.border_list(sil)) > 3 * 4096
    pts = [np.stack([rng.integers(0, W, 300), rng.integers(0, H, 300)], 1) for _ in range(2)]
    R, t = _poses(rng, 2)
    K = np.tile(np.array([572.4, 573.6, 325.3, 242.0]), (2, 1))
    got, stats = _check_step(gpu, depth, pts, R, t, K)
    assert stats == [0, 0] and got["match"][0].max() > 4096


def test_bad_arguments(gpu):
    import torch
    from zebrapose_amd import _lib as L
    lib = L.lib
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=gpu)
    p, q = buf.data_ptr(), buf.data_ptr() + 4096
    assert lib.zp_edge_refine_ws_bytes(1, 480, 640) > 0 and lib.zp_edge_refine_ws_bytes(2, 540, 720) > 0
    for bad in [(0, 64, 64), (1, 0, 64), (1, 64, 0), (1, 1024, 1024), (1, 1, 40000), (70000, 8, 8)]:
        assert lib.zp_edge_refine_ws_bytes(*bad) == -1, bad

    def step(B=1, H=16, W=16, depth=p, counts=p, xy=p, cap=4, R=p, t=p, K=p, lr=LR, lt=LT, Ro=q, to=q, cost=q, status=q,
             bcap=0, ws=p):
        return lib.zp_edge_refine_step(B, H, W, depth, counts, xy, cap, R, t, K, lr, lt, Ro, to, cost, status, None, None,
                                       bcap, None, None, ws, None)

    for kw in [dict(B=0), dict(H=0), dict(W=40000), dict(H=1024, W=1024), dict(cap=0), dict(cap=(1 << 20) + 1),
               dict(depth=None), dict(counts=None), dict(xy=None), dict(R=None), dict(t=None), dict(K=None),
               dict(Ro=None), dict(to=None), dict(cost=None), dict(status=None), dict(ws=None), dict(lr=0.0),
               dict(lt=-1.0), dict(lr=float("nan")), dict(Ro=p), dict(to=p)]:
        assert step(**kw) == 1, kw
        assert b"zp_edge_refine_step" in lib.zp_last_error()
    for args in [(0, 16, p, None, p, 4, q, q), (1, 0, p, None, p, 4, q, q), (1, 1024, p, None, p, 4, q, q),
                 (1, 16, None, None, p, 4, q, q), (1, 16, p, None, None, 4, q, q), (1, 16, p, None, p, 0, q, q),
                 (1, 16, p, None, p, 4, None, q), (1, 16, p, None, p, 4, q, None)]:
        assert lib.zp_mask_contour(*args, None) == 1, args
    torch.cuda.synchronize()


def test_end_to_end_against_the_oracle_loop(gpu, tmp_path):
    """96 x 96, the deformed icosphere, B = 4 perturbed poses: the contour from a device-rendered mask,
    EdgeRefiner.refine against refine_ref.refine; then py_edge_refine from a PLY file."""
    import torch
    from zebrapose_amd.refine import EdgeRefiner, mask_contour, py_edge_refine
    from zebrapose_amd.render import MeshRenderer
    H = W = 96
    verts, faces, K, Rg, tg, pts, _ = scene(H, W)
    rend = MeshRenderer(verts, faces, device=gpu)
    Kr = K + np.array([0, 0, 0.5, 0.5])
    mask = rend.render(Rg[None], tg[None], Kr[None], H, W, outputs=("mask",))["mask"]
    counts, xy = mask_contour(mask, None, np.array([[0, 0, W, W]]))
    assert int(counts[0]) == len(pts) and np.array_equal(xy[0, :len(pts)].cpu().numpy(), pts)
    seeds = [2, 4, 5, 7]
    start = [perturbed(Rg, tg, s) for s in seeds]
    R0, t0 = np.stack([p[0] for p in start]), np.stack([p[1] for p in start])
    ref = EdgeRefiner(rend, H, W)
    Rd, td, status, cost = ref.refine(torch.from_numpy(R0).to(gpu), torch.from_numpy(t0).to(gpu), K,
                                      counts.expand(4).contiguous(), xy.expand(4, -1, -1).contiguous())
    Rd, td, status, cost = (a.cpu().numpy() for a in (Rd, td, status, cost))
    for b in range(4):
        margins = []
        Rw, tw, sw, cw = RF.refine(verts, faces, R0[b], t0[b], K, H, W, pts,
                                   on_pose=lambda R, t: margins.append(RF.snap_margin(verts, R, t, Kr)))
        # oracle side: no rendered pose has a vertex within 1e-6 of a 1/256-px snap boundary, and a
        # 1e-12 pose difference moves a projection by far less
        assert min(margins) >= 1e-6, (b, min(margins))
        assert sw == 0 and status[b] == 0
        assert cost[:, b].tolist() == cw, (b, cost[:, b].tolist(), cw)
        assert np.abs(Rd[b] - Rw).max() <= 1e-6 and np.abs(td[b] - tw).max() <= 1e-6, b
        assert RF.add_error(verts, Rd[b], td[b], Rg, tg) < 0.5 * RF.add_error(verts, R0[b], t0[b], Rg, tg)

    # a pose whose render is empty stops with status 1 and comes back as it went in
    far = t0[:1] + np.array([0, 0, -1000.0])
    Rs, ts, ss, _ = ref.refine(R0[:1], far, K, counts, xy)
    assert int(ss[0]) == 1 and np.array_equal(Rs[0].cpu().numpy(), R0[0]) and np.array_equal(ts[0].cpu().numpy(), far[0])

    ply = tmp_path / "obj.ply"
    with open(ply, "w") as fh:
        fh.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(verts), len(faces)))
        for v in verts:
            fh.write("%.9g %.9g %.9g\n" % tuple(float(c) for c in v))
        for f in faces:
            fh.write("3 %d %d %d\n" % tuple(int(i) for i in f))
    Rp, tp = py_edge_refine(R0[0], t0[0] / 1000.0, K[0], K[1], K[2], K[3], W, H, pts.astype(np.float32), str(ply),
                            str(tmp_path))
    Ru, tu, _, _ = ref.refine(R0[:1], (t0[0] / 1000.0)[None] / 0.001, K, counts, xy)
    assert Rp.dtype == np.float32 and Rp.shape == (3, 3) and tp.shape == (3,)
    assert np.array_equal(Rp, Ru[0].cpu().numpy().astype(np.float32))
    assert np.array_equal(tp, (tu[0].cpu().numpy() * 0.001).astype(np.float32))
