"""ICP refinement on the device (zp_depth_points, zp_icp; zebrapose_amd/icp.py) against the numpy
restatement tests/icp_ref.py.

Point clouds: order and f64 bits are equal (single IEEE operations); the statistics differ in the order
of summation, 1e-12 of the largest coordinate.  Neighbour indices are exact wherever the oracle's NN
margin (relative gap between the best and second-best squared distance) is at least 1e-9, which every
test asserts for its own inputs.  One fit: |dR| <= 8 * 2 * (1e-12 max|H|) * 3 / (s2 + s3) with H and the
singular values from the oracle (1e-12 max|H|: a reordered f64 sum; 2 / (s2 + s3): the polar factor's
perturbation bound; 3: Frobenius over max norm; 8: the solver's own rounding), the smaller of the bounds
of the two fits behind T; t to that bound times the cloud's radius (the largest distance of a subsample
point from their centroid).  Loops: equal iteration counts and poses within 1e-6.  Every call runs twice and
gives the same bits."""
import numpy as np
import pytest

from tests import icp_ref as IR
from tests import refine_ref as RF
from tests.test_icp_host import cloud, moved

pytestmark = pytest.mark.gpu

MARGIN = 1e-9


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _points(gpu, depth, K, cap=None, filt=None, factor=2.0):
    """depth_points twice (equal bits), as numpy"""
    import torch
    from zebrapose_amd.icp import depth_points
    runs = []
    for _ in range(2):
        o = depth_points(torch.from_numpy(depth).to(gpu), K, cap=cap, filter=filt, factor=factor, want_stats=True)
        runs.append([v.cpu().numpy() for v in o])
    for a, b in zip(*runs):
        assert np.array_equal(_bits(a), _bits(b))
    return runs[0]


def _check_points(gpu, depth, K, cap=None, filt=None, factor=2.0):
    counts, pts, stats = _points(gpu, depth, K, cap, filt, factor)
    want = []
    for b in range(len(depth)):
        w = IR.depth_points(depth[b], K[b], cap, None if filt is None else filt[b], factor)
        assert w["edge"] >= MARGIN, (b, w["edge"])
        assert counts[b] == w["count"], (b, counts[b], w["count"])
        assert np.array_equal(_bits(pts[b, :len(w["pts"])]), _bits(w["pts"])), b
        scale = max(np.abs(w["pts"]).max(), 1.0) if len(w["pts"]) else 1.0
        assert np.abs(stats[b] - w["stats"]).max() <= 1e-12 * scale, (b, stats[b], w["stats"])
        want.append(w)
    return want


def images(H, W, seed):
    """all zero; full; one pixel in the last row and column; sparse random with a NaN and a negative value"""
    rng = np.random.default_rng(seed)
    d = np.zeros((4, H, W), np.float32)
    d[1] = 500 + 100 * rng.random((H, W))
    d[2, H - 1, W - 1] = 321.5
    sp = rng.random((H, W)) < 0.15
    d[3][sp] = (400 + 300 * rng.random(sp.sum())).astype(np.float32)
    ys, xs = np.nonzero(sp)
    d[3, ys[3], xs[3]], d[3, ys[10], xs[10]], d[3, ys[20], xs[20]] = np.nan, -250.0, np.inf
    K = np.stack([[150.0 + b, 148.0, W / 2.0 - 0.25 * b, H / 2.0 + 0.5] for b in range(4)])
    return d, K


@pytest.mark.parametrize("shape", [(37, 45), (64, 64)])
def test_depth_points_small(gpu, shape):
    d, K = images(*shape, seed=shape[0])
    want = _check_points(gpu, d, K)
    assert [w["count"] for w in want][:3] == [0, shape[0] * shape[1], 1] and want[3]["count"] > 100
    assert np.isfinite(want[3]["pts"]).all() and (want[3]["pts"][:, 2] > 0).all()
    _check_points(gpu, d, K, cap=50)  # the true count, the first fifty points
    # a filter that cuts each cloud: its own centroid and 0.6 of its radius
    filt = np.stack([w["stats"] for w in want])
    cut = _check_points(gpu, d, K, filt=filt, factor=0.6)
    assert cut[0]["count"] == 0 and 0 < cut[1]["count"] < want[1]["count"] and 0 < cut[3]["count"] < want[3]["count"]
    assert cut[2]["count"] == 0  # one point, radius 0: nothing is closer than 0
    _check_points(gpu, d, K, cap=7, filt=filt, factor=0.6)


def test_depth_points_vga(gpu):
    """480 x 640: 300 tiles of 1024 pixels, the running base carries the order across them"""
    rng = np.random.default_rng(7)
    H, W = 480, 640
    d = np.zeros((1, H, W), np.float32)
    yy, xx = np.mgrid[:H, :W]
    blob = ((yy - 250) / 130.0) ** 2 + ((xx - 300) / 170.0) ** 2 < 1
    d[0][blob] = (700 + 60 * rng.random(blob.sum())).astype(np.float32)
    sp = rng.random((H, W)) < 0.01
    d[0][sp] = 1500.0
    K = np.array([[572.4, 573.6, 325.3, 242.0]])
    want = _check_points(gpu, d, K)
    assert want[0]["count"] > 60000
    far = _check_points(gpu, d, K, cap=3000, filt=np.array([[0.0, 10.0, 730.0, 150.0]]), factor=2.0)
    assert 3000 < far[0]["count"] < want[0]["count"]


def _icp(gpu, src, dst, draws_s, draws_d, R, t, N, max_iterations=200, tolerance=5e-7, mode=0, src_cap=None,
         dst_cap=None):
    """zp_icp twice (equal bits) on lists of per-pose clouds, with the debug outputs; as numpy"""
    import torch
    from zebrapose_amd import _lib as L
    B = len(src)
    scap = src_cap or max(1, max(len(p) for p in src))
    dcap = dst_cap or max(1, max(len(p) for p in dst))

    def pack(lst, cap):
        a = np.full((B, cap, 3), np.nan)
        for b, p in enumerate(lst):
            a[b, :min(len(p), cap)] = np.asarray(p, np.float64).reshape(-1, 3)[:cap]
        return a

    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for k, v in dict(
        src=pack(src, scap), dst=pack(dst, dcap), ns=np.array([len(p) for p in src], np.int32),
        nd=np.array([len(p) for p in dst], np.int32), ds=np.asarray(draws_s, np.float64).reshape(B, N),
        dd=np.asarray(draws_d, np.float64).reshape(B, N), R=np.asarray(R, np.float64).reshape(B, 9),
        t=np.asarray(t, np.float64).reshape(B, 3)).items()}
    assert L.lib.zp_icp_ws_bytes(B, N) == 0
    runs = []
    for _ in range(2):
        o = dict(R=torch.full((B, 9), np.nan, dtype=torch.float64, device=gpu),
                 t=torch.full((B, 3), np.nan, dtype=torch.float64, device=gpu),
                 status=torch.full((B,), -7, dtype=torch.int32, device=gpu),
                 iterations=torch.full((B,), -7, dtype=torch.int32, device=gpu),
                 mean_error=torch.full((B,), np.nan, dtype=torch.float64, device=gpu),
                 nn=torch.full((B, N), -7, dtype=torch.int32, device=gpu),
                 T=torch.full((B, 16), np.nan, dtype=torch.float64, device=gpu))
        L.call("zp_icp", B, N, d["src"].data_ptr(), d["ns"].data_ptr(), scap, d["dst"].data_ptr(), d["nd"].data_ptr(),
               dcap, d["ds"].data_ptr(), d["dd"].data_ptr(), max_iterations, tolerance, mode, IR.MIN_FRACTION,
               IR.ANGLE_LIMIT, d["R"].data_ptr(), d["t"].data_ptr(), o["R"].data_ptr(), o["t"].data_ptr(),
               o["status"].data_ptr(), o["iterations"].data_ptr(), o["mean_error"].data_ptr(), o["nn"].data_ptr(),
               o["T"].data_ptr(), None, L.stream_ptr())
        torch.cuda.synchronize()
        runs.append({k: v.cpu().numpy() for k, v in o.items()})
    for k in runs[0]:
        assert np.array_equal(_bits(runs[0][k]), _bits(runs[1][k])), k
    return runs[0]


def fit_bound(H, S):
    return 8 * 2 * (1e-12 * np.abs(H).max()) * 3 / (S[1] + S[2])


def pair(seed, n, extra=(5, 9), deg=4.0, shift=(2.0, -1.5, 2.5), noise=0.3):
    """source list (n + extra[0] points) and destination list (n + extra[1]): a second draw of the same
    distribution, moved, with noise; and the draws of both subsamples"""
    rng = np.random.default_rng(seed)
    A = cloud(seed, n + extra[0])
    Bm = moved(cloud(seed + 1000, n + extra[1]), rng.normal(size=3), deg, shift)[0]
    Bm = Bm + rng.normal(size=Bm.shape) * noise
    return A, Bm, rng.random(n), rng.random(n)


R0 = RF.rodrigues([1, 2, 3], 0.4)
T0 = np.array([1.0, 2.0, 500.0])


@pytest.mark.parametrize("n", [7, 64, 65, 1023, 1025, 3000, 4096])
def test_one_iteration(gpu, n):
    """max_iterations = 1: the neighbours exactly, T through both fits within the bound of the header"""
    A, Bm, us, ud = pair(n, n)
    w = IR.icp_pose(A, Bm, us, ud, R0, T0, max_iterations=1)
    assert w["status"] == 0 and w["n"] == n and w["margins"][0] >= MARGIN
    _, _, _, Hf, Sf = IR.best_fit_transform(w["A"], w["A"] @ w["T"][:3, :3].T + w["T"][:3, 3])
    bound = min(fit_bound(w["H"], w["S"]), fit_bound(Hf, Sf))
    assert bound < 1e-8, bound
    got = _icp(gpu, [A], [Bm], us, ud, R0, T0, n, max_iterations=1)
    assert got["status"][0] == 0 and got["iterations"][0] == 1
    assert np.array_equal(got["nn"][0], w["nn"])
    T = got["T"][0].reshape(4, 4)
    assert np.array_equal(T[3], [0, 0, 0, 1])
    radius = np.linalg.norm(w["A"] - w["A"].mean(0), axis=1).max()  # the cloud's radius, as stats has it
    dR, dt = np.abs(T[:3, :3] - w["T"][:3, :3]).max(), np.abs(T[:3, 3] - w["T"][:3, 3]).max()
    print(f"n {n}: |dR| {dR:.3e} (bound {bound:.3e}), |dt| {dt:.3e} (bound {bound * radius:.3e})")
    assert dR <= bound, (dR, bound)
    assert dt <= bound * radius, (dt, bound * radius)
    assert abs(got["mean_error"][0] - w["mean_error"]) <= 1e-12 * w["mean_error"]
    # the pose out is the device's own T applied to the pose in: five f64 operations an entry, each
    # rounding at 2^-53 of a term no larger than max|t|
    Re, te = T[:3, :3] @ R0, T[:3, :3] @ T0 + T[:3, 3]
    eps = 8 * 2.0 ** -53 * max(np.abs(te).max(), 1.0)
    assert np.abs(got["R"][0].reshape(3, 3) - Re).max() <= eps and np.abs(got["t"][0] - te).max() <= eps


def test_ties_go_to_the_lowest_index(gpu):
    """Duplicated destination points, and source points midway between two lattice points: every
    coordinate is a small integer or a half, so the equal distances are equal in f64 too."""
    lat = np.array([[x, y, 600.0] for y in (0, 4, 8) for x in (0, 4, 8)], np.float64)
    dst = np.concatenate([lat, lat[[2, 5]], lat[[2]]])      # 9 and 11 repeat point 2, 10 repeats point 5
    src = np.array([[8, 0, 601], [8, 4, 599],               # on the repeated points
                    [2, 0, 600], [6, 4, 600], [4, 6, 600],  # midway between 0 | 1, 4 | 5, 4 | 7
                    [2, 2, 600], [6.5, 6, 600], [0, 8, 600.5], [1, 7, 600], [8, 8, 600], [3, 3, 600], [4, 0, 602]],
                   np.float64)
    n = len(dst)
    assert len(src) == n
    u = (np.arange(n) + 0.5) / n
    w = IR.icp_pose(src, dst, u, u, R0, T0, max_iterations=1)
    assert w["nn"][:6].tolist() == [2, 5, 0, 4, 4, 0]
    got = _icp(gpu, [src], [dst], u, u, R0, T0, n, max_iterations=1)
    assert np.array_equal(got["nn"][0], w["nn"])


def status_batch():
    """normal; a 30 degree turn about z; no rendered points; fewer than 1 / 20 measured points"""
    A = cloud(3, 80)
    ok = moved(A, [0.1, 0.2, 0.9], 3.0, [1.0, 0.5, -2.0])[0]
    big = moved(A, [0, 0, 1], 30.0, [0, 0, 0])[0]
    return [A, A, np.zeros((0, 3)), A], [ok, big, ok, ok[:3]]


@pytest.mark.parametrize("mode", [IR.FULL, IR.DEPTH_ONLY, IR.NO_DEPTH])
def test_modes_and_statuses(gpu, mode):
    src, dst = status_batch()
    N, B = 80, 4
    u = np.tile((np.arange(N) + 0.5) / N, (B, 1))
    Rs = np.stack([RF.rodrigues([1, 2, 3], 0.4 + 0.1 * b) for b in range(B)])
    ts = T0 + np.arange(B)[:, None]
    got = _icp(gpu, src, dst, u, u, Rs, ts, N, mode=mode)
    want = [IR.icp_pose(src[b], dst[b], u[b], u[b], Rs[b], ts[b], mode=mode) for b in range(B)]
    assert [w["status"] for w in want] == [0, 3 if mode == IR.NO_DEPTH else 0, 1, 2]
    for b, w in enumerate(want):
        assert all(m >= MARGIN for m in w["margins"]), b
        assert got["status"][b] == w["status"] and got["iterations"][b] == w["iterations"], b
        T = got["T"][b].reshape(4, 4)
        if w["status"] != 0:  # the pose bits go through
            assert np.array_equal(_bits(got["R"][b]), _bits(Rs[b].reshape(9))) and np.array_equal(_bits(got["t"][b]), _bits(ts[b]))
        else:
            assert np.abs(got["R"][b].reshape(3, 3) - w["R"]).max() <= 1e-6 and np.abs(got["t"][b] - w["t"]).max() <= 1e-6
        if w["status"] in (1, 2):
            assert np.array_equal(T, np.eye(4)) and got["mean_error"][b] == 0 and (got["nn"][b] == -1).all()
        else:
            assert np.abs(T - w["T"]).max() <= 1e-6
            if mode == IR.DEPTH_ONLY:
                assert np.array_equal(T[:3, :3], np.eye(3))
            if mode == IR.NO_DEPTH:
                assert T[2, 3] == 0.0


LOOP_SEEDS = [11, 12, 13]


@pytest.mark.parametrize("seed", LOOP_SEEDS)
def test_loop(gpu, seed):
    n = 200
    A, Bm, us, ud = pair(seed, n)
    w = IR.icp_pose(A, Bm, us, ud, R0, T0)
    assert w["status"] == 0 and 3 < w["iterations"] < 200 and min(w["margins"]) >= MARGIN, (w["iterations"], min(w["margins"]))
    got = _icp(gpu, [A], [Bm], us, ud, R0, T0, n)
    assert got["status"][0] == 0 and got["iterations"][0] == w["iterations"]
    assert np.array_equal(got["nn"][0], w["nn"])
    assert np.abs(got["R"][0].reshape(3, 3) - w["R"]).max() <= 1e-6 and np.abs(got["t"][0] - w["t"]).max() <= 1e-6
    assert abs(got["mean_error"][0] - w["mean_error"]) <= 1e-6


def test_loop_stops_at_max_iterations(gpu):
    n = 200
    A, Bm, us, ud = pair(LOOP_SEEDS[0], n)
    w = IR.icp_pose(A, Bm, us, ud, R0, T0, max_iterations=3)
    assert w["iterations"] == 3 and min(w["margins"]) >= MARGIN
    got = _icp(gpu, [A], [Bm], us, ud, R0, T0, n, max_iterations=3)
    assert got["iterations"][0] == 3 and np.array_equal(got["nn"][0], w["nn"])
    assert np.abs(got["t"][0] - w["t"]).max() <= 1e-6


E2E_N = 800
E2E_SEEDS = [21, 22, 23, 24]


def e2e_scene():
    """tests.test_refine_host.scene()'s mesh and GT pose; B = 4 starts, translation-dominant (the mesh
    is near-spherical: depth says little about its rotation); draws for both subsamples.  Point-to-point
    ICP between two subsamples of pixel-grid clouds settles 1 to 2.7 units of ADD from the truth here (a
    pixel is 1.3 units across at this distance) wherever it starts, so the starts are 5 to 9 units off.
    The floor stayed in that range on the oracle with the band narrowed or moved and with 400 to 1200
    points, so it is not the band's position or the subsample noise alone; what remains is rendered
    points behind the band matching its edges and the rotation a near-spherical surface leaves free.
    The parts were not separated further."""
    from tests.test_refine_host import scene
    verts, faces, K, Rg, tg, _, _ = scene()
    R, t = [], []
    for s in E2E_SEEDS:
        rng = np.random.default_rng(s)
        R.append(Rg @ RF.rodrigues(rng.normal(size=3), np.deg2rad(rng.uniform(0.5, 1.5))))
        t.append(tg + rng.uniform(-1, 1, 3) * np.array([5.0, 5.0, 10.0]))
    draws = np.random.default_rng(5).random((2, len(E2E_SEEDS), E2E_N))
    return verts, faces, K, Rg, tg, np.stack(R), np.stack(t), draws


def measured(gt_depth):
    """the GT render with a band of rows zeroed (an occluder) and a far plane behind the object"""
    d = np.array(gt_depth, np.float32)
    d[d == 0] = 900.0
    d[40:47] = 0.0
    return d


def test_end_to_end(gpu):
    import torch
    from zebrapose_amd.icp import ICPRefiner
    from zebrapose_amd.render import MeshRenderer
    verts, faces, K, Rg, tg, R, t, draws = e2e_scene()
    B, H, W = len(R), 96, 96
    rend = MeshRenderer(verts, faces, device=gpu)
    Kr = K + np.array([0, 0, 0.5, 0.5])
    gt = rend.render(Rg.reshape(1, 9), tg[None], Kr[None], H, W, outputs=("depth",))["depth"][0].cpu().numpy()
    dm = measured(gt)
    ref = ICPRefiner(rend, (W, H), n_points=E2E_N, device=gpu)
    dmb = torch.from_numpy(np.repeat(dm[None], B, 0)).to(gpu)
    runs = [[v.cpu().numpy() for v in ref.refine_batch(dmb, torch.from_numpy(R).to(gpu), t, K, draws=draws)]
            for _ in range(2)]
    for a, b in zip(*runs):
        assert np.array_equal(_bits(a), _bits(b))
    Ro, to, status, iters, err = runs[0]
    for b in range(B):
        w = IR.refine(verts, faces, dm, R[b], t[b], K, draws[0, b], draws[1, b])
        assert w["edge"] >= MARGIN and min(w["margins"]) >= MARGIN, (b, w["edge"], min(w["margins"]))
        assert status[b] == w["status"] == 0 and iters[b] == w["iterations"], (b, status[b], iters[b], w["iterations"])
        assert np.abs(Ro[b] - w["R"]).max() <= 1e-6 and np.abs(to[b] - w["t"]).max() <= 1e-6, b
        before, after = RF.add_error(verts, R[b], t[b], Rg, tg), RF.add_error(verts, Ro[b], to[b], Rg, tg)
        assert after < before / 2, (b, before, after)
    # the reference's one-pose signature: row 0 of the batch, bit for bit
    K33 = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]])
    R1, t1 = ref.refine(dm, R[0], t[0].reshape(3, 1), K33, draws=draws[:, :1])
    assert R1.shape == (3, 3) and t1.shape == (3,)
    assert np.array_equal(_bits(R1), _bits(Ro[0])) and np.array_equal(_bits(t1), _bits(to[0]))
    # no_depth and depth_only run through the same signature
    R2, t2 = ref.refine(dm, R[0], t[0], K33, depth_only=True, draws=draws[:, :1])
    assert np.array_equal(_bits(R2), _bits(R[0]))  # R = I: the rotation goes through
    assert RF.add_error(verts, R2, t2, Rg, tg) < RF.add_error(verts, R[0], t[0], Rg, tg)
