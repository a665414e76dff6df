"""The edge-refinement oracle itself (tests/refine_ref.py), on the CPU: border sets against answers
written out by hand, the Jacobian against central differences, the unit invariance of a step, and
convergence of the ten-step loop on a shape whose silhouette pins the pose."""
import numpy as np
import pytest

from tests import refine_ref as RF

# '.' unset, '#' set, 'B' set and on the outer border
GRIDS = {
    "block": ["......",
              ".BBBB.",
              ".B##B.",
              ".B##B.",
              ".BBBB.",
              "......"],
    # the pixels around the hole touch unset pixels, but not the outside
    "ring": [".........",
             ".BBBBBBB.",
             ".B#####B.",
             ".B#...#B.",
             ".B#...#B.",
             ".B#...#B.",
             ".B#####B.",
             ".BBBBBBB.",
             "........."],
    # a component inside the hole has no outer border of its own
    "island": ["BBBBBBBBB",
               "B#######B",
               "B#.....#B",
               "B#.....#B",
               "B#..#..#B",
               "B#.....#B",
               "B#.....#B",
               "B#######B",
               "BBBBBBBBB"],
    "two": ["BBB....",
            "B#B....",
            "BBB..BB",
            ".....BB"],
    "frame": ["BBBBB",
              "B###B",
              "BBBBB",
              ".....",
              "....B"],
    "line": [".......",
             ".BBBBB.",
             "......."],
    "diagonal": ["BB....",
                 "BB....",
                 "..BB..",
                 "..BB..",
                 "....B.",
                 ".....B"],
    # the centre's only unset neighbour is diagonal: not a border pixel
    "corner": [".....",
               "..BB.",
               ".B#B.",
               ".BBB.",
               "....."],
    "empty": ["....",
              "....",
              "...."],
    "full": ["BBBBB",
             "B###B",
             "B###B",
             "BBBBB"],
    # an unset pocket open to the outside through a one-pixel gap: its walls are border pixels
    "pocket": ["BBBBBBB",
               ".....BB",
               "BBBB.BB",
               "B##B.BB",
               "B###B#B",
               "BBBBBBB"],
}


def grid(name):
    """(image u8 [H, W], expected border bool [H, W])"""
    rows = GRIDS[name]
    a = np.array([list(r) for r in rows])
    return (a != ".").astype(np.uint8), a == "B"


def embed(img, H, W, y0=0, x0=0, scale=1):
    """img scaled by an integer factor, pasted at (y0, x0) of an H x W canvas"""
    out = np.zeros((H, W), img.dtype)
    big = np.kron(img, np.ones((scale, scale), img.dtype))
    out[y0:y0 + big.shape[0], x0:x0 + big.shape[1]] = big
    return out


def spiral(H, W):
    """A one-pixel wall spiralling inwards from the frame, pitch 2: the corridor beside it is open to
    the outside at one end only, so the fill has to walk it turn by turn."""
    a = np.zeros((H, W), np.uint8)
    y0, x0, y1, x1 = 0, 0, H - 1, W - 1
    a[0, 2:] = 1  # the top wall leaves the corridor's mouth open at the left
    while y1 - y0 >= 4 and x1 - x0 >= 4:
        a[y0:y1 + 1, x1] = 1
        a[y1, x0:x1 + 1] = 1
        a[y0 + 2:y1 + 1, x0] = 1
        a[y0 + 2, x0:x1 - 1] = 1
        y0, x0, y1, x1 = y0 + 2, x0 + 2, y1 - 2, x1 - 2
    return a


def staircase_cells(S):
    """The cells (x, y) of a one-pixel corridor through a solid S x S image, in the order the outside
    reaches them: staircases (right 1, down 1, ...) three columns apart, so that neighbouring ones
    touch only at corners, joined alternately at their far and near ends into one serpentine with
    its mouth at (0, 1) on the frame.  Row and column sweeps both stop at every corner: a fill pass
    (rows, then columns) advances one stair."""
    free = np.zeros((S, S), bool)
    k = 0
    while 3 * k + 4 <= S - 2:
        y_end = S - 3 - 3 * k
        for y in range(1, y_end + 1):
            free[y, y + 3 * k:y + 3 * k + 2] = True
        if 3 * (k + 1) + 4 <= S - 2:
            if k % 2 == 0:
                free[y_end - 3:y_end + 1, S - 2] = True  # the far ends, down the last inner column
            else:
                free[1, 3 * k + 3] = True                # the near ends, along the first inner row
        k += 1
    free[1, 0] = True
    # breadth-first from the mouth: the order of arrival
    order, seen, front = [], np.zeros_like(free), [(0, 1)]
    seen[1, 0] = True
    while front:
        order += front
        nxt = []
        for x, y in front:
            for u, v in ((x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)):
                if 0 <= u < S and 0 <= v < S and free[v, u] and not seen[v, u]:
                    seen[v, u] = True
                    nxt.append((u, v))
        front = nxt
    assert len(order) == free.sum()  # one corridor: everything is reached
    return order


def staircase(S, length=None):
    """u8 [S, S]: solid but for the first `length` cells (default: all) of staircase_cells(S)."""
    a = np.ones((S, S), np.uint8)
    cells = staircase_cells(S)
    for x, y in cells[:len(cells) if length is None else length]:
        a[y, x] = 0
    return a


STAIR_S = 54  # the smallest S at which the whole serpentine takes more than 4 (S + S) passes


_STAIRS = {}


def staircase_at_cap(S=None):
    """(over, last, under): the whole serpentine (more changing passes than the cap 4 (S + S)), the
    longest prefix whose last changing pass is pass `cap` (the fill is complete, the device's next
    pass would have found nothing to do, and there is no next pass), and the longest whose last
    changing pass is pass `cap - 1` (the device's last pass sees that nothing changes)."""
    S = S or STAIR_S
    if S not in _STAIRS:
        cap, n = 8 * S, len(staircase_cells(S))

        def longest(passes):  # the pass count does not fall as the corridor grows
            lo, hi = 1, n
            while lo < hi:
                mid = (lo + hi + 1) // 2
                lo, hi = (mid, hi) if RF.fill_passes(staircase(S, mid)) <= passes else (lo, mid - 1)
            return staircase(S, lo)

        _STAIRS[S] = (staircase(S), longest(cap), longest(cap - 1))
    return _STAIRS[S]


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_border_sets_on_hand_written_grids(name):
    img, want = grid(name)
    got = RF.outer_border(img)
    assert np.array_equal(got, want), "\n".join("".join("B" if b else "." for b in r) for r in got)
    lst = RF.border_list(img)
    assert len(lst) == want.sum() and all(want[y, x] for x, y in lst)
    assert [tuple(p) for p in lst[:, ::-1]] == sorted(tuple(p) for p in lst[:, ::-1])  # row-major
    if name in ("block", "ring", "line", "corner"):  # drawn with a margin: the same anywhere on a canvas
        for y0, x0 in [(0, 0), (3, 5), (16 - img.shape[0], 16 - img.shape[1])]:
            assert np.array_equal(RF.outer_border(embed(img, 16, 16, y0, x0)),
                                  embed(want.astype(np.uint8), 16, 16, y0, x0) != 0)


def test_fill_pass_counts():
    """Convex shapes are filled by the first row sweep; the spiral needs many passes, fewer than the cap."""
    assert RF.fill_passes(grid("empty")[0]) == 0
    assert RF.fill_passes(embed(grid("block")[0], 16, 16, 3, 3)) <= 1
    sp = spiral(45, 37)
    n = RF.fill_passes(sp)
    assert 8 <= n < 4 * (45 + 37), n
    # the corridor is outside: both faces of the wall are border pixels, the whole wall
    assert np.array_equal(RF.outer_border(sp), sp != 0)


def test_mask_contour_filters_and_maps():
    img, _ = grid("block")
    ent = embed(img, 16, 16, 0, 0, 2)  # block at 2 .. 9
    pts = RF.mask_contour(ent, None, (10, 20, 16, 16))
    assert len(pts) == 28 and pts.min(0).tolist() == [12, 22]
    ent0 = embed(np.ones((4, 4), np.uint8), 16, 16)  # touches x = 0 and y = 0: those pixels are dropped
    p0 = RF.mask_contour(ent0, None, (0, 0, 16, 16))
    assert sorted(map(tuple, p0)) == [(1, 3), (2, 3), (3, 1), (3, 2), (3, 3)]
    vis = np.zeros((16, 16), np.uint8)
    assert len(RF.mask_contour(ent, vis, (0, 0, 16, 16))) == 0
    vis[2, 2] = 1  # supports (2, 2), (3, 2), (2, 3) and the interior pixel (3, 3)
    assert sorted(map(tuple, RF.mask_contour(ent, vis, (0, 0, 16, 16)))) == [(2, 2), (2, 3), (3, 2)]
    half = RF.mask_contour(ent, None, (5, 7, 8, 8))  # w < S: truncation makes duplicates, which are kept
    assert len(half) == 28 and len({tuple(p) for p in half}) < 28


def _project(X, K):
    return np.array([K[0] * X[0] / X[2] + K[2], K[1] * X[1] / X[2] + K[3]])


def test_jacobian_against_central_differences():
    rng = np.random.default_rng(5)
    K = np.array([570.0, 575.0, 320.0, 240.0])
    for _ in range(5):
        R = RF.rodrigues(rng.normal(size=3), rng.uniform(0.2, 2.5))
        t = np.array([rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(400, 900)])
        Xb = rng.uniform(-60, 60, 3)
        obs = rng.uniform(0, 600, 2)

        def e(th):
            return obs - _project(R @ RF.exp_so3(th[:3]) @ (Xb + th[3:]) + t, K)

        J = RF.jacobian(R @ Xb + t, R, t, K)
        num = np.zeros((2, 6))
        for k in range(6):
            h = np.zeros(6)
            h[k] = 1e-5 if k < 3 else 1e-3
            num[:, k] = (e(h) - e(-h)) / (2 * h[k])
        # central differences: O(h^2) truncation plus rounding, both far below 1e-6 of the scale
        assert np.abs(J - num).max() <= 1e-6 * np.abs(J).max()


def scene(H=96, W=96):
    """The deformed icosphere in front of a 96 x 96 camera: (verts, faces, K, R_true, t_true, observed
    contour of the true pose)."""
    from tests import render_ref as RR
    verts, faces = RF.deformed_icosphere(2)
    K = np.array([150.0, 150.0, W / 2.0, H / 2.0])
    Rg = RF.rodrigues([0.3, -0.8, 0.5], 0.9)
    tg = np.array([2.0, -3.0, 200.0])
    Kr = K + np.array([0, 0, 0.5, 0.5])
    depth = RR.render(verts, faces, None, Rg.reshape(1, 9), tg[None], Kr[None], H, W)["depth"][0]
    pts = RF.mask_contour((depth > 0).astype(np.uint8), None, (0, 0, W, W)) if H == W else None
    return verts, faces, K, Rg, tg, pts, depth


def perturbed(Rg, tg, seed):
    rng = np.random.default_rng(seed)
    R = Rg @ RF.rodrigues(rng.normal(size=3), np.deg2rad(rng.uniform(6.0, 10.0)))
    return R, tg + rng.uniform(-1, 1, 3) * np.array([4.0, 4.0, 12.0])


def test_step_is_invariant_to_the_unit():
    """Millimetres with lambda_trans 0.5 and metres with 500000 are the same problem: the same
    rotation, the translation update scaled by the unit."""
    from tests import render_ref as RR
    verts, faces, K, Rg, tg, pts, _ = scene()
    R, t = perturbed(Rg, tg, 1)
    Kr = K + np.array([0, 0, 0.5, 0.5])
    depth = RR.render(verts, faces, None, R.reshape(1, 9), t[None], Kr[None], 96, 96)["depth"][0]
    mm = RF.step(depth, pts, R, t, K, 5000.0, 500000.0 * 0.001 ** 2)
    m = RF.step(depth.astype(np.float64) * 0.001, pts, R, t * 0.001, K, 5000.0, 500000.0)
    assert mm["status"] == 0 and m["status"] == 0 and mm["cost"] == m["cost"] and mm["cost"] > 0
    assert np.array_equal(mm["match"], m["match"])
    c = np.linalg.cond(mm["A"])
    tol = 64 * c * 2.0 ** -52
    assert np.abs(mm["theta"][:3] - m["theta"][:3]).max() <= tol * np.abs(mm["theta"]).max()
    assert np.abs(mm["theta"][3:] * 0.001 - m["theta"][3:]).max() <= tol * np.abs(m["theta"][3:]).max() + 1e-15
    assert np.abs(mm["R"] - m["R"]).max() <= tol
    assert np.abs(mm["t"] * 0.001 - m["t"]).max() <= tol * np.abs(m["t"]).max()


def test_ten_steps_reduce_cost_and_add():
    verts, faces, K, Rg, tg, pts, _ = scene()
    R0, t0 = perturbed(Rg, tg, 2)
    R, t, status, costs = RF.refine(verts, faces, R0, t0, K, 96, 96, pts)
    assert status == 0 and len(costs) == 10
    assert costs[-1] < costs[0] / 4, costs
    before, after = RF.add_error(verts, R0, t0, Rg, tg), RF.add_error(verts, R, t, Rg, tg)
    assert after < before / 2, (before, after)
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12


def test_short_border_and_no_points_copy_the_pose_through():
    depth = np.zeros((16, 16), np.float32)
    depth[4:8, 4:8] = 500.0  # 12 border pixels
    R, t = RF.rodrigues([1, 2, 3], 0.4), np.array([1.0, 2.0, 500.0])
    s = RF.step(depth, [[5, 5]], R, t, [100, 100, 8, 8], 5000.0, 0.5)
    assert s["status"] == 1 and np.array_equal(s["R"], R) and np.array_equal(s["t"], t) and s["cost"] == 0
    depth[2:12, 2:12] = 500.0
    assert RF.step(depth, np.zeros((0, 2)), R, t, [100, 100, 8, 8], 5000.0, 0.5)["status"] == 1
    assert RF.step(depth, [[5, 5]], R, t, [100, 100, 8, 8], 5000.0, 0.5)["status"] == 0


def border_of(n):
    """A 16 x 16 depth image whose silhouette has exactly n = 19 or 20 border pixels: a 6 x 6 square
    (20: its perimeter), less one corner (19: the corner's diagonal neighbour has no unset 4-neighbour)."""
    d = np.zeros((16, 16), np.float32)
    d[5:11, 4:10] = 500.0
    if n == 19:
        d[5, 4] = 0.0
    return d


def test_min_border_boundary():
    R, t = RF.rodrigues([1, 2, 3], 0.4), np.array([1.0, 2.0, 500.0])
    for n, status in [(19, 1), (20, 0)]:
        d = border_of(n)
        assert len(RF.border_list(d > 0)) == n
        assert RF.step(d, [[5, 5], [12, 3]], R, t, [100, 100, 8, 8], 5000.0, 0.5)["status"] == status


def test_staircase_serpentine_reaches_the_sweep_cap():
    """STAIR_S is the smallest size whose serpentine outlasts the cap; of the two tuned prefixes one
    stops changing in pass cap - 1 (the fill succeeds) and one in pass cap (complete, but reported as
    capped: the device has no pass left in which to see that nothing changes)."""
    S, cap = STAIR_S, 8 * STAIR_S
    assert RF.fill_passes(staircase(S - 1)) <= 8 * (S - 1) and RF.fill_passes(staircase(S)) > cap
    over, last, under = staircase_at_cap()
    assert RF.fill_passes(over) > cap and RF.fill_passes(last) == cap and RF.fill_passes(under) == cap - 1
    assert (last != under).sum() >= 1 and (over != last).sum() >= 1
    R, t = RF.rodrigues([1, 2, 3], 0.4), np.array([1.0, 2.0, 500.0])
    K = [100, 100, S / 2, S / 2]
    for m, status in [(over, 2), (last, 2), (under, 0)]:
        s = RF.step(np.where(m != 0, 500.0, 0.0).astype(np.float32), [[5, 5], [30, 40]], R, t, K, 5000.0, 0.5)
        assert s["status"] == status
        if status == 2:
            assert np.array_equal(s["R"], R) and np.array_equal(s["t"], t) and s["cost"] == 0 and len(s["border"]) == 0
    # in the prefix that succeeds the whole corridor is outside: every wall pixel beside it is border
    b = RF.outer_border(under)
    cells = np.array(staircase_cells(S)[:int((under == 0).sum())])
    assert b[cells[:, 1] + 1, cells[:, 0]].sum() + b[cells[:, 1] - 1, cells[:, 0]].sum() > len(cells) / 2
