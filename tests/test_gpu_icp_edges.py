"""zp_icp and zp_depth_points at their edges, against tests/icp_ref.py on the inputs of
tests/icp_cases.py (whose preconditions tests/test_icp_cases_host.py asserts on the oracle alone).

One fit (max_iterations = 1): neighbours exactly; where the rotation is unique, R within
tests/test_gpu_icp.py's fit_bound(H, S) (the oracle's own conditioning) and t within that bound times
the cloud's radius, thin clouds included.  Where it is not unique (rank 0, rank 1, a reflection) the
result is checked by value:
  |R^T R - I| and |det R - 1| <= 64 max(the oracle's own figure on that input, 2^-52): the device's R
      is a sum of three outer products of vectors that came through up to 40 Jacobi sweeps and a
      Gram-Schmidt step, each a handful of roundings, where LAPACK's comes from two small products;
  the summed squared residual of T over the pairs <= the oracle's (1 + 1e-9) + n (64 2^-53 max|b|)^2: the
      residual is stationary at the best rotation (an error d of R changes it by the order of d^2 times
      the scatter), 1e-9 is the margin every neighbour already has, and the last term is the rounding of
      the transformed points themselves;
  status and iterations equal, nothing NaN.
Invariants are compared bit for bit.  Every launch runs twice and gives the same bits."""
import numpy as np
import pytest

from tests import icp_cases as C
from tests import icp_ref as IR
from tests.test_gpu_icp import MARGIN, _bits, _check_points, _icp, _points, fit_bound, pair
from tests.test_gpu_icp import R0 as G_R0, T0 as G_T0

pytestmark = pytest.mark.gpu

KEYS = ("R", "t", "status", "iterations", "mean_error", "nn", "T")


def launch(gpu, cases, src_counts=None, dst_counts=None, src_cap=None, dst_cap=None, fill=np.nan):
    """zp_icp twice (equal bits) on a batch of cases that share N and kw; rows between a list's end and
    the cap hold `fill`; counts default to the lists' lengths.  As numpy."""
    import torch
    from zebrapose_amd import _lib as L
    B, N, kw = len(cases), cases[0]["N"], cases[0]["kw"]
    assert all(c["N"] == N and c["kw"] == kw for c in cases)
    scap = src_cap or max(1, max(len(c["src"]) for c in cases))
    dcap = dst_cap or max(1, max(len(c["dst"]) for c in cases))

    def pack(key, cap):
        a = np.full((B, cap, 3), fill, np.float64)
        for b, c in enumerate(cases):
            a[b, :min(len(c[key]), cap)] = c[key][:cap]
        return a

    ns = np.array([len(c["src"]) for c in cases] if src_counts is None else src_counts, np.int32)
    nd = np.array([len(c["dst"]) for c in cases] if dst_counts is None else dst_counts, np.int32)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for k, v in dict(
        src=pack("src", scap), dst=pack("dst", dcap), ns=ns, nd=nd, ds=np.stack([c["us"] for c in cases]),
        dd=np.stack([c["ud"] for c in cases]), R=np.stack([c["R"].reshape(9) for c in cases]),
        t=np.stack([c["t"] for c in cases])).items()}
    assert d["ds"].shape == (B, N) and d["dd"].shape == (B, N) and L.lib.zp_icp_ws_bytes(B, N) == 0
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
               dcap, d["ds"].data_ptr(), d["dd"].data_ptr(), int(kw.get("max_iterations", 200)),
               float(kw.get("tolerance", 5e-7)), int(kw.get("mode", 0)), float(kw.get("min_fraction", IR.MIN_FRACTION)),
               float(kw.get("angle_limit", IR.ANGLE_LIMIT)), d["R"].data_ptr(), d["t"].data_ptr(), o["R"].data_ptr(),
               o["t"].data_ptr(), o["status"].data_ptr(), o["iterations"].data_ptr(), o["mean_error"].data_ptr(),
               o["nn"].data_ptr(), o["T"].data_ptr(), None, L.stream_ptr())
        torch.cuda.synchronize()
        runs.append({k: v.cpu().numpy() for k, v in o.items()})
    for k in KEYS:
        assert np.array_equal(_bits(runs[0][k]), _bits(runs[1][k])), k
    return runs[0]


def same_bits(a, i, b, j, what):
    for k in KEYS:
        assert np.array_equal(_bits(a[k][i]), _bits(b[k][j])), (what, k, a[k][i], b[k][j])


def check_exact(got, b, w, N):
    """status, iterations and the neighbour list of pose b against the oracle's"""
    assert got["status"][b] == w["status"] and got["iterations"][b] == w["iterations"], (
        got["status"][b], w["status"], got["iterations"][b], w["iterations"])
    n = len(w["nn"])
    assert np.array_equal(got["nn"][b, :n], w["nn"]) and (got["nn"][b, n:] == -1).all()
    assert got["nn"].shape[1] == N


def check_fit(name, got, w):
    """the unique fit of pose 0 within the oracle's conditioning bound; returns the printed figures"""
    _, _, _, Hf, Sf = IR.best_fit_transform(w["A"], w["A"] @ w["T"][:3, :3].T + w["T"][:3, 3])
    bound = min(fit_bound(w["H"], w["S"]), fit_bound(Hf, Sf))
    T = got["T"][0].reshape(4, 4)
    assert np.array_equal(T[3], [0, 0, 0, 1])
    radius = np.linalg.norm(w["A"] - w["A"].mean(0), axis=1).max()
    dR, dt = np.abs(T[:3, :3] - w["T"][:3, :3]).max(), np.abs(T[:3, 3] - w["T"][:3, 3]).max()
    print(f"{name}: s2/s1 {w['S'][1] / w['S'][0]:.2e} s3/s2 {w['S'][2] / w['S'][1]:.2e} |dR| {dR:.3e} (bound {bound:.3e}), "
          f"|dt| {dt:.3e} (bound {bound * radius:.3e})")
    assert dR <= bound, (name, dR, bound)
    assert dt <= bound * radius, (name, dt, bound * radius)
    assert abs(got["mean_error"][0] - w["mean_error"]) <= 1e-12 * w["mean_error"]
    # the pose out is the device's own T applied to the pose in (tests/test_gpu_icp.py::test_one_iteration)
    Re, te = T[:3, :3] @ C.R0, T[:3, :3] @ C.T0 + T[:3, 3]
    eps = 8 * 2.0 ** -53 * max(np.abs(te).max(), 1.0)
    assert np.abs(got["R"][0].reshape(3, 3) - Re).max() <= eps and np.abs(got["t"][0] - te).max() <= eps


def check_by_value(name, got, w):
    """a fit whose rotation is not unique: a rotation, no worse than the oracle's, nothing NaN"""
    for k in KEYS:
        assert not np.isnan(got[k][0].astype(np.float64)).any(), (name, k)
    T, Tw = got["T"][0].reshape(4, 4), w["T"]
    assert np.array_equal(T[3], [0, 0, 0, 1])

    def orth(M):
        return max(np.abs(M.T @ M - np.eye(3)).max(), abs(np.linalg.det(M) - 1.0))

    o_dev, o_ref = orth(T[:3, :3]), orth(Tw[:3, :3])
    src, dst = w["A"], w["B"][w["nn"]]

    def residual(M):
        e = src @ M[:3, :3].T + M[:3, 3] - dst
        return float((e * e).sum())

    r_dev, r_ref = residual(T), residual(Tw)
    floor = len(src) * (64 * 2.0 ** -53 * np.abs(dst).max()) ** 2
    print(f"{name}: orthonormality {o_dev:.2e} (oracle {o_ref:.2e}), residual {r_dev:.6e} (oracle {r_ref:.6e}), "
          f"|dR| {np.abs(T[:3, :3] - Tw[:3, :3]).max():.2e}")
    assert o_dev <= 64 * max(o_ref, 2.0 ** -52), (name, o_dev, o_ref)
    assert r_dev <= r_ref * (1 + 1e-9) + floor, (name, r_dev, r_ref)
    Ro = got["R"][0].reshape(3, 3)
    assert orth(Ro) <= 64 * max(orth(w["R"]), 2.0 ** -52)


@pytest.mark.parametrize("name", sorted(C.fit_cases()))
def test_one_fit_on_conditioned_clouds(gpu, name):
    """full rank, planar, and thin clouds down to s2 / s1 = 1e-6 (DESIGN.md carries the printed table)"""
    c = C.fit_cases()[name][0]
    w = C.run(c)
    got = launch(gpu, [c])
    check_exact(got, 0, w, c["N"])
    check_fit(name, got, w)


@pytest.mark.parametrize("n,N", C.SIZE_PAIRS)
def test_one_fit_sizes(gpu, n, N):
    """n pairs in a launch of N: the nn tail, threads and waves without a point, the template edges"""
    c = C.sized(n, N)
    w = C.run(c)
    assert w["n"] == n
    got = launch(gpu, [c])
    check_exact(got, 0, w, N)
    if n >= 63:
        check_fit(c["name"], got, w)
    else:
        check_by_value(c["name"], got, w)


@pytest.mark.parametrize("name", sorted(C.degenerate_cases()))
def test_one_fit_degenerate_by_value(gpu, name):
    c = C.degenerate_cases()[name][0]
    w = C.run(c)
    got = launch(gpu, [c])
    check_exact(got, 0, w, c["N"])
    check_by_value(name, got, w)


def _base_cases():
    """the poses whose bits must not depend on their surroundings: a whole loop with n < N (short
    lists), a one-fit thin cloud (the polished path) and a pose that ends with status 3"""
    A, _, us, ud = C._loop_pair(12, 100)
    rng = np.random.default_rng(5)
    pad = np.full(28, 0.5)
    Bm = C.moved(A[:100], [0.1, 0.1, 1.0], 5.0, [1.0, 0.5, 0.0])[0] + rng.normal(size=(100, 3)) * 0.3
    loop = C.case("loop", A[:100], Bm[rng.permutation(100)], np.concatenate([us, pad]), np.concatenate([ud, pad]), "",
                  N=128, mode=IR.NO_DEPTH)
    thin = C.fit_cases()["thin_1e-6"][0]
    thin = C.case("thin", thin["src"][:128], thin["dst"], thin["us"][:128], thin["ud"][:128], "", N=128, mode=IR.NO_DEPTH)
    big = C.case("turned", A[:100], C.moved(A[:100], [0, 0, 1], 30.0, [0, 0, 0])[0], loop["us"], loop["us"], "", N=128,
                 mode=IR.NO_DEPTH)
    return [loop, thin, big]


def _filler(b):
    """what stands in the other slots: status-1 and status-2 neighbours and other loops"""
    (s1, d1), (s2, d2) = C.neighbours()
    u = np.full(128, 0.5)
    if b % 3 == 0:
        return C.case("status1", s1, d1, u, u, "", N=128, mode=IR.NO_DEPTH)
    if b % 3 == 1:
        return C.case("status2", s2, d2, u, u, "", N=128, mode=IR.NO_DEPTH)
    A, Bm, us, ud = C._loop_pair(200 + b, 90)
    return C.case("other", A, Bm, np.concatenate([us, u[:38]]), np.concatenate([ud, u[:38]]), "", N=128, mode=IR.NO_DEPTH)


def test_outputs_do_not_depend_on_batch_slot_or_neighbours(gpu):
    bases = _base_cases()
    want = [C.run(c) for c in bases]
    assert [w["status"] for w in want] == [0, 0, 3] and all(min(w["margins"]) >= MARGIN for w in want)
    alone = [launch(gpu, [c]) for c in bases]
    for a, w in zip(alone, want):
        check_exact(a, 0, w, 128)
    for B in (17, 65):
        for k, c in enumerate(bases):
            slots = [0, B // 2, B - 1]
            batch = [_filler(b + k) for b in range(B)]  # k shifts which kind stands next to the pose
            for s in slots:
                batch[s] = c
            got = launch(gpu, batch)
            for s in slots:
                same_bits(got, s, alone[k], 0, (B, k, s))
            for b in range(B):  # the neighbours themselves: status 1 and 2 copy the pose through
                if batch[b]["name"] in ("status1", "status2"):
                    assert got["status"][b] == (1 if batch[b]["name"] == "status1" else 2)
                    assert got["iterations"][b] == 0 and got["mean_error"][b] == 0 and (got["nn"][b] == -1).all()
                    assert np.array_equal(_bits(got["R"][b]), _bits(C.R0.reshape(9))) and np.array_equal(_bits(got["t"][b]), _bits(C.T0))
                    assert np.array_equal(got["T"][b].reshape(4, 4), np.eye(4))


def test_rows_past_the_count_and_count_clamps(gpu):
    """NaN, huge and ordinary values in the rows between count and cap; counts above the cap equal
    counts at the cap; negative counts equal 0"""
    loop, thin, _ = _base_cases()
    for c in (loop, thin):
        ns, nd = len(c["src"]), len(c["dst"])
        ref = launch(gpu, [c])
        for fill in (np.nan, 1e300, -7.0, np.inf):
            same_bits(launch(gpu, [c], src_cap=ns + 37, dst_cap=nd + 11, fill=fill), 0, ref, 0, fill)
        same_bits(launch(gpu, [c], src_counts=[ns + 7], dst_counts=[nd + 100000]), 0, ref, 0, "counts above cap")
        same_bits(launch(gpu, [c], src_counts=[2 ** 31 - 1], dst_counts=[2 ** 31 - 1]), 0, ref, 0, "INT_MAX")
        # a cap below the list: the same as a list cut there
        cut = dict(c, src=c["src"][:ns - 9], dst=c["dst"][:nd - 4])
        same_bits(launch(gpu, [c], src_cap=ns - 9, dst_cap=nd - 4), 0, launch(gpu, [cut]), 0, "cap below the list")
    empty_s = launch(gpu, [loop], src_counts=[0])
    empty_d = launch(gpu, [loop], dst_counts=[0])
    assert empty_s["status"][0] == 1 and empty_d["status"][0] == 2
    for neg in (-1, -5, -2 ** 31):
        same_bits(launch(gpu, [loop], src_counts=[neg]), 0, empty_s, 0, neg)
        same_bits(launch(gpu, [loop], dst_counts=[neg]), 0, empty_d, 0, neg)
    both = launch(gpu, [loop], src_counts=[-3], dst_counts=[-3])
    assert both["status"][0] == 1  # no source points comes first


def _check_loop(gpu, c, w):
    got = launch(gpu, [c])
    check_exact(got, 0, w, c["N"])
    if w["status"] == 0:
        assert np.abs(got["R"][0].reshape(3, 3) - w["R"]).max() <= 1e-6 and np.abs(got["t"][0] - w["t"]).max() <= 1e-6
    else:
        assert np.array_equal(_bits(got["R"][0]), _bits(c["R"].reshape(9))) and np.array_equal(_bits(got["t"][0]), _bits(c["t"]))
    if w["status"] in (0, 3):
        assert abs(got["mean_error"][0] - w["mean_error"]) <= 1e-6
    return got


def test_draw_ends(gpu):
    c = C.draw_ends()
    w = C.run(c)
    got = _check_loop(gpu, c, w)
    assert np.abs(got["T"][0].reshape(4, 4) - w["T"]).max() <= 1e-6


@pytest.mark.parametrize("name", sorted(C.loop_cases()))
def test_loop_exits(gpu, name):
    c, its = C.loop_cases()[name]
    w = C.run(c)
    got = _check_loop(gpu, c, w)
    if its is not None:
        assert got["iterations"][0] == its
    if name == "subset":
        assert got["mean_error"][0] == 0.0


def test_status_boundaries(gpu):
    for c, status in C.fraction_cases():
        w = C.run(c)
        got = _check_loop(gpu, c, w)
        assert got["status"][0] == status, c["name"]
    for c, status in C.angle_cases()[1]:
        w = C.run(c)
        got = _check_loop(gpu, c, w)
        assert got["status"][0] == status, c["name"]
        assert np.abs(got["T"][0].reshape(4, 4) - w["T"]).max() <= 1e-6  # T is written with status 3 too


@pytest.mark.parametrize("name", sorted(C.depth_cases()))
def test_depth_points_special_values_and_shapes(gpu, name):
    d = C.depth_cases()[name]
    if not d["exact"]:
        want = _check_points(gpu, d["depth"], d["K"], d["cap"], d["filt"], d["factor"])
        if d["cap"] is not None:
            assert all(w["count"] > d["cap"] for w in want)
        return
    # a point exactly on the radius: the oracle's margin is 0 by construction, and every value is an
    # integer, so the comparison is exact on both sides
    counts, pts, stats = _points(gpu, d["depth"], d["K"], d["cap"], d["filt"], d["factor"])
    for b in range(len(d["depth"])):
        w = IR.depth_points(d["depth"][b], d["K"][b], d["cap"], d["filt"][b], d["factor"])
        assert counts[b] == w["count"], (counts[b], w["count"])
        assert np.array_equal(_bits(pts[b, :len(w["pts"])]), _bits(w["pts"]))
        assert np.abs(stats[b] - w["stats"]).max() <= 1e-12 * max(np.abs(w["pts"]).max() if len(w["pts"]) else 1.0, 1.0)


ONE_ITERATION_N = [7, 64, 65, 1023, 1025, 3000, 4096]


def test_well_conditioned_fits_keep_their_bits(gpu, golden):
    """The polish of thin clouds leaves every other fit alone: test_one_iteration's inputs and one whole
    loop give the bits recorded from the kernel before the change (tests/golden/icp_bits.npz)."""
    rec = golden("icp_bits.npz")
    for n in ONE_ITERATION_N:
        A, Bm, us, ud = pair(n, n)
        got = _icp(gpu, [A], [Bm], us, ud, G_R0, G_T0, n, max_iterations=1)
        for k in ("R", "t", "T", "mean_error", "nn"):
            assert np.array_equal(_bits(got[k][0]), _bits(rec[f"n{n}_{k}"])), (n, k)
    A, Bm, us, ud = pair(11, 200)
    got = _icp(gpu, [A], [Bm], us, ud, G_R0, G_T0, 200)
    for k in ("R", "t", "T", "mean_error", "iterations"):
        assert np.array_equal(_bits(got[k][0]), _bits(rec[f"loop_{k}"])), k
