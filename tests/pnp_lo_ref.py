"""Executable definition of zp_pnp_lo (include/zp.h, "PnP local optimisation") in numpy: rounds of
inlier re-selection under the current pose, each followed by Levenberg-Marquardt on the selected
set.  Plain numpy, f64, no GPU.

Per-point quantities follow the header's operation order, one IEEE operation per step, so they are
the device's bit for bit; only the order of the sums over points differs (numpy's pairwise sum here,
a fixed tree on the device).  ``refine`` records what the tests need besides the outputs: every
round's r^2 at selection time and every accept / reject decision (C, C').
"""
import numpy as np

MIN_SET = 6
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-3, 1e-9, 1e6
REL_DECREASE = 1e-10


def kvec(K):
    K = np.asarray(K, np.float64)
    return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])


def project(pw, uv, R, t, kv):
    """-> (X, Y, Z, ex, ey, r2) of every point; pw f64 [n,3], uv f64 [n,2], R [3,3], t [3]"""
    fx, fy, cx, cy = kv
    X = ((R[0, 0] * pw[:, 0] + R[0, 1] * pw[:, 1]) + R[0, 2] * pw[:, 2]) + t[0]
    Y = ((R[1, 0] * pw[:, 0] + R[1, 1] * pw[:, 1]) + R[1, 2] * pw[:, 2]) + t[1]
    Z = ((R[2, 0] * pw[:, 0] + R[2, 1] * pw[:, 1]) + R[2, 2] * pw[:, 2]) + t[2]
    with np.errstate(all="ignore"):
        ex = uv[:, 0] - ((fx * X) / Z + cx)
        ey = uv[:, 1] - ((fy * Y) / Z + cy)
        r2 = ex * ex + ey * ey
    return X, Y, Z, ex, ey, r2


def select(pw, uv, R, t, kv, thr2):
    """-> (mask, r2): Z > 0, r2 finite and r2 <= thr2"""
    _, _, Z, _, _, r2 = project(pw, uv, R, t, kv)
    with np.errstate(invalid="ignore"):
        return (Z > 0) & np.isfinite(r2) & (r2 <= thr2), r2


def truncated_cost(pw, uv, R, t, K, reproj_err=2.0):
    """M(pose) = sum_i min(r2_i, thr^2), a point that fails the inlier test counting thr^2"""
    pw, uv = np.asarray(pw, np.float64), np.asarray(uv, np.float64)
    thr2 = float(reproj_err) * float(reproj_err)
    m, r2 = select(pw, uv, np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3), kvec(K), thr2)
    return float(np.where(m, r2, thr2).sum())


def jacobian_rows(X, Y, Z, kv):
    """J0, J1 [n,6]: the rows of Jp [-[Xc]x | I]"""
    fx, fy = kv[0], kv[1]
    a = fx / Z
    b = fy / Z
    zz = Z * Z
    c = -((fx * X) / zz)
    d = -((fy * Y) / zz)
    J0 = np.stack([c * Y, a * Z - c * X, -(a * Y), a, np.zeros_like(a), c], 1)
    J1 = np.stack([d * Y - b * Z, -(d * X), b * X, np.zeros_like(b), b, d], 1)
    return J0, J1


def normal_equations(pw, uv, R, t, kv, mask):
    """-> (Hb [28]: upper triangle of H by rows, g, C;  absHb [28]: the same sums over the absolute
    values of the products, the scale of the worst-case summation bound)"""
    X, Y, Z, ex, ey, r2 = (v[mask] for v in project(pw, uv, R, t, kv))
    J0, J1 = jacobian_rows(X, Y, Z, kv)
    out, ab = np.zeros(28), np.zeros(28)
    k = 0
    for r in range(6):
        for c in range(r, 6):
            p0, p1 = J0[:, r] * J0[:, c], J1[:, r] * J1[:, c]
            out[k] = (p0 + p1).sum()
            ab[k] = (np.abs(p0) + np.abs(p1)).sum()
            k += 1
    for r in range(6):
        p0, p1 = J0[:, r] * ex, J1[:, r] * ey
        out[21 + r] = (p0 + p1).sum()
        ab[21 + r] = (np.abs(p0) + np.abs(p1)).sum()
    out[27] = r2.sum()
    ab[27] = r2.sum()
    return out, ab


def damped(Hb, lam):
    """A = H + lam diag(H), full 6 x 6"""
    A = np.zeros((6, 6))
    k = 0
    for r in range(6):
        for c in range(r, 6):
            A[r, c] = A[c, r] = Hb[k]
            k += 1
    for r in range(6):
        A[r, r] = A[r, r] + lam * A[r, r]
    return A


def chol_solve(A, g):
    """-> theta or None (a pivot that is not positive and finite)"""
    L = np.zeros((6, 6))
    with np.errstate(all="ignore"):
        for j in range(6):
            s = A[j, j]
            for k in range(j):
                s = s - L[j, k] * L[j, k]
            if not (s > 0 and np.isfinite(s)):
                return None
            l = np.sqrt(s)
            L[j, j] = l
            for i in range(j + 1, 6):
                v = A[i, j]
                for k in range(j):
                    v = v - L[i, k] * L[j, k]
                L[i, j] = v / l
        th = np.zeros(6)
        for i in range(6):
            v = g[i]
            for k in range(i):
                v = v - L[i, k] * th[k]
            th[i] = v / L[i, i]
        for i in range(5, -1, -1):
            v = th[i]
            for k in range(i + 1, 6):
                v = v - L[k, i] * th[k]
            th[i] = v / L[i, i]
    return th


def update(R, t, th):
    """R' = E R, t' = E t + theta_t, E = exp([theta_r]x) (the series below |theta_r| = 1e-8)"""
    wx, wy, wz = th[0], th[1], th[2]
    with np.errstate(all="ignore"):
        a2 = (wx * wx + wy * wy) + wz * wz
        an = np.sqrt(a2)
        if an < 1e-8:
            ca, cc = 1.0 - a2 / 6.0, 0.5 - a2 / 24.0
        else:
            sh = np.sin(0.5 * an)
            ca, cc = np.sin(an) / an, 2.0 * sh * sh / a2
        Kx = np.array([[0, -wz, wy], [wz, 0, -wx], [-wy, wx, 0]])
        E = np.zeros((3, 3))
        for r in range(3):
            for c in range(3):
                k2 = (Kx[r, 0] * Kx[0, c] + Kx[r, 1] * Kx[1, c]) + Kx[r, 2] * Kx[2, c]
                E[r, c] = ((1.0 if r == c else 0.0) + ca * Kx[r, c]) + cc * k2
        Rn, tn = np.zeros((3, 3)), np.zeros(3)
        for r in range(3):
            for c in range(3):
                Rn[r, c] = (E[r, 0] * R[0, c] + E[r, 1] * R[1, c]) + E[r, 2] * R[2, c]
            tn[r] = ((E[r, 0] * t[0] + E[r, 1] * t[1]) + E[r, 2] * t[2]) + th[3 + r]
    return Rn, tn


def trial_cost(pw, uv, R, t, kv, mask):
    """sum of r2 over the set; a point of it with Z <= 0 under the trial pose makes it +inf"""
    _, _, Z, _, _, r2 = (v[mask] for v in project(pw, uv, R, t, kv))
    with np.errstate(invalid="ignore"):
        if not np.all(Z > 0):
            return np.inf
    return float(r2.sum())


def refine(pw, uv, K, R, t, reproj_err=2.0, rounds=4, steps=10, active=True):
    """One crop.  pw [n,3] (f32 values), uv [n,2] integer pixels, K 3x3, R 3x3, t [3].
    -> dict(R, t, inliers, cost, status, trace [rounds,2], Hb [28] or None, absHb, A0 (the first damped
    matrix), theta0, r2_rounds (r2 of all points at each selection), decisions [(C, C')])"""
    pw = np.asarray(pw, np.float32).astype(np.float64).reshape(-1, 3)
    uv = np.asarray(uv).astype(np.float64).reshape(-1, 2)
    kv = kvec(K)
    R0 = np.array(R, np.float64).reshape(3, 3)
    t0 = np.array(t, np.float64).reshape(3)
    n = len(pw)
    thr2 = float(reproj_err) * float(reproj_err)
    trace = np.full((rounds, 2), -1, np.int32)
    out = {"R": R0.copy(), "t": t0.copy(), "inliers": 0, "cost": 0.0, "status": 1, "trace": trace, "Hb": None,
           "absHb": None, "A0": None, "theta0": None, "r2_rounds": [], "decisions": []}
    if not active or n < MIN_SET or not (np.all(np.isfinite(R0)) and np.all(np.isfinite(t0))):
        return out
    Rc, tc = R0.copy(), t0.copy()
    prev = None
    cnt = 0
    for r in range(rounds):
        mask, r2 = select(pw, uv, Rc, tc, kv, thr2)
        cnt = int(mask.sum())
        out["r2_rounds"].append(r2)
        trace[r] = (cnt, 0)
        if cnt < MIN_SET:
            if r == 0:
                out["status"], out["inliers"] = 2, cnt
                return out
            break
        if r > 0 and np.array_equal(mask, prev):
            break
        prev = mask
        lam, its = LAMBDA0, 0
        Hb = None
        while its < steps:
            its += 1
            if Hb is None:
                Hb, ab = normal_equations(pw, uv, Rc, tc, kv, mask)
                if out["Hb"] is None:
                    out["Hb"], out["absHb"] = Hb.copy(), ab
            C = Hb[27]
            A = damped(Hb, lam)
            th = chol_solve(A, Hb[21:27])
            if out["A0"] is None:
                out["A0"], out["theta0"] = A, th
            accept = False
            if th is not None:
                Rn, tn = update(Rc, tc, th)
                Cn = trial_cost(pw, uv, Rn, tn, kv, mask)
                accept = bool(np.isfinite(Cn) and Cn < C)
                out["decisions"].append((C, Cn))
            if accept:
                Rc, tc, Hb = Rn, tn, None
                lam = max(0.1 * lam, LAMBDA_MIN)
                if C - Cn <= REL_DECREASE * C:
                    break
            else:
                lam = 10.0 * lam
                if lam > LAMBDA_MAX:
                    break
        trace[r] = (cnt, its)
    # the set under the final pose
    mask, r2 = select(pw, uv, Rc, tc, kv, thr2)
    out.update(R=Rc, t=tc, inliers=int(mask.sum()), cost=float(r2[mask].sum()), status=0)
    return out
