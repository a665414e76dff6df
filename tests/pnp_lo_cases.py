"""Deterministic inputs of the PnP local optimisation, shared by tests/test_pnp_lo_host.py (the
reference alone and the host program) and the device tests.  Plain numpy, no GPU.  The builders of
tests/pnp_cases.py are reused; a scene is ``(pw f32 [n,3], uv int32 [n,2], R, t)`` as there."""
import functools

import numpy as np

from oracle import pnp_ref
from tests import pnp_cases as PC
from tests import pnp_lo_ref as LO

K0 = PC.K0
THR = 2.0

# the noisy scenes of the whole-loop tests: (n, seed).  The seeds are fixed so that every scene
# passes tests/test_pnp_lo_host.py's preconditions; none is left out at run time.
NOISY = ((300, 31), (300, 74), (300, 95), (300, 100), (1500, 110), (1500, 252), (1500, 391), (1500, 511))


def noisy_scene(n, seed, sigma=0.7, outliers=0.3, K=K0):
    """n points of a +-60 mm box; pixels with sigma px of Gaussian noise, truncated to integers as the
    decode does; a share of them moved by up to +-120 px"""
    rng = np.random.default_rng(1000 * n + seed)
    R, t = PC._pose(rng, K=K)
    pw = rng.uniform(-60, 60, (n, 3)).astype(np.float32)
    uv = np.trunc(PC.project(pw, R, t, K)[0] + rng.normal(0, sigma, (n, 2))).astype(np.int32)
    return PC.add_outliers(rng, (pw, uv, R, t), outliers)


@functools.lru_cache(maxsize=None)
def ransac_pose(n, seed):
    """the oracle's RANSAC-EPnP pose of noisy_scene(n, seed): the optimiser's input"""
    pw, uv, _, _ = noisy_scene(n, seed)
    ref = pnp_ref.solve_pnp_ransac(pw, uv.astype(np.float32), K0)
    assert ref["success"]
    return ref["R"], ref["t"], ref["inliers"]


def perturbed(R, t, deg=0.5, mm=2.0, seed=0):
    """the pose turned by `deg` degrees about a seeded axis and moved by `mm` along another"""
    rng = np.random.default_rng(seed)
    ax = rng.normal(0, 1, 3)
    d = rng.normal(0, 1, 3)
    return PC.rodrigues(np.radians(deg) * ax / np.linalg.norm(ax)) @ R, t + mm * d / np.linalg.norm(d)


def edge_cases():
    """one scene per size of pnp_cases.EXACT_SIZES with its own K, 25 % outliers where n >= 63, and the
    start pose: the true one perturbed by 0.5 degrees and 2 mm -> [(scene, K, R0, t0)]"""
    out = []
    for k, (sc, K) in enumerate(PC.exact_cases(per_crop_K=True)):
        n = len(sc[0])
        if n >= 63:
            sc = PC.add_outliers(np.random.default_rng(300 + k), sc, 0.25)
        R0, t0 = perturbed(sc[2], sc[3], seed=k)
        out.append((sc, K, R0, t0))
    return out


def behind_scene():
    """a box around the camera centre's depth plane under the start pose: half the points have
    Xc.z <= 0 there.  The pixels are those of a pose 800 mm further out."""
    rng = np.random.default_rng(4242)
    R, t = PC._pose(rng)
    pw = rng.uniform(-60, 60, (400, 3)).astype(np.float32)
    uv = np.round(PC.project(pw, R, t, K0)[0]).astype(np.int32)
    t0 = np.array([t[0], t[1], 0.0])
    return (pw, uv, R, t), R, t0


def kvecs(Ks):
    return np.ascontiguousarray(np.stack([LO.kvec(K) for K in Ks]))


def margins(ref, thr=THR):
    """-> (sel, dec, last).  sel: the smallest |r2 - thr^2| / thr^2 over every selection.  dec: the
    smallest |C' - C| / C over the accept / reject decisions, except the accepted steps that end an LM
    run (C - C' <= 1e-10 C, inside any band around 0 by construction); last: the (C - C') / C of those."""
    thr2 = thr * thr
    sel = min(float(np.nanmin(np.abs(r2 - thr2))) for r2 in ref["r2_rounds"]) / thr2
    rel = [(c - cn) / c for c, cn in ref["decisions"]]
    last = [d for d in rel if 0 < d <= LO.REL_DECREASE]
    dec = min((abs(d) for d in rel if not 0 < d <= LO.REL_DECREASE), default=np.inf)
    return sel, dec, last


EDGE_THR = 8.0  # px: the 0.5 degree / 2 mm perturbation moves the pixels by ~3, the outliers by up to 120


@functools.lru_cache(maxsize=None)
def noisy_ref(n, seed):
    """-> (ref, tolR, tolt): the reference on noisy_scene(n, seed) from ransac_pose, and 16 x its own
    largest pose difference among three runs, two of them with the points permuted (seeded)"""
    pw, uv, _, _ = noisy_scene(n, seed)
    R, t, _ = ransac_pose(n, seed)
    runs = [LO.refine(pw, uv, K0, R, t)]
    for ps in (1, 2):
        p = np.random.default_rng(ps).permutation(n)
        runs.append(LO.refine(pw[p], uv[p], K0, R, t))
    pairs = ((0, 1), (0, 2), (1, 2))
    dR = max(np.abs(runs[i]["R"] - runs[j]["R"]).max() for i, j in pairs)
    dt = max(np.abs(runs[i]["t"] - runs[j]["t"]).max() for i, j in pairs)
    return runs, 16 * dR, 16 * dt


@functools.lru_cache(maxsize=None)
def edge_refs():
    """the reference's single step (rounds = 1, steps = 1) on edge_cases()"""
    return [LO.refine(sc[0], sc[1], K, R0, t0, reproj_err=EDGE_THR, rounds=1, steps=1)
            for sc, K, R0, t0 in edge_cases()]


def hb_bound(ref, n):
    """n 2^-52 sum |products|: the worst-case bound of summing the 2 n products of an entry in any order"""
    return n * 2.0 ** -52 * ref["absHb"]


def step_tol(ref):
    """64 cond(H + lambda diag H) 2^-52 (tests/test_gpu_refine_edges.py's rule): R absolute, t relative"""
    return 64 * np.linalg.cond(ref["A0"]) * 2.0 ** -52
