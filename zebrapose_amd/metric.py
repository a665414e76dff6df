"""Drop-in for reference ``zebrapose/metric.py``: ADD / ADI pose errors
computed on the device (``zp_pose_error``, csrc/zp_metric.hip).

``Calculate_ADD_Error_BOP`` / ``Calculate_ADI_Error_BOP`` keep the reference signatures
(metric.py:8-18: host arrays in, float out); ``pose_errors`` is the batched device form.

The BOP errors (``zp_pose_error_sym`` / ``zp_vsd``, csrc/zp_bop.hip; contracts in include/zp.h):
``pose_errors_sym`` (MSSD / MSPD), ``vsd_errors`` / ``vsd_from_depth`` are the batched device
forms; ``mssd`` / ``mspd`` / ``vsd`` keep the argument order of lib/pysixd/pose_error.py:22-179
(host arrays in, floats out).  VSD is the 'step' cost under 'bop19' visibility, on depth rendered by
``MeshRenderer`` (zp_render), not by OpenGL.  ``symmetry_transformations`` is
misc.get_symmetry_transformations (misc.py:206-254); ``bop_recall`` averages recalls over thresholds.

``add_scores`` / ``auc_posecnn`` are the tail of test.py (:62-82, :465-483, :515-523) that turns
per-sample errors and the model's diameter (``modelinfo.model_diameter``) into the paper's numbers:
the pass rates at 0.1 / 0.05 / 0.02 d and the two AUCs.  They are glue on torch in f64, host or device.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L

ADD, ADI = 0, 1
MSSD, MSPD = 2, 3

# lib/pysixd/scripts/eval_calc_errors.py:37-53 and BOP'19's recall thresholds (fractions of the diameter
# for VSD / MSSD; MSPD's are 5 r .. 50 r px with r = image width / 640)
BOP19_TAUS = np.arange(0.05, 0.51, 0.05)
BOP19_THRESHOLDS = np.arange(0.05, 0.51, 0.05)
BOP19_VSD_DELTA = 15.0


def pose_errors(pts, R_est, t_est, R_gt, t_gt, mode=ADD):
    """pts [n,3] (one model), R [B,3,3], t [B,3] (host or device) -> f64 [B] on the device."""
    dev = torch.device("cuda")
    p = torch.as_tensor(np.asarray(pts) if not torch.is_tensor(pts) else pts, dtype=torch.float32).reshape(-1, 3)
    p = p.to(dev).contiguous()

    def d64(x, shape):
        x = torch.as_tensor(x if torch.is_tensor(x) else np.asarray(x), dtype=torch.float64)
        return x.to(dev).reshape(shape).contiguous()
    Re = d64(R_est, (-1, 9))
    B = Re.shape[0]
    te, Rg, tg = d64(t_est, (B, 3)), d64(R_gt, (B, 9)), d64(t_gt, (B, 3))
    n = p.shape[0]
    out = torch.empty(B, dtype=torch.float64, device=dev)
    ws = torch.empty(int(L.lib.zp_pose_error_ws_bytes(B, n, mode)), dtype=torch.uint8, device=dev)
    L.call("zp_pose_error", B, p.data_ptr(), n, Re.data_ptr(), te.data_ptr(), Rg.data_ptr(), tg.data_ptr(), int(mode),
           out.data_ptr(), ws.data_ptr(), L.stream_ptr())
    return out


def Calculate_ADD_Error_BOP(R_GT, t_GT, R_predict, t_predict, vertices):
    """metric.py:8-12 -> pose_error.add(R_predict, t_predict, R_GT, t_GT, vertices)."""
    return float(pose_errors(vertices, R_predict, t_predict, R_GT, t_GT, ADD)[0].item())


def Calculate_ADI_Error_BOP(R_GT, t_GT, R_predict, t_predict, vertices):
    """metric.py:14-18 -> pose_error.adi(R_predict, t_predict, R_GT, t_GT, vertices)."""
    return float(pose_errors(vertices, R_predict, t_predict, R_GT, t_GT, ADI)[0].item())


# ---- BOP errors: symmetry set, MSSD / MSPD ----------------------------------------------------------

def _axis_angle(angle, axis):
    """Rotation by ``angle`` about ``axis`` (normalised here): cos I + (1 - cos) a a^T + sin [a]x."""
    a = np.asarray(axis, dtype=np.float64).reshape(3)
    a = a / np.linalg.norm(a)
    c, s = np.cos(angle), np.sin(angle)
    cross = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return c * np.eye(3) + (1.0 - c) * np.outer(a, a) + s * cross


def symmetry_transformations(model_info, max_sym_disc_step=0.01):
    """misc.get_symmetry_transformations (misc.py:206-254) for one entry of BOP's models_info.json:
    the identity and the discrete symmetries, each combined with every step of the discretised
    continuous ones (ceil(pi / max_sym_disc_step) steps per turn, the zero turn left out), in the
    reference's order: discrete outermost.  Returns (R f64 [S, 3, 3], t f64 [S, 3]) on the host."""
    disc = [(np.eye(3), np.zeros(3))]
    for sym in model_info.get("symmetries_discrete", []):
        m = np.asarray(sym, dtype=np.float64).reshape(4, 4)
        disc.append((m[:3, :3], m[:3, 3]))
    cont = []
    for sym in model_info.get("symmetries_continuous", []):
        offset = np.asarray(sym["offset"], dtype=np.float64).reshape(3)
        steps = int(np.ceil(np.pi / max_sym_disc_step))
        step = 2.0 * np.pi / steps
        for i in range(1, steps):
            R = _axis_angle(i * step, sym["axis"])
            cont.append((R, -R @ offset + offset))
    if cont:
        both = [(Rc @ Rd, Rc @ td + tc) for Rd, td in disc for Rc, tc in cont]
    else:
        both = disc
    return np.stack([R for R, _ in both]), np.stack([t for _, t in both])


def _sym_arrays(syms):
    """(R [S,3,3], t [S,3]) or the reference's list of {'R', 't'} dicts -> f64 [S, 9], [S, 3]."""
    if isinstance(syms, (list, tuple)) and len(syms) and isinstance(syms[0], dict):
        R = np.stack([np.asarray(s["R"], dtype=np.float64).reshape(3, 3) for s in syms])
        t = np.stack([np.asarray(s["t"], dtype=np.float64).reshape(3) for s in syms])
    else:
        R, t = syms
        R = np.asarray(R.cpu() if torch.is_tensor(R) else R, dtype=np.float64)
        t = np.asarray(t.cpu() if torch.is_tensor(t) else t, dtype=np.float64)
    R, t = R.reshape(-1, 9), t.reshape(-1, 3)
    if len(R) == 0 or len(R) != len(t):
        raise ValueError("syms needs as many rotations as translations, and at least one")
    return R, t


def _dev(x, dtype, shape, dev):
    x = torch.as_tensor(x if torch.is_tensor(x) else np.asarray(x), dtype=dtype)
    return x.to(dev).reshape(shape).contiguous()


def _k4(K, B, dev):
    """One 3 x 3 camera matrix, one (fx, fy, cx, cy) row, or B of either -> f64 [B, 4] on the device."""
    k = torch.as_tensor(K if torch.is_tensor(K) else np.asarray(K), dtype=torch.float64)
    if k.shape[-2:] == (3, 3):
        k = torch.stack([k[..., 0, 0], k[..., 1, 1], k[..., 0, 2], k[..., 1, 2]], dim=-1)
    k = k.reshape(-1, 4)
    if len(k) == 1 and B > 1:
        k = k.expand(B, 4)
    if len(k) != B:
        raise ValueError(f"K has {len(k)} rows for a batch of {B}")
    return k.to(dev).contiguous()


def pose_errors_sym(pts, R_est, t_est, R_gt, t_gt, syms, mode, K=None):
    """MSSD / MSPD over B pose pairs of one model (zp_pose_error_sym).  pts [n,3], R [B,3,3], t [B,3]
    (host or device); ``syms`` from symmetry_transformations or the reference's list of dicts;
    ``K`` (MSPD only) one camera for all or B of them.  Returns f64 [B] on the device."""
    if mode not in (MSSD, MSPD):
        raise ValueError("mode must be MSSD or MSPD")
    dev = torch.device("cuda")
    p = _dev(pts, torch.float32, (-1, 3), dev)
    Re = _dev(R_est, torch.float64, (-1, 9), dev)
    B, n = Re.shape[0], p.shape[0]
    te, Rg, tg = (_dev(x, torch.float64, s, dev) for x, s in ((t_est, (B, 3)), (R_gt, (B, 9)), (t_gt, (B, 3))))
    sR, st = _sym_arrays(syms)
    S = len(sR)
    sym = torch.from_numpy(np.concatenate([sR.ravel(), st.ravel()])).to(dev)
    if mode == MSPD and K is None:
        raise ValueError("MSPD needs K")
    Kd = _k4(K, B, dev) if mode == MSPD else None
    need = int(L.lib.zp_pose_error_sym_ws_bytes(B, n, S, mode))
    if need < 0:
        raise ValueError(f"sizes out of range: B {B}, n {n}, S {S}")
    out = torch.empty(B, dtype=torch.float64, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    L.call("zp_pose_error_sym", B, p.data_ptr(), n, Re.data_ptr(), te.data_ptr(), Rg.data_ptr(), tg.data_ptr(),
           L.ptr(Kd), sym.data_ptr(), sym[9 * S:].data_ptr(), S, int(mode), out.data_ptr(), ws.data_ptr(),
           L.stream_ptr())
    return out


def mssd(R_est, t_est, R_gt, t_gt, pts, syms):
    """pose_error.mssd (pose_error.py:131-153): one pose pair, host arrays in, float out."""
    return float(pose_errors_sym(pts, R_est, t_est, R_gt, t_gt, syms, MSSD)[0].item())


def mspd(R_est, t_est, R_gt, t_gt, K, pts, syms):
    """pose_error.mspd (pose_error.py:156-179): one pose pair, K 3 x 3, host arrays in, float out."""
    return float(pose_errors_sym(pts, R_est, t_est, R_gt, t_gt, syms, MSPD, K=K)[0].item())


# ---- VSD ---------------------------------------------------------------------------------------------

def vsd_from_depth(depth_est, depth_gt, depth_test, K, delta=BOP19_VSD_DELTA, taus=BOP19_TAUS,
                   normalized_by_diameter=True, diameter=None, test_index=None, return_counts=False):
    """VSD's pixel stage (zp_vsd) on depth images that exist already: depth_est / depth_gt f32
    [B, H, W], depth_test f32 [n_test, H, W] (or one [H, W] image for all), host or device, 0 = no
    surface.  ``test_index`` int [B] names each pose's test image (default: image b, or image 0 when
    there is one).  ``diameter`` a scalar or [B], used when ``normalized_by_diameter``.  Returns
    f64 [B, ntau] on the device; with ``return_counts`` also i32 [B, 2 + ntau] = (union, inter, cost_k)."""
    dev = torch.device("cuda")
    de = _dev(depth_est, torch.float32, tuple(np.shape(depth_est)), dev)
    if de.dim() == 2:
        de = de[None]
    B, H, W = de.shape
    dg = _dev(depth_gt, torch.float32, (B, H, W), dev)
    dt = _dev(depth_test, torch.float32, (-1, H, W), dev)
    n_test = dt.shape[0]
    if test_index is None and n_test == 1 and B > 1:
        test_index = np.zeros(B, np.int32)
    ti = None
    if test_index is not None:
        tih = np.asarray(test_index.cpu() if torch.is_tensor(test_index) else test_index).reshape(-1)
        if len(tih) != B or tih.min() < 0 or tih.max() >= n_test:
            raise ValueError("test_index needs one index in [0, n_test) per pose")
        ti = torch.from_numpy(tih.astype(np.int32)).to(dev)
    elif n_test < B:
        raise ValueError(f"{n_test} test images for {B} poses: give test_index")
    tau = np.ascontiguousarray(np.asarray(taus, dtype=np.float64).reshape(-1))
    ntau = len(tau)
    diam = None
    if normalized_by_diameter:
        if diameter is None:
            raise ValueError("normalized_by_diameter needs the diameter")
        d = torch.as_tensor(diameter if torch.is_tensor(diameter) else np.asarray(diameter), dtype=torch.float64)
        diam = d.reshape(-1).expand(B).to(dev).contiguous() if d.numel() == 1 else _dev(d, torch.float64, (B,), dev)
    need = int(L.lib.zp_vsd_ws_bytes(B, H, W, ntau))
    if need < 0:
        raise ValueError(f"sizes out of range: B {B}, {H} x {W}, {ntau} taus")
    Kd = _k4(K, B, dev)
    out = torch.empty((B, ntau), dtype=torch.float64, device=dev)
    counts = torch.empty((B, 2 + ntau), dtype=torch.int32, device=dev) if return_counts else None
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    L.call("zp_vsd", B, de.data_ptr(), dg.data_ptr(), dt.data_ptr(), n_test, L.ptr(ti), H, W, Kd.data_ptr(),
           float(delta), tau.ctypes.data_as(L.C.POINTER(L.f64)), ntau, L.ptr(diam), out.data_ptr(), L.ptr(counts),
           ws.data_ptr(), L.stream_ptr())
    return (out, counts) if return_counts else out


def vsd_errors(renderer, R_est, t_est, R_gt, t_gt, depth_test, K, delta=BOP19_VSD_DELTA, taus=BOP19_TAUS,
               normalized_by_diameter=True, diameter=None, test_index=None, return_counts=False):
    """VSD of B pose pairs of ``renderer``'s mesh (a MeshRenderer): the est and gt depth images are
    rendered in one batch of 2 B at depth_test's size, then vsd_from_depth.  f64 [B, ntau] on the device."""
    Re = np.asarray(R_est.cpu() if torch.is_tensor(R_est) else R_est, dtype=np.float64).reshape(-1, 9)
    B = len(Re)
    Rg, te, tg = (np.asarray(x.cpu() if torch.is_tensor(x) else x, dtype=np.float64).reshape(B, c)
                  for x, c in ((R_gt, 9), (t_est, 3), (t_gt, 3)))
    dev = torch.device("cuda")
    H, W = np.shape(depth_test)[-2:]
    Kd = _k4(K, B, dev)
    Kh = Kd.cpu().numpy()
    depth = renderer.render(np.concatenate([Re, Rg]), np.concatenate([te, tg]), np.concatenate([Kh, Kh]), H, W,
                            outputs=("depth",))["depth"]
    return vsd_from_depth(depth[:B], depth[B:], depth_test, Kd, delta, taus, normalized_by_diameter, diameter,
                          test_index, return_counts)


def vsd(R_est, t_est, R_gt, t_gt, depth_test, K, delta, taus, normalized_by_diameter, diameter, renderer,
        obj_id=None, cost_type="step"):
    """pose_error.vsd (pose_error.py:22-128) for one pose pair: host arrays in, a list of floats out.
    ``renderer`` is a MeshRenderer holding the object (``obj_id`` is accepted and ignored); only the
    'step' cost exists."""
    if cost_type != "step":
        raise NotImplementedError("only the 'step' cost is implemented")
    out = vsd_errors(renderer, R_est, t_est, R_gt, t_gt, depth_test, K, delta, taus, normalized_by_diameter, diameter)
    return [float(v) for v in out[0].cpu().tolist()]


def bop_recall(errors, thresholds):
    """BOP's average recall: the mean over ``thresholds`` of the share of ``errors`` strictly below
    the threshold.  errors [N] (MSSD / MSPD), or VSD's [N, ntau]: then every tau is compared with every
    threshold and the mean runs over both, as BOP's AR_VSD does.  Host or device; returns a float."""
    e = torch.as_tensor(errors, dtype=torch.float64)
    th = torch.as_tensor(np.asarray(thresholds) if not torch.is_tensor(thresholds) else thresholds,
                         dtype=torch.float64).to(e.device)
    return float((e.unsqueeze(-1) < th).to(torch.float64).mean().item())


# ---- the score tail of test.py -------------------------------------------------------------------------

FAILED_ERROR = 10000.0  # test.py:465-469: what a failed PnP or a NaN error counts as (mm)


def _errors64(errors):
    e = torch.as_tensor(errors if torch.is_tensor(errors) else np.asarray(errors))
    return e.to(torch.float64).reshape(-1)


def auc_posecnn(errors_m):
    """compute_auc_posecnn (test.py:62-82) on errors in metres, host or device: the area under the
    accuracy-over-threshold curve up to 0.1 m, times 10.  The errors are sorted ascending; entry k
    (from 1) carries the accuracy k / N, values above 0.1 (and NaN) drop out of the curve but stay in
    N; the curve is made monotone and integrated over the steps between distinct values, from 0 to 0.1,
    each step at the accuracy of the first entry at its upper end.  NaN when nothing is <= 0.1."""
    d, _ = torch.sort(_errors64(errors_m))
    N = d.numel()
    keep = d <= 0.1
    k = int(keep.sum().item())
    if k == 0:
        return float("nan")
    d = d[keep]
    acc = torch.arange(1, k + 1, dtype=torch.float64, device=d.device) / N
    edge = torch.tensor([0.0], dtype=torch.float64, device=d.device)
    rec = torch.cat([edge, d, edge + 0.1])
    pre = torch.cummax(torch.cat([edge, acc, acc[-1:]]), 0).values
    step = rec[1:] - rec[:-1]
    return float((torch.where(step != 0, step * pre[1:], torch.zeros_like(step)).sum() * 10).item())


def add_scores(errors, diameter, success=None, fractions=(0.1, 0.05, 0.02)):
    """The numbers test.py prints from per-sample ADD / ADI errors in millimetres (:465-483, :515-523).
    ``errors`` [N] host or device; ``success`` bool [N] or None (all succeeded): a failed sample and a
    NaN error count as 10000.  Returns a dict of floats: ``pass`` (one rate per fraction, strict
    ``error < diameter * f``), ``auc_steps`` (the mean share of the thresholds 10, 20 .. 100 an error
    is strictly below), ``auc_posecnn`` (of the errors / 1000) and ``mean_error``."""
    e = _errors64(errors)
    if e.numel() == 0:
        raise ValueError("no errors")
    bad = e.isnan()
    if success is not None:
        s = torch.as_tensor(success if torch.is_tensor(success) else np.asarray(success)).reshape(-1)
        if s.numel() != e.numel():
            raise ValueError(f"{s.numel()} success flags for {e.numel()} errors")
        bad = bad | ~s.to(device=e.device, dtype=torch.bool)
    e = torch.where(bad, torch.full_like(e, FAILED_ERROR), e)
    d = float(diameter)
    th = torch.tensor([d * float(f) for f in fractions], dtype=torch.float64, device=e.device)
    rates = (e.unsqueeze(-1) < th).to(torch.float64).mean(0)
    steps = torch.linspace(10, 100, 10, dtype=torch.float64, device=e.device)
    # the counts are exact; the mean of the shares count / 10 is numpy's, as the reference's is (test.py:519):
    # a sum of tenths depends on its order, and this one equals np.mean(AUC_ADX_error) bit for bit
    below = (e.unsqueeze(-1) < steps).sum(-1).to(torch.uint8).cpu().numpy()
    auc_steps = np.mean(below / 10)
    return {"pass": [float(r) for r in rates.cpu().tolist()], "auc_steps": float(auc_steps),
            "auc_posecnn": auc_posecnn(e / 1000.0), "mean_error": float(e.mean().item())}
