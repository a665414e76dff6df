"""Time zp_pose_error_sym and zp_vsd at BOP sizes (device events around the C calls, inputs resident).

    python tools/bop_bench.py [--reps 20]

MSSD / MSPD: B = 32 poses of a 20 000-point model with S = 314 (one continuous symmetry at
max_sym_disc_step = 0.01), S = 628 and S = 1.  VSD: B = 32 at 480 x 640 with the 10 BOP'19 taus, the
object covering about 6 % of each image (a disc), and every pixel covered as the worst case.
Prints one JSON line per case: median and min milliseconds per call over --reps calls after 3 warm-ups.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zebrapose_amd import _lib as L  # noqa: E402
from zebrapose_amd.metric import BOP19_TAUS, MSPD, MSSD, symmetry_transformations  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    B, n = 32, 20000
    pts = torch.from_numpy(rng.uniform(-60, 60, (n, 3)).astype(np.float32)).to(dev)
    R = torch.from_numpy(np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(2 * B)])).to(dev)
    t = torch.from_numpy(rng.uniform(-50, 50, (2 * B, 3)) + np.array([0, 0, 800.0])).to(dev)
    K = torch.from_numpy(np.tile([600.0, 600.0, 320.0, 240.0], (B, 1))).to(dev)
    out = torch.empty(B, dtype=torch.float64, device=dev)
    cont = {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}
    both = dict(cont, symmetries_discrete=[[1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]])
    for name, syms in (("S314", symmetry_transformations(cont)), ("S628", symmetry_transformations(both)),
                       ("S1", (np.eye(3)[None], np.zeros((1, 3))))):
        sR, st = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in syms)
        S = len(sR)
        for mode, mname in ((MSSD, "mssd"), (MSPD, "mspd")):
            ws = torch.empty(int(L.lib.zp_pose_error_sym_ws_bytes(B, n, S, mode)), dtype=torch.uint8, device=dev)

            def run():
                L.call("zp_pose_error_sym", B, pts.data_ptr(), n, R[:B].data_ptr(), t[:B].data_ptr(), R[B:].data_ptr(),
                       t[B:].data_ptr(), K.data_ptr(), sR.data_ptr(), st.data_ptr(), S, mode, out.data_ptr(),
                       ws.data_ptr(), L.stream_ptr())
            med, mn = timed(run, args.reps)
            print(json.dumps({"case": f"{mname}_B{B}_n{n}_{name}", "ms_median": round(med, 4), "ms_min": round(mn, 4),
                              "point_transforms": B * n * (S + 1)}))

    H, W, ntau = 480, 640, len(BOP19_TAUS)
    yy, xx = np.mgrid[:H, :W]
    for name, mask in (("disc6pct", (yy - 240) ** 2 + (xx - 320) ** 2 < 77 ** 2), ("full", np.ones((H, W), bool))):
        gt = np.where(mask, 800.0, 0.0).astype(np.float32)
        est = np.where(np.roll(mask, 5, 1), 810.0, 0.0).astype(np.float32)
        dg, de = (torch.from_numpy(np.repeat(a[None], B, 0)).to(dev) for a in (gt, est))
        dt = torch.full((B, H, W), 805.0, dtype=torch.float32, device=dev)
        o = torch.empty((B, ntau), dtype=torch.float64, device=dev)
        diam = torch.full((B,), 100.0, dtype=torch.float64, device=dev)
        taus = np.ascontiguousarray(BOP19_TAUS, dtype=np.float64)
        ws = torch.empty(int(L.lib.zp_vsd_ws_bytes(B, H, W, ntau)), dtype=torch.uint8, device=dev)

        def run():
            L.call("zp_vsd", B, de.data_ptr(), dg.data_ptr(), dt.data_ptr(), B, None, H, W, K.data_ptr(), 15.0,
                   taus.ctypes.data_as(L.C.POINTER(L.f64)), ntau, diam.data_ptr(), o.data_ptr(), None, ws.data_ptr(),
                   L.stream_ptr())
        med, mn = timed(run, args.reps)
        print(json.dumps({"case": f"vsd_B{B}_{H}x{W}_tau{ntau}_{name}", "ms_median": round(med, 4),
                          "ms_min": round(mn, 4), "bytes_read_at_most": 3 * 4 * B * H * W}))


if __name__ == "__main__":
    main()
