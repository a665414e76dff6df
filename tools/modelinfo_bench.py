"""Time zp_model_info once at model-sized point counts (device events, points resident).

    python tools/modelinfo_bench.py [--reps 5] [--log2n 16 18]

Uniformly random f32 points in (-100, 100).  Prints one JSON line per size: median and min
milliseconds of the zp_model_info call alone (both kernels, no copy back), the n (n + 1) / 2 pairs it
covers and the pairs per second that makes, and whether the device's own square root (out[6]) had
the bits of the host's math.sqrt(d2max).
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zebrapose_amd import _lib as L  # noqa: E402
from tools.bop_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2n", type=int, nargs="+", default=[16, 18])
    args = ap.parse_args()
    dev = torch.device("cuda")
    for k in args.log2n:
        n = 1 << k
        pts = torch.from_numpy(np.random.default_rng(k).uniform(-100, 100, (n, 3)).astype(np.float32)).to(dev)
        ws = torch.empty(int(L.lib.zp_model_info_ws_bytes(n)), dtype=torch.uint8, device=dev)
        res = torch.empty(10, dtype=torch.float64, device=dev)

        def call():
            L.call("zp_model_info", pts.data_ptr(), n, res.data_ptr(), res[8:].data_ptr(), res[9:].data_ptr(),
                   ws.data_ptr(), L.stream_ptr(dev))

        ms, ms_min = timed(call, args.reps)
        out = res.cpu().numpy()
        pairs = n * (n + 1) // 2
        print(json.dumps({"case": f"model_info_n{n}", "ms_median": round(ms, 3), "ms_min": round(ms_min, 3),
                          "pairs": pairs, "Gpairs_per_s_at_median": round(pairs / 1e6 / ms, 1),
                          "diameter": float(out[6]), "device_sqrt_equals_host": bool(out[6] == math.sqrt(out[7])),
                          "pair": out[8:].view(np.int32)[:2].tolist(), "status": int(out[8:].view(np.int32)[2]),
                          "reps": args.reps}), flush=True)


if __name__ == "__main__":
    main()
