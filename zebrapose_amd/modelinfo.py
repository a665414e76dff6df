"""Model diameter and ``models_info.json`` entries from a model's points on the device
(``zp_model_info``, csrc/zp_modelinfo.hip).

The reference reads the diameter from the ``models_info.json`` that ships with a BOP dataset
(test.py:136, train_v6.py:118, tools_for_BOP/bop_io.py:31,191); a mesh coded here (``encode_mesh``) has
no such file.  Its own routine, lib/pysixd/misc.py:952-966 ``calc_pts_diameter``, is a Python loop of n
numpy passes over all n (n + 1) / 2 pairs; ``model_diameter`` is that all-pairs maximum on the device,
bit for bit (the contract is in include/zp.h, restated in numpy in tests/modelinfo_ref.py).  The one
square root is taken on the host from the device's exact d2max, so the diameter is ``math.sqrt`` of it.
``model_info`` adds the box (``min_*`` / ``size_*``), ``save_models_info`` writes the file.
"""
from __future__ import annotations

import json
import math

import numpy as np
import torch

from . import _lib as L


def _points_f32(vertices, dev):
    """[n, 3] numpy array or tensor -> f32 [n, 3] contiguous on ``dev``.  An f32 device tensor is used
    in place; anything that is not f32 must survive the round trip through f32 (NaN is left to the
    kernel's status)."""
    v = vertices if torch.is_tensor(vertices) else torch.from_numpy(np.ascontiguousarray(np.asarray(vertices)))
    if v.dim() != 2 or v.shape[1] != 3:
        raise ValueError(f"vertices must be [n, 3], got {tuple(v.shape)}")
    if v.shape[0] == 0:
        raise ValueError("vertices is empty: a model needs at least one point")
    if v.dtype != torch.float32:
        if v.is_complex() or v.dtype == torch.bool:
            raise ValueError(f"vertices of dtype {v.dtype}")
        v = v.to(dev)
        w = v.to(torch.float64)
        v = w.to(torch.float32)
        if not bool(((v.to(torch.float64) == w) | w.isnan()).all().item()):
            raise ValueError("vertices do not survive the round trip through f32: the diameter is defined on f32 "
                             "points (the reference's f64 arrays are copies of f32 files)")
    return v.to(dev).contiguous()


def _run(vertices, device):
    """-> (out: 8 floats, (i, j)); raises ValueError for a bad shape or a non-finite coordinate."""
    dev = vertices.device if torch.is_tensor(vertices) and vertices.is_cuda else torch.device(device)
    with torch.cuda.device(dev):
        p = _points_f32(vertices, dev)
        n = p.shape[0]
        need = int(L.lib.zp_model_info_ws_bytes(n))
        if need < 0:
            raise ValueError(f"{n} points are out of range")
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        res = torch.empty(10, dtype=torch.float64, device=dev)  # out f64 [8] | pair i32 [2] | status i32 [1]
        L.call("zp_model_info", p.data_ptr(), n, res.data_ptr(), res[8:].data_ptr(), res[9:].data_ptr(), ws.data_ptr(),
               L.stream_ptr(dev))
        host = res.cpu().numpy()
    tail = host[8:].view(np.int32)
    if tail[2] != 0:
        raise ValueError("vertices hold a coordinate that is not finite")
    return [float(x) for x in host[:8]], (int(tail[0]), int(tail[1]))


def model_diameter(vertices, return_pair=False, device="cuda"):
    """The largest distance between two of the points, as the reference's ``calc_pts_diameter``
    computes it on the f64 copy of f32 points: sqrt of the largest (dx dx + dy dy) + dz dz.
    ``vertices`` [n, 3], a numpy array or a tensor (a device tensor is used in place); f64 input is
    accepted only if every value is an f32 value.  Returns a float, with ``return_pair`` also the
    lexicographically lowest (i, j), i <= j, that attains it."""
    out, pair = _run(vertices, device)
    d = math.sqrt(out[7])
    return (d, pair) if return_pair else d


def calc_pts_diameter(pts):
    """lib/pysixd/misc.py:952-966, name and signature: nx3 points in, the diameter out."""
    return model_diameter(pts)


def model_info(vertices, device="cuda", symmetries_discrete=None, symmetries_continuous=None):
    """One entry of BOP's models_info.json: ``diameter``, ``min_x/y/z`` and ``size_x/y/z`` as floats.
    ``symmetries_discrete`` / ``symmetries_continuous`` are copied in unchanged when given, so that
    ``metric.symmetry_transformations`` takes the result as it is."""
    out, _ = _run(vertices, device)
    info = {"diameter": math.sqrt(out[7]), "min_x": out[0], "min_y": out[1], "min_z": out[2],
            "size_x": out[3], "size_y": out[4], "size_z": out[5]}
    if symmetries_discrete is not None:
        info["symmetries_discrete"] = symmetries_discrete
    if symmetries_continuous is not None:
        info["symmetries_continuous"] = symmetries_continuous
    return info


def _jsonable(x):
    if isinstance(x, (np.ndarray, np.generic)):
        return x.tolist()
    if torch.is_tensor(x):
        return x.tolist()
    raise TypeError(f"{type(x).__name__} is not JSON serialisable")


def save_models_info(path, infos):
    """Write ``{obj_id: info}`` as models_info.json has it: the top-level keys are ``str(obj_id)``."""
    with open(path, "w") as f:
        json.dump({str(k): v for k, v in infos.items()}, f, indent=2, default=_jsonable)
