"""Synthetic checkpoint of the d-ary code network (BinaryCodeNet_Deeplab(34, L, d != 2)), shared by
tools/capture_nonbinary_fixtures.py and the tests: oracle.ref_cpu.synthetic_state's trunk (every key
but the binary head's) plus the head pair ``net.aspp.conv_1x1_4_mask`` / ``conv_1x1_4_code`` drawn
by the same recipe (He-normal weights, bias ~ N(0, 0.01), generator seeded by (seed, crc32(key)))."""
import zlib
from collections import OrderedDict

import numpy as np
import torch

from oracle import ref_cpu


CODES = ((4, 8), (16, 4), (256, 2))  # (d, L) of config_ablation/exp_lmo_ablation_4_8 / 16_4 / 256_2


def nb_loss_inputs(d, L, B=2, H=12, W=20):
    """Inputs of the 'CE' loss fixtures (nb_loss*.npz hold the reference's outputs for them; the
    d = 256 logits alone would not fit a committed file): f32 logits scaled x 3, an f64 0/1 mask with
    both values present, uniform digits.  240 pixels leave a tail in any 64- or 256-wide block."""
    rng = np.random.default_rng([101, d, L])
    code = (rng.standard_normal((B, L * d, H, W)) * 3).astype(np.float32)
    mask = (rng.random((B, 1, H, W)) < 0.6).astype(np.float64)
    gt = rng.integers(0, d, (B, L, H, W)).astype(np.uint8)
    return code, mask, gt


def nb_synthetic_state(code_length, d, seed=0, bn_buffers=None):
    trunk = ref_cpu.synthetic_state(34, 16, seed, bn_buffers)
    out = OrderedDict((k, v) for k, v in trunk.items() if not k.startswith("net.aspp.conv_1x1_4."))
    for name, cout in (("conv_1x1_4_mask", 1), ("conv_1x1_4_code", code_length * d)):
        for leaf, shape in (("weight", (cout, 320, 1, 1)), ("bias", (cout,))):
            key = f"net.aspp.{name}.{leaf}"
            rng = np.random.default_rng([seed, zlib.crc32(key.encode())])
            a = rng.standard_normal(shape) * (np.sqrt(2.0 / 320) if leaf == "weight" else 0.01)
            out[key] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return out
