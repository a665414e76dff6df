"""Reference and case builder of zp_conv2d_wgrad (include/zp.h), in numpy f64.

ref() restates the contract: for each sub-problem, grid point (n, gy, gx) and tap t, the input pixel
is (gy*sy + ty[t], gx*sx + tx[t]) -- skipped outside IH x IW --, the output pixel (gy*oys + oyo,
gx*oxs + oxo), and dy[n, out pixel, cdy0 + co] * x[n, in pixel, cx0 + ci] is added to
dw[co][ci][ky[t]][kx[t]] ([ci][co][..] with transposed_w), for ci < Cw and ky >= 0 only.

build() fills an L.WgradArgs and the host arrays of one launch.  What the buffers hold besides the
operands is what makes a misread visible:
  * activation channels outside [cx0, cx0 + Cin) of x and outside [cdy0, cdy0 + roundup(Cout, E)) of dy
    (E = 8 bf16, 4 f32: the kernels' 16-byte chunk) hold NaN;
  * the padded channels inside those windows (Cw..Cin of x, Cout..roundup of dy) hold non-zero values
    that must not reach dw;
  * dw lies between two guards of a sentinel value, and so does the workspace, which is exactly
    zp_conv2d_wgrad_ws_bytes() long.

Integer operands (the default) make the comparison exact: x and dy are drawn from +-{1, 2, 3} (one of
them from +-[1, 4095] with `wide`), so every product and every partial sum is an integer below 2^24
(tests/test_wgrad_ref_host.py checks that for each case), exact in f32 in any order, under any split
and on any tile.  No operand is zero, so one dropped, doubled or misplaced term changes the result."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

BF16, F32 = "bf16", "f32"
SENTINEL = -12345.0   # guards around dw and the workspace
GARBAGE = 777.0       # dw before a launch that overwrites it
GUARD = 64            # guard floats on either side


def chunk(dtype):
    return 8 if dtype == BF16 else 4


def roundup(v, m):
    return (v + m - 1) // m * m


def ref(a, x, dys, pix=None):
    """dw (f64, the weight's own layout) of the launch `a` describes, from the host arrays
    x [N][IH][IW][ldx] and dys[sub] [N][OH][OW][lddy].  `pix` (bool [N*GH*GW]) keeps only those grid
    points: the sum a kernel would have made of a definite pixel subset."""
    N, GH, GW, Cin, Cout, Cw = a.N, a.GH, a.GW, a.Cin, a.Cout, a.Cw
    dw = np.zeros((Cw, Cout, a.kh, a.kw) if a.transposed_w else (Cout, Cw, a.kh, a.kw))
    gy, gx = np.meshgrid(np.arange(GH), np.arange(GW), indexing="ij")
    keep = np.ones(N * GH * GW, bool) if pix is None else np.asarray(pix, bool).reshape(N * GH * GW)
    for s in range(a.nsub):
        S, dy = a.sub[s], dys[s]
        oy, ox = gy * S.oys + S.oyo, gx * S.oxs + S.oxo
        assert oy.max() < S.OH and ox.max() < S.OW and dy.shape[1:3] == (S.OH, S.OW)
        D = dy[:, oy, ox, S.cdy0:S.cdy0 + Cout].reshape(N * GH * GW, Cout)
        for t in range(S.ntaps):
            ky, kx = int(S.ky[t]), int(S.kx[t])
            if ky < 0:
                continue
            iy, ix = gy * a.sy + int(S.ty[t]), gx * a.sx + int(S.tx[t])
            ok = (iy >= 0) & (iy < a.IH) & (ix >= 0) & (ix < a.IW)
            X = x[:, np.clip(iy, 0, a.IH - 1), np.clip(ix, 0, a.IW - 1), a.cx0:a.cx0 + Cw].reshape(N * GH * GW, Cw)
            m = np.broadcast_to(ok, (N, GH, GW)).reshape(-1) & keep
            g = D[m].T @ X[m]  # [Cout][Cw]
            if a.transposed_w:
                dw[:, :, ky, kx] += g.T
            else:
                dw[:, :, ky, kx] += g
    return dw


def _to_bf16(v):
    """round to nearest even onto bf16's grid (finite values), kept as f64"""
    u = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def _draw(rng, shape, kind, dtype):
    if kind == "real":
        v = rng.standard_normal(shape)
        return _to_bf16(v) if dtype == BF16 else v.astype(np.float32).astype(np.float64)
    hi = 4096 if kind == "wide" else 4
    return (rng.integers(1, hi, shape) * rng.choice([-1, 1], shape)).astype(np.float64)


@dataclass
class Built:
    a: object                 # L.WgradArgs (pointers set when built for a device)
    dtype: str
    x: np.ndarray             # [N][IH][IW][ldx] f64
    dy: np.ndarray            # [N][OH][OW][lddy] f64 (every sub-problem reads the same buffer)
    dw0: np.ndarray           # dw before the launch (added to when a.accumulate)
    ws_bytes: int
    dev: dict = field(default_factory=dict)   # device tensors: x, dy, dw (guarded), ws (guarded)

    @property
    def dys(self):
        return [self.dy] * self.a.nsub

    @property
    def M(self):
        return self.a.N * self.a.GH * self.a.GW

    @property
    def cols_max(self):
        return max(self.a.sub[s].ntaps for s in range(self.a.nsub)) * self.a.Cin

    @property
    def splits(self):
        """the launch plan's split count, read from the workspace size"""
        per = self.a.nsub * self.a.Cout * self.cols_max * 4
        assert self.ws_bytes > 0 and self.ws_bytes % per == 0, (self.ws_bytes, per)
        return self.ws_bytes // per

    def want(self):
        r = ref(self.a, self.x, self.dys)
        return r + self.dw0 if self.a.accumulate else r

    def bound(self):
        """sum |dy| |x| per element of dw: bounds every partial sum in magnitude"""
        return ref(self.a, np.abs(self.x), [np.abs(self.dy)] * self.a.nsub)

    # ---- device side (torch only here)
    def reset(self):
        """dw and its guards as before a launch"""
        import torch
        host = np.full(2 * GUARD + self.dw0.size, SENTINEL, np.float32)
        host[GUARD:GUARD + self.dw0.size] = self.dw0.reshape(-1)
        self.dev["dw"].copy_(torch.from_numpy(host))

    def launch(self):
        """one zp_conv2d_wgrad -> (return code, dw as f32 in the weight's layout); asserts the guards"""
        import torch
        from zebrapose_amd import _lib as L
        self.reset()
        rc = L.lib.zp_conv2d_wgrad(C.byref(self.a), self.dev["ws"].data_ptr() + 4 * GUARD, L.stream_ptr())
        torch.cuda.synchronize()
        dw, ws = self.dev["dw"].cpu().numpy(), self.dev["ws"].cpu().numpy()
        sent = np.float32(SENTINEL).view(np.uint32)
        for name, buf in (("dw", dw), ("workspace", ws)):
            assert (buf[:GUARD].view(np.uint32) == sent).all(), f"{name}: guard before it overwritten"
            assert (buf[-GUARD:].view(np.uint32) == sent).all(), f"{name}: guard after it overwritten"
        return rc, dw[GUARD:-GUARD].reshape(self.dw0.shape).copy()


def build(dtype, N, IH, IW, plan, Cin, Cw, Cout, *, kh, kw, transposed_w=0, cx0=0, ldx=None, cdy0=0, lddy=None,
          accumulate=0, values="int", wide=None, seed=0, device=None):
    """A filled L.WgradArgs and its host arrays.  `plan`: a geometry.Plan (conv_fwd, convT_fwd or
    convT_dgrad); x is N x IH x IW, dy as large as the plan's output pixels reach.  values: "int"
    (+-{1, 2, 3}; `wide` = "x" or "dy" draws that operand from +-[1, 4095]) or "real" (N(0, 1) on the
    dtype's grid).  With a device the buffers are uploaded and the pointers set."""
    from zebrapose_amd import _lib as L
    E = chunk(dtype)
    ldx = Cin + cx0 if ldx is None else ldx
    cout_r = roundup(Cout, E)
    lddy = cdy0 + cout_r if lddy is None else lddy
    OH = max((plan.GH - 1) * sb.oys + sb.oyo for sb in plan.subs) + 1
    OW = max((plan.GW - 1) * sb.oxs + sb.oxo for sb in plan.subs) + 1
    rng = np.random.default_rng(seed)
    kx_ = "real" if values == "real" else ("wide" if wide == "x" else "int")
    kd_ = "real" if values == "real" else ("wide" if wide == "dy" else "int")
    x = np.full((N, IH, IW, ldx), np.nan)
    x[..., cx0:cx0 + Cin] = _draw(rng, (N, IH, IW, Cin), kx_, dtype)
    dy = np.full((N, OH, OW, lddy), np.nan)
    dy[..., cdy0:cdy0 + cout_r] = _draw(rng, (N, OH, OW, cout_r), kd_, dtype)
    shape = (Cw, Cout, kh, kw) if transposed_w else (Cout, Cw, kh, kw)
    if accumulate:
        dw0 = (rng.integers(1, 100, shape) * rng.choice([-1, 1], shape)).astype(np.float64)
    else:
        dw0 = np.full(shape, GARBAGE)

    a = L.WgradArgs()
    a.dtype = L.ZP_BF16 if dtype == BF16 else L.ZP_F32
    a.ldx, a.cx0, a.IH, a.IW, a.Cin = ldx, cx0, IH, IW, Cin
    a.N, a.GH, a.GW, a.sy, a.sx = N, plan.GH, plan.GW, plan.sy, plan.sy
    a.Cout, a.Cw, a.kh, a.kw, a.transposed_w = Cout, Cw, kh, kw, transposed_w
    a.nsub, a.accumulate = len(plan.subs), accumulate
    for i, sb in enumerate(plan.subs):
        S = a.sub[i]
        S.lddy, S.cdy0, S.OH, S.OW = lddy, cdy0, OH, OW
        S.oys, S.oyo, S.oxs, S.oxo = sb.oys, sb.oyo, sb.oxs, sb.oxo
        S.ntaps = len(sb.taps)
        for t, ((ky, kx), (ty, tx)) in enumerate(zip(sb.taps, sb.offs)):
            S.ky[t], S.kx[t], S.ty[t], S.tx[t] = ky, kx, ty, tx
    b = Built(a, dtype, x, dy, dw0, int(L.lib.zp_conv2d_wgrad_ws_bytes(C.byref(a))))
    if device is not None:
        import torch
        tdt = torch.bfloat16 if dtype == BF16 else torch.float32
        d = b.dev
        d["x"] = torch.from_numpy(x.astype(np.float32)).to(device, tdt)
        d["dy"] = torch.from_numpy(dy.astype(np.float32)).to(device, tdt)
        d["dw"] = torch.empty(2 * GUARD + dw0.size, dtype=torch.float32, device=device)
        # the workspace: NaN inside (a partial the reduce reads but no kernel wrote shows), guards outside
        assert b.ws_bytes % 4 == 0
        ws = torch.full((2 * GUARD + b.ws_bytes // 4,), float("nan"), dtype=torch.float32, device=device)
        ws[:GUARD] = SENTINEL
        ws[-GUARD:] = SENTINEL
        d["ws"] = ws
        a.x = d["x"].data_ptr()
        for i in range(a.nsub):
            a.sub[i].dy = d["dy"].data_ptr()
        a.dw = d["dw"].data_ptr() + 4 * GUARD
    return b


def lean_eligible(a, key3=1):
    """zp_wgrad.hip's wgrad2_eligible, restated: the launches k_wgrad2 (the lean kernel) takes; every
    other bf16 launch runs k_wgrad_lds.  key3: zp_conv_tuning key 3."""
    from zebrapose_amd import _lib as L
    if not key3 or a.dtype != L.ZP_BF16 or a.nsub != 1 or a.sy != a.sx or a.sy not in (1, 2):
        return False
    if a.IH != a.sy * a.GH or a.IW != a.sx * a.GW or a.GW not in (32, 64, 128):
        return False
    if (a.GH * a.GW) % 64 or a.Cin % 64:
        return False
    S = a.sub[0]
    return (S.oys, S.oxs, S.oyo, S.oxo, S.OH, S.OW) == (1, 1, 0, 0, a.GH, a.GW)
