"""Reference and case builder of zp_conv2d / zp_conv2d_head (include/zp.h), in numpy f64.

acc() restates zp_conv_sub's contract: for every sub-problem, grid point (n, gy, gx) and tap t the input
pixel is (gy*sy + ty[t], gx*sx + tx[t]) -- zero outside IH x IW --, channel cx0 + c of it is multiplied
by w[co][c][ky[t]][kx[t]] (w[c][co][..] for transposed packing) and summed; Built.want() applies the
epilogue (scale, shift, the residual at cr0 + co, ReLU), rounds once to the stored type and writes the
output pixel (gy*oys + oyo, gx*oxs + oxo) at channel cy0 + co of a copy of y as it was before the launch.

build() fills an L.ConvArgs and the host arrays of one launch.  What the buffers hold besides the
operands is what makes a misread or a stray store visible:
  * channels of x outside [cx0, cx0 + Cin) and of the residual outside [cr0, cr0 + Cout) hold NaN;
  * every device buffer (x, the packed weights, the residual, y, y2, the statistics, ...) lies between
    two guards of GUARD elements of GARBAGE, and y is GARBAGE throughout before a launch: the whole
    guarded buffer must come back as want() says, bit for bit;
  * the weights are an f32 OIHW (IOHW) tensor packed by the device's own zp_pack_weight with the
    plan's taps, into zp_conv_rows_pad rows.

Integer operands make the comparison exact: x and w are drawn from +-{1, 2, 3} ("int3"), +-1 ("pm1"),
{-1, 0, 0, 1} ("half", weights only) or +-[1, 4095] ("wide", one side of an f32 case), scales are
+-{1, 2}, shifts and residuals small integers, so every product and every partial sum in any order is
an integer below 2^24.  A 16-bit store could hide a lost product inside its rounding, so a case either
stores f32 (ZP_OUT_NHWC_F32) or draws operands whose every stored value is below 256 (bf16) / 2048
(fp16) and on the type's grid; tests/test_conv_ref_host.py proves that on the actual draw."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from tests.wgrad_ref import GARBAGE, GUARD, _to_bf16, roundup  # noqa: F401  (roundup: re-exported)

BF16, F16, F32 = "bf16", "f16", "f32"
NHWC, HEAD, NHWC_F32, X3, H2 = 0, 1, 2, 3, 4   # zp_conv_args.out_mode
GARBAGE_WORD = 0x4242                          # a split-plane word before the launch
EXACT_BELOW = {BF16: 256.0, F16: 2048.0}       # integers below it are on the 16-bit grid


def chunk(dtype):
    return 4 if dtype == F32 else 8


def to_store(v, kind):
    """RNE onto the grid of `kind` (finite values), kept as f64"""
    v32 = np.asarray(v, np.float64).astype(np.float32)
    if kind == BF16:
        return _to_bf16(v32)
    if kind == F16:
        return v32.astype(np.float16).astype(np.float64)
    return v32.astype(np.float64)


def _draw(rng, shape, kind, dtype):
    if kind == "real":
        return to_store(rng.standard_normal(shape), dtype)
    if kind == "half":
        return rng.choice([-1.0, 0.0, 0.0, 1.0], shape)
    hi = {"int3": 4, "pm1": 2, "wide": 4096}[kind]
    return (rng.integers(1, hi, shape) * rng.choice([-1, 1], shape)).astype(np.float64)


def tap_matrix(w, transposed, ky, kx, cin):
    """[Cout][cin] matrix of one weight tap (the weight's channels zero-padded to cin)"""
    m = w[:, :, ky, kx].T if transposed else w[:, :, ky, kx]
    out = np.zeros((m.shape[0], cin))
    out[:, :m.shape[1]] = m
    return out


def acc(a, x, subs, s, absolute=False):
    """the exact sums [N][GH][GW][Cout] of sub-problem s.  subs[s] = (w, transposed, taps).
    absolute: sum |w| |x| instead, which bounds every partial sum."""
    N, GH, GW, Cin = a.N, a.GH, a.GW, a.Cin
    S = a.sub[s]
    w, transposed, taps = subs[s]
    assert len(taps) == S.ntaps
    gy, gx = np.meshgrid(np.arange(GH), np.arange(GW), indexing="ij")
    xs = x[..., a.cx0:a.cx0 + Cin]
    out = np.zeros((N * GH * GW, a.Cout))
    for t, (ky, kx) in enumerate(taps):
        iy, ix = gy * a.sy + int(S.ty[t]), gx * a.sx + int(S.tx[t])
        ok = (iy >= 0) & (iy < a.IH) & (ix >= 0) & (ix < a.IW)
        X = xs[:, np.clip(iy, 0, a.IH - 1), np.clip(ix, 0, a.IW - 1)] * ok[None, :, :, None]
        Wm = tap_matrix(w, transposed, ky, kx, Cin)
        if absolute:
            X, Wm = np.abs(X), np.abs(Wm)
        out += X.reshape(N * GH * GW, Cin) @ Wm.T
    return out.reshape(N, GH, GW, a.Cout)


def join_planes(words, mode):
    """f32 values of split planes [NPL][...] of 16-bit words, joined as zp_common.h's join3 /
    SplitF32<2>::join do"""
    words = np.asarray(words, np.uint16)
    if mode == X3:
        p = (words.astype(np.uint32) << 16).view(np.float32)
        return (p[0] + p[1]) + p[2]
    hi, lo = words[0].view(np.float16).astype(np.float64), words[1].view(np.float16).astype(np.float64)
    return (lo * 2.0 ** -11 + hi).astype(np.float32)  # (one rounding: the fma)


@dataclass
class Built:
    a: object                 # L.ConvArgs (pointers set when built for a device)
    dtype: str
    store: str                # the type y holds: dtype, F32 (f32 calls, NHWC_F32, HEAD) or "planes"
    x: np.ndarray             # [N][IH][IW][ldx] f64, NaN outside the slice
    subs: list                # per sub (w f64 in the weight's layout, transposed, taps [(ky, kx)])
    scale: list               # per sub f64 [Cout] or None
    shift: list
    res: np.ndarray           # [N][OH][OW][ldr] f64 (NaN outside the slice) or None
    OH: int
    OW: int
    bnr_x: np.ndarray = None      # [N][OH][OW][Cout]
    bnr_save: np.ndarray = None   # [4][Cout]
    dev: dict = field(default_factory=dict)
    keep: list = field(default_factory=list)

    @property
    def M(self):
        return self.a.N * self.a.GH * self.a.GW

    def acc(self, s, absolute=False):
        return acc(self.a, self.x, self.subs, s, absolute)

    def values(self, s):
        """sub s after the epilogue, before the store's rounding: [N][GH][GW][Cout]"""
        a, S = self.a, self.a.sub[s]
        v = self.acc(s)
        if self.scale[s] is not None:
            v = v * self.scale[s]
        if self.shift[s] is not None:
            v = v + self.shift[s]
        if self.res is not None:
            oy, ox = self.out_pixels(s)
            v = v + self.res[:, oy, ox, a.cr0:a.cr0 + a.Cout]
        return (np.maximum(v, 0.0) if a.relu else v) + 0.0

    def out_pixels(self, s):
        S = self.a.sub[s]
        gy, gx = np.meshgrid(np.arange(self.a.GH), np.arange(self.a.GW), indexing="ij")
        oy, ox = gy * S.oys + S.oyo, gx * S.oxs + S.oxo
        assert oy.max() < self.OH and ox.max() < self.OW
        return oy, ox

    def stored(self, s):
        return to_store(self.values(s), F32 if self.store == "planes" else self.store)

    def y_shape(self):
        a = self.a
        if a.out_mode == HEAD:
            return (a.N, 1, self.OH, self.OW)
        return (a.N, self.OH, self.OW, a.sub[0].ldy)

    def want(self):
        """y (and y2) after the launch as f64 -- GARBAGE on the store's grid where nothing is written.
        Split outputs: (values [N][OH][OW][ldy], written mask)."""
        a = self.a
        g = float(to_store(GARBAGE, F32 if self.store == "planes" else self.store))
        y = np.full(self.y_shape(), g)
        if a.out_mode == HEAD:
            v = self.stored(0).transpose(0, 3, 1, 2)
            assert (self.OH, self.OW) == (a.GH, a.GW)
            return v[:, :1].copy(), v[:, 1:].copy()
        written = np.zeros(y.shape, bool)
        for s in range(a.nsub):
            oy, ox = self.out_pixels(s)
            c0 = a.sub[s].cy0
            y[:, oy, ox, c0:c0 + a.Cout] = self.stored(s)
            written[:, oy, ox, c0:c0 + a.Cout] = True
        return (y, written) if self.store == "planes" else y

    # ---- statistics and the fused BN backward reduce: what one part holds
    def part_pixels(self, tp):
        """pixel ranges [lo, hi) of the grid's tiles of tp pixels"""
        return [(lo, min(lo + tp, self.M)) for lo in range(0, self.M, tp)]

    def bnr_terms(self, s):
        """(g, g * xhat) per output element of sub s, [M][Cout] (zp.h bnr_*)"""
        a = self.a
        oy, ox = self.out_pixels(s)
        g = self.stored(s).reshape(self.M, a.Cout)
        xr = self.bnr_x[:, oy, ox].reshape(self.M, a.Cout)
        mean, inv, sc, sh = self.bnr_save
        g = np.where(xr * sc + sh > 0, g, 0.0)
        return g, g * (xr - mean) * inv

    # ---- device side (torch only here)
    def guarded(self, name, host, tdt=None):
        """upload a host array between two guards; the pointer of its first element"""
        import torch
        tdt = tdt or torch.float32
        flat = torch.from_numpy(np.ascontiguousarray(host).reshape(-1))
        if flat.dtype == torch.float64:
            flat = flat.to(torch.float32)
        buf = torch.full((2 * GUARD + flat.numel(),), GARBAGE_WORD if tdt == torch.int16 else GARBAGE, dtype=tdt)
        buf[GUARD:GUARD + flat.numel()] = flat.to(tdt)
        self.dev[name] = buf.to(self.dev["device"])
        self.dev[name + "@"] = buf
        return self.dev[name].data_ptr() + GUARD * buf.element_size()

    def reset(self, name):
        self.dev[name].copy_(self.dev[name + "@"])

    def read(self, name, shape=None):
        """(buffer as numpy in its own dtype, without the guards; True when the guards are intact)"""
        import torch
        got, was = self.dev[name].cpu(), self.dev[name + "@"]
        v = (lambda t: t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t.view(torch.int32))
        ok = bool((v(got[:GUARD]) == v(was[:GUARD])).all() and (v(got[-GUARD:]) == v(was[-GUARD:])).all())
        body = got[GUARD:-GUARD]
        body = body.numpy() if body.dtype in (torch.float32, torch.int16) else body.to(torch.float32).numpy()
        return (body if shape is None else body.reshape(shape)), ok

    def inputs_intact(self):
        """no input buffer (x, weights, residual, ...) and no guard of one changed"""
        import torch
        for name in self.dev:
            if name.endswith("@") or name == "device" or name in self.outputs:
                continue
            got, was = self.dev[name].cpu(), self.dev[name + "@"]
            bits = torch.int16 if got.element_size() == 2 else torch.int32
            if not bool((got.view(bits) == was.view(bits)).all()):
                return False
        return True

    outputs = ("y", "y2", "stats", "bnr_part", "mask", "code", "ws")

    def launch(self, head=None):
        """one zp_conv2d (zp_conv2d_head with head = its L.HeadArgs) on buffers as before a launch -> rc"""
        import torch
        from zebrapose_amd import _lib as L
        for name in self.outputs:
            if name in self.dev:
                self.reset(name)
        if head is not None:
            rc = L.lib.zp_conv2d_head(C.byref(self.a), C.byref(head), L.stream_ptr())
        else:
            rc = L.lib.zp_conv2d(C.byref(self.a), L.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def config(self):
        """(variant, tc, tp, stages) of zp_conv2d_config"""
        from zebrapose_amd import _lib as L
        tc, tp, st, var = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        assert L.lib.zp_conv2d_config(C.byref(self.a), C.byref(tc), C.byref(tp), C.byref(st), C.byref(var)) == 0
        return var.value, tc.value, tp.value, st.value


def torch_dtype(kind):
    import torch
    return {BF16: torch.bfloat16, F16: torch.float16, F32: torch.float32, "planes": torch.int16}[kind]


def build(dtype, N, IH, IW, plan, Cin, Cout, *, weights, cx0=0, ldx=None, cy0=0, ldy=None, out_hw=None,
          res=False, cr0=0, ldr=None, relu=0, scale=False, shift=False, out_mode=NHWC, stats=False, bnr=False,
          small=None, k_pad=None, xdraw="int3", wdraw="int3", seed=0, device=None):
    """A filled L.ConvArgs and its host arrays.  `plan`: a geometry.Plan.  weights: per sub
    (index of the weight tensor, its shape, transposed) -- subs that share an index share one tensor
    (the ConvT phases, the data-gradient phases).  cy0: one offset or one per sub.  small: (kw, dil,
    pad), the arithmetic taps of the small-Cin form.  With a device the buffers are uploaded, the
    weights packed by zp_pack_weight, and the pointers set."""
    from zebrapose_amd import _lib as L
    E = chunk(dtype)
    KE = 8 * E
    nsub = len(plan.subs)
    ldx = Cin + cx0 if ldx is None else ldx
    cy0s = [cy0] * nsub if isinstance(cy0, int) else list(cy0)
    ldy = max(cy0s) + Cout if ldy is None else ldy
    ldr = cr0 + Cout if ldr is None else ldr
    OH = max((plan.GH - 1) * sb.oys + sb.oyo for sb in plan.subs) + 1
    OW = max((plan.GW - 1) * sb.oxs + sb.oxo for sb in plan.subs) + 1
    if out_hw:
        assert out_hw[0] >= OH and out_hw[1] >= OW
        OH, OW = out_hw
    rng = np.random.default_rng(seed)
    x = np.full((N, IH, IW, ldx), np.nan)
    x[..., cx0:cx0 + Cin] = _draw(rng, (N, IH, IW, Cin), xdraw, dtype)
    tensors = {}
    for idx, shape, _ in weights:
        if idx not in tensors:
            tensors[idx] = _draw(rng, shape, wdraw, dtype)
    subs = [(tensors[idx], tr, list(sb.taps)) for (idx, _, tr), sb in zip(weights, plan.subs)]
    sign = lambda n: rng.choice([-1.0, 1.0], n)  # noqa: E731
    scales = [rng.choice([1.0, 2.0], Cout) * sign(Cout) if scale else None for _ in range(nsub)]
    shifts = [rng.integers(-8, 9, Cout).astype(np.float64) if shift else None for _ in range(nsub)]
    resv = None
    if res:
        resv = np.full((N, OH, OW, ldr), np.nan)
        resv[..., cr0:cr0 + Cout] = _draw(rng, (N, OH, OW, Cout), "real" if xdraw == "real" else "int3", dtype)
    kp = max(roundup(len(sb.taps) * Cin, KE) for sb in plan.subs)
    k_pad = kp if k_pad is None else k_pad
    store = F32 if (dtype == F32 or out_mode in (HEAD, NHWC_F32)) else dtype
    if out_mode in (X3, H2):
        store = "planes"

    a = L.ConvArgs()
    a.dtype = {BF16: L.ZP_BF16, F16: L.ZP_F16, F32: L.ZP_F32}[dtype]
    a.ldx, a.cx0, a.IH, a.IW, a.Cin = ldx, cx0, IH, IW, Cin
    a.N, a.GH, a.GW, a.sy, a.sx = N, plan.GH, plan.GW, plan.sy, plan.sy
    a.Cout, a.k_pad, a.w_rows = Cout, k_pad, int(L.lib.zp_conv_rows_pad(Cout))
    a.ldr, a.cr0 = (ldr, cr0) if res else (0, 0)
    a.relu, a.out_mode, a.nsub = relu, out_mode, nsub
    for i, sb in enumerate(plan.subs):
        S = a.sub[i]
        S.ldy, S.cy0, S.OH, S.OW = (0 if out_mode == HEAD else ldy), cy0s[i], OH, OW
        S.oys, S.oyo, S.oxs, S.oxo = sb.oys, sb.oyo, sb.oxs, sb.oxo
        S.ntaps = len(sb.taps)
        for t, (ty, tx) in enumerate(sb.offs):
            S.ty[t], S.tx[t] = ty, tx
        if small is not None:
            S.kw, S.dil, S.pad = small
    b = Built(a, dtype, store, x, subs, scales, shifts, resv, OH, OW)
    if bnr:
        b.bnr_x = _draw(rng, (N, OH, OW, Cout), "int3", dtype)
        b.bnr_save = np.stack([rng.integers(-2, 3, Cout).astype(np.float64), rng.choice([0.5, 1.0, 2.0], Cout),
                               rng.choice([0.5, 1.0, 2.0], Cout) * sign(Cout),
                               rng.integers(-2, 3, Cout).astype(np.float64)])
    if device is None:
        return b
    import torch
    tdt = torch_dtype(dtype)
    b.dev["device"] = device
    a.x = b.guarded("x", x, tdt)
    packed = {}
    for i, ((idx, shape, tr), sb) in enumerate(zip(weights, plan.subs)):
        key = (idx, tuple(sb.taps))
        if key not in packed:
            src = torch.from_numpy(tensors[idx].astype(np.float32)).to(device)
            b.keep.append(src)
            dst = b.guarded(f"w{i}", np.full(a.w_rows * k_pad, GARBAGE), tdt)
            ky, kx = [t[0] for t in sb.taps], [t[1] for t in sb.taps]
            rc = L.lib.zp_pack_weight(src.data_ptr(), shape[0], shape[1], shape[2], shape[3], tr, len(sb.taps),
                                      (C.c_int * len(ky))(*ky), (C.c_int * len(kx))(*kx), Cin, a.dtype, dst,
                                      a.w_rows, k_pad, L.stream_ptr())
            assert rc == 0, L.lib.zp_last_error()
            torch.cuda.synchronize()
            b.dev[f"w{i}@"] = b.dev[f"w{i}"].cpu()  # as packed: an input from here on
            packed[key] = dst
        a.sub[i].w = packed[key]
        if scales[i] is not None:
            a.sub[i].scale = b.guarded(f"scale{i}", scales[i])
        if shifts[i] is not None:
            a.sub[i].shift = b.guarded(f"shift{i}", shifts[i])
    if res:
        a.res = b.guarded("res", resv, tdt)
    sdt = torch_dtype(store)
    ny = int(np.prod(b.y_shape())) * (1 if store != "planes" else (3 if out_mode == X3 else 2))
    y = b.guarded("y", np.full(ny, GARBAGE_WORD if store == "planes" else GARBAGE,
                               np.int16 if store == "planes" else np.float64), sdt)
    y2 = b.guarded("y2", np.full(max(1, N * (Cout - 1) * OH * OW), GARBAGE), sdt) if out_mode == HEAD else None
    for i in range(nsub):
        a.sub[i].y, a.sub[i].y2 = y, y2
    if stats:
        parts = int(L.lib.zp_conv2d_stat_parts(C.byref(a)))
        a.stats = b.guarded("stats", np.full(3 * parts * Cout, GARBAGE))
    if bnr:
        a.bnr_x = b.guarded("bnr_x", b.bnr_x, tdt)
        a.bnr_save = b.guarded("bnr_save", b.bnr_save)
        parts = int(L.lib.zp_conv2d_bnr_parts(C.byref(a)))
        a.bnr_part = b.guarded("bnr_part", np.full(2 * (parts + 1) * Cout, GARBAGE))
    return b
