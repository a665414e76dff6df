"""zp_pack_weight and zp_pack_weight_multi (csrc/zp_pack.hip), each pinned to tests/pack_ref.py -- the element
map and the stored forms as include/zp.h states them -- and not to one another.

Every case runs through both entries in all five dtypes.  A destination is prefilled with a canary and lies
between guard words; the multi call packs all its jobs in one launch into adjacent destinations of one
buffer.  The whole buffer is compared as uint16 words: the map, the roundings, the zeroed padding rows,
channels and k_pad tail, and nothing written outside.

Value passes:  "random" f32 draws (all below the ZP_F32H2 weight bound; where a case uses a subset of the
taps, an out-of-range value sits at an UNUSED tap and must not raise the range flag); "index" (f32 only)
a unique integer per source element, which pins the map itself; "inside" +-0, a denormal and the largest
weight below 31.984375; "outside" 31.984375, 65504 and 65520, which raise the flag for ZP_F32H2 and for no
other dtype."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import pack_ref as R

pytestmark = pytest.mark.gpu

CANARY, GUARD = 0xCAFE, 16  # words


def _taps(kh, kw, order):
    return [(t // kw, t % kw) for t in order]


KERNELS = {
    "1x1": (1, 1, [0]),
    "3x3": (3, 3, list(range(9))),
    "3x3rev": (3, 3, list(range(8, -1, -1))),
    "3x3sub1": (3, 3, [4]),
    "3x3sub2": (3, 3, [7, 2]),
    "3x3sub4": (3, 3, [4, 0, 8, 5]),
    "3x3sub6": (3, 3, [1, 0, 7, 3, 8, 5]),
    "2x2": (2, 2, [0, 1, 2, 3]),
    "7x7": (7, 7, list(range(49))),
}
CHANS = [(3, 3), (3, 8), (64, 64), (64, 72), (65, 65), (65, 72), (130, 130), (130, 136)]   # (chans, cstride)
ROWS = [(1, 1), (1, 8), (8, 8), (17, 20), (17, 24), (70, 70), (70, 128)]                   # (rows, rows_pad)
TAILS = ["0", "8", "wide"]                                                                 # k_pad - ntaps * cstride


def _cases():
    out, i = {}, 0
    for name, (kh, kw, order) in KERNELS.items():
        for tr in (0, 1):
            chans, cstride = CHANS[i % len(CHANS)]
            rows, rows_pad = ROWS[i % len(ROWS)]
            tail = TAILS[i % len(TAILS)]
            if name == "7x7":  # kept small: the stem's own shape, and one across a 64-channel tile
                (chans, cstride), (rows, rows_pad), tail = [((3, 3), (17, 20), "wide"), ((65, 72), (8, 8), "8")][tr]
            k_pad = len(order) * cstride + {"0": 0, "8": 8, "wide": cstride + 5}[tail]
            out[f"{name}-t{tr}-c{chans}s{cstride}-r{rows}p{rows_pad}-k{k_pad}"] = dict(
                kh=kh, kw=kw, taps=_taps(kh, kw, order), tr=tr, chans=chans, cstride=cstride, rows=rows,
                rows_pad=rows_pad, k_pad=k_pad, seed=i)
            i += 1
    return out


CASES = _cases()
PASSES = ["random", "index", "inside", "outside"]
DTYPES = list(R.DTYPES)


@functools.lru_cache(maxsize=None)
def source(case, vpass):
    c = CASES[case]
    d0, d1 = (c["chans"], c["rows"]) if c["tr"] else (c["rows"], c["chans"])
    shape = (d0, d1, c["kh"], c["kw"])
    rng = np.random.default_rng(c["seed"])
    n = int(np.prod(shape))
    if vpass == "index":
        return (np.arange(n, dtype=np.float32) + 1).reshape(shape)
    src = rng.standard_normal(shape).astype(np.float32)
    used = np.zeros((c["kh"], c["kw"]), bool)
    for ky, kx in c["taps"]:
        used[ky, kx] = True
    if vpass == "random":
        if not used.all():
            ky, kx = np.argwhere(~used)[0]
            src[:, :, ky, kx] = 1000.0  # never packed: must not raise the flag
        return src
    lim = R.H2_WEIGHT_LIMIT
    special = {"inside": [0.0, -0.0, 1e-40, -1e-40, np.nextafter(lim, np.float32(0)), -np.nextafter(lim, np.float32(0))],
               "outside": [lim, -lim, 65504.0, 65520.0, -65520.0]}[vpass]
    ky, kx = c["taps"][-1]
    flat = src[:, :, ky, kx].reshape(-1)  # (a copy)
    pos = rng.permutation(flat.size)[:len(special)]
    flat[pos] = np.array(special, np.float32)[:len(pos)]
    src[:, :, ky, kx] = flat.reshape(src.shape[:2])
    return src


@functools.lru_cache(maxsize=None)
def packed(case, vpass):
    c = CASES[case]
    m = R.pack(source(case, vpass), c["tr"], c["taps"], c["cstride"], c["rows_pad"], c["k_pad"])
    m.setflags(write=False)
    return m


def words(case, vpass, dt):
    return np.ascontiguousarray(R.store(packed(case, vpass), R.DTYPES[dt])).reshape(-1).view(np.uint16)


class Layout:
    """destinations side by side in one buffer of 16-bit words, GUARD canary words around each, starts
    16-byte aligned"""

    def __init__(self, jobs):
        self.jobs, self.start, pos = jobs, [], 0
        for j in jobs:
            pos = (pos + GUARD + 7) // 8 * 8
            self.start.append(pos)
            pos += words(*j).size
        self.total = pos + GUARD
        self.want = np.full(self.total, CANARY, np.uint16)
        for j, s in zip(jobs, self.start):
            w = words(*j)
            self.want[s:s + w.size] = w

    def check(self, got, what):
        bad = np.flatnonzero(got != self.want)
        if bad.size:
            k = int(np.searchsorted(self.start, bad[0], side="right")) - 1
            raise AssertionError((what, f"{bad.size} words differ; first in / after job", self.jobs[max(k, 0)],
                                  "word", int(bad[0] - self.start[max(k, 0)]), hex(got[bad[0]]), hex(self.want[bad[0]])))


def _flag_word(L, gpu):
    return L.range_flag(gpu)


def _run_single(L, gpu, case, vpass, dt):
    """one zp_pack_weight -> (the buffer's words, the layout, the flag afterwards)"""
    import torch
    c = CASES[case]
    lay = Layout([(case, vpass, dt)])
    src = torch.from_numpy(source(case, vpass)).to(gpu)
    buf = torch.from_numpy(np.full(lay.total, CANARY, np.uint16).view(np.int16)).to(gpu)
    ky = (C.c_int * len(c["taps"]))(*[t[0] for t in c["taps"]])
    kx = (C.c_int * len(c["taps"]))(*[t[1] for t in c["taps"]])
    d0, d1 = source(case, vpass).shape[:2]
    word = _flag_word(L, gpu)
    saved = word.clone()
    try:
        word.zero_()
        L.call("zp_pack_weight", src.data_ptr(), d0, d1, c["kh"], c["kw"], c["tr"], len(c["taps"]), ky, kx, c["cstride"],
               R.DTYPES[dt], buf.data_ptr() + 2 * lay.start[0], c["rows_pad"], c["k_pad"], L.stream_ptr())
        torch.cuda.synchronize()
        raised = int(word.item())
    finally:
        word.copy_(saved)
    return buf.cpu().numpy().view(np.uint16), lay, raised


def _passes(dt):
    return [p for p in PASSES if p != "index" or dt == "f32"]


@pytest.mark.parametrize("case", list(CASES))
def test_pack_weight(gpu, case):
    from zebrapose_amd import _lib as L
    for dt in DTYPES:
        for vpass in _passes(dt):
            got, lay, raised = _run_single(L, gpu, case, vpass, dt)
            lay.check(got, ("zp_pack_weight", case, vpass, dt))
            assert raised == int(R.raises_flag(packed(case, vpass), R.DTYPES[dt])), ("range flag", case, vpass, dt, raised)
            assert raised == int(dt == "h2" and vpass == "outside")


def _run_multi(L, gpu, jobs):
    import torch
    lay = Layout(jobs)
    buf = torch.from_numpy(np.full(lay.total, CANARY, np.uint16).view(np.int16)).to(gpu)
    keep, table, prefix = {}, (L.PackJob * len(jobs))(), [0]
    for i, (case, vpass, dt) in enumerate(jobs):
        c = CASES[case]
        if (case, vpass) not in keep:
            keep[(case, vpass)] = torch.from_numpy(source(case, vpass)).to(gpu)
        j = table[i]
        j.src, j.dst = keep[(case, vpass)].data_ptr(), buf.data_ptr() + 2 * lay.start[i]
        j.d0, j.d1 = source(case, vpass).shape[:2]
        j.kh, j.kw, j.transposed, j.ntaps = c["kh"], c["kw"], c["tr"], len(c["taps"])
        j.cstride, j.rows_pad, j.k_pad, j.dtype = c["cstride"], c["rows_pad"], c["k_pad"], R.DTYPES[dt]
        for t, (ky, kx) in enumerate(c["taps"]):
            j.ky[t], j.kx[t] = ky, kx
        prefix.append(prefix[-1] + c["rows_pad"] * c["k_pad"])
    raw = np.frombuffer(bytes(table), np.uint8).copy()
    jobs_d = torch.from_numpy(raw).to(gpu)
    prefix_d = torch.tensor(prefix, dtype=torch.int64, device=gpu)
    word = _flag_word(L, gpu)
    saved = word.clone()
    try:
        word.zero_()
        L.call("zp_pack_weight_multi", len(jobs), jobs_d.data_ptr(), prefix_d.data_ptr(), prefix[-1], L.stream_ptr())
        torch.cuda.synchronize()
        raised = int(word.item())
    finally:
        word.copy_(saved)
    return buf.cpu().numpy().view(np.uint16), lay, raised


def test_pack_weight_multi_in_range(gpu):
    """every case, dtype and pass in ONE launch, the out-of-range pass for every dtype but ZP_F32H2: all
    destinations exact, and neither the padding nor another dtype's large weights raise the flag"""
    from zebrapose_amd import _lib as L
    jobs = [(case, vpass, dt) for case in CASES for dt in DTYPES for vpass in _passes(dt)
            if not (dt == "h2" and vpass == "outside")]
    got, lay, raised = _run_multi(L, gpu, jobs)
    lay.check(got, "zp_pack_weight_multi")
    assert raised == 0


def test_pack_weight_multi_out_of_range(gpu):
    """the ZP_F32H2 jobs of the out-of-range pass, one launch each way: exact planes, flag raised; a single
    such job among in-range ones raises it too"""
    from zebrapose_amd import _lib as L
    jobs = [(case, "outside", "h2") for case in CASES]
    got, lay, raised = _run_multi(L, gpu, jobs)
    lay.check(got, "zp_pack_weight_multi outside")
    assert raised == 1
    some = list(CASES)[:6]
    jobs = [(case, "random", dt) for case in some for dt in DTYPES] + [(some[3], "outside", "h2")]
    got, lay, raised = _run_multi(L, gpu, jobs)
    lay.check(got, "zp_pack_weight_multi one outside")
    assert raised == 1
