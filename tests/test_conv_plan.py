"""The launch plans of zp_conv2d and zp_conv2d_wgrad, pinned without a GPU: for a fixed list of
synthetic geometries, under every tuning key and environment override the plans honour, what the
host queries answer (zp_conv2d_config, _grid, _stat_parts, _bnr_parts, _head_ok, _split_ws;
zp_conv2d_wgrad_ws_bytes) equals tests/golden/conv_plan_table.json row for row.  The engine sizes
device buffers from these answers, and the launches read the same plan.

The golden table is written by this module from the library of the commit BEFORE a change to the
plan code, never from the code under test:
    ZP_LIB=<that commit's libzp.so> python tests/test_conv_plan.py --write <that commit's hash>
Without a device the library takes 256 compute units, the MI355X's count, so the table is the same
with and without one."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("ZP_QUIET", "1")

from zebrapose_amd import _lib as L  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "conv_plan_table.json")
PTR = 16  # a non-NULL pointer no query dereferences
CHANNELS = [(8, 64), (64, 64), (64, 128), (128, 128), (256, 256), (512, 512), (320, 17), (64, 320), (256, 48),
            (2048, 256)]
SPLIT = (L.ZP_F32X3, L.ZP_F32H2)


def _sub(a, s, taps, OH, OW, oys=1, oyo=0, oxs=1, oxo=0):
    S = a.sub[s]
    S.ntaps, S.ldy, S.OH, S.OW = len(taps), a.Cout, OH, OW
    S.oys, S.oyo, S.oxs, S.oxo = oys, oyo, oxs, oxo
    for t, (ty, tx) in enumerate(taps):
        S.ty[t], S.tx[t] = ty, tx


def _conv_base(dtype, N, H, W, Cin, Cout, maxtaps):
    a = L.ConvArgs()
    a.dtype, a.N, a.IH, a.GH, a.IW, a.GW, a.sy, a.sx = dtype, N, H, H, W, W, 1, 1
    a.Cin, a.ldx, a.Cout, a.k_pad = Cin, Cin, Cout, maxtaps * Cin
    a.w_rows = L.lib.zp_conv_rows_pad(Cout)
    return a


def _square(k, d):
    return [((t // k - k // 2) * d, (t % k - k // 2) * d) for t in range(k * k)]


def conv(dtype, N, H, W, Cin, Cout, k, d):
    """One k x k stride-1 same-size conv (tests/asan/abi_driver.cpp's conv())."""
    a = _conv_base(dtype, N, H, W, Cin, Cout, k * k)
    a.nsub = 1
    _sub(a, 0, _square(k, d), H, W)
    return a


def convt_phases(dtype, N, W, Cin, Cout):
    """The four phases of ConvTranspose2d(3, stride 2, padding 1, output_padding 1): 1 / 2 / 2 / 4 taps."""
    a = _conv_base(dtype, N, W, W, Cin, Cout, 4)
    a.nsub = 4
    for py in range(2):
        for px in range(2):
            taps = [((py + 1 - ky) // 2, (px + 1 - kx) // 2) for ky in range(3) if (ky - py - 1) % 2 == 0
                    for kx in range(3) if (kx - px - 1) % 2 == 0]
            _sub(a, 2 * py + px, taps, 2 * W, 2 * W, 2, py, 2, px)
    return a


def aspp(dtype, N, W, Cin, Cout):
    """A merged ASPP-like launch: a 1x1 and three dilated 3x3 branches (1 + 9 + 9 + 9 taps)."""
    a = _conv_base(dtype, N, W, W, Cin, Cout, 9)
    a.nsub = 4
    _sub(a, 0, [(0, 0)], W, W)
    for s, d in enumerate((6, 12, 18), 1):
        _sub(a, s, _square(3, d), W, W)
    return a


@functools.lru_cache(None)
def conv_geometries():
    base = []
    for dtype in range(5):
        for N in (1, 4, 32):
            for HW in (8, 16, 32, 64, 128):
                for Cin, Cout in CHANNELS:
                    if dtype in SPLIT and Cin % 32:  # (zp_conv2d refuses it)
                        continue
                    for k, d in ((1, 1), (3, 1), (3, 4)):
                        base.append(lambda dtype=dtype, N=N, HW=HW, Cin=Cin, Cout=Cout, k=k, d=d:
                                    conv(dtype, N, HW, HW, Cin, Cout, k, d))
            for W in (32, 64):
                for Cin, Cout in ((64, 64), (256, 256), (320, 256), (512, 128)):
                    base.append(lambda dtype=dtype, N=N, W=W, Cin=Cin, Cout=Cout: convt_phases(dtype, N, W, Cin, Cout))
            base.append(lambda dtype=dtype, N=N: aspp(dtype, N, 32, 512, 256))
    out = []
    for mode in ("plain", "stats", "bnr"):
        for make in base:
            a = make()
            if mode == "stats":
                a.stats = PTR
            elif mode == "bnr":
                if a.dtype not in (L.ZP_F32, L.ZP_BF16) or a.Cout % 4:  # (zp_conv2d refuses it)
                    continue
                a.bnr_part = a.bnr_x = a.bnr_save = PTR
            out.append(a)
    return out


def wgrad(dtype, N, GW, stride, Cin, Cout, k):
    a = L.WgradArgs()
    a.dtype, a.N, a.GH, a.GW, a.sy, a.sx = dtype, N, GW, GW, stride, stride
    a.IH = a.IW = stride * GW
    a.Cin = a.Cw = a.ldx = Cin
    a.Cout, a.kh, a.kw, a.nsub = Cout, k, k, 1
    S = a.sub[0]
    S.ntaps, S.lddy, S.OH, S.OW, S.oys, S.oxs = k * k, Cout, GW, GW, 1, 1
    for t in range(k * k):
        S.ky[t], S.kx[t], S.ty[t], S.tx[t] = t // k, t % k, t // k - k // 2, t % k - k // 2
    return a


def wgrad_phases(dtype, N, W, Cin, Cout):
    """The weight gradient of the same ConvTranspose2d, phase by phase (four sub-problems)."""
    a = wgrad(dtype, N, W, 1, Cin, Cout, 3)
    a.nsub = 4
    for py in range(2):
        for px in range(2):
            S = a.sub[2 * py + px]
            taps = [(ky, kx) for ky in range(3) if (ky - py - 1) % 2 == 0 for kx in range(3) if (kx - px - 1) % 2 == 0]
            S.ntaps, S.lddy, S.OH, S.OW, S.oys, S.oyo, S.oxs, S.oxo = len(taps), Cout, 2 * W, 2 * W, 2, py, 2, px
            for t, (ky, kx) in enumerate(taps):
                S.ky[t], S.kx[t], S.ty[t], S.tx[t] = ky, kx, (py + 1 - ky) // 2, (px + 1 - kx) // 2
    return a


@functools.lru_cache(None)
def wgrad_geometries():
    out = []
    for dtype in (L.ZP_F32, L.ZP_BF16):
        for N in (1, 4, 32):
            for GW in (16, 32, 64, 128):
                for Cout in (64, 128, 256, 320, 512):
                    for Cin in (8, 64, 256):
                        for stride in (1, 2):
                            for k in (1, 3):
                                out.append(wgrad(dtype, N, GW, stride, Cin, Cout, k))
            for W in (32, 64):
                out.append(wgrad_phases(dtype, N, W, 320, 256))
    return out


def conv_row(a):
    tc, tp, st, var = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    p = C.byref(a)
    assert L.lib.zp_conv2d_config(p, C.byref(tc), C.byref(tp), C.byref(st), C.byref(var)) == 0
    return [tc.value, tp.value, st.value, var.value, L.lib.zp_conv2d_grid(p), L.lib.zp_conv2d_stat_parts(p),
            L.lib.zp_conv2d_bnr_parts(p), L.lib.zp_conv2d_head_ok(p), L.lib.zp_conv2d_split_ws(p)]


def wgrad_row(a):
    return [L.lib.zp_conv2d_wgrad_ws_bytes(C.byref(a))]


# name -> (which geometries, zp_conv_tuning (key, value) or None): swept in one process
TUNING = {"default": ("both", None)}
for _key, _vals, _which in ((0, (1, 1024, 1 << 30), "conv"), (1, (-1, 94, 30, 94 + 128), "conv"), (2, (0, 1), "conv"),
                            (3, (0, 1), "wgrad"), (4, (1, 2), "wgrad"), (5, (0, 1), "wgrad"), (6, (1, 256), "conv")):
    for _v in _vals:
        TUNING[f"key{_key}={_v}"] = (_which, (_key, _v))
# name -> (which geometries, environment): read once per process, so each runs in a child process.
# The conv ones are tests/test_gpu_conv_overrides.py's CONFIGS (FORCE256: zp_conv_tuning(0, 1)).
ENV = {
    "tp128": ("conv", {"ZP_CONV_TP": "128"}),
    "tp256": ("conv", {"ZP_CONV_TP": "256"}),
    "no_tc256": ("conv", {"ZP_CONV_TC256": "0"}),
    "no_strip": ("conv", {"ZP_CONV_STRIP": "0"}),
    "force_tc256": ("conv", {"FORCE256": "1"}),
    "force_tc256_tp128": ("conv", {"FORCE256": "1", "ZP_CONV_TP": "128", "ZP_CONV_STRIP": "0"}),
    "wgrad0": ("wgrad", {"ZP_WGRAD": "0"}),
    "wgrad_big0": ("wgrad", {"ZP_WGRAD_BIG": "0"}),
    "wgrad_big2": ("wgrad", {"ZP_WGRAD_BIG": "2"}),
}


def rows_of(which):
    rows = []
    if which in ("conv", "both"):
        rows += [conv_row(a) for a in conv_geometries()]
    if which in ("wgrad", "both"):
        rows += [wgrad_row(a) for a in wgrad_geometries()]
    return rows


def measure():
    """{config name: rows} of the loaded library under every configuration."""
    kids = {name: subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", name], cwd=ROOT,
                                   env=dict(os.environ, **env), stdout=subprocess.PIPE, text=True)
            for name, (_, env) in ENV.items()}
    out = {}
    for name, (which, kv) in TUNING.items():
        old = L.lib.zp_conv_tuning(*kv) if kv else None
        try:
            out[name] = rows_of(which)
        finally:
            if kv:
                L.lib.zp_conv_tuning(kv[0], old)
    for name, p in kids.items():
        stdout, _ = p.communicate(timeout=120)
        assert p.returncode == 0, name
        out[name] = json.loads(stdout.splitlines()[-1])
    return out


def expected(table):
    """{config name: rows} of the table: the default configuration in full, every other one as the
    geometries whose row differs from the default's."""
    rows, base = table["rows"], table["default"]
    nconv = len(conv_geometries())
    out = {"default": [rows[i] for i in base]}
    for name, (which, _) in list(TUNING.items())[1:] + list(ENV.items()):
        idx = list(base[:nconv] if which == "conv" else base[nconv:])
        for g, r in table["changes"][name]:
            idx[g] = r
        out[name] = [rows[i] for i in idx]
    return out


def test_plans_match_the_parent_commits_table():
    with open(TABLE) as f:
        want = expected(json.load(f))
    got = measure()
    assert set(got) == set(want)
    bad = []
    for name, rows in got.items():
        assert len(rows) == len(want[name]), (name, len(rows), len(want[name]))
        bad += [(name, i, r, w) for i, (r, w) in enumerate(zip(rows, want[name])) if r != w]
    assert not bad, f"{len(bad)} rows differ (config, geometry index, got, golden): {bad[:10]}"


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        if os.environ.get("FORCE256") == "1":
            L.lib.zp_conv_tuning(0, 1)
        print(json.dumps(rows_of(ENV[sys.argv[2]][0])))
    elif sys.argv[1] == "--write":
        uniq, nconv = {}, len(conv_geometries())
        got = {name: [uniq.setdefault(tuple(r), len(uniq)) for r in rows] for name, rows in measure().items()}
        base = got.pop("default")
        which = {name: w for name, (w, _) in list(TUNING.items()) + list(ENV.items())}
        changes = {name: [[g, r] for g, (r, b) in
                          enumerate(zip(idx, base[:nconv] if which[name] == "conv" else base[nconv:])) if r != b]
                   for name, idx in got.items()}
        head = {"generated_from": f"libzp.so of commit {sys.argv[2]}",
                "conv_columns": ["tc", "tp", "stages", "variant", "grid", "stat_parts", "bnr_parts", "head_ok",
                                 "split_ws"],
                "wgrad_columns": ["ws_bytes"],
                "layout": "rows: the distinct rows; default[i]: index into rows of geometry i (conv_geometries() then "
                          "wgrad_geometries()); changes[config]: [geometry index in the config's own list, row "
                          "index] where the config differs from default"}
        enc = lambda v: json.dumps(v, separators=(",", ":"))  # noqa: E731
        with open(TABLE, "w") as f:  # one line per field and per configuration
            f.write("{" + ",\n".join(f'"{k}":{enc(v)}' for k, v in head.items()))
            f.write(',\n"rows":' + enc([list(r) for r in uniq]) + ',\n"default":' + enc(base) + ',\n"changes":{\n')
            f.write(",\n".join(f'"{k}":{enc(v)}' for k, v in changes.items()) + "}}\n")
        print(f"{TABLE}: {len(uniq)} distinct rows, {sum(map(len, changes.values()))} changed entries")
