"""tests/pack_ref.py checked by hand and against the bounds include/zp.h states (no GPU needed)."""
import numpy as np

from tests import pack_ref as R


def _src():
    # src[a][b][ky][kx] = 1000 a + 100 b + 10 ky + kx: every element names its own index
    a, b, ky, kx = np.meshgrid(np.arange(2), np.arange(2), np.arange(3), np.arange(3), indexing="ij")
    return (1000 * a + 100 * b + 10 * ky + kx).astype(np.float32)


def test_map_by_hand():
    src = _src()
    taps = [(2, 1), (0, 0)]  # not in scan order
    got = R.pack(src, 0, taps, cstride=3, rows_pad=3, k_pad=8)
    want = np.array([[21, 121, 0, 0, 100, 0, 0, 0],          # r = 0: c = 0, 1 of tap (2, 1); pad; tap (0, 0); tail
                     [1021, 1121, 0, 1000, 1100, 0, 0, 0],   # r = 1
                     [0, 0, 0, 0, 0, 0, 0, 0]], np.float32)  # the padding row
    assert np.array_equal(got, want)
    got = R.pack(src, 1, taps, cstride=3, rows_pad=3, k_pad=8)   # dst[r][t * 3 + c] = src[c][r][ky][kx]
    want = np.array([[21, 1021, 0, 0, 1000, 0, 0, 0],
                     [121, 1121, 0, 100, 1100, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0, 0]], np.float32)
    assert np.array_equal(got, want)


def test_identity_and_reversed_taps():
    src = _src()
    ident = [(t // 3, t % 3) for t in range(9)]
    got = R.pack(src, 0, ident, cstride=2, rows_pad=2, k_pad=18)
    assert np.array_equal(got.reshape(2, 9, 2), src.reshape(2, 2, 9).transpose(0, 2, 1))
    rev = ident[::-1]
    got = R.pack(src, 1, rev, cstride=2, rows_pad=2, k_pad=18)
    assert np.array_equal(got.reshape(2, 9, 2), src.reshape(2, 2, 9)[:, :, ::-1].transpose(1, 2, 0))


def test_roundings_by_hand():
    v = np.array([1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, -0.0, 65504.0, 65520.0, 1e-40,
                  np.inf], np.float32)
    #                 tie -> even (down)  tie -> even (up)       above the tie
    assert R.bf16_bits(v).tolist() == [0x3F80, 0x3F80, 0x3F82, 0x3F81, 0x8000, 0x4780, 0x4780, 0x0001, 0x7F80]
    assert R.f16_bits(v[4:]).tolist() == [0x8000, 0x7BFF, 0x7C00, 0x0000, 0x7C00]
    assert R.store(v, R.F32).tolist() == v.view(np.uint32).tolist()
    assert R.store(v, R.X3).shape == (3, 9) and R.store(v, R.H2).shape == (2, 9)


def _values():
    rng = np.random.default_rng(3)
    v = (rng.standard_normal(200000) * np.exp(rng.uniform(-9, 10, 200000))).astype(np.float32)
    return np.concatenate([v, np.array([0.0, -0.0, 1.0, -1.0, 31.984375, 65504.0, 2.0 ** -14, 2.0 ** -24], np.float32)])


def test_x3_joins_back_exactly():
    v = _values()
    w = R.split3(v)
    j = R.join3(w)
    assert np.array_equal(j, v)  # as values: -0 splits to (-0, +0, +0), whose sum is +0
    nz = v != 0
    assert np.array_equal(j[nz].view(np.uint32), v[nz].view(np.uint32))
    s = R.split3(np.array([np.inf, -np.inf, np.nan], np.float32))
    assert s[1].tolist() == [0, 0, 0] and s[2].tolist() == [0, 0, 0] and s[0, :2].tolist() == [0x7F80, 0xFF80]


def test_h2_joins_back_within_its_bounds():
    v = _values()
    v = v[np.abs(v) < 65504.0]
    j = R.join2(R.split2(v)).astype(np.float64)
    err, a = np.abs(j - v.astype(np.float64)), np.abs(v.astype(np.float64))
    # lo' = (v - hi) * 2^11 is at most 2^e for |v| in [2^e, 2^(e + 1)): a normal fp16, rounded to 2^-12 of
    # itself, from e = -13 up; below that lo' is an fp16 denormal, rounded to 2^-25 absolute.  Times 2^-11:
    wide = a >= 2.0 ** -13
    assert wide.sum() > 1000 and (~wide).sum() > 1000
    assert (err[wide] <= 2.0 ** -23 * a[wide]).all()
    assert (err[~wide] <= 2.0 ** -36).all()
    s = R.split2(np.array([65520.0, -1e9, np.inf], np.float32))   # hi overflows: lo is zero
    assert s[0].tolist() == [0x7C00, 0xFC00, 0x7C00] and s[1].tolist() == [0, 0, 0]


def test_h2_weight_range_rule():
    lim = np.float32(31.984375)
    below = np.nextafter(lim, np.float32(0))
    v = np.array([lim, -lim, below, -below, 0.0, np.inf, -np.inf, np.nan, 65504.0], np.float32)
    assert R.h2_weight_out_of_range(v).tolist() == [True, True, False, False, False, False, False, False, True]
    dst = R.pack(np.full((1, 1, 1, 1), lim, np.float32), 0, [(0, 0)], 8, 8, 16)
    assert R.raises_flag(dst, R.H2) and not any(R.raises_flag(dst, d) for d in (R.F32, R.BF16, R.F16, R.X3))
    assert not R.raises_flag(R.pack(np.full((1, 1, 1, 1), below, np.float32), 0, [(0, 0)], 8, 8, 16), R.H2)
