"""Unique 2D-3D correspondences on the device (``zp_decode_unique``, ``Decoder(unique=True)`` /
``Decoder.unique``) against the numpy oracle (tests/decode_unique_ref.py) and the reference's own
output (tests/golden/decode_unique.npz).  Every comparison is exact: counts, xy, xyz, mult, ids, and
the f64 means bit for bit.  LUTs come from ``make_lut`` (none is stored)."""
import numpy as np
import pytest
import torch

from tests import decode_unique_ref as ref
from tests import pnp_cases

pytestmark = pytest.mark.gpu

CASES = tuple(ref.cases())


@pytest.fixture(scope="module")
def lut64():
    return ref.make_lut(ref.LUT_CLASSES)


@pytest.fixture(scope="module")
def dec16(lut64):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zebrapose_amd.decode import Decoder
    return Decoder(lut64, device="cuda")


@pytest.fixture(scope="module")
def cases():
    return ref.cases()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(u, b, want, ids=None):
    """crop b of a device result against the oracle's Unique, exactly"""
    n = int(u.counts[b])
    assert n == want.count, (b, n, want.count)
    np.testing.assert_array_equal(u.xy[b, :n].cpu().numpy(), want.xy)
    assert u.xyz[b, :n].cpu().numpy().tobytes() == np.ascontiguousarray(want.xyz, np.float32).tobytes()
    np.testing.assert_array_equal(u.mult[b, :n].cpu().numpy(), want.mult)
    assert u.mean_xy[b, :n].cpu().numpy().tobytes() == np.ascontiguousarray(want.mean).tobytes()
    if ids is not None:
        np.testing.assert_array_equal(u.ids[b].cpu().numpy(), ids)


def _run16(dec, masks, ids, bboxes, size, **kw):
    masks, ids = np.asarray(masks), np.asarray(ids)
    return dec.unique(_dev(ref.mask_to_logits(masks)), _dev(ref.bits_to_logits(ids, 16)), np.asarray(bboxes),
                      bbox_size=size, **kw)


@pytest.mark.parametrize("name", CASES)
def test_cases_match_oracle_and_reference(gpu, golden, dec16, lut64, cases, name):
    """40 x 36 (two tiles, vector path), 37 x 29 (scalar tail), 8 x 8; empty mask, one class, all
    distinct, groups of 3 and 7, the near-integer groups, ids that agree in their low 12 bits"""
    mask, ids, bbox, size = cases[name]
    u = _run16(dec16, mask[None], ids[None], [bbox], size)
    _check(u, 0, ref.unique_crop(mask, ids, ref.coarsen_lut(lut64, 0), bbox, size), ids)
    fx = golden("decode_unique.npz")
    n = int(u.counts[0])
    assert u.mean_xy[0, :n].cpu().numpy().tobytes() == fx[f"{name}_p2d"].tobytes()
    np.testing.assert_array_equal(u.xy[0, :n].cpu().numpy(), fx[f"{name}_orig"])
    np.testing.assert_array_equal(u.xyz[0, :n].cpu().numpy(), fx[f"{name}_p3d"].astype(np.float32))
    # the PnP-shaped call returns the same rows
    c2, xy2, xyz2, ids2 = dec16(_dev(ref.mask_to_logits(mask[None])), _dev(ref.bits_to_logits(ids[None], 16)),
                                np.asarray([bbox]), bbox_size=size, return_ids=True, unique=True)
    assert int(c2[0]) == n and torch.equal(xy2[0, :n], u.xy[0, :n]) and torch.equal(xyz2[0, :n], u.xyz[0, :n])
    assert torch.equal(ids2, u.ids)


def test_all_distinct_equals_the_non_unique_decode(gpu, dec16, cases):
    mask, ids, bbox, size = cases["distinct"]
    m, c = _dev(ref.mask_to_logits(mask[None])), _dev(ref.bits_to_logits(ids[None], 16))
    cu, xyu, xyzu = dec16(m, c, np.asarray([bbox]), bbox_size=size, unique=True)
    cn, xyn, xyzn = dec16(m, c, np.asarray([bbox]), bbox_size=size)
    n = int(cn[0])
    assert int(cu[0]) == n == int(mask.sum())
    assert torch.equal(xyu[0, :n], xyn[0, :n]) and torch.equal(xyzu[0, :n], xyzn[0, :n])


def test_batch_luts_and_nan_rows(gpu, lut64, cases):
    """B = 3: different masks over the same ids (no cross-talk), lut_index selects between two LUTs,
    a NaN LUT row gives (0, 0, 0)"""
    from zebrapose_amd.decode import Decoder
    _, ids, bbox, size = cases["two_tiles"]
    rng = np.random.default_rng(5)
    masks = np.stack([cases["two_tiles"][0], rng.random(ids.shape) < 0.3, rng.random(ids.shape) < 0.95])
    present = np.unique(ids)
    lutB = ref.make_lut(ref.LUT_CLASSES, nan_rows=present[::3]) * np.array([-1.0, 0.5, 2.0])
    dec = Decoder([lut64, lutB], device="cuda")
    bbs = [bbox, (-100, 50, 300, 250), (0, 0, 37, 37)]
    li = [1, 0, 1]
    u = _run16(dec, masks, np.stack([ids] * 3), bbs, size, lut_index=li)
    zero_rows = 0
    for b in range(3):
        want = ref.unique_crop(masks[b], ids, ref.coarsen_lut((lut64, lutB)[li[b]], 0), bbs[b], size)
        _check(u, b, want, ids)
        zero_rows += int((want.xyz == 0).all(1).sum())
    assert zero_rows > 10


def test_ignore_bit(gpu, lut64, cases):
    """ignore_bit=3 on 16-bit logits: the top 13 channels, the coarsened LUT"""
    from zebrapose_amd.decode import Decoder
    dec = Decoder(lut64, device="cuda", ignore_bit=3)
    for name in ("two_tiles", "tail"):
        mask, ids, bbox, size = cases[name]
        u = _run16(dec, mask[None], ids[None], [bbox], size)
        _check(u, 0, ref.unique_crop(mask, ids >> 3, ref.coarsen_lut(lut64, 3), bbox, size), ids >> 3)


@pytest.mark.parametrize("d,fold", [(4, 256), (16, 65536)])
def test_class_base(gpu, cases, d, fold):
    """d-ary codes, 4 steps of d classes"""
    from zebrapose_amd.decode import Decoder
    lut = ref.make_lut(d ** 4, nan_rows=(7,))
    dec = Decoder(lut, device="cuda", class_base=d)
    for name in ("two_tiles", "tail"):
        mask, ids, bbox, size = cases[name]
        ids = ids % fold
        u = dec.unique(_dev(ref.mask_to_logits(mask[None])), _dev(ref.digits_to_logits(ids[None], 4, d)),
                       np.asarray([bbox]), bbox_size=size)
        _check(u, 0, ref.unique_crop(mask, ids, ref.coarsen_lut(lut, 0), bbox, size), ids)


def _block_scene(n_classes):
    """40 x 36 crop of a 5 x 5 pixel box (ratio 1 / 8 exactly): each class fills one 8 x 8 block, so all
    its pixels, and their mean, map to one original pixel; the class's 3D point is that pixel's ray
    cut at a chosen depth under a planted pose: noise-free in both forms."""
    H, W, size, bbox = 40, 36, 40, (300, 200, 5, 5)
    K = np.array([[20.0, 0.0, 302.0], [0.0, 20.0, 202.0], [0.0, 0.0, 1.0]])
    rng = np.random.default_rng(77)
    R, t = pnp_cases._pose(rng)
    blocks = [(0, 0), (3, 4), (1, 2), (2, 0), (0, 3), (3, 1)][:n_classes]
    cls = 1000 + 37 * np.arange(n_classes)
    mask = np.zeros((H, W), bool)
    ids = np.zeros((H, W), np.int64)
    uv = []
    for k, (bx, by) in enumerate(blocks):
        mask[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = True
        ids[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = cls[k]
        uv.append((bbox[0] + bx, bbox[1] + by))
    lut = ref.make_lut(ref.LUT_CLASSES)
    lut[cls] = pnp_cases._from_depth(np.asarray(uv, np.float64), rng.uniform(700, 900, n_classes).round(), R, t, K)
    return mask, ids, bbox, size, lut, K


def test_success_needs_six_unique(gpu):
    """5 classes over 320 pixels: no pose from the unique form, one from the non-unique form; 6 classes:
    a pose (CNN_output_to_pose.py:126 counts the unique correspondences)"""
    from zebrapose_amd.decode import Decoder
    from zebrapose_amd.pnp import PnP
    m5, i5, bbox, size, lut5, K = _block_scene(5)
    m6, i6, _, _, lut6, _ = _block_scene(6)
    np.testing.assert_array_equal(lut5[i5[m5]], lut6[i5[m5]])
    dec = Decoder(lut6, device="cuda")
    m = _dev(ref.mask_to_logits(np.stack([m5, m6])))
    c = _dev(ref.bits_to_logits(np.stack([i5, i6]), 16))
    bb = np.asarray([bbox, bbox])
    counts, xy, xyz = dec(m, c, bb, bbox_size=size, unique=True)
    assert counts.tolist() == [5, 6] and int(m5.sum()) == 320
    _, _, ok, _ = PnP()(counts, xy, xyz, K)
    assert ok.tolist() == [False, True]
    counts, xy, xyz = dec(m, c, bb, bbox_size=size)
    assert counts.tolist() == [320, 384]
    _, _, ok, _ = PnP()(counts, xy, xyz, K)
    assert bool(ok[0])


def test_reproducible_and_default_path_unchanged(gpu, golden, dec16, cases):
    """the same call twice around a different input, one Decoder: bitwise equal; unique=False still
    gives the reference's recorded non-unique decode (tests/golden/decode.npz)"""
    mask, ids, bbox, size = cases["table_stress"]
    first = _run16(dec16, mask[None], ids[None], [bbox], size)
    n = int(first.counts[0])
    other = cases["one_class"]
    _run16(dec16, other[0][None], other[1][None], [other[2]], other[3])
    again = _run16(dec16, mask[None], ids[None], [bbox], size)
    assert int(again.counts[0]) == n
    for a, b in zip(first[1:5], again[1:5]):
        assert torch.equal(a[0, :n], b[0, :n])
    assert torch.equal(first.ids, again.ids)
    from zebrapose_amd.decode import Decoder
    d = golden("decode.npz")
    ml, cl = torch.from_numpy(d["mask_logits"]).cuda(), torch.from_numpy(d["code_logits"]).cuda()
    for ib in (0, 2):
        dec = Decoder(d["lut"], device="cuda", ignore_bit=ib)
        dec.unique(ml, cl, d["bboxes"], bbox_size=128)
        counts, xy, xyz, idsd = dec(ml, cl, d["bboxes"], bbox_size=128, return_ids=True)
        for b, (p2d, p3d) in enumerate(Decoder.to_host(counts, xy, xyz)):
            assert len(p2d) == int(d[f"ib{ib}_b{b}_count"])
            np.testing.assert_array_equal(idsd[b].cpu().numpy(), d[f"ib{ib}_b{b}_ids"])
            np.testing.assert_array_equal(p2d, d[f"ib{ib}_b{b}_p2d"])
            np.testing.assert_array_equal(p3d, d[f"ib{ib}_b{b}_p3d"])


def test_graph_capture(gpu, dec16, lut64, cases):
    """Decoder(unique=True) captured on one stream; two replays with the static inputs overwritten in
    between both match the oracle (the workspace is re-initialised inside the call)"""
    a, b = cases["two_tiles"], cases["table_stress"]
    ma, ca = _dev(ref.mask_to_logits(a[0][None])), _dev(ref.bits_to_logits(a[1][None], 16))
    mb, cb = _dev(ref.mask_to_logits(b[0][None])), _dev(ref.bits_to_logits(b[1][None], 16))
    m, c = ma.clone(), ca.clone()
    bb = torch.tensor([a[2]], dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dec16(m, c, bb, bbox_size=a[3], unique=True)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        counts, xy, xyz = dec16(m, c, bb, bbox_size=a[3], unique=True)
    lut32 = ref.coarsen_lut(lut64, 0)
    for case, (ms, cs) in ((a, (ma, ca)), (b, (mb, cb)), (a, (ma, ca))):
        m.copy_(ms)
        c.copy_(cs)
        g.replay()
        torch.cuda.synchronize()
        want = ref.unique_crop(case[0], case[1], lut32, a[2], a[3])
        n = int(counts[0])
        assert n == want.count
        np.testing.assert_array_equal(xy[0, :n].cpu().numpy(), want.xy)
        np.testing.assert_array_equal(xyz[0, :n].cpu().numpy(), want.xyz)


def test_dropin_unique_pose(gpu):
    """CNN_outputs_to_object_pose(unique=True) on the scene of test_gpu_pnp's decoded-correspondence
    test (128 x 128 crop, box (260, 180, 128, 128), noise-free projections), with the pose
    tests/pnp_cases.py plants and pairs of horizontal neighbours sharing a class (the mean, x + 0.5,
    truncates onto the left pixel).  Tolerance: that test's (0.05 degree, 1.0 in t)."""
    from zebrapose_amd.binary_code_helper.CNN_output_to_pose import (CNN_outputs_to_object_pose,
                                                                     decode_correspondences)
    K = pnp_cases.K0
    rng = np.random.default_rng(9)
    R, t = pnp_cases._pose(rng)
    bbox = np.array([260, 180, 128, 128])
    H = W = 128
    mask = np.zeros((H, W), bool)
    mask[20:100, 30:110] = True
    ys, xs = np.nonzero(mask)
    pair = (ys - 20) * 40 + (xs - 30) // 2  # 3200 classes of two pixels
    cls = pair * 7 + 11
    ids = rng.integers(0, 65536, (H, W))
    ids[ys, xs] = cls
    left = (xs - 30) % 2 == 0
    uv = np.stack([xs[left] + bbox[0], ys[left] + bbox[1]], 1).astype(np.float64)
    lut = ref.make_lut(ref.LUT_CLASSES)
    lut[cls[left]] = pnp_cases._from_depth(uv, rng.uniform(760, 840, len(uv)).round(), R, t, K)
    lut_dict = {float(i): lut[i] for i in range(len(lut))}
    bits = ref.bits_to_logits(ids, 16) > 0
    code_image = bits.transpose(1, 2, 0).astype(np.float64)
    p2d, p3d = decode_correspondences(mask.astype(np.float64), code_image, bbox, 128, lut_dict, unique=True)
    assert len(p2d) == 3200
    np.testing.assert_array_equal(p2d, uv.astype(np.int64))
    rot, tv, success = CNN_outputs_to_object_pose(mask.astype(np.float64), code_image, bbox, 128, 2, lut_dict, K,
                                                  unique=True)
    assert success and tv.shape == (3, 1)
    ang = pnp_cases.rot_angle_deg(np.asarray(rot), R)
    assert ang < 0.05 and np.linalg.norm(tv.reshape(3) - t) < 1.0, (ang, tv.reshape(3), t)
