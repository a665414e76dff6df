"""GT masks and info, the parts that need no GPU: tests/gtinfo_ref.py against what the reference's own
visibility.estimate_visib_mask_gt (both modes), misc.depth_im_to_dist_im_fast and
misc.calc_2d_bbox_xywh returned (tests/golden/gt_info.npz, tools/capture_gtinfo_fixtures.py), the
ZP_ERR_ARG paths of zp_scene_depth / zp_gt_info, and the Python wrappers' refusals."""
import ctypes
import json

import numpy as np
import pytest

from tests import bop_ref as BR
from tests import gtinfo_ref as GR


@pytest.fixture(scope="module")
def fx(golden):
    return golden("gt_info.npz")


def test_distance_images_equal_the_reference_fixture(fx):
    for b, ti in enumerate(fx["test_index"]):
        dg = BR.dist_image(fx["depth_gt"][b], fx["K"][b])
        dt = BR.dist_image(fx["depth_test"][ti], fx["K"][b])
        assert np.array_equal(dg.view(np.int64), fx["dist_gt"][b].view(np.int64))
        assert np.array_equal(dt.view(np.int64), fx["dist_test"][b].view(np.int64))


@pytest.mark.parametrize("mode", ["bop19", "bop18"])
def test_masks_counts_and_boxes_equal_the_reference_fixture(fx, mode):
    delta = float(fx["delta"])
    assert GR.margin_ok(fx["depth_gt"], (0, 0), fx["depth_test"], fx["K"], fx["test_index"], delta)
    mask, visib, info = GR.gt_info(fx["depth_gt"], (0, 0), fx["depth_test"], fx["K"], fx["test_index"], delta, mode)
    want = fx["visib_" + mode]
    assert np.array_equal(visib, want * 255)
    assert np.array_equal(mask, (fx["depth_gt"] > 0) * 255)
    assert np.array_equal(info[:, 2], want.sum((1, 2))) and np.array_equal(info[:, 0], (mask > 0).sum((1, 2)))
    # the reference's box is the inclusive form; per box, not under the both-or-none rule of bboxes()
    col = {"bop19": 1, "bop18": 2}[mode]
    for b in range(len(info)):
        for c, k in ((3, 0), (7, col)):
            x0, y0, x1, y1 = info[b, c:c + 4]
            box = [-1, -1, -1, -1] if x0 == -1 and x1 == -1 else [x0, y0, x1 - x0 + 1, y1 - y0 + 1]
            assert box == fx["bbox_xywh"][b, k].tolist(), (b, c)
    obj, vis = GR.bboxes(info, inclusive=True)
    seen = info[:, 2] > 0
    assert np.array_equal(obj[seen], fx["bbox_xywh"][seen, 0]) and np.array_equal(vis[seen], fx["bbox_xywh"][seen, col])
    assert np.all(obj[~seen] == -1) and np.all(vis[~seen] == -1) and (~seen).sum() == 1


def test_the_two_modes_differ_only_where_the_scene_has_no_depth(fx):
    a = GR.gt_info(fx["depth_gt"], (0, 0), fx["depth_test"], fx["K"], fx["test_index"], 15.0, "bop19")[1]
    b = GR.gt_info(fx["depth_gt"], (0, 0), fx["depth_test"], fx["K"], fx["test_index"], 15.0, "bop18")[1]
    hole = fx["depth_test"][fx["test_index"]] == 0
    assert np.any(a != b) and np.all(hole[a != b]) and np.all(b[hole] == 0)


def test_restatement_on_a_hand_made_scene():
    """5 x 6 image in a 15 x 18 render: a 3 x 4 block crossing the top-left corner of the frame."""
    H, W = 5, 6
    gt = np.zeros((3 * H, 3 * W), np.float32)
    gt[H - 1:H + 2, W - 2:W + 2] = 500.0     # image rows -1 .. 1, columns -2 .. 1
    test = np.full((H, W), 400.0, np.float32)
    test[0, 0] = 0                            # a hole: visible under bop19 only
    test[1, 1] = 600.0                        # the scene behind the object: visible
    K4 = [1e6, 1e6, 3.0, 2.5]                 # a long focal length: dist == depth to well below delta
    for mode, nvis, box in (("bop19", 2, [0, 0, 1, 1]), ("bop18", 1, [1, 1, 1, 1])):
        mask, visib, info = GR.gt_info_one(gt, W, H, test, K4, 15.0, mode)
        assert info.tolist() == [12, 3, nvis, -2, -1, 1, 1] + box
        assert mask.sum() == 4 * 255 and visib.sum() == nvis * 255 and visib[1, 1] == 255
    info = np.array([[12, 3, 2, -2, -1, 1, 1, 0, 0, 1, 1], [7, 0, 0, 30, 2, 33, 4, -1, -1, -1, -1],
                     [0, 0, 0, -1, -1, -1, -1, -1, -1, -1, -1]])
    obj, vis = GR.bboxes(info)
    assert obj.tolist() == [[-2, -1, 3, 2], [-1] * 4, [-1] * 4] and vis.tolist() == [[0, 0, 1, 1], [-1] * 4, [-1] * 4]
    assert GR.bboxes(info, inclusive=True)[0][0].tolist() == [-2, -1, 4, 3]
    assert GR.visib_fract(info).tolist() == [2 / 12, 0.0, 0.0]
    recs = GR.scene_gt_info(info)
    assert json.loads(json.dumps(recs)) == recs and set(recs[0]) == {
        "bbox_obj", "bbox_visib", "px_count_all", "px_count_valid", "px_count_visib", "visib_fract"}


def test_scene_depth_restatement():
    d = np.zeros((4, 2, 3), np.float32)
    d[0, 0, 0], d[1, 0, 0], d[2, 0, 0] = 7.0, 5.0, 5.0     # instances 1 and 2 tie: 1 wins
    d[3, 1, 2] = 9.0                                        # an index out of range contributes nothing
    d[0, 1, 1] = 3.0
    scene, inst = GR.scene_depth(d, [2, 0, 0, 5], 3)
    assert scene[0, 0, 0] == 5.0 and inst[0, 0, 0] == 1 and scene[2, 0, 0] == 7.0 and inst[2, 1, 1] == 0
    assert np.all(scene[1] == 0) and np.all(inst[1] == -1) and scene.sum() == 15.0 and (inst >= 0).sum() == 3


# ---- argument checks of the C functions ----------------------------------------------------------------

def _cases(fn, good, cases):
    from zebrapose_amd import _lib
    for bad, word in cases:
        a = dict(good, **bad)
        assert fn(*[a[k] for k in good]) == 1, bad
        assert word in _lib.lib.zp_last_error(), (bad, _lib.lib.zp_last_error())


def test_scene_depth_argument_checks_without_gpu():
    from zebrapose_amd import _lib
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    good = dict(B=2, depth=p, img_index=p, n_img=2, H=4, W=4, scene=p, instance=p, stream=None)
    cases = [(dict(B=0), b"B 0"), (dict(B=65536), b"B 65536"), (dict(n_img=0), b"n_img 0"),
             (dict(n_img=65536), b"n_img 65536"), (dict(H=0), b"0 x 4"), (dict(W=-1), b"4 x -1"),
             (dict(H=65536, W=32768), b"65536 x 32768")]
    cases += [({k: None}, b"NULL") for k in ("depth", "img_index", "scene")]
    _cases(_lib.lib.zp_scene_depth, good, cases)


def test_gt_info_argument_checks_without_gpu():
    from zebrapose_amd import _lib
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    good = dict(B=2, depth_gt=p, Hg=12, Wg=12, ox=4, oy=4, H=4, W=4, depth_test=p, n_test=2, test_index=p, K=p,
                delta=15.0, visib_mode=0, mask=p, mask_visib=p, info=p, stream=None)
    cases = [(dict(B=0), b"B 0"), (dict(B=65536), b"B 65536"), (dict(Hg=0), b"render 0 x 12"),
             (dict(H=0), b"image 0 x 4"), (dict(W=-1), b"image 4 x -1"), (dict(Hg=65536, Wg=32768), b"65536 x 32768"),
             (dict(ox=-1), b"at (-1, 4)"), (dict(oy=-1), b"at (4, -1)"), (dict(ox=9), b"at (9, 4)"),
             (dict(oy=9), b"at (4, 9)"), (dict(W=13, ox=0), b"window 4 x 13"), (dict(visib_mode=2), b"visib_mode 2"),
             (dict(visib_mode=-1), b"visib_mode -1"), (dict(n_test=0), b"n_test 0"),
             (dict(n_test=1, test_index=None), b"n_test 1")]
    cases += [({k: None}, b"NULL") for k in ("depth_gt", "depth_test", "K")]
    _cases(_lib.lib.zp_gt_info, good, cases)


# ---- the Python wrappers' refusals -----------------------------------------------------------------------

def test_wrappers_refuse_bad_shapes_and_dtypes():
    import torch
    from zebrapose_amd.gtinfo import GtInfo, SceneLabeler, gt_info, scene_depth
    d = torch.zeros((2, 12, 15), dtype=torch.float32)
    t = torch.zeros((2, 4, 5), dtype=torch.float32)
    K = [100.0, 100.0, 2.0, 2.0]
    bad = [
        lambda: gt_info(d.double(), t, K, window=(5, 4)),              # dtype
        lambda: gt_info(d.numpy(), t, K, window=(5, 4)),               # not a tensor
        lambda: gt_info(d[0], t, K, window=(5, 4)),                    # dims
        lambda: gt_info(d, t[:, :0], K, window=(5, 4)),                # empty
        lambda: gt_info(d, t, K),                                      # sizes differ and no window
        lambda: gt_info(d, t, K, window=(11, 4)),                      # the window leaves the render
        lambda: gt_info(d, t, K, window=(5, -1)),
        lambda: gt_info(d, t, K, window=(5, 4), visib_mode="bop20"),
        lambda: gt_info(d, t, K, window=(5, 4), outputs=("depth",)),
        lambda: gt_info(d, t, K, window=(5, 4), outputs=()),
        lambda: gt_info(d, t, K, window=(5, 4), delta=float("nan")),
        lambda: gt_info(d, t, K, window=(5, 4), test_index=[0]),       # one index per instance
        lambda: gt_info(torch.zeros((3, 12, 15)), t, K, window=(5, 4)),  # 2 images for 3 instances, no index
        lambda: gt_info(d, t, np.zeros((3, 4)), window=(5, 4)),        # K rows
        lambda: gt_info(d, t, K, window=(5, 4)),                       # all well, but not on a device
        lambda: scene_depth(d.half(), [0, 1], 2),
        lambda: scene_depth(d[0], [0], 1),
        lambda: scene_depth(d, [0, 1], 0),
        lambda: scene_depth(d, [0, 1, 1], 2),
        lambda: scene_depth(d, [0, 1], 2),                             # not on a device
        lambda: SceneLabeler({}),
        lambda: GtInfo(None, None, None).bboxes(),
        lambda: GtInfo(None, None, None).visib_fract(),
    ]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {k} was accepted")


def test_result_object_on_host_tensors():
    """bboxes / visib_fract / scene_gt_info are plain tensor arithmetic: they agree with the restatement."""
    import torch
    from zebrapose_amd.gtinfo import GtInfo
    info = np.array([[12, 3, 2, -2, -1, 1, 1, 0, 0, 1, 1], [7, 0, 0, 30, 2, 33, 4, -1, -1, -1, -1],
                     [0, 0, 0, -1, -1, -1, -1, -1, -1, -1, -1], [977, 400, 331, 3, 4, 40, 50, 5, 6, 30, 44]], np.int32)
    r = GtInfo(None, None, torch.from_numpy(info))
    for inc in (False, True):
        for got, want in zip(r.bboxes(inc), GR.bboxes(info, inc)):
            assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(r.visib_fract().numpy().view(np.int64), GR.visib_fract(info).view(np.int64))
    recs = r.scene_gt_info()
    assert recs == GR.scene_gt_info(info) and json.loads(json.dumps(recs)) == recs
    assert all(type(v) is int for v in recs[3]["bbox_visib"]) and type(recs[3]["visib_fract"]) is float
