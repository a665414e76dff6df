"""GT masks and info on the device (zp_scene_depth, zp_gt_info; zebrapose_amd/gtinfo.py) against the
numpy restatement tests/gtinfo_ref.py.

Comparison rule: masks, info, scene and instance exactly equal, visib_fract bitwise equal.  The depth
inputs carry margins as bop_ref.vsd_scene's do (the visibility differences lie near -40, -5, 5, 40
and from 75 up, none near delta = 15), asserted on the reference-side arrays over every pixel of every instance
(gtinfo_ref.margin_ok), so a 1-ulp difference in a square root cannot flip a pixel."""
import json

import numpy as np
import pytest

from tests import bop_ref as BR
from tests import gtinfo_ref as GR
from tests import render_ref as RR

pytestmark = pytest.mark.gpu

DELTA = 15.0
MODES = ("bop19", "bop18")
# H, W, truncated (render 3 H x 3 W with the window at (W, H)) or not (render = image).  3 x 1100: a row
# is longer than the 1024 pixels a workgroup covers per step, and 9 x 3300 floats take the float4 path.
SHAPES = [(37, 53, True), (37, 53, False), (1, 1, True), (1, 1, False), (3, 1100, True)]
_CASES = {}


def _case(H, W, trunc, B):
    """Inputs and their gtinfo_ref results, computed once per case.  B = 7: 0 ordinary, 1 nothing
    rendered, 2 wholly outside the window (truncated renders only), 3 crossing the left / top edge,
    4 fully occluded, 5 and 6 ordinary; test_index repeats images and leaves [0, n_test)."""
    key = (H, W, trunc, B)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(1000 * H + 10 * W + B + (5 if trunc else 0))
    Hg, Wg, ox, oy = (3 * H, 3 * W, W, H) if trunc else (H, W, 0, 0)
    n_test = 3 if B > 1 else 1
    ti = np.array([0, 2, 1, 1, -3, 9, 0][:B])
    tic = np.clip(ti, 0, n_test - 1)
    yy, xx = np.mgrid[:Hg, :Wg].astype(np.float64)
    # one smooth surface per scene image over the whole render; the window of it is the scene
    surf = np.stack([rng.uniform(550, 1050) + 60 * np.sin(xx / 7 + rng.uniform(0, 6)) + 40 * np.cos(yy / 5)
                     for _ in range(n_test)])
    scene = surf[:, oy:oy + H, ox:ox + W]
    test = scene + rng.choice([-40.0, -5.0, 5.0, 40.0], scene.shape) + rng.uniform(-1, 1, scene.shape)
    test[rng.random(scene.shape) < 0.15] = 0
    test = test.astype(np.float32)
    shape = (B, Hg, Wg)
    gt = np.where(rng.random(shape) < 0.6, surf[tic] + np.where(rng.random(shape) < 0.3, 80.0, 0.0), 0.0)
    if B > 1:
        gt[1] = 0
        if trunc:
            gt[2, oy:oy + H, ox:ox + W] = 0
        keep = np.zeros((Hg, Wg), bool)
        keep[max(oy - 3, 0):oy + (H + 1) // 2, max(ox - 4, 0):ox + (W + 1) // 2] = True
        gt[3] = np.where(keep, gt[3], 0.0)
        win = test[tic[4]].astype(np.float64)
        gt[4] = 0
        gt[4, oy:oy + H, ox:ox + W] = np.where(win > 0, win + 100.0, 0.0)
    gt = gt.astype(np.float32)
    K = np.stack([rng.uniform(5.5, 6.5, B) * W, rng.uniform(5.5, 6.5, B) * W, W / 2 + rng.uniform(-3, 3, B),
                  H / 2 + rng.uniform(-3, 3, B)], 1)
    # no pixel and no instance is left out of the margin check
    assert GR.margin_ok(gt, (ox, oy), test, K, ti, DELTA), key
    want = {m: GR.gt_info(gt, (ox, oy), test, K, ti, DELTA, m) for m in MODES}
    _CASES[key] = dict(gt=gt, test=test, K=K, ti=ti, window=(ox, oy), want=want)
    return _CASES[key]


def _run(c, dev, mode, **kw):
    import torch
    from zebrapose_amd.gtinfo import gt_info
    return gt_info(torch.from_numpy(c["gt"]).to(dev), torch.from_numpy(c["test"]).to(dev), c["K"], window=c["window"],
                   test_index=c["ti"], delta=DELTA, visib_mode=mode, **kw)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("H,W,trunc", SHAPES)
def test_gt_info_matches_the_restatement_exactly(gpu, H, W, trunc, B, mode):
    c = _case(H, W, trunc, B)
    r = _run(c, gpu, mode)
    mask, visib, info = c["want"][mode]
    got = r.info.cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, info), (got, info)
    assert np.array_equal(r.mask.cpu().numpy(), mask)
    assert np.array_equal(r.mask_visib.cpu().numpy(), visib)
    assert np.array_equal(r.visib_fract().cpu().numpy().view(np.int64), GR.visib_fract(info).view(np.int64))
    for inc in (False, True):
        for g, w in zip(r.bboxes(inc), GR.bboxes(info, inc)):
            assert np.array_equal(g, w)
    assert r.scene_gt_info() == GR.scene_gt_info(info)
    again = _run(c, gpu, mode)
    assert all(bool((getattr(r, k) == getattr(again, k)).all()) for k in ("mask", "mask_visib", "info"))


def test_the_special_instances_are_what_they_are_meant_to_be():
    """On the reference side (no GPU needed, but the cases are this file's): each edge case occurs."""
    c = _case(37, 53, True, 7)
    i19, i18 = c["want"]["bop19"][2], c["want"]["bop18"][2]
    assert np.all(i19[1] == [0, 0, 0] + [-1] * 8)                                   # nothing rendered
    assert i19[2, 0] > 0 and i19[2, 2] == 0 and np.all(i19[2, 7:] == -1)              # outside the window
    assert np.all(np.stack(GR.bboxes(i19))[:, 2] == -1)                              # ... so both boxes are -1
    assert i19[3, 3] < 0 and i19[3, 4] < 0 and i19[3, 7] >= 0 and i19[3, 2] > 0       # crossing the left / top edge
    assert i19[4, 0] > 0 and i19[4, 1] == i19[4, 0] and i19[4, 2] == 0 and i18[4, 2] == 0  # fully occluded
    assert i19[0, 5] >= 53 and i19[0, 6] >= 37                                       # the box exceeds the frame
    # the modes differ, and only where the scene has no depth under the object
    for b in (0, 3, 5, 6):
        v19, v18 = c["want"]["bop19"][1][b], c["want"]["bop18"][1][b]
        hole = c["test"][np.clip(c["ti"], 0, 2)[b]] == 0
        assert np.any(v19 != v18) and np.all(hole[v19 != v18]) and i19[b, 2] > i18[b, 2] > 0
    assert np.array_equal(i19[:, :2], i18[:, :2]) and np.array_equal(i19[:, 3:7], i18[:, 3:7])


@pytest.mark.parametrize("drop", ["mask", "mask_visib", "info"])
def test_gt_info_each_output_left_out_in_turn(gpu, drop):
    c = _case(37, 53, True, 7)
    keep = tuple(k for k in ("mask", "mask_visib", "info") if k != drop)
    r = _run(c, gpu, "bop19", outputs=keep)
    assert getattr(r, drop) is None
    for k in keep:
        want = c["want"]["bop19"][("mask", "mask_visib", "info").index(k)]
        assert np.array_equal(getattr(r, k).cpu().numpy(), want), k


def test_gt_info_without_test_index_and_with_one_image(gpu):
    """No test_index: instance b reads image b; one scene image serves every instance."""
    import torch
    from zebrapose_amd.gtinfo import gt_info
    c = _case(37, 53, True, 7)
    gt, test, K = c["gt"][:3], c["test"], c["K"][:3]
    assert GR.margin_ok(gt, c["window"], test, K, None, DELTA)
    assert GR.margin_ok(gt, c["window"], test[1:2], K, [0] * 3, DELTA)
    dg, dt = torch.from_numpy(gt).to(gpu), torch.from_numpy(test).to(gpu)
    for r, want in ((gt_info(dg, dt, K, window=c["window"], delta=DELTA), GR.gt_info(gt, c["window"], test, K, None, DELTA)),
                    (gt_info(dg, dt[1:2], K, window=c["window"], delta=DELTA),
                     GR.gt_info(gt, c["window"], test[1:2], K, [0] * 3, DELTA))):
        for g, w in zip((r.mask, r.mask_visib, r.info), want):
            assert np.array_equal(g.cpu().numpy(), w)


# ---- zp_scene_depth ---------------------------------------------------------------------------------

def _depths(rng, B, H, W):
    d = rng.uniform(400, 1200, (B, H, W)).astype(np.float32)
    d[rng.random((B, H, W)) < 0.5] = 0
    return d


@pytest.mark.parametrize("H,W", [(37, 53), (8, 12), (1, 1), (2, 1100)])
def test_scene_depth_matches_the_restatement_exactly(gpu, H, W):
    import torch
    from zebrapose_amd.gtinfo import scene_depth
    rng = np.random.default_rng(H * W)
    d = _depths(rng, 6, H, W)
    d[4] = d[1]                                   # two identical instances: the tie goes to the lower index
    ii = np.array([4, 2, 2, 7, 2, 0])             # descending, image 1 and 3 without an instance, 7 out of range
    scene, inst = GR.scene_depth(d, ii, 5)
    assert np.all(scene[[1, 3]] == 0) and np.all(inst[[1, 3]] == -1) and not np.any(inst == 4) and not np.any(inst == 3)
    if H * W > 100:
        assert np.any(inst == 1) and np.any(inst == 2) and np.any(inst[2] == -1)
    dd = torch.from_numpy(d).to(gpu)
    s, i = scene_depth(dd, ii, 5)
    assert s.dtype == torch.float32 and i.dtype == torch.int32
    assert np.array_equal(s.cpu().numpy().view(np.int32), scene.view(np.int32)) and np.array_equal(i.cpu().numpy(), inst)
    s2, i2 = scene_depth(dd, torch.from_numpy(ii).to(gpu), 5)
    assert bool((s == s2).all()) and bool((i == i2).all())
    only, none = scene_depth(dd, ii, 5, return_instance=False)
    assert none is None and bool((only == s).all())
    # a permutation of the instances: the same scene, and the same instances once mapped back
    perm = rng.permutation(6)
    sp, ip = scene_depth(torch.from_numpy(np.ascontiguousarray(d[perm])).to(gpu), ii[perm], 5)
    ip = ip.cpu().numpy()
    back = np.where(ip >= 0, perm[np.maximum(ip, 0)], -1)
    back[back == 4] = 1                           # the identical pair: either name is the same surface
    assert np.array_equal(sp.cpu().numpy().view(np.int32), scene.view(np.int32)) and np.array_equal(back, inst)


# ---- end to end ---------------------------------------------------------------------------------------

H2, W2 = 48, 64
_E2E = {}


def _e2e():
    """Two small meshes, four instances over two images, in an order that grouping by object has to
    undo; image 0: object 2 in front of object 1; image 1: object 1 crosses the left edge."""
    if _E2E:
        return _E2E
    v1, f1 = BR.icosphere(1)
    v2, f2 = BR.icosphere(0)
    meshes = {1: (v1 * np.float32(30.0), f1), 2: (v2 * np.array([25.0, 18.0, 25.0], np.float32), f2)}
    obj_ids = np.array([2, 1, 1, 2])
    img_index = np.array([0, 0, 1, 1])
    rng = np.random.default_rng(4)
    R = np.stack([BR.rot(rng) for _ in range(4)])
    t = np.array([[10.0, 2.0, 250.0], [0.0, 0.0, 300.0], [-115.0, 5.0, 300.0], [40.0, 20.0, 280.0]])
    K = np.array([80.0, 80.0, 32.0, 24.0])
    big = np.zeros((4, 3 * H2, 3 * W2), np.float32)
    for oid, (v, f) in meshes.items():
        idx = np.flatnonzero(obj_ids == oid)
        Ks = np.repeat((K + np.array([0, 0, W2, H2]))[None], len(idx), 0)
        big[idx] = RR.render(v, f, None, R[idx], t[idx], Ks, 3 * H2, 3 * W2)["depth"]
    win = np.ascontiguousarray(big[:, H2:2 * H2, W2:2 * W2])
    scene, inst = GR.scene_depth(win, img_index, 2)
    occ = scene.copy()
    occ[0, :, :30] = 150.0                        # an occluder in front of the left part of image 0
    K4 = np.repeat(K[None], 4, 0)
    for dt in (scene, occ):
        assert GR.margin_ok(big, (W2, H2), dt, K4, img_index, DELTA)
    _E2E.update(meshes=meshes, obj_ids=obj_ids, img_index=img_index, R=R, t=t, K=K, big=big, scene=scene, inst=inst,
                occ=occ, want=GR.gt_info(big, (W2, H2), scene, K4, img_index, DELTA),
                want_occ=GR.gt_info(big, (W2, H2), occ, K4, img_index, DELTA))
    return _E2E


def test_e2e_reference_side_has_occlusion_and_truncation():
    e = _e2e()
    info, info_occ = e["want"][2], e["want_occ"][2]
    assert np.all(info[:, 0] > 100)
    assert info[0, 2] == (e["big"][0, H2:2 * H2, W2:2 * W2] > 0).sum()          # object 2 in front: all visible
    assert 0 < info[1, 2] < 0.8 * info[1, 0]                                   # object 1 behind it
    assert info[2, 3] < 0 and 0 < info[2, 2] < info[2, 0]                      # crossing the left edge
    assert np.all(info_occ[:2, 2] < info[:2, 2]) and np.array_equal(info_occ[2:], info[2:])
    assert set(np.unique(e["inst"][0])) == {-1, 0, 1} and set(np.unique(e["inst"][1])) == {-1, 2, 3}


def _labeler(e, dev):
    from zebrapose_amd.gtinfo import SceneLabeler
    from zebrapose_amd.render import MeshRenderer
    return SceneLabeler({oid: MeshRenderer(v, f, device=dev) for oid, (v, f) in e["meshes"].items()})


def _same(r, want):
    return all(np.array_equal(g.cpu().numpy(), w) for g, w in zip((r.mask, r.mask_visib, r.info), want))


def test_scene_labeler_composes_the_scene_and_labels_it(gpu):
    e = _e2e()
    lab = _labeler(e, gpu)
    r, scene, inst = lab.labels(e["obj_ids"], e["img_index"], e["R"], e["t"], e["K"], H2, W2, delta=DELTA)
    assert np.array_equal(scene.cpu().numpy().view(np.int32), e["scene"].view(np.int32))
    assert np.array_equal(inst.cpu().numpy(), e["inst"])
    assert _same(r, e["want"])
    recs = r.scene_gt_info()
    assert json.loads(json.dumps(recs)) == recs == GR.scene_gt_info(e["want"][2])
    # more than one chunk per object: rendered twice, the same labels
    import zebrapose_amd.gtinfo as G
    old = G.MAX_RENDER_BYTES
    G.MAX_RENDER_BYTES = 4 * 9 * H2 * W2
    try:
        r1, scene1, inst1 = lab.labels(e["obj_ids"], e["img_index"], e["R"], e["t"], e["K"], H2, W2, delta=DELTA)
    finally:
        G.MAX_RENDER_BYTES = old
    assert _same(r1, e["want"]) and bool((scene1 == scene).all()) and bool((inst1 == inst).all())


def test_scene_labeler_with_a_measured_depth_and_without_truncation(gpu):
    import torch
    e = _e2e()
    lab = _labeler(e, gpu)
    occ = torch.from_numpy(e["occ"]).to(gpu)
    r, scene, inst = lab.labels(e["obj_ids"], e["img_index"], e["R"], e["t"], e["K"], H2, W2, depth_test=occ, delta=DELTA)
    assert inst is None and scene is occ and _same(r, e["want_occ"])
    # truncation=False: the in-frame render with a zero origin
    Ks = np.repeat(e["K"][None], 4, 0)
    small = np.zeros((4, H2, W2), np.float32)
    for oid, (v, f) in e["meshes"].items():
        idx = np.flatnonzero(e["obj_ids"] == oid)
        small[idx] = RR.render(v, f, None, e["R"][idx], e["t"][idx], Ks[idx], H2, W2)["depth"]
    assert GR.margin_ok(small, (0, 0), e["occ"], Ks, e["img_index"], DELTA)
    r2, _, _ = lab.labels(e["obj_ids"], e["img_index"], e["R"], e["t"], e["K"], H2, W2, depth_test=occ, truncation=False,
                          delta=DELTA)
    assert _same(r2, GR.gt_info(small, (0, 0), e["occ"], Ks, e["img_index"], DELTA))


def test_labels_feed_the_crop_pipeline(gpu):
    import torch
    from zebrapose_amd.crop import CropPipeline
    e = _e2e()
    r, _, _ = _labeler(e, gpu).labels(e["obj_ids"], e["img_index"], e["R"], e["t"], e["K"], H2, W2, delta=DELTA)
    mask_w, visib_w, info_w = e["want"]
    box = r.bboxes()[1]
    assert np.array_equal(box, GR.bboxes(info_w)[1]) and np.all(box[:, 2] > 0)
    pipe = CropPipeline(crop_size_img=32, crop_size_gt=16, code_bits=16)
    pad, _ = pipe.boxes(box, W2, H2)
    rng = np.random.default_rng(9)
    images = torch.from_numpy(rng.integers(0, 256, (2, H2, W2, 3), dtype=np.uint8)).to(gpu)
    per_instance = images[torch.from_numpy(e["img_index"]).to(gpu)].contiguous()
    got = pipe(per_instance, np.arange(4), pad, masks=r.mask_visib, entire_masks=r.mask)
    want = pipe(per_instance, np.arange(4), pad, masks=torch.from_numpy(visib_w).to(gpu),
                entire_masks=torch.from_numpy(mask_w).to(gpu))
    for k in ("x", "mask", "entire_mask"):
        assert bool((got[k] == want[k]).all()), k
    assert float(got["mask"].sum()) > 0 and float(got["entire_mask"].sum()) >= float(got["mask"].sum())
