"""The scene compositor, the parts that need no GPU: tests/scene_ref.py on a hand-worked case and
against tests/gtinfo_ref.py's scene composition, the ZP_ERR_ARG paths of zp_scene_compose, and the
refusals of scene_compose, SceneBatcher and CropPipeline's gt_index that come before the device is
needed."""
import ctypes
import inspect

import numpy as np
import pytest

from tests import gtinfo_ref as GR
from tests import scene_ref as SR

NAN, INF = float("nan"), float("inf")


def test_restatement_on_a_hand_worked_scene():
    """2 x 3 pixels, instances 0 and 1 in image 0, instance 2 in image 1."""
    depth = np.array([[[2, 0, 5], [3, 0, 0]],
                      [[2, 4, 1], [0, 0, NAN]],
                      [[0, 0, 0], [0, 7, -1]]], np.float32)
    shaded = np.zeros((3, 2, 3, 3), np.uint8)
    for b in range(3):
        shaded[b] = [10 * (b + 1), 10 * (b + 1) + 1, 10 * (b + 1) + 2]
    o = SR.scene_compose(depth, [0, 0, 1], 2, shaded)
    # (0, 0): a tie, the lowest instance; (0, 2): 1 is nearer; (1, 2): NaN is no surface; image 1: -1 is none
    assert o["scene"].tolist() == [[[2, 4, 1], [3, 0, 0]], [[0, 0, 0], [0, 7, 0]]]
    assert o["instance"].tolist() == [[[0, 1, 1], [0, -1, -1]], [[-1, -1, -1], [-1, 2, -1]]]
    assert o["fg"].tolist() == [[[255, 255, 255], [255, 0, 0]], [[0, 0, 0], [0, 255, 0]]]
    a, b, c, z = [10, 11, 12], [20, 21, 22], [30, 31, 32], [0, 0, 0]
    assert o["image"].tolist() == [[[a, b, b], [a, z, z]], [[z, z, z], [z, c, z]]]
    assert o["mask_visib"].tolist() == [[[255, 0, 0], [255, 0, 0]], [[0, 255, 255], [0, 0, 0]], [[0, 0, 0], [0, 255, 0]]]
    assert o["info"].tolist() == [[3, 2, 0, 0, 1, 0], [3, 2, 0, 1, 0, 2], [1, 1, 1, 1, 1, 1]]
    assert o["scene"].dtype == np.float32 and o["instance"].dtype == np.int32 and o["info"].dtype == np.int32
    h = SR.host_fields(o["info"])
    assert h["bbox_visib"].tolist() == [[0, 0, 1, 2], [1, 0, 2, 1], [1, 1, 1, 1]]
    assert h["visib_fract"].tolist() == [2 / 3, 2 / 3, 1.0] and h["px_count_all"].tolist() == [3, 3, 1]
    # an instance of no image: counted, never shown, the empty box
    o = SR.scene_compose(depth[[1, 0, 0]], [0, 0, 5], 1)
    assert o["image"] is None and o["info"].tolist() == [[3, 3, 0, 0, 0, 2], [3, 1, 1, 0, 1, 0], [3, 0, 0, 0, -1, -1]]
    assert not o["mask_visib"][2].any() and o["instance"].tolist() == [[[0, 0, 0], [1, -1, -1]]]
    h = SR.host_fields(np.array([[3, 0, 0, 0, -1, -1], [0, 0, 0, 0, -1, -1]]))
    assert h["bbox_visib"].tolist() == [[0, 0, 0, 0]] * 2 and h["visib_fract"].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_scene_and_instance_equal_the_gt_info_restatement(seed):
    r = np.random.default_rng(seed)
    B, n_img, H, W = 9, 3, 6, 10
    depth = r.integers(0, 4, (B, H, W)).astype(np.float32)  # many zeros and many ties
    depth[r.random((B, H, W)) < 0.05] = NAN
    depth[r.random((B, H, W)) < 0.05] = -1.0
    depth[r.random((B, H, W)) < 0.05] = INF
    depth[r.random((B, H, W)) < 0.05] = np.float32(1e-45)
    idx = r.integers(-1, n_img + 1, B)
    assert (idx < 0).any() or (idx >= n_img).any()
    o = SR.scene_compose(depth, idx, n_img)
    with np.errstate(invalid="ignore"):
        scene, inst = GR.scene_depth(depth, idx, n_img)
    assert np.array_equal(o["scene"].view(np.int32), scene.view(np.int32)) and np.array_equal(o["instance"], inst)
    assert (inst >= 0).any() and (inst < 0).any()


def test_c_argument_checks_without_gpu():
    from zebrapose_amd import _lib
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    good = dict(B=2, n_img=2, H=4, W=4, depth=p, shaded=p, img_index=p, image=p, fg=p, scene=p, instance=p,
                mask_visib=p, info=p, ws=p, stream=None)
    cases = [(dict(B=0), b"B 0"), (dict(B=65536), b"B 65536"), (dict(n_img=0), b"n_img 0"),
             (dict(n_img=65536), b"n_img 65536"), (dict(H=0), b"0 x 4"), (dict(W=-1), b"4 x -1"),
             (dict(H=32769), b"32769 x 4"), (dict(W=32769), b"4 x 32769"),
             (dict(B=3, H=32768, W=32768), b"32768 x 32768"), (dict(n_img=3, H=32768, W=32768), b"32768 x 32768"),
             (dict(depth=None), b"NULL"), (dict(img_index=None), b"NULL"), (dict(shaded=None), b"image needs shaded"),
             (dict(ws=None), b"info needs the workspace")]
    for bad, word in cases:
        a = dict(good, **bad)
        assert _lib.lib.zp_scene_compose(*[a[k] for k in good]) == 1, bad
        assert word in _lib.lib.zp_last_error(), (bad, _lib.lib.zp_last_error())
        if "depth" not in bad and "img_index" not in bad and "shaded" not in bad and "ws" not in bad:
            assert _lib.lib.zp_scene_compose_ws_bytes(a["B"], a["n_img"], a["H"], a["W"]) == -1, bad
    assert _lib.lib.zp_scene_compose_ws_bytes(2, 2, 4, 4) == 256
    assert _lib.lib.zp_scene_compose_ws_bytes(2, 1, 32768, 32767) >= 48
    # nothing asked for: nothing to do, no device call
    none = dict(good, image=None, fg=None, scene=None, instance=None, mask_visib=None, info=None, ws=None)
    assert _lib.lib.zp_scene_compose(*[none[k] for k in good]) == 0


def test_scene_compose_refuses_bad_arguments():
    import torch
    from zebrapose_amd.synth import SCENE_OUTPUTS, scene_compose
    assert SCENE_OUTPUTS == ("image", "fg", "scene", "instance", "mask_visib", "info")
    d = torch.zeros((2, 4, 5), dtype=torch.float32)
    s = torch.zeros((2, 4, 5, 3), dtype=torch.uint8)
    bad = [
        lambda: scene_compose(d.double(), [0, 1], 2),                  # dtype
        lambda: scene_compose(d.numpy(), [0, 1], 2),                   # not a tensor
        lambda: scene_compose(d[0], [0], 1),                           # dims
        lambda: scene_compose(d[:, :0], [0, 1], 2),                    # empty
        lambda: scene_compose(d, [0, 1], 0),
        lambda: scene_compose(d, [0, 1], 65536),
        lambda: scene_compose(d, [0, 1, 1], 2),                        # one index per instance
        lambda: scene_compose(d, [0, 1], 2, outputs=()),
        lambda: scene_compose(d, [0, 1], 2, outputs=("depth",)),
        lambda: scene_compose(d, [0, 1], 2, outputs=("image",)),       # image needs shaded
        lambda: scene_compose(d, [0, 1], 2, shaded=s[:1]),             # shaded's shape
        lambda: scene_compose(d, [0, 1], 2, shaded=s.float()),
        lambda: scene_compose(d, [0, 1], 2, shaded=s[..., :2]),
        lambda: scene_compose(d, [0, 1], 2),                           # all well, but not on a device
        lambda: scene_compose(d, [0, 1], 2, shaded=s),
    ]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {k} was accepted")


class _Stub:
    """Stands for a MeshRenderer where only its device is looked at."""

    def __init__(self, device="cpu"):
        import torch
        self.device = torch.device(device)


def test_scene_batcher_refuses_bad_arguments():
    from zebrapose_amd.gtinfo import MAX_RENDER_BYTES
    from zebrapose_amd.synth import SceneBatcher
    bgs = np.zeros((2, 8, 8, 3), np.uint8)
    a, b = _Stub(), _Stub()
    for f in (lambda: SceneBatcher({}, {}, bgs),
              lambda: SceneBatcher({1: a}, {2: a}, bgs),               # the two maps name other objects
              lambda: SceneBatcher({1: a}, {1: _Stub("meta")}, bgs),   # two devices
              lambda: SceneBatcher({1: a}, {1: a}, bgs[0]),            # backgrounds' shape
              lambda: SceneBatcher({1: a}, {1: a}, bgs[:0]),
              lambda: SceneBatcher({1: a}, {1: a}, bgs, phong=(0.4, 0.8))):
        with pytest.raises(ValueError):
            f()
    sb = SceneBatcher({1: a, 2: b}, {1: a, 2: b}, bgs, rng=np.random.default_rng(0))
    with pytest.raises(ValueError):
        sb.sample(0)
    d = sb.sample(3)
    assert d["light"].shape == (3, 3) and d["phong"].shape == (3, 3) and d["bg_index"].shape == (3,)
    assert set(d) == {"light", "phong", "bg_index"} and (d["light"][:, 2] <= 0).all() and d["bg_index"].max() < 2
    # the draws are SyntheticBatcher's, in its order, without the truncation pair
    from zebrapose_amd.synth import SyntheticBatcher
    one = SyntheticBatcher(a, a, bgs, truncate_fg=False, rng=np.random.default_rng(0)).sample(3)
    for k in d:
        assert np.array_equal(d[k], one[k]), k
    fixed = SceneBatcher({1: a}, {1: a}, bgs, random_light=False, rng=np.random.default_rng(0)).sample(2)
    assert fixed["light"].tolist() == [[400.0, 400.0, -400.0]] * 2 and fixed["phong"].tolist() == [[0.4, 0.8, 0.3]] * 2
    R, t, K = np.tile(np.eye(3), (2, 1, 1)), np.array([[0, 0, 2.0]] * 2), [20.0, 20.0, 16.0, 12.0]
    ok = dict(obj_ids=[1, 2], img_index=np.array([0, 0]), R=R, t=t, K=K, height=24, width=32)
    for bad in (dict(obj_ids=[]), dict(obj_ids=[1, 3]), dict(img_index=np.array([0, -1])), dict(img_index=np.array([0])),
                dict(img_index=np.array([0.0, 1.0])), dict(R=R[:1]), dict(t=t[:1]), dict(K=np.zeros((3, 4))),
                dict(height=0), dict(targets=[2]), dict(targets=[-1]), dict(targets=[0, 0]), dict(targets=[0.5]),
                dict(targets=[[0]]), dict(min_visib_fract=1.5), dict(min_visib_fract=NAN),
                dict(img_index=np.array([0, 3]), draws=d),              # draws has three images
                dict(draws=dict(d, light=d["light"][:2]))):
        with pytest.raises(ValueError):
            sb(**dict(ok, **bad))
            pytest.fail(f"{bad} was accepted")
    # the memory bound names the largest batch that fits
    n = MAX_RENDER_BYTES // (8 * 480 * 640)
    assert n == 109
    big = dict(obj_ids=[1] * (n + 1), img_index=np.zeros(n + 1, np.int64), R=np.tile(np.eye(3), (n + 1, 1, 1)),
               t=np.tile([0, 0, 2.0], (n + 1, 1)), K=K, height=480, width=640)
    with pytest.raises(ValueError, match=f"at most {n} fit"):
        sb(**big)


def test_gt_index_is_an_optional_last_argument():
    """CropPipeline's own checks need device tensors (tests/test_gpu_scene.py has gt_index's refusals);
    here: the argument exists, defaults to None and comes last, so existing calls are unchanged."""
    from zebrapose_amd.crop import CropPipeline
    for f in (CropPipeline.__call__, CropPipeline.train_batch, CropPipeline._check):
        p = list(inspect.signature(f).parameters.values())[-1]
        assert p.name == "gt_index" and p.default is None
    import torch
    with pytest.raises(ValueError, match="uint8 CUDA tensor"):
        CropPipeline()(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), [0], [[0, 0, 4, 4]], gt_index=[0])
