"""zp_pnp_lo on the device against tests/pnp_lo_ref.py: the whole loop on the noisy scenes whose
decisions tests/test_pnp_lo_host.py shows to stand clear of rounding (trace and inliers exact, the pose
within 16 x the reference's own spread over summation orders, the truncated cost not rising),
reproducibility, and the Python layers (PnPLocalOptimiser, PnP(local_optimisation=True),
MultiObjectPose, the drop-in keyword)."""
import numpy as np
import pytest
import torch

from tests import pnp_cases as PC
from tests import pnp_lo_cases as C
from tests import pnp_lo_ref as LO

pytestmark = pytest.mark.gpu


def run_lo(gpu, counts, xy, xyz, Ks, R, t, active=None, reproj_err=2.0, rounds=4, steps=10):
    """raw zp_pnp_lo call with every optional output -> dict of numpy arrays"""
    from zebrapose_amd import _lib as L
    B, HW = xy.shape[0], xy.shape[1]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    c_, xy_, xyz_, k_ = d(counts.astype(np.int32)), d(xy), d(xyz), d(C.kvecs(Ks))
    R_, t_ = d(np.asarray(R, np.float64).reshape(B, 9)), d(np.asarray(t, np.float64).reshape(B, 3))
    a_ = None if active is None else d(np.asarray(active, np.int32))
    out = {"R": torch.empty((B, 9), dtype=torch.float64, device=gpu), "t": torch.empty((B, 3), dtype=torch.float64, device=gpu),
           "inliers": torch.empty(B, dtype=torch.int32, device=gpu), "cost": torch.empty(B, dtype=torch.float64, device=gpu),
           "status": torch.empty(B, dtype=torch.int32, device=gpu),
           "trace": torch.empty((B, rounds, 2), dtype=torch.int32, device=gpu),
           "Hb": torch.empty((B, 28), dtype=torch.float64, device=gpu)}
    ws = torch.empty(int(L.lib.zp_pnp_lo_ws_bytes(B, HW)), dtype=torch.uint8, device=gpu)
    L.call("zp_pnp_lo", B, HW, c_.data_ptr(), xy_.data_ptr(), xyz_.data_ptr(), k_.data_ptr(), R_.data_ptr(), t_.data_ptr(),
           L.ptr(a_), float(reproj_err), rounds, steps, out["R"].data_ptr(), out["t"].data_ptr(), out["inliers"].data_ptr(),
           out["cost"].data_ptr(), out["status"].data_ptr(), out["trace"].data_ptr(), out["Hb"].data_ptr(), ws.data_ptr(),
           L.stream_ptr())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


_NOISY = []


@pytest.fixture
def noisy(gpu):
    """the eight noisy scenes in one batch, from the oracle's RANSAC poses (run once per session)"""
    if not _NOISY:
        _NOISY.append(_run_noisy(gpu))
    return _NOISY[0]


def _run_noisy(gpu):
    scenes = [C.noisy_scene(n, s) for n, s in C.NOISY]
    poses = [C.ransac_pose(n, s) for n, s in C.NOISY]
    counts, xy, xyz = PC.batch(scenes, HW=1500, garbage_tail=True)
    R, t = np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses])
    return scenes, R, t, run_lo(gpu, counts, xy, xyz, [C.K0] * len(scenes), R, t)


@pytest.mark.parametrize("k", range(len(C.NOISY)))
def test_whole_loop_matches_reference(noisy, k):
    scenes, R, t, got = noisy
    n, seed = C.NOISY[k]
    runs, tolR, tolt = C.noisy_ref(n, seed)
    ref = runs[0]
    assert got["status"][k] == 0
    assert np.array_equal(got["trace"][k], ref["trace"]), (got["trace"][k], ref["trace"])
    assert got["inliers"][k] == ref["inliers"]
    assert np.all(np.abs(got["Hb"][k] - ref["Hb"]) <= C.hb_bound(ref, n))
    dR = np.abs(got["R"][k].reshape(3, 3) - ref["R"]).max()
    dt = np.abs(got["t"][k] - ref["t"]).max()
    print(f"n {n} seed {seed}: device - reference |dR| {dR:.3g} (bound {tolR:.3g}), |dt| {dt:.3g} (bound {tolt:.3g})")
    assert dR <= tolR and dt <= tolt
    pw, uv = scenes[k][0], scenes[k][1]
    m0 = LO.truncated_cost(pw, uv, R[k], t[k], C.K0)
    m1 = LO.truncated_cost(pw, uv, got["R"][k].reshape(3, 3), got["t"][k], C.K0)
    assert m1 <= m0 * (1 + n * 2.0 ** -50)
    assert abs(got["cost"][k] - ref["cost"]) <= n * 2.0 ** -50 * ref["cost"]


def test_two_runs_and_two_places_give_the_same_bytes(gpu, noisy):
    scenes, R, t, first = noisy
    counts, xy, xyz = PC.batch(scenes, HW=1500, garbage_tail=True)
    again = run_lo(gpu, counts, xy, xyz, [C.K0] * len(scenes), R, t)
    for key in first:
        assert np.array_equal(first[key].view(np.uint8), again[key].view(np.uint8)), key
    # scene 4 alone, and in slot 5 of a batch of 8 among other neighbours
    one = PC.batch([scenes[4]], HW=1500)
    alone = run_lo(gpu, *one, [C.K0], R[4:5], t[4:5])
    order = [7, 0, 6, 1, 2, 4, 3, 5]
    mixed = PC.batch([scenes[i] for i in order], HW=1777, garbage_tail=True)
    among = run_lo(gpu, *mixed, [C.K0] * 8, R[order], t[order])
    assert order[5] == 4
    for key in alone:
        assert np.asarray(alone[key][0]).tobytes() == np.asarray(among[key][5]).tobytes(), key
        assert np.asarray(alone[key][0]).tobytes() == np.asarray(first[key][4]).tobytes(), key


def _tensors(gpu, scenes, HW):
    counts, xy, xyz = PC.batch(scenes, HW=HW)
    return [torch.from_numpy(a).to(gpu) for a in (counts, xy, xyz)]


def test_python_layers(gpu):
    from zebrapose_amd import _lib as L
    from zebrapose_amd.pnp import PnP, PnPLocalOptimiser
    scenes = [C.noisy_scene(n, s) for n, s in C.NOISY[:5]] + [(C.noisy_scene(300, 31)[0][:4], C.noisy_scene(300, 31)[1][:4])]
    counts, xy, xyz = _tensors(gpu, scenes, 1500)
    B = len(scenes)
    # the flag off: today's call, bit for bit
    R, t, ok, inl = PnP()(counts, xy, xyz)
    kv = torch.from_numpy(np.tile(LO.kvec(C.K0), (B, 1))).to(gpu)
    R2 = torch.empty((B, 3, 3), dtype=torch.float64, device=gpu)
    t2 = torch.empty((B, 3), dtype=torch.float64, device=gpu)
    ok2, inl2 = torch.empty(B, dtype=torch.int32, device=gpu), torch.empty(B, dtype=torch.int32, device=gpu)
    ws = torch.empty(int(L.lib.zp_pnp_ws_bytes(B, 150)), dtype=torch.uint8, device=gpu)
    L.call("zp_pnp_ransac", B, 1500, counts.data_ptr(), xy.data_ptr(), xyz.data_ptr(), kv.data_ptr(), 150, 2.0, 0.99,
           R2.data_ptr(), t2.data_ptr(), ok2.data_ptr(), inl2.data_ptr(), ws.data_ptr(), L.stream_ptr())
    assert torch.equal(R, R2) and torch.equal(t, t2) and torch.equal(inl, inl2)
    assert torch.equal(ok, (ok2 != 0) & (counts >= 6)) and ok.tolist() == [True] * 5 + [False]
    # the flag on: PnP() followed by PnPLocalOptimiser()
    Rl, tl, okl, inll = PnP(local_optimisation=True)(counts, xy, xyz)
    Ro, to, inlo, cost, status, trace, Hb = PnPLocalOptimiser()(counts, xy, xyz, None, R, t, ok, debug=True)
    assert status.tolist() == [0] * 5 + [1] and trace.shape == (B, 4, 2) and Hb.shape == (B, 28)
    assert torch.equal(Rl, Ro) and torch.equal(tl, to) and torch.equal(okl, ok)
    assert torch.equal(inll, torch.where(status == 0, inlo, inl))
    assert torch.equal(Ro[5], R[5]) and torch.equal(to[5], t[5]) and not torch.equal(Ro[:5], R[:5])
    five = PnPLocalOptimiser()(counts, xy, xyz, C.K0, R, t, ok)
    assert len(five) == 5 and torch.equal(five[0], Ro) and torch.equal(five[3], cost)
    with pytest.raises(ValueError):
        PnPLocalOptimiser()(counts, xy, xyz.double(), None, R, t)
    with pytest.raises(ValueError):
        PnPLocalOptimiser()(counts, xy, xyz, None, R.float(), t)
    with pytest.raises(ValueError):
        PnPLocalOptimiser()(counts, xy, xyz, None, R.cpu(), t)
    with pytest.raises(L.ZPError):
        PnPLocalOptimiser(rounds=0)(counts, xy, xyz, None, R, t)


def _net(seed, bn, layers=34):
    from oracle import ref_cpu
    from zebrapose_amd.model.BinaryCodeNet import BinaryCodeNet_Deeplab
    net = BinaryCodeNet_Deeplab(layers, 16, 2, concat=True, output_kernel_size=1)
    sd = ref_cpu.synthetic_state(layers, 16, seed, bn)
    net.load_state_dict(sd)
    return net.cuda().eval()


def test_multi_object_with_local_optimisation(gpu, golden):
    """the small fixture of tests/test_gpu_multi_object.py: with the optimiser the truncated cost of a
    crop's pose over the crop's own correspondences is not above the default's"""
    from zebrapose_amd.multi_object import MultiObjectPose
    from zebrapose_amd.pnp import PnP
    K = PC.K0
    rng = np.random.default_rng(3)
    bn = dict(golden("r34_bn_buffers.npz"))
    nets = [_net(s, bn) for s in (0, 1, 2)]
    luts = [rng.uniform(-60, 60, (65536, 3)) for _ in nets]
    luts[1][::97] = np.nan
    B = 7
    obj = np.array([2, 0, 2, 1, 0, 2, 1])
    x = torch.from_numpy(rng.normal(0, 1, (B, 3, 128, 128)).astype(np.float32)).cuda()
    bb = np.stack([rng.integers(-20, 300, B), rng.integers(-20, 200, B), rng.integers(64, 300, B),
                   rng.integers(64, 300, B)], 1)
    Ks = np.broadcast_to(K, (B, 3, 3)).copy()
    Ks[:, 0, 2] += np.arange(B)
    base = MultiObjectPose(nets, luts, precision="fp16")(x, obj, bb, Ks)
    lo = MultiObjectPose(nets, luts, precision="fp16", pnp=PnP(local_optimisation=True))(x, obj, bb, Ks)
    torch.cuda.synchronize()
    assert torch.equal(base["counts"], lo["counts"]) and torch.equal(base["success"], lo["success"])
    for b in range(B):
        n = int(base["counts"][b])
        pw, uv = base["xyz"][b, :n].cpu().numpy(), base["xy"][b, :n].cpu().numpy()
        assert np.all(np.isfinite(lo["R"][b].cpu().numpy())) and np.all(np.isfinite(lo["t"][b].cpu().numpy()))
        if not bool(base["success"][b]):
            continue
        m0 = LO.truncated_cost(pw, uv, base["R"][b].cpu().numpy(), base["t"][b].cpu().numpy(), Ks[b])
        m1 = LO.truncated_cost(pw, uv, lo["R"][b].cpu().numpy(), lo["t"][b].cpu().numpy(), Ks[b])
        assert m1 <= m0 * (1 + n * 2.0 ** -50), (b, m0, m1)
    del nets
    torch.cuda.empty_cache()


def test_dropin_keyword_reaches_the_device_branch(gpu, monkeypatch):
    import dropin.binary_code_helper.CNN_output_to_pose as D
    import zebrapose_amd.binary_code_helper.CNN_output_to_pose as Z
    assert D.CNN_outputs_to_object_pose is Z.CNN_outputs_to_object_pose
    pw, uv, _, _ = C.noisy_scene(300, 31)
    monkeypatch.setattr(Z, "USE_PYPROGRESSIVEX", False)
    monkeypatch.setattr(Z, "decode_correspondences", lambda *a, **k: (uv, pw))
    args = (None, None, None, 128)
    R0, t0, ok0 = Z.CNN_outputs_to_object_pose(*args, intrinsic_matrix=C.K0)
    R1, t1, ok1 = Z.CNN_outputs_to_object_pose(*args, intrinsic_matrix=C.K0, local_optimisation=True)
    assert ok0 and ok1 and R1.shape == (3, 3) and t1.shape == (3, 1)
    from zebrapose_amd.pnp import PnP
    counts, xy, xyz = _tensors(gpu, [(pw, uv)], len(pw))
    for flag, Rg, tg in ((False, R0, t0), (True, R1, t1)):
        Rp, tp, _, _ = PnP(local_optimisation=flag)(counts, xy, xyz, C.K0)
        assert np.array_equal(Rp[0].cpu().numpy(), Rg) and np.array_equal(tp[0].cpu().numpy().reshape(3, 1), tg)
    assert not np.array_equal(R0, R1)
    assert LO.truncated_cost(pw, uv, R1, t1, C.K0) < LO.truncated_cost(pw, uv, R0, t0, C.K0)
