"""d-ary surface codes (the code-radix ablation: 'CE' loss, radix decode, GT digits, the
DeepLabV3_non_binary network) on the GPU against the golden vectors captured from the reference
(tools/capture_nonbinary_fixtures.py -> tests/golden/nb_*.npz, r34nb_*.npz).

Bounds: the f64 loss rtol 1e-12 (the f64 BCE loss's bound); its f32 gradient 1 f32 ulp per element
(both sides compute in f64 and round once); digits / ids / decode exact (the fixture's top two
logits of every group differ by >= 1/32); forward and train step: tests/test_gpu_parity.py's bounds
for the same engines on r34_fwd64 / r34_train_step (the networks differ in head width only); the
513-wide head: tests/test_gpu_units.py's forward bound of a unit of that dtype.
"""
import numpy as np
import pytest
import torch

from tests.nb_state import CODES, nb_loss_inputs, nb_synthetic_state

pytestmark = pytest.mark.gpu
THR = np.float32(8.940696716308594e-08)
IDS = [f"d{d}_L{L}" for d, L in CODES]


@pytest.fixture(scope="module")
def nb_net(golden):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zebrapose_amd.model.BinaryCodeNet import BinaryCodeNet_Deeplab
    sd = nb_synthetic_state(4, 16, 0, dict(golden("r34_bn_buffers.npz")))
    net = BinaryCodeNet_Deeplab(34, 4, 16, concat=True, output_kernel_size=1, precision="fp32")
    net.load_state_dict(sd)
    return net.cuda().eval(), sd


# ------------------------------------------------------------------------------------ loss
def _loss_case(golden, d, L, mc):
    f = golden("nb_loss.npz")
    tag = f"d{d}_L{L}"
    code, mask, gt = nb_loss_inputs(d, L)
    s = np.array([code.astype(np.float64).sum(), np.abs(code.astype(np.float64)).sum()])
    assert np.array_equal(s, f[f"{tag}_code_sum"]), "the regenerated logits are not the captured ones"
    assert np.array_equal(mask, f[f"{tag}_mask"]) and np.array_equal(gt, f[f"{tag}_gt"])
    grad = golden(f"nb_loss_d256_mc{int(mc)}.npz")["grad"] if d == 256 else f[f"{tag}_grad_mc{int(mc)}"]
    return code, mask, gt, float(f[f"{tag}_loss_mc{int(mc)}"]), grad


@pytest.mark.parametrize("mc", [True, False], ids=["masked", "unmasked"])
@pytest.mark.parametrize("d,L", CODES, ids=IDS)
def test_ce_loss_forward_and_backward(gpu, golden, d, L, mc):
    from zebrapose_amd.model.BinaryCodeNet import BinaryCodeLoss
    code, mask, gt, loss_ref, grad_ref = _loss_case(golden, d, L, mc)
    fn = BinaryCodeLoss("CE", mc, d, False)
    m01 = torch.from_numpy(mask).to(gpu)
    mlog = torch.from_numpy(np.where(mask > 0.5, 1.0, -1.0).astype(np.float32)).to(gpu)
    forms = [("mask01/u8", lambda c: fn(c, m01, torch.from_numpy(gt).to(gpu))),
             ("mask01/f64", lambda c: fn(c, m01, torch.from_numpy(gt.astype(np.float64)).to(gpu))),
             ("logits/u8", lambda c: fn.forward_from_logits(c, mlog, torch.from_numpy(gt).to(gpu)))]
    for name, call in forms:
        c = torch.from_numpy(code).to(gpu).requires_grad_(True)
        loss = call(c)
        assert loss.dtype == torch.float64
        rel = abs(loss.item() - loss_ref) / abs(loss_ref)
        print(f"CE d={d} L={L} mask_code={mc} {name}: loss {loss.item():.15g} ref {loss_ref:.15g} rel {rel:.3g}")
        np.testing.assert_allclose(loss.item(), loss_ref, rtol=1e-12)
        loss.backward()
        assert c.grad.dtype == torch.float32
        got = c.grad.cpu().numpy()
        ulps = np.abs(got.astype(np.float64) - grad_ref.astype(np.float64)) / np.spacing(np.abs(grad_ref)).astype(np.float64)
        print(f"  gradient: max {ulps.max():.3g} ulp, {(ulps > 0).mean():.3g} of the elements differ")
        assert ulps.max() <= 1.0
        if mc:
            off = np.broadcast_to(mask == 0, (code.shape[0], code.shape[1]) + mask.shape[2:])
            assert off.any() and np.all(got[off] == 0.0)


def test_ce_loss_gradient_scale(gpu, golden):
    """3 * loss_b, as the train step weighs it: the gradient scales in f64 before the one rounding."""
    from zebrapose_amd.model.BinaryCodeNet import BinaryCodeLoss
    code, mask, gt, _, grad_ref = _loss_case(golden, 16, 4, True)
    c = torch.from_numpy(code).to(gpu).requires_grad_(True)
    (3 * BinaryCodeLoss("CE", True, 16, False)(c, torch.from_numpy(mask).to(gpu), torch.from_numpy(gt).to(gpu))).backward()
    np.testing.assert_allclose(c.grad.cpu().numpy(), 3 * grad_ref.astype(np.float64), rtol=2.0 ** -22, atol=0)


# ------------------------------------------------------------------------------------ digits / decode
@pytest.mark.parametrize("d,L", CODES, ids=IDS)
def test_digits_and_radix_decode_exact(gpu, golden, d, L):
    from zebrapose_amd import common_ops
    from zebrapose_amd.binary_code_helper import CNN_output_to_pose as C
    from zebrapose_amd.decode import Decoder
    f = golden("nb_decode.npz")
    lut = golden("decode.npz")["lut"]
    tag = f"d{d}_L{L}"
    ml = torch.from_numpy(f[f"{tag}_mask_logits"]).to(gpu)
    cl = torch.from_numpy(f[f"{tag}_code_logits"].astype(np.float32)).to(gpu)
    digits = common_ops.from_output_to_class_binary_code(cl, "CE", divided_num_each_interation=d, binary_code_length=L)
    assert digits.dtype == np.float64 and digits.shape == f[f"{tag}_digits"].shape
    assert np.array_equal(digits, f[f"{tag}_digits"])
    dec = Decoder(lut, device=gpu, class_base=d)
    assert dec.steps == L
    counts, xy, xyz, ids = dec(ml, cl, f["bboxes"], bbox_size=128, return_ids=True)
    res = Decoder.to_host(counts, xy, xyz)
    ids = ids.cpu().numpy()
    nan_hits = 0
    for b, (p2d, p3d) in enumerate(res):
        assert np.array_equal(ids[b], f[f"{tag}_b{b}_ids"])
        assert len(p2d) == int(f[f"{tag}_b{b}_count"])
        assert np.array_equal(p2d, f[f"{tag}_b{b}_p2d"]) and np.array_equal(p3d, f[f"{tag}_b{b}_p3d"])
        nan_hits += int((p3d == 0).all(axis=1).sum())
    print(f"decode d={d} L={L}: counts {[len(r[0]) for r in res]}, {nan_hits} NaN classes -> 0")
    assert [len(r[0]) for r in res][1] == 0 and f["bboxes"][0][0] < 0  # an empty mask, a negative origin
    # the drop-in's host-array entry decodes the same digits through the radix path
    lut_dict = {float(i): lut[i] for i in range(65536)}
    mask_bits = (f[f"{tag}_mask_logits"][2, 0] > THR).astype(np.float64)
    p2d, p3d = C.decode_correspondences(mask_bits, digits[2].transpose(1, 2, 0), f["bboxes"][2], 128, lut_dict,
                                        class_base=d)
    assert np.array_equal(p2d, f[f"{tag}_b2_p2d"]) and np.array_equal(p3d, f[f"{tag}_b2_p3d"])
    R, t, ok = C.CNN_outputs_to_object_pose(mask_bits, digits[2].transpose(1, 2, 0), f["bboxes"][2], 128, class_base=d,
                                            dict_class_id_3D_points=lut_dict)
    assert ok and np.asarray(R).shape == (3, 3) and np.asarray(t).shape == (3, 1)
    C.clear_decoder_cache()


@pytest.mark.parametrize("d,L", CODES, ids=IDS)
def test_gt_digits_exact(gpu, golden, d, L):
    from zebrapose_amd import _lib as Lb
    from zebrapose_amd.crop import CropPipeline
    f = golden("nb_gt_digits.npz")
    ids = f["ids"]
    H, W = ids.shape
    bits = np.stack([(ids >> (15 - j)) & 1 for j in range(16)]).astype(np.uint8)[None]
    s = d.bit_length() - 1
    bt = torch.from_numpy(bits).to(gpu)
    out = torch.empty((1, L, H, W), dtype=torch.uint8, device=gpu)
    Lb.call("zp_pack_digits", bt.data_ptr(), 1, 16, H, W, s, out.data_ptr(), Lb.stream_ptr())
    assert np.array_equal(out.cpu().numpy()[0], f[f"d{d}_L{L}"])
    # through the crop pipeline: the same crop's bit planes and digit planes agree
    rng = np.random.default_rng(5)
    gt_img = torch.from_numpy(rng.integers(0, 256, (2, 48, 40, 3), dtype=np.uint8)).to(gpu)
    img = torch.zeros_like(gt_img)
    boxes = np.array([[3, 5, 30, 30], [-4, 10, 25, 37], [8, 2, 20, 20]], dtype=np.int32)
    kw = dict(crop_size_img=16, crop_size_gt=24)
    b2 = CropPipeline(**kw)(img, [0, 1, 1], boxes, gt_images=gt_img)["code"].cpu().numpy().astype(np.int64)
    dg = CropPipeline(class_base=d, iterations=L, **kw)(img, [0, 1, 1], boxes, gt_images=gt_img)["code"]
    assert dg.dtype == torch.uint8 and tuple(dg.shape) == (3, L, 24, 24)
    want = sum(b2[:, j::s] << (s - 1 - j) for j in range(s))
    assert np.array_equal(dg.cpu().numpy(), want)


# ------------------------------------------------------------------------------------ network forward
def _bits_check(got, ref, band):
    amb = np.abs(ref) <= band
    bad = ((got > THR) != (ref > THR)) & ~amb
    return int(bad.sum()), int(amb.sum())


@pytest.mark.parametrize("split", ["x3", "h2", False], ids=["split_x3", "split_h2", "f32_mfma"])
def test_forward_fp32_matches_reference(nb_net, golden, split):
    """test_gpu_parity.test_forward_fp32_matches_reference's bounds on the (16, 4) network."""
    net, _ = nb_net
    net.set_precision("fp32")
    net.net.f32_split = split
    f = golden("r34nb_fwd64.npz")
    with torch.no_grad():
        m, c = net(torch.from_numpy(f["fwd64_x"]).cuda())
    net.net.f32_split = True
    assert tuple(m.shape) == (2, 1, 32, 32) and tuple(c.shape) == (2, 64, 32, 32)
    m, c = m.cpu().numpy(), c.cpu().numpy()
    for got, ref in ((m, f["fwd64_mask"]), (c, f["fwd64_code"])):
        print(f"fp32 split={split}: max|d| {np.abs(got - ref).max():.3g}")
        np.testing.assert_allclose(got, ref, atol=1e-3, rtol=1e-4)
        bad, amb = _bits_check(got, ref, 1e-3)
        assert bad == 0 and amb <= 0.01 * ref.size


@pytest.mark.parametrize("prec,rel_max,agree_min", [("bf16", 0.20, 0.99), ("fp16", 0.06, 0.97)])
def test_forward_16bit_within_conditioning_band(nb_net, golden, prec, rel_max, agree_min):
    """test_gpu_parity's bf16 / fp16 bands on the (16, 4) network."""
    net, _ = nb_net
    net.set_precision(prec)
    f = golden("r34nb_fwd64.npz")
    with torch.no_grad():
        m, c = net(torch.from_numpy(f["fwd64_x"]).cuda())
    net.set_precision("fp32")
    for got, ref in ((m.cpu().numpy(), f["fwd64_mask"]), (c.cpu().numpy(), f["fwd64_code"])):
        assert np.isfinite(got).all()
        rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
        out = np.abs(ref) > 0.25
        agree = ((got > THR) == (ref > THR))[out].mean()
        print(f"{prec} @64: rel-L2 {rel:.4g}, signs agree {agree:.4f} outside |ref| <= 0.25")
        assert rel <= rel_max, rel
        assert agree >= agree_min, agree


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-4), ("bf16", 3e-2), ("fp16", 4e-3)])
def test_head_513_wide(nb_net, golden, prec, tol):
    """The (256, 2) code's head width, 1 + 2 * 256 = 513 channels, as one head launch over the
    (16, 4) network's own [up2 | x_128] activations, against an f64 matmul on the host of the stored
    activations (and, for the 16-bit engines, the weights rounded as the kernel packs them)."""
    from zebrapose_amd.engine import Engine, Unit, joined
    net, _ = nb_net
    net.set_precision(prec)
    net.net.f32_split = False
    eng = net.net.eval_engine()
    eng.trace = []
    f = golden("r34nb_fwd64.npz")
    try:
        with torch.no_grad():
            net(torch.from_numpy(f["fwd64_x"]).cuda())
        head_in = [t for t in eng.trace if t[0] == "head"][0][2]
    finally:
        eng.trace = None
        net.net.f32_split = True
    assert (head_in.C, head_in.H, head_in.W) == (320, 32, 32)
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(320, 513, 1).cuda()
    B = head_in.B
    mask = torch.empty((B, 1, 32, 32), dtype=torch.float32, device="cuda")
    code = torch.empty((B, 512, 32, 32), dtype=torch.float32, device="cuda")
    Engine(torch.nn.Module(), eng.dtype).head_fwd(Unit(conv, None, False), head_in, mask, code, None)
    net.set_precision("fp32")
    x = joined(head_in.buf).double().cpu().reshape(-1, 320)
    w = conv.weight.detach().reshape(513, 320)
    if prec != "fp32":
        w = w.to(eng.dtype)
    ref = (x @ w.double().cpu().t() + conv.bias.detach().double().cpu()).reshape(B, 32, 32, 513).permute(0, 3, 1, 2)
    got = torch.cat([mask, code], 1).double().cpu()
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    print(f"513-wide head {prec}: max|d| {err:.3g} (scale {scale:.3g})")
    assert err <= tol * max(1.0, scale)


# ------------------------------------------------------------------------------------ training
HEAD = ["net.aspp.conv_1x1_4_mask.weight", "net.aspp.conv_1x1_4_mask.bias", "net.aspp.conv_1x1_4_code.weight",
        "net.aspp.conv_1x1_4_code.bias"]


def test_train_step_fp32_matches_reference(nb_net, golden):
    """test_gpu_parity.test_train_step_fp32_matches_reference's bounds, with the CE code loss."""
    from zebrapose_amd import common_ops
    from zebrapose_amd.model.BinaryCodeNet import BinaryCodeNet_Deeplab, BinaryCodeLoss, MaskLoss
    _, sd = nb_net
    f = golden("r34nb_train_step.npz")
    net = BinaryCodeNet_Deeplab(34, 4, 16, True, 1, precision="fp32")
    net.load_state_dict(sd)
    net = net.cuda().train()
    pm, pc = net(torch.from_numpy(f["x"]).cuda())
    np.testing.assert_allclose(pm.detach().cpu().numpy(), f["mask_logits"], atol=3e-3)
    np.testing.assert_allclose(pc.detach().cpu().numpy(), f["code_logits"], atol=3e-3)
    mask01 = torch.tensor(common_ops.from_output_to_class_mask(pm)).cuda()
    bcl, ml = BinaryCodeLoss("CE", True, 16, False), MaskLoss()
    lb = bcl(pc, mask01, torch.from_numpy(f["gt_code"]).cuda())
    lm = ml(pm, torch.from_numpy(f["gt_mask"]).cuda())
    print(f"loss_b {lb.item():.9g} ref {float(f['loss_b']):.9g}; loss_m {lm.item():.9g} ref {float(f['loss_m']):.9g}")
    np.testing.assert_allclose(lb.item(), float(f["loss_b"]), rtol=1e-4)
    np.testing.assert_allclose(lm.item(), float(f["loss_m"]), rtol=1e-4)
    (3 * lb + lm).backward()
    named = dict(net.named_parameters())
    assert all("grad:" + k in f for k in HEAD)
    for k in f:
        if k.startswith("grad:"):
            name = k[5:]
            ref = f[k]
            got = named[name].grad.cpu().numpy()
            got = got if name in HEAD else got[:8]
            assert got.shape == ref.shape, name
            rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
            print(f"{name}: rel-L2 {rel:.3g}")
            budget = 0.01 if "aspp.conv_1x1_4" in name else 0.05
            assert rel <= budget, (name, rel)
    sd2 = net.state_dict()
    for k in f:
        if k.startswith("after:"):
            np.testing.assert_allclose(sd2[k[6:]].cpu().numpy(), f[k], rtol=1e-3, atol=1e-4)


def test_train_step_bf16_runs(nb_net, golden):
    from zebrapose_amd.model.BinaryCodeNet import BinaryCodeNet_Deeplab
    from zebrapose_amd.train import TrainStep
    _, sd = nb_net
    f = golden("r34nb_train_step.npz")
    net = BinaryCodeNet_Deeplab(34, 4, 16, True, 1, precision="bf16")
    net.load_state_dict(sd)
    net = net.cuda().train()
    ts = TrainStep(net, ddp=False, binary_code_loss_type="CE", divided_number_each_iteration=16)
    grads = {}
    ts.optimizer.step = lambda: grads.update({n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None})
    loss, lb, lm = ts(torch.from_numpy(f["x"]).cuda(), torch.from_numpy(f["gt_code"]).cuda(),
                      torch.from_numpy(f["gt_mask"]).cuda())
    assert torch.isfinite(loss) and torch.isfinite(lb) and torch.isfinite(lm)
    assert len(grads) == 154 and all(k in grads for k in HEAD)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert all(float(grads[k].abs().max()) > 0 for k in HEAD)


# ------------------------------------------------------------------------------------ binary path unchanged
def test_binary_defaults_call_the_old_entries(gpu, golden, monkeypatch):
    from zebrapose_amd import _lib as Lb
    from zebrapose_amd.decode import Decoder
    from zebrapose_amd.model.BinaryCodeNet import BinaryCodeNet_Deeplab
    from zebrapose_amd.train import TrainStep
    from oracle import ref_cpu
    called = []
    real = Lb.call
    monkeypatch.setattr(Lb, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    d = golden("decode.npz")
    dec = Decoder(d["lut"], device=gpu, class_base=2)
    counts, xy, xyz = dec(torch.from_numpy(d["mask_logits"]).to(gpu), torch.from_numpy(d["code_logits"]).to(gpu),
                          d["bboxes"], bbox_size=128)
    for b, (p2d, p3d) in enumerate(Decoder.to_host(counts, xy, xyz)):
        assert np.array_equal(p2d, d[f"ib0_b{b}_p2d"]) and np.array_equal(p3d, d[f"ib0_b{b}_p3d"])
    assert "zp_decode" in called and "zp_decode_radix" not in called
    f = golden("r34_train_step.npz")
    net = BinaryCodeNet_Deeplab(34, 16, 2, True, 1, precision="bf16")
    net.load_state_dict(ref_cpu.synthetic_state(34, 16, 0, dict(golden("r34_bn_buffers.npz"))))
    ts = TrainStep(net.cuda().train(), ddp=False)
    loss, _, _ = ts(torch.from_numpy(f["x"]).cuda(), torch.from_numpy(f["gt_code"]).cuda(),
                    torch.from_numpy(f["gt_mask"]).cuda())
    assert torch.isfinite(loss)
    assert "zp_code_loss" in called and "zp_code_loss_bwd" in called
    assert not any(n.startswith("zp_ce_loss") or n in ("zp_code_digits", "zp_pack_digits") for n in called)
