"""CPU: the oracle restatement (oracle/yolo_oracle.py) against what the UNMODIFIED reference modules compute on inputs that differ from the
other golden fixtures.  The reference's outputs are stored in tests/golden/crosscheck_*.npz (oracle/make_golden.py:gen_crosscheck, which runs the
reference through oracle/ref_shim.py on the same inputs); the oracle side is computed here.  The two large outputs (TTA, trained weights) are
stored quantized with a recorded error bound `err`; their checks subtract (1 + rtol) * err from atol, so passing one still means
|oracle - reference| <= atol + rtol * |reference| with the original atol and rtol (oracle/make_golden.py:xc_quantize)."""
import numpy as np
import pytest
import torch

from oracle import detgen, yolo_oracle as yo
from oracle.make_golden import XC_LABELS, load_crosscheck, xc_metrics_batches, xc_train_setup


@pytest.fixture(scope="module")
def G(golden_dir):
    return load_crosscheck(golden_dir)


def test_build_targets_and_loss_match_live_reference(G):
    anchors = torch.from_numpy(G["loss_anchors"])
    pn = [detgen.uniform((3, 3, s, s, 85), -3.0, 3.0, name=f"v{s}", seed=31) for s in (24, 12, 6)]
    tn = detgen.synth_targets(3, 11, seed=31)
    p2 = [torch.from_numpy(a).clone().requires_grad_(True) for a in pn]
    t = torch.from_numpy(tn)
    o_tcls, o_tbox, o_idx, o_anch = yo.build_targets([q.shape for q in p2], t, anchors)
    for i in range(3):
        r_idx = torch.from_numpy(G[f"loss_idx{i}"])
        assert len(o_idx[i]) == len(r_idx) and all(torch.equal(a, b) for a, b in zip(r_idx, o_idx[i]))
        assert torch.equal(torch.from_numpy(G[f"loss_tcls{i}"]), o_tcls[i]) and torch.equal(torch.from_numpy(G[f"loss_tbox{i}"]), o_tbox[i])
        assert torch.equal(torch.from_numpy(G[f"loss_anch{i}"]), o_anch[i])
    ol, oi = yo.compute_loss(p2, t, anchors)
    ol.backward()
    np.testing.assert_allclose(ol.detach().numpy(), G["loss_loss"], rtol=1e-6)
    np.testing.assert_allclose(oi.numpy(), G["loss_items"], rtol=1e-6)
    for i, b in enumerate(p2):
        np.testing.assert_allclose(b.grad.numpy(), G[f"loss_grad{i}"], rtol=1e-5, atol=1e-10)


def test_autobalance_matches_live_reference(G):
    """ComputeLoss(autobalance=True) (utils/loss.py:127, :173-177): four calls of the reference against the oracle's restatement -- losses and
    the drifting balance list (Python doubles) step by step."""
    assert int(G["ab_ssi"]) == 1
    anchors = torch.from_numpy(G["ab_anchors"])
    bal = [4.0, 1.0, 0.4]
    for step in range(4):
        p = [torch.from_numpy(detgen.uniform((2, 3, s, s, 85), -3.0, 3.0, name=f"ab{s}", seed=40 + step)) for s in (16, 8, 4)]
        t = torch.from_numpy(detgen.synth_targets(2, 6, seed=40 + step))
        loss_o, items_o = yo.compute_loss(p, t, anchors, nc=80, balance=bal, autobalance_ssi=1)
        torch.testing.assert_close(loss_o, torch.from_numpy(G[f"ab_loss{step}"]), rtol=1e-6, atol=0)
        torch.testing.assert_close(items_o, torch.from_numpy(G[f"ab_items{step}"]), rtol=1e-6, atol=0)
        assert bal == G[f"ab_balance{step}"].tolist(), (step, bal, G[f"ab_balance{step}"])
    assert bal[1] == 1.0 and bal[0] != 4.0


def test_forward_augment_matches_live_reference(G):
    """models/yolo.py:269-312 (TTA: scales 1 / 0.83 / 0.67 + left-right flip, _descale_pred, _clip_augmented): the reference's
    model(x, augment=True) against oracle.forward_augment on the same weights."""
    cfg = yo.model_cfg("yolov5n")
    sd = yo.det_state_dict(cfg, 3, fused=False)
    x = torch.from_numpy(detgen.uniform((2, 3, 96, 128), 0.0, 1.0, name="tta", seed=5))
    zr = torch.from_numpy(G["tta_k"] * float(G["tta_q"]))   # the reference's output to within tta_err, in float64
    rtol, atol = 1e-5, 1e-5 - (1 + 1e-5) * float(G["tta_err"])
    assert 0 < atol
    with torch.no_grad():
        zo = yo.forward_augment(cfg, sd, x)
    assert zr.shape == zo.shape
    torch.testing.assert_close(zo.double(), zr, rtol=rtol, atol=atol)


def test_nms_matches_live_reference(G):
    pred = detgen.synth_predictions(2, 1500, 85, obj_pow=3, seed=41)
    out = yo.non_max_suppression(pred, 0.25, 0.45, max_det=300)
    assert len(out) == 2
    for i, o in enumerate(out):
        assert np.array_equal(G[f"nms_{i}"], o)


def test_nms_with_apriori_labels_matches_live_reference(G):
    """general.py:706-712 (`labels`, val.py --save-hybrid): the a-priori label rows join the candidates with confidence 1; one image without labels,
    multi_label on and off."""
    pred = detgen.synth_predictions(3, 800, 15, obj_pow=3, seed=43)
    for ml in (False, True):
        out = yo.non_max_suppression(pred, 0.25, 0.45, labels=XC_LABELS, multi_label=ml, max_det=300)
        assert len(out) == 3
        for i, o in enumerate(out):
            assert np.array_equal(G[f"nmslab{int(ml)}_{i}"], o)
        assert (out[0][:2, 4] == 1.0).all() and {int(c) for c in out[0][:2, 5]} == {2, 7}


def test_process_batch_and_ap_match_live_reference(G):
    """utils/metrics.py process_batch / ap_per_class (unmodified) vs the oracle restatement on a batch that is not in the fixtures."""
    iouv = torch.linspace(0.5, 0.95, 10).numpy()
    stats = []
    for i, (det, lab) in enumerate(xc_metrics_batches()):
        ref = G[f"pb_{i}"]
        assert np.array_equal(yo.process_batch(det, lab, iouv), ref)
        stats.append((ref, det[:, 4], det[:, 5], lab[:, 0]))
    tp, conf, pcls, tcls = (np.concatenate(x, 0) for x in zip(*stats))
    o = yo.ap_per_class(tp, conf, pcls, tcls)
    n = len([k for k in G if k.startswith("ap_")])
    assert n == len(o) == 7
    for i, b in enumerate(o):
        np.testing.assert_allclose(G[f"ap_{i}"], np.asarray(b, np.float64), rtol=0, atol=1e-12)


def test_training_loop_restatement_matches_reference_pieces(G):
    """oracle/train_oracle.py (the fp32 yardstick of the train-loop tests) against the same schedule driven through the REFERENCE's own
    DetectionModel (train mode), ComputeLoss, smart_optimizer and ModelEMA (train.py:234-248,372-434; oracle/make_golden.py:gen_crosscheck):
    per-iteration loss items, final parameters and EMA must agree to fp32 round-off."""
    from oracle import train_oracle as to

    cfg, imgs, tpi, bs, epochs, hyp = xc_train_setup()
    sd = yo.det_state_dict(cfg, 9, fused=False)
    init = {k: v.numpy().astype(np.float64) for k, v in sd.items()}   # (the stored weights are steps above these; the EMA, steps above the weights)
    ref = to.train_oracle(cfg, sd, imgs, tpi, bs, hyp=dict(hyp), epochs=epochs, cos_lr=True)
    np.testing.assert_allclose(ref["losses"].numpy(), G["train_losses"], rtol=2e-4, atol=1e-6)
    assert ref["updates"] == int(G["train_updates"])
    q, rtol = float(G["train_q"]), 2e-3
    atol = 2e-5 - (1 + rtol) * float(G["train_err"])
    assert 0 < atol
    n = 0
    for k, v in ref["sd"].items():
        if v.dtype.is_floating_point and not k.endswith("anchors"):
            w = init[k] + G[f"train_sd:{k}"] * q
            np.testing.assert_allclose(v.numpy(), w, rtol=rtol, atol=atol, err_msg=k)
            np.testing.assert_allclose(ref["ema"][k].numpy(), w + G[f"train_ema:{k}"] * q, rtol=rtol, atol=atol, err_msg="ema " + k)
            n += 1
    assert n == len([k for k in G if k.startswith("train_sd:")])
