"""Golden vectors produced by the REFERENCE's own classes (oracle/make_golden.py) hold

  (a) the oracle restatement (oracle/ssn_oracle.py)            -- CPU tier: pins the oracle;
  (b) the product ops (mirror classes -> C ABI -> HIP kernels)   -- emulator on CPU, real library with -m gpu.

STPP segment assignment, OHEM selection and row routing are exact; floating point within 1e-5 relative
for single ops and 1e-4 relative (the north-star tolerance) for the end-to-end SSN logits / losses.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import action_detection_amd  # noqa: F401
import ssn_oracle as O
from action_detection_amd.ops import ssn_ops as P
from conftest import GOLDEN
from test_kernels import rel_err


def load(name):
    """A fixture; one that oracle/make_golden.py split into <stem>.npz, <stem>_2.npz, ... (save_parts) is read back whole."""
    stem = os.path.join(GOLDEN, name[:-len(".npz")])
    g, k = dict(np.load(stem + ".npz", allow_pickle=False)), 2
    while os.path.exists("%s_%d.npz" % (stem, k)):
        g.update(np.load("%s_%d.npz" % (stem, k), allow_pickle=False))
        k += 1
    return g


# ----------------------------------------------------------------------------- (a) oracle vs reference
def test_oracle_stpp_matches_reference():
    g = load("ref_stpp.npz")
    for ci in range(4):
        cfg = eval(str(g["c%d_cfg" % ci]))
        split = [int(v) for v in g["c%d_split" % ci]]
        ft = torch.from_numpy(g["c%d_ft" % ci]).requires_grad_()
        act, stpp = O.stpp_forward(ft, torch.from_numpy(g["c%d_sc" % ci]), split, cfg, True)
        assert rel_err(act, torch.from_numpy(g["c%d_act" % ci])) < 1e-6
        assert rel_err(stpp, torch.from_numpy(g["c%d_stpp" % ci])) < 1e-6
        ((act * torch.from_numpy(g["c%d_ga" % ci])).sum() + (stpp * torch.from_numpy(g["c%d_gs" % ci])).sum()).backward()
        assert rel_err(ft.grad, torch.from_numpy(g["c%d_dft" % ci])) < 1e-6
    for row in g["ticks_kat"]:
        length, n_part = int(row[0]), int(row[1])
        want = [int(v) for v in row[2:] if v >= 0]
        assert O.stage_ticks(length, n_part) == want, (length, n_part)       # index-exact
        assert P._stage_ticks(length, n_part) == want, (length, n_part)      # host side of the product


def test_oracle_losses_match_reference():
    g = load("ref_losses.npz")
    for ci in range(2):
        pred = torch.from_numpy(g["comp%d_pred" % ci])
        loss, grad = O.completeness_loss(pred, g["comp%d_labels" % ci], 1, 7)
        assert abs(loss - g["comp%d_loss" % ci][0]) < 1e-6 * abs(g["comp%d_loss" % ci][0])
        np.testing.assert_allclose(grad, g["comp%d_grad" % ci], rtol=1e-6, atol=0)
    pred = torch.from_numpy(g["reg_pred"]).requires_grad_()
    loss = O.classwise_regression_loss(pred, torch.from_numpy(g["reg_labels"]), torch.from_numpy(g["reg_targets"]))
    loss.backward()
    assert rel_err(loss.reshape(1), torch.from_numpy(g["reg_loss"]).reshape(1)) < 1e-6
    assert rel_err(pred.grad, torch.from_numpy(g["reg_grad"])) < 1e-6
    loss, grad = O.ohem_hinge(torch.from_numpy(g["ohem_pred"]), g["ohem_labels"], -1, 0.5, 4)
    assert abs(loss - g["ohem_loss"][0]) < 1e-6 * abs(g["ohem_loss"][0])
    np.testing.assert_array_equal(grad, g["ohem_grad"])


def test_oracle_reorg_matches_reference():
    g = load("ref_reorg.npz")
    for ci, cfg in enumerate(((1, 1, 1), (1, (1, 2), 1))):
        a, c, r = O.stpp_reorganized(g["r%d_scores" % ci], g["r%d_ticks" % ci], g["r%d_scaling" % ci], 21, 20, 40, cfg)
        for got, key in ((a, "act"), (c, "comp"), (r, "reg")):
            assert rel_err(torch.from_numpy(got), torch.from_numpy(g["r%d_%s" % (ci, key)])) < 1e-6


def _build_pair(tag, cls, size=32):
    from action_detection_amd.synthetic import init_backbone_synthetic, init_heads_synthetic, make_batch
    modality, cfg = ("RGB", (1, 1, 1)) if tag == "rgb" else ("Flow", (1, (1, 2), 1))
    torch.manual_seed(0)
    m = cls(20, 2, 5, 2, modality, dropout=0, stpp_cfg=cfg)
    init_backbone_synthetic(m.base_model)
    init_heads_synthetic(m)
    m.train()
    return m, make_batch(2, modality, 20, seed=3, input_size=size)


@pytest.mark.parametrize("tag", ["rgb", "flow"])
def test_oracle_ssn_matches_reference(tag):
    """Whole SSN wiring (heads, row selection, losses, grads, test_fc folding) of the restatement."""
    g = load("ref_ssn.npz")
    m, batch = _build_pair(tag, O.OracleSSN)
    out = m(*batch)
    for i, t in enumerate(out):
        assert rel_err(t.float(), torch.from_numpy(g["%s_out%d" % (tag, i)]).float()) < 1e-6, i
    total, a, c, r = O.ssn_total_loss(out, 2)
    np.testing.assert_allclose([a.item(), c.item(), r.item(), total.item()], g["%s_losses" % tag], rtol=1e-6)
    total.backward()
    grads = dict((n, p.grad) for n, p in m.named_parameters() if p.grad is not None)
    names = [str(n) for n in g["%s_grad_names" % tag]]
    assert sorted(names) == sorted(grads)
    for n, (norm, s) in zip(names, g["%s_grad_stats" % tag]):
        assert abs(float(grads[n].double().norm()) - norm) <= 1e-5 * norm + 1e-12, n
    assert rel_err(m.activity_fc.weight.grad, torch.from_numpy(g["%s_grad_act_w" % tag])) < 1e-5
    assert rel_err(m.base_model.inception_5b_1x1.weight.grad, torch.from_numpy(g["%s_grad_5b_1x1_w" % tag])) < 1e-5
    assert sorted(m.state_dict().keys()) == [str(k) for k in g["%s_state_keys" % tag]]
    m.test_mode = True
    m.prepare_test_fc()
    m.eval()
    size = batch[0].shape[-1]
    frames = batch[0].reshape(-1, batch[0].shape[1] // 72, size, size)[:12]
    with torch.no_grad():
        scores, base = m(frames)
    assert rel_err(scores, torch.from_numpy(g["%s_test_scores" % tag])) < 1e-6
    assert rel_err(base, torch.from_numpy(g["%s_test_base" % tag])) < 1e-6


# ----------------------------------------------------------------------------- (b) product ops vs reference
def test_product_stpp_matches_reference(backend):
    g = load("ref_stpp.npz")
    for ci in range(4):
        cfg = eval(str(g["c%d_cfg" % ci]))
        split = [int(v) for v in g["c%d_split" % ci]]
        mod = P.StructuredTemporalPyramidPooling(16, True, configs=cfg)
        # index-exact segment assignment: the part table equals the oracle's (which equals the reference)
        assert mod.part_table(tuple(split)) == O.stpp_part_table(split, cfg)
        ft = backend.put(torch.from_numpy(g["c%d_ft" % ci])).requires_grad_()
        act, stpp = mod(ft, backend.put(torch.from_numpy(g["c%d_sc" % ci])), split)
        assert rel_err(act, torch.from_numpy(g["c%d_act" % ci])) < 1e-6
        assert rel_err(stpp, torch.from_numpy(g["c%d_stpp" % ci])) < 1e-6
        torch.autograd.backward([act, stpp], [backend.put(torch.from_numpy(g["c%d_ga" % ci])),
                                              backend.put(torch.from_numpy(g["c%d_gs" % ci]))])
        assert rel_err(ft.grad, torch.from_numpy(g["c%d_dft" % ci])) < 1e-6


def test_product_losses_match_reference(backend):
    g = load("ref_losses.npz")
    for ci in range(2):
        pred = backend.put(torch.from_numpy(g["comp%d_pred" % ci])).requires_grad_()
        loss = P.CompletenessLoss()(pred, backend.put(torch.from_numpy(g["comp%d_labels" % ci])), 1, 7)
        loss.backward()
        assert rel_err(loss, torch.from_numpy(g["comp%d_loss" % ci])) < 1e-6
        got, want = pred.grad.cpu().numpy(), g["comp%d_grad" % ci]
        assert np.array_equal(got != 0, want != 0), "OHEM kept a different row set"     # exact selection
        np.testing.assert_allclose(got, want, rtol=1e-6)
    pred = backend.put(torch.from_numpy(g["reg_pred"])).requires_grad_()
    loss = P.ClassWiseRegressionLoss()(pred, backend.put(torch.from_numpy(g["reg_labels"])),
                                       backend.put(torch.from_numpy(g["reg_targets"])))
    loss.backward()
    assert rel_err(loss.reshape(1), torch.from_numpy(g["reg_loss"]).reshape(1)) < 1e-6
    assert rel_err(pred.grad, torch.from_numpy(g["reg_grad"])) < 1e-6
    pred = backend.put(torch.from_numpy(g["ohem_pred"])).requires_grad_()
    loss = P.OHEMHingeLoss.apply(pred, backend.put(torch.from_numpy(g["ohem_labels"])), -1, 0.5, 4)
    loss.backward()
    assert rel_err(loss, torch.from_numpy(g["ohem_loss"])) < 1e-6
    assert np.array_equal(pred.grad.cpu().numpy(), g["ohem_grad"])


def test_objective_in_one_launch_matches_the_reference_losses(backend):
    """[r6] ops.ssn_ops.SSNObjective on the reference-generated loss fixtures: its completeness / regression components equal the
    reference's own CompletenessLoss / ClassWiseRegressionLoss values (fixture), the activity component torch's CrossEntropyLoss, the
    total the driver's mix (ssn_train.py:210-214), gradients those of the separate criterions -- with and without the regression head
    (ssn_models.py:288-289), with weights other than the defaults, and with a data-parallel share of the denominator."""
    g = load("ref_losses.npz")
    rng = np.random.RandomState(3)
    comp = torch.from_numpy(g["comp0_pred"])
    comp_t = torch.from_numpy(g["comp0_labels"])
    reg, reg_lbl, reg_t = torch.from_numpy(g["reg_pred"]), torch.from_numpy(g["reg_labels"]), torch.from_numpy(g["reg_targets"])
    act = torch.from_numpy(rng.standard_normal((2 * comp.shape[0] // 7, 21)).astype(np.float32) * 2)
    act_t = torch.from_numpy(rng.randint(0, 21, size=act.shape[0]).astype(np.int64))
    ce = F.cross_entropy(act.double(), act_t).item()
    for with_reg, (wc, wr), rows in ((True, (0.1, 0.1), None), (False, (0.1, 0.1), None), (True, (0.3, 0.7), None),
                                     (True, (0.1, 0.1), 4 * comp.shape[0])):
        leaves = [backend.put(t.clone()).requires_grad_() for t in (act, comp, reg)]
        obj = P.SSNObjective(wc, wr)
        args = [leaves[0], backend.put(act_t), leaves[1], backend.put(comp_t)]
        if with_reg:
            args += [leaves[2], backend.put(reg_lbl), backend.put(reg_t)]
        total = obj(*args, sample_split=1, sample_group_size=7, global_rows=rows)
        parts = obj.parts.cpu().double()
        assert abs(parts[0].item() - ce) < 1e-6 * max(1.0, abs(ce))
        if rows is None:
            assert rel_err(parts[1].reshape(1), torch.from_numpy(g["comp0_loss"]).reshape(1)) < 1e-6
        if with_reg:
            assert rel_err(parts[2].reshape(1), torch.from_numpy(g["reg_loss"]).reshape(1)) < 1e-6
        else:
            assert parts[2].item() == 0.0
        want = parts[0] + wc * parts[1] + (wr * parts[2] if with_reg else 0.0)
        assert abs(total.item() - want.item()) < 2e-7 * max(1.0, abs(want.item()))
        total.backward()
        sep = [backend.put(t.clone()).requires_grad_() for t in (act, comp, reg)]
        ref_total = P.ActivityLoss()(sep[0], backend.put(act_t)) + wc * P.CompletenessLoss()(sep[1], backend.put(comp_t), 1, 7, global_rows=rows)
        if with_reg:
            ref_total = ref_total + wr * P.ClassWiseRegressionLoss()(sep[2], backend.put(reg_lbl), backend.put(reg_t))
        ref_total.backward()
        for k in range(3 if with_reg else 2):
            assert rel_err(leaves[k].grad, sep[k].grad) < 1e-6, (with_reg, wc, wr, rows, k)
        if rows is None and (wc, wr) == (0.1, 0.1):
            assert np.array_equal(leaves[1].grad.cpu().numpy() != 0, g["comp0_grad"] != 0), "OHEM kept a different row set"
        assert leaves[2].grad is None or with_reg


def test_product_reorg_matches_reference(backend):
    g = load("ref_reorg.npz")
    for ci, cfg in enumerate(((1, 1, 1), (1, (1, 2), 1))):
        scores = g["r%d_scores" % ci]
        mod = P.STPPReorgainzed(scores.shape[1], 21, 20, 40, True, True, stpp_cfg=cfg)
        a, c, r = mod.forward(backend.put(torch.from_numpy(scores)), torch.from_numpy(g["r%d_ticks" % ci]),
                              g["r%d_scaling" % ci])
        for got, key in ((a, "act"), (c, "comp"), (r, "reg")):
            assert rel_err(got, torch.from_numpy(g["r%d_%s" % (ci, key)])) < 1e-6, key
    # [r6] without the stand-alone activity classifier: the activity scores pooled by stages and parts (ops/ssn_ops.py:160-161)
    scores = g["r2_scores"]
    mod = P.STPPReorgainzed(scores.shape[1], 21, 20, 40, False, True, stpp_cfg=(1, (1, 2), 1))
    a, c, r = mod.forward(backend.put(torch.from_numpy(scores)), torch.from_numpy(g["r2_ticks"]), g["r2_scaling"])
    for got, key in ((a, "act"), (c, "comp"), (r, "reg")):
        assert rel_err(got, torch.from_numpy(g["r2_%s" % key])) < 1e-6, key
    want = O.stpp_reorganized(scores, g["r2_ticks"], g["r2_scaling"], 21, 20, 40, stpp_cfg=(1, (1, 2), 1), standalone_classifier=False)
    for w_, key in zip(want, ("act", "comp", "reg")):
        np.testing.assert_allclose(w_, g["r2_%s" % key], rtol=1e-5, atol=1e-6)      # (the oracle against the reference's own class)


def _product_vs_golden(tag, device):
    from action_detection_amd.ssn_models import SSN
    g = load("ref_ssn.npz")
    m, batch = _build_pair(tag, SSN)
    m.to(device)
    out = m(*[t.to(device) for t in batch])
    for i, t in enumerate(out):
        want = torch.from_numpy(g["%s_out%d" % (tag, i)])
        if i % 2 == 1 or i == 6:
            assert torch.equal(t.cpu(), want), i                        # labels / targets: exact routing
        else:
            assert rel_err(t, want) < 1e-4, i                           # logits: north-star tolerance
    a = P.ActivityLoss()(out[0], out[1])
    c = P.CompletenessLoss()(out[2], out[3], 1, 7)
    r = P.ClassWiseRegressionLoss()(out[4], out[5], out[6])
    total = a + 0.1 * c + 0.1 * r
    np.testing.assert_allclose([a.item(), c.item(), r.item(), total.item()], g["%s_losses" % tag], rtol=1e-4)
    total.backward()
    grads = dict((n, p.grad) for n, p in m.named_parameters() if p.grad is not None)
    # [r6] the one-launch objective (ops.ssn_ops.SSNObjective): same loss bodies -> bit-identical components, the total within one
    # rounding of the Python mix (0.1 is a double there, a float in the kernel), the same gradients at the logits
    fresh = [t.detach().clone().requires_grad_() if t.is_floating_point() and i in (0, 2, 4) else t for i, t in enumerate(out)]
    obj = P.SSNObjective()
    tot2 = obj(*fresh)
    assert torch.equal(obj.parts.cpu(), torch.stack([a.detach().reshape(()), c.detach().reshape(()), r.detach().reshape(())]).cpu())
    assert abs(tot2.item() - total.item()) <= 2e-7 * abs(total.item())
    tot2.backward()
    sep = [t.detach().clone().requires_grad_() for t in (out[0], out[2], out[4])]
    (P.ActivityLoss()(sep[0], out[1]) + 0.1 * P.CompletenessLoss()(sep[1], out[3], 1, 7) + 0.1 * P.ClassWiseRegressionLoss()(sep[2], out[5], out[6])).backward()
    for f_, s_ in zip((fresh[0], fresh[2], fresh[4]), sep):
        assert rel_err(f_.grad, s_.grad) < 1e-6
    # gradient norms, as a distribution.  The loss is only piecewise smooth: a ReLU unit whose pre-activation is within
    # rounding of zero takes different branches in two fp32 implementations, and at 32^2 -- the 7x7-stage planes are
    # single pixels -- one such unit moves a whole tensor by 1e-3..1e-2 (profiles/r2_grad_flip_diag.txt: the reference's
    # own fp32 CPU path is 2.4e-3 off float64 on one tensor at 224^2).  Which units flip is an accident of rounding; a
    # wiring error moves the bulk.  So: the median within 3e-4, at most 5 % of the tensors beyond 3e-3, none beyond 3e-2.
    names = [str(x) for x in g["%s_grad_names" % tag]]
    e = torch.tensor([abs(float(grads[n].double().norm()) - norm) / (norm + 1e-12)
                      for n, (norm, s) in zip(names, g["%s_grad_stats" % tag])])
    assert e.median() < 3e-4 and e.max() < 3e-2 and int((e > 3e-3).sum()) <= max(3, len(e) // 20), (e.median(), e.max())
    # element-wise gradients: 5e-3 for the deepest chain (conv1: ~60 fp32 reductions in a different order on
    # each side; tests/test_model_gpu.py referees such differences against float64), 1e-3 / 1e-4 near the loss
    assert rel_err(m.base_model.conv1_7x7_s2.bias.grad, torch.from_numpy(g["%s_grad_conv1_b" % tag])) < 5e-3
    assert rel_err(m.base_model.inception_5b_1x1.weight.grad, torch.from_numpy(g["%s_grad_5b_1x1_w" % tag])) < 1e-3
    assert rel_err(m.activity_fc.weight.grad, torch.from_numpy(g["%s_grad_act_w" % tag])) < 1e-4
    pol = m.get_optim_policies()
    assert [[len(x["params"]), sum(p.numel() for p in x["params"])] for x in pol] == g["%s_policy_sizes" % tag].tolist()
    assert sorted(m.state_dict().keys()) == [str(k) for k in g["%s_state_keys" % tag]]
    m.test_mode = True
    m.prepare_test_fc()
    m.eval()
    size = batch[0].shape[-1]
    frames = batch[0].reshape(-1, batch[0].shape[1] // 72, size, size)[:12].to(device)
    with torch.no_grad():
        scores, base = m(frames)
    assert rel_err(scores, torch.from_numpy(g["%s_test_scores" % tag])) < 1e-4
    assert rel_err(base, torch.from_numpy(g["%s_test_base" % tag])) < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["rgb", "flow"])
def test_product_ssn_matches_reference_gpu(tag, hip_library):
    """Full SSN (144 frames of 32x32 through all 69 convs) on the MI355X vs the reference's own numbers."""
    _product_vs_golden(tag, "cuda:0")


@pytest.mark.slow_emu
@pytest.mark.skipif(os.environ.get("SSN_SLOW") != "1", reason="~10 min through the host emulator; set SSN_SLOW=1")
def test_product_ssn_matches_reference_emulated(emu):
    _product_vs_golden("rgb", "cpu")


def test_sharded_completeness_loss_averages_to_the_gathered_loss(backend):
    """Data parallelism: per-rank CompletenessLoss(global_rows=) averaged over the ranks -- what
    the gradient all-reduce does -- equals the reference loss on the gathered batch, values and gradients; V = 100
    videos is a case where the global int() truncation differs from the sum of the per-rank ones."""
    rng = np.random.RandomState(5)
    # (32, 8) = BASELINE.json configs[3]: 4 videos per GPU on 8 GPUs, denominator V + int(6 V 0.17) = 32 + 32
    for v, world in ((4, 2), (100, 4), (32, 8)):
        c = 20
        assert int(6 * v * 0.17) == {4: 4, 100: 102, 32: 32}[v]
        pred = torch.from_numpy((rng.standard_normal((7 * v, c)) * 1.5).astype(np.float32))
        labels = torch.from_numpy(rng.randint(1, c + 1, size=7 * v).astype(np.int64))
        full_loss, full_grad = O.completeness_loss(pred, labels.numpy(), 1, 7)
        per = v // world
        tot, grads = 0.0, []
        for r in range(world):
            p = backend.put(pred[7 * per * r:7 * per * (r + 1)].clone()).requires_grad_()
            l = P.CompletenessLoss()(p, backend.put(labels[7 * per * r:7 * per * (r + 1)]), 1, 7, global_rows=7 * v)
            l.backward()
            tot += float(l) / world
            grads.append(p.grad.cpu() / world)
        assert abs(tot - float(full_loss)) < 1e-6 * max(1.0, abs(float(full_loss)))
        assert np.allclose(torch.cat(grads).numpy(), full_grad, rtol=1e-5, atol=1e-8)


# ---------------------------------------------------------------------------------------------------------------------
# bn_mode 'partial' / 'full' (/root/reference/ssn_models.py:95-105,156-174): fixture ref_ssn_bn.npz from the reference's
# own SSN class -- outputs, losses, every gradient norm (BatchNorm gamma / beta included), running statistics after one
# training forward, which BatchNorm2d modules stay in training mode, optimiser groups.
def _bn_pair(mode, cls):
    from action_detection_amd.synthetic import init_backbone_synthetic, init_heads_synthetic, make_batch
    torch.manual_seed(0)
    m = cls(20, 2, 5, 2, "RGB", dropout=0, stpp_cfg=(1, 1, 1), bn_mode=mode)
    init_backbone_synthetic(m.base_model)
    init_heads_synthetic(m)
    m.train()
    return m, make_batch(2, "RGB", 20, seed=3, input_size=32)


def _grad_norm_errors(grads, names, stats):
    return torch.tensor([abs(float(grads[n].double().norm()) - norm) / (norm + 1e-12) for n, (norm, _) in zip(names, stats)])


@pytest.mark.parametrize("mode", ["partial", "full"])
def test_oracle_bn_modes_match_reference(mode):
    g = load("ref_ssn_bn.npz")
    m, batch = _bn_pair(mode, O.OracleSSN)
    training = [n for n, mod in m.base_model.named_modules() if isinstance(mod, torch.nn.BatchNorm2d) and mod.training]
    assert training == [str(x) for x in g["%s_training_bn" % mode]]
    out = m(*batch)
    for i, t in enumerate(out):
        assert rel_err(t.float(), torch.from_numpy(g["%s_out%d" % (mode, i)]).float()) < 1e-6, i
    total, a, c, r = O.ssn_total_loss(out, 2)
    np.testing.assert_allclose([a.item(), c.item(), r.item(), total.item()], g["%s_losses" % mode], rtol=1e-6)
    total.backward()
    grads = dict((n, p.grad) for n, p in m.named_parameters() if p.grad is not None)
    names = [str(n) for n in g["%s_grad_names" % mode]]
    assert sorted(names) == sorted(grads)
    assert _grad_norm_errors(grads, names, g["%s_grad_stats" % mode]).max() < 1e-4
    bn1 = m.base_model.conv1_7x7_s2_bn
    assert rel_err(bn1.running_mean, torch.from_numpy(g["%s_bn1_running_mean" % mode])) < 1e-6
    assert rel_err(bn1.running_var, torch.from_numpy(g["%s_bn1_running_var" % mode])) < 1e-6


def _product_bn_vs_golden(mode, device):
    from action_detection_amd.ssn_models import SSN
    g = load("ref_ssn_bn.npz")
    m, batch = _bn_pair(mode, SSN)
    m.to(device)
    training = [n for n, mod in m.base_model.named_modules() if isinstance(mod, torch.nn.BatchNorm2d) and mod.training]
    assert training == [str(x) for x in g["%s_training_bn" % mode]]
    out = m(*[t.to(device) for t in batch])
    for i, t in enumerate(out):
        want = torch.from_numpy(g["%s_out%d" % (mode, i)])
        if i % 2 == 1 or i == 6:
            assert torch.equal(t.cpu(), want), i
        else:
            assert rel_err(t, want) < 1e-4, (i, rel_err(t, want))                 # logits: north-star tolerance
    a = P.ActivityLoss()(out[0], out[1])
    c = P.CompletenessLoss()(out[2], out[3], 1, 7)
    r = P.ClassWiseRegressionLoss()(out[4], out[5], out[6])
    total = a + 0.1 * c + 0.1 * r
    np.testing.assert_allclose([a.item(), c.item(), r.item(), total.item()], g["%s_losses" % mode], rtol=1e-4)
    total.backward()
    bn1, bn5 = m.base_model.conv1_7x7_s2_bn, m.base_model.inception_5b_1x1_bn
    assert rel_err(bn1.running_mean, torch.from_numpy(g["%s_bn1_running_mean" % mode])) < 1e-5
    assert rel_err(bn1.running_var, torch.from_numpy(g["%s_bn1_running_var" % mode])) < 1e-5
    assert rel_err(bn5.running_mean, torch.from_numpy(g["%s_bn5b_running_mean" % mode])) < 1e-4
    assert rel_err(bn5.running_var, torch.from_numpy(g["%s_bn5b_running_var" % mode])) < 1e-4
    assert [int(bn1.num_batches_tracked), int(bn5.num_batches_tracked)] == g["%s_bn1_batches" % mode].tolist()
    grads = dict((n, p.grad) for n, p in m.named_parameters() if p.grad is not None)
    names = [str(n) for n in g["%s_grad_names" % mode]]
    assert sorted(names) == sorted(grads)
    # The bias of a convolution in front of a training-mode BatchNorm has an exactly zero gradient (the batch mean absorbs
    # it); both sides hold rounding noise there -- checked against the weight gradient's size, not against each other.
    training_convs = [n[:-len("_bn")] for n in training]
    stats = g["%s_grad_stats" % mode]
    keep = [i for i, n in enumerate(names) if not any(n == "base_model.%s.bias" % c for c in training_convs)]
    for c in training_convs:
        gb, gw = grads["base_model.%s.bias" % c], grads["base_model.%s.weight" % c]
        assert float(gb.double().norm()) < 1e-4 * float(gw.double().norm()) + 1e-12, c
    names, stats = [names[i] for i in keep], stats[keep]
    # gradient norms as a distribution (ReLU sign flips, see _product_vs_golden): the bulk within 1e-3, every tensor within 3e-2
    e = _grad_norm_errors(grads, names, stats)
    assert e.median() < 1e-3 and e.max() < 3e-2 and int((e > 5e-3).sum()) <= max(3, len(e) // 20), (e.median(), e.max())
    assert rel_err(bn1.weight.grad, torch.from_numpy(g["%s_bn1_dgamma" % mode])) < 3e-2      # (element-wise: see below)
    assert rel_err(bn1.bias.grad, torch.from_numpy(g["%s_bn1_dbeta" % mode])) < 3e-2
    # (element-wise, the deepest chain at 32^2: the same ReLU-flip sensitivity as the norms above, hence their 3e-2 cap)
    assert rel_err(m.base_model.conv1_7x7_s2.weight.grad, torch.from_numpy(g["%s_conv1_dw" % mode])) < 3e-2
    pol = m.get_optim_policies()
    assert [[len(x["params"]), sum(p.numel() for p in x["params"])] for x in pol] == g["%s_policy_sizes" % mode].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["partial", "full"])
def test_product_bn_modes_match_reference_gpu(mode, hip_library):
    _product_bn_vs_golden(mode, "cuda:0")


@pytest.mark.slow_emu
@pytest.mark.skipif(os.environ.get("SSN_SLOW") != "1", reason="~10 min through the host emulator; set SSN_SLOW=1")
@pytest.mark.parametrize("mode", ["partial", "full"])
def test_product_bn_modes_match_reference_emulated(mode, emu):
    _product_bn_vs_golden(mode, "cpu")


# ---------------------------------------------------------------------------------------------------------------------
# RGBDiff modality (/root/reference/ssn_models.py:302-316,345-376): fixture ref_ssn_rgbdiff.npz from the reference's own
# class (its Python-2 `filter(...)[0]` shimmed, oracle/make_golden.py).
def _rgbdiff_pair(cls):
    from action_detection_amd.synthetic import init_backbone_synthetic, init_heads_synthetic, make_batch
    torch.manual_seed(0)
    m = cls(20, 2, 5, 2, "RGBDiff", dropout=0, stpp_cfg=(1, 1, 1))
    init_backbone_synthetic(m.base_model)
    init_heads_synthetic(m)
    m.train()
    return m, make_batch(2, "RGBDiff", 20, seed=3, input_size=32)


def test_oracle_rgbdiff_matches_reference():
    g = load("ref_ssn_rgbdiff.npz")
    m, batch = _rgbdiff_pair(O.OracleSSN)
    assert list(m.base_model.conv1_7x7_s2.weight.shape) == g["conv1_weight_shape"].tolist() == [64, 15, 7, 7]
    out = m(*batch)
    for i, t in enumerate(out):
        assert rel_err(t.float(), torch.from_numpy(g["out%d" % i]).float()) < 1e-6, i
    total, a, c, r = O.ssn_total_loss(out, 2)
    np.testing.assert_allclose([a.item(), c.item(), r.item(), total.item()], g["losses"], rtol=1e-6)
    total.backward()
    grads = dict((n, p.grad) for n, p in m.named_parameters() if p.grad is not None)
    names = [str(n) for n in g["grad_names"]]
    assert sorted(names) == sorted(grads)
    assert _grad_norm_errors(grads, names, g["grad_stats"]).max() < 1e-4


def test_frame_diff_kernel(backend):
    """ssn_frame_diff == SSN._get_diff of the reference (bit-exact: one fp32 subtraction per element)."""
    g = load("ref_ssn_rgbdiff.npz")
    from action_detection_amd import kernels as K
    from action_detection_amd.synthetic import make_batch
    x = make_batch(2, "RGBDiff", 20, seed=3, input_size=32)[0]
    d = K.frame_diff(backend.put(x), 5, 3)
    assert tuple(d.shape) == (2 * 8 * 9, 15, 32, 32)
    assert torch.equal(d[:3].cpu(), torch.from_numpy(g["diff_sample"]))
    v = x.reshape(-1, 9, 6, 3, 32, 32)
    assert torch.equal(d.cpu(), (v[:, :, 1:] - v[:, :, :-1]).reshape(-1, 15, 32, 32))


def _product_rgbdiff_vs_golden(device):
    from action_detection_amd.ssn_models import SSN
    g = load("ref_ssn_rgbdiff.npz")
    m, batch = _rgbdiff_pair(SSN)
    assert list(m.base_model.conv1_7x7_s2.weight.shape) == [64, 15, 7, 7] and list(m.input_mean) == g["input_mean"].tolist()
    assert sorted(m.state_dict().keys()) == [str(k) for k in g["state_keys"]]
    m.to(device)
    out = m(*[t.to(device) for t in batch])
    for i, t in enumerate(out):
        want = torch.from_numpy(g["out%d" % i])
        if i % 2 == 1 or i == 6:
            assert torch.equal(t.cpu(), want), i
        else:
            assert rel_err(t, want) < 1e-4, (i, rel_err(t, want))
    a = P.ActivityLoss()(out[0], out[1])
    c = P.CompletenessLoss()(out[2], out[3], 1, 7)
    r = P.ClassWiseRegressionLoss()(out[4], out[5], out[6])
    total = a + 0.1 * c + 0.1 * r
    np.testing.assert_allclose([a.item(), c.item(), r.item(), total.item()], g["losses"], rtol=1e-4)
    total.backward()
    grads = dict((n, p.grad) for n, p in m.named_parameters() if p.grad is not None)
    names = [str(n) for n in g["grad_names"]]
    e = _grad_norm_errors(grads, names, g["grad_stats"])
    assert e.median() < 3e-4 and e.max() < 3e-2 and int((e > 3e-3).sum()) <= max(3, len(e) // 20), (e.median(), e.max())
    assert rel_err(m.base_model.conv1_7x7_s2.weight.grad, torch.from_numpy(g["conv1_dw"])) < 5e-3


@pytest.mark.gpu
def test_product_rgbdiff_matches_reference_gpu(hip_library):
    _product_rgbdiff_vs_golden("cuda:0")


@pytest.mark.slow_emu
@pytest.mark.skipif(os.environ.get("SSN_SLOW") != "1", reason="~10 min through the host emulator; set SSN_SLOW=1")
def test_product_rgbdiff_matches_reference_emulated(emu):
    _product_rgbdiff_vs_golden("cpu")


def test_product_reorg_clamps_range_ends_like_python_slices(backend):
    """A proposal whose ticks run past the last score row: the reference's ``raw_scores[pl:pr]`` (ops/ssn_ops.py:149,157)
    clamps the END of the slice to the rows that exist, and a slice that starts past the last row is empty (mean = NaN); so
    does the product (negative starts, which Python would count from the end, raise)."""
    rng = np.random.RandomState(5)
    t, cfg = 40, (1, (1, 2), 1)
    mod = P.STPPReorgainzed(21 + 20 * 5 + 40 * 5, 21, 20, 40, True, True, stpp_cfg=cfg)
    scores = rng.standard_normal((t, mod.feat_dim)).astype(np.float32)
    ticks = np.array([[30, 34, 39, 47], [20, 36, 44, 52], [0, 3, 9, 12]], np.int64)     # ends beyond row 40
    scaling = rng.uniform(0, 1, (3, 2))
    want = O.stpp_reorganized(scores, ticks, scaling, 21, 20, 40, stpp_cfg=cfg)
    got = mod.forward(backend.put(torch.from_numpy(scores)), torch.from_numpy(ticks), scaling)
    for g_, w_ in zip(got, want):
        g_, w_ = g_.cpu().numpy(), np.asarray(w_)
        assert np.array_equal(np.isnan(g_), np.isnan(w_))
        np.testing.assert_allclose(np.nan_to_num(g_), np.nan_to_num(w_), rtol=1e-5, atol=1e-6)
    assert np.isnan(want[1][1]).any() and not np.isnan(want[1][0]).any()      # second proposal: a part starts at row 40 = T
    with pytest.raises(IndexError):
        mod.forward(backend.put(torch.from_numpy(scores)), torch.from_numpy(np.array([[-3, 1, 4, 7]], np.int64)), scaling[:1])
