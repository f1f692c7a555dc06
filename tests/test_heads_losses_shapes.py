"""The kernels behind the backbone (csrc/heads_losses.hip, csrc/stpp.hip) at the shapes the product runs and at the edges where
such kernels go wrong: STPP, the fused heads and the chain of separate kernels they replace, the three losses and the objective in
one launch, the label selection, the re-organised STPP of dense testing, crop_mean / reg_denorm.

Every case runs through the host emulator (CPU tier) and, with ``-m gpu``, through the gfx950 library.  The emulator cases may use
fewer proposals than the GPU ones, never a smaller feature width, class count or part count.  References are float64 torch or the
oracle (oracle/ssn_oracle.py); integer decisions (part boundaries, OHEM selection, row routing) are exact.

Bounds.  Heads: fused against separate 1e-6, either against float64 2e-6 (those of test_fused_heads_match_the_separate_kernels).
Completeness loss 1e-6, kept rows exact, gradient rtol 1e-6 (those of test_product_losses_match_reference).  Cross entropy: loss 1e-6
relative with a floor of 1e-6 absolute, gradient 5e-6 (fp32 expf).  Re-organised STPP 1e-6 / allclose(1e-5, 1e-6) (those of
test_product_reorg_matches_reference).  The class-wise smooth-L1 bound is derived where it is used."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import action_detection_amd  # noqa: F401
import ssn_oracle as O
from action_detection_amd import functional as FN
from action_detection_amd import kernels as K
from action_detection_amd.ops import ssn_ops as P
from test_kernels import heads_float64, rel_err

STD_TYPES = (0, 1, 1, 1, 1, 1, 1, 2)      # one video of the sampler: 1 foreground, 6 incomplete, 1 background proposal


def err(a, b):
    """rel_err for tensors that may be empty (a head that nobody selected); shapes must agree."""
    assert tuple(a.shape) == tuple(b.shape), (tuple(a.shape), tuple(b.shape))
    return rel_err(a, b) if a.numel() else 0.0


def misaligned(t, backend):
    """A contiguous copy of t on the backend's device that starts 4 bytes into its storage (not 8- or 16-byte aligned)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=backend.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def prop_types(pattern, p):
    return torch.tensor([pattern[i % len(pattern)] for i in range(p)])


class HeadsCase:
    """Seeded operands of one (config, D, C, split, P, prop_type) point: features, scaling, weights, biases, row sets, output gradients."""

    def __init__(self, cfg, d, c, split, p, pattern=STD_TYPES, with_reg=True, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.key = (cfg, d, c, split, p, pattern, with_reg)
        self.split, self.n_seg, self.with_reg = split, split[2], with_reg
        self.stpp = P.StructuredTemporalPyramidPooling(d, True, configs=cfg)
        m = self.stpp.feat_multiplier
        self.table = self.stpp.table_for(split)
        self.ft = torch.randn(p * self.n_seg, d, generator=g)
        self.sc = torch.rand(p, 2, generator=g)
        self.ws = [torch.randn(c + 1, d, generator=g) * 0.1, torch.randn(c, m * d, generator=g) * 0.1,
                   torch.randn(2 * c, m * d, generator=g) * 0.1 if with_reg else None]
        self.bs = [torch.randn(c + 1, generator=g), torch.randn(c, generator=g), torch.randn(2 * c, generator=g) if with_reg else None]
        ptype = prop_types(pattern, p)
        sets = ((ptype == 0) | (ptype == 2), (ptype == 0) | (ptype == 1), ptype == 0)      # (ssn_models.py:275-289)
        self.idx = [torch.nonzero(q).reshape(-1) for q in sets]
        self.pos = [(torch.cumsum(q.to(torch.int32), 0, dtype=torch.int32) - 1).masked_fill(~q, -1) for q in sets]
        self.gouts = [torch.randn(i.numel(), w.shape[0], generator=g) if w is not None else None for i, w in zip(self.idx, self.ws)]

    def float64(self):
        return heads_float64(self.ft, self.sc, self.ws, self.bs, self.idx, self.gouts, self.stpp.part_table(self.split), self.split)

    def run(self, backend, fused, shift=()):
        """Outputs, then gradients (features, weights, biases).  shift: names ("ft", "w0", "w1", "w2") of operands to hand over as
        contiguous views that are not 16-byte aligned."""
        def leaf(t, name):
            if t is None:
                return None
            v = misaligned(t, backend) if name in shift else backend.put(t).clone()
            return v.requires_grad_()

        f = leaf(self.ft, "ft")
        w_ = [leaf(t, "w%d" % h) for h, t in enumerate(self.ws)]
        b_ = [leaf(t, "b") for t in self.bs]
        di = [backend.put(t) for t in self.idx]
        sc = backend.put(self.sc)
        if fused:
            dp = [backend.put(t) for t in self.pos]
            if not self.with_reg:
                di, dp = [di[0], di[1], None], [dp[0], dp[1], None]
            outs = FN.HeadsFn.apply(f, sc, self.table, self.n_seg, tuple(di), tuple(dp), w_[0], b_[0], w_[1], b_[1], w_[2], b_[2])
        else:
            a, st = FN.StppFn.apply(f, sc, self.table, self.n_seg)
            full = [FN.LinearFn.apply(a, w_[0], b_[0]), FN.LinearFn.apply(st, w_[1], b_[1]),
                    FN.LinearFn.apply(st, w_[2], b_[2]) if self.with_reg else None]
            outs = [None if o is None else FN.RowGatherFn.apply(o, i) for o, i in zip(full, di)]
        loss = sum((o * backend.put(go)).sum() for o, go in zip(outs, self.gouts) if o is not None)
        loss.backward()
        return [o for o in outs if o is not None] + [t.grad for t in [f] + w_ + b_ if t is not None]


PRODUCT = (1, (1, 2), 1)            # the reference's default STPP configuration: 5 parts
WIDE = ((1, 2), (1, 2, 4), (1, 2))  # 13 parts; with split (4, 12, 16) over the 16 segments the kernels admit
# cfg, D, C, seg_split, P on the GPU, P on the emulator, prop_type pattern, regression head
HEADS_GRID = [
    pytest.param(PRODUCT, 1024, 20, (2, 7, 9), 256, 32, STD_TYPES, True, id="bninception-thumos"),
    pytest.param(PRODUCT, 2048, 200, (2, 7, 9), 256, 8, STD_TYPES, True, id="inceptionv3-activitynet"),      # 101 output chunks, 48 KiB LDS
    pytest.param(PRODUCT, 1000, 20, (2, 7, 9), 64, 8, STD_TYPES, True, id="D1000"),                          # not a multiple of 256
    pytest.param((1, 1, 1), 257, 5, (2, 7, 9), 24, 8, STD_TYPES, True, id="D257-odd"),
    pytest.param(((1, 1), 1, 1), 6, 3, (2, 7, 9), 16, 16, STD_TYPES, True, id="m4-D6"),                      # m * D % 4 == 0, D % 4 != 0
    pytest.param(((1, 1), 1, 1), 7, 3, (2, 7, 9), 16, 16, STD_TYPES, True, id="m4-D7"),
    pytest.param(WIDE, 260, 7, (4, 12, 16), 32, 8, STD_TYPES, True, id="13parts-16segments"),
    pytest.param(WIDE, 1168, 4, (4, 12, 16), 8, 2, (0, 1, 2), True, id="13parts-LDS-brim"),                  # 14 * 1168 * 4 = 65408 of 65536 bytes
    pytest.param(PRODUCT, 1024, 20, (1, 7, 8), 16, 8, STD_TYPES, True, id="single-segment-stages"),
    pytest.param(PRODUCT, 64, 5, (2, 7, 9), 1, 1, (0,), True, id="P1-foreground"),
    pytest.param(PRODUCT, 64, 5, (2, 7, 9), 1, 1, (1,), True, id="P1-incomplete"),                           # activity and regression heads empty
    pytest.param(PRODUCT, 260, 20, (2, 7, 9), 24, 8, (1, 2, 1, 1, 2), True, id="no-foreground"),             # regression head: n = 0
    pytest.param(PRODUCT, 260, 20, (2, 7, 9), 24, 8, (0,), True, id="all-foreground"),
    pytest.param(PRODUCT, 1024, 20, (2, 7, 9), 64, 8, STD_TYPES, False, id="no-regression-head"),
    pytest.param(PRODUCT, 2048, 200, (2, 7, 9), 32, 4, STD_TYPES, False, id="no-regression-head-C200"),
]


@pytest.mark.parametrize("cfg,d,c,split,p_gpu,p_emu,pattern,with_reg", HEADS_GRID)
def test_heads_fused_and_separate_against_float64(backend, cfg, d, c, split, p_gpu, p_emu, pattern, with_reg):
    """functional.HeadsFn and the StppFn + LinearFn + RowGatherFn chain: every output and every gradient (features, three weights, three
    biases) against each other (1e-6) and against float64 torch (2e-6)."""
    case = HeadsCase(cfg, d, c, split, p_gpu if backend.is_gpu else p_emu, pattern, with_reg, seed=d + c)
    fused, chain, ref = case.run(backend, True), case.run(backend, False), case.float64()
    assert len(fused) == len(chain) == len(ref) == (10 if with_reg else 7)
    for k, (a, b, r) in enumerate(zip(fused, chain, ref)):
        figures = (err(a, b), err(a, r), err(b, r))
        print("heads", case.key, "tensor", k, "fused/chain %.2e fused/f64 %.2e chain/f64 %.2e" % figures)
        assert figures[0] < 1e-6 and figures[1] < 2e-6 and figures[2] < 2e-6, (case.key, k, figures)
    if with_reg and case.idx[2].numel() == 0:
        # nobody selected the regression head: its weight and bias gradients are exactly zero, whichever path
        n_out = 3
        for got in (fused, chain):
            assert got[2].shape == (0, 2 * c)
            assert not got[n_out + 3].any() and not got[n_out + 6].any()


def test_heads_and_stpp_refuse_what_the_kernels_cannot_hold(backend):
    """One past each limit of the ABI is an error before any launch: 25 parts, 17 segments per proposal (fused heads), pooled features
    beyond the 64 KiB of LDS of the fused forward."""
    g = torch.Generator().manual_seed(1)
    # 25 parts: refused when the table is made, and by the entry points themselves for a table made by hand
    stpp = P.StructuredTemporalPyramidPooling(8, True, configs=((1, 2, 4), (1, 2, 4, 8), (1, 2)))
    assert stpp.feat_multiplier == 25
    with pytest.raises(ValueError):
        stpp.table_for((8, 16, 24))
    table = K.make_stpp_table(stpp.part_table((8, 16, 24))[:24], 24, 8, 16)
    table.n_parts = 25
    ft, sc = backend.put(torch.randn(2 * 24, 8, generator=g)), backend.put(torch.rand(2, 2, generator=g))
    with pytest.raises(RuntimeError):
        FN.StppFn.apply(ft, sc, table, 24)
    with pytest.raises(RuntimeError):
        K.stpp_bwd(backend.put(torch.zeros(2, 8)), backend.put(torch.zeros(2, 25 * 8)), sc, backend.put(torch.zeros(48, 8)), table)

    def heads(cfg, d, split, table=None):
        case = HeadsCase(cfg, d, 3, split, 2, (0,), True, seed=2)
        if table is not None:
            case.table = table
        return case.run(backend, True)

    with pytest.raises(RuntimeError):
        heads(WIDE, 8, (8, 16, 24), table)      # 25 parts
    # 17 segments: one more than the fused forward keeps in registers
    with pytest.raises(RuntimeError, match="16 segments"):
        heads(PRODUCT, 8, (4, 13, 17))
    assert len(heads(PRODUCT, 8, (4, 12, 16))) == 10
    # (1 + 5) * 2732 * 4 = 65568 bytes > 65536; 2730 (65520 bytes) is the last width that fits
    with pytest.raises(RuntimeError, match="LDS"):
        heads(PRODUCT, 2732, (2, 7, 9))
    got, ref = heads(PRODUCT, 2730, (2, 7, 9)), HeadsCase(PRODUCT, 2730, 3, (2, 7, 9), 2, (0,), True, seed=2).float64()
    for a, r in zip(got, ref):
        assert err(a, r) < 2e-6


STPP_GRID = [
    (PRODUCT, 1024, (2, 7, 9), 256, 32), (PRODUCT, 2048, (2, 7, 9), 256, 16), (PRODUCT, 1000, (2, 7, 9), 64, 8),
    ((1, 1, 1), 257, (2, 7, 9), 24, 8), (((1, 1), 1, 1), 6, (2, 7, 9), 16, 16), (WIDE, 260, (4, 12, 16), 32, 8),
    (PRODUCT, 1024, (1, 7, 8), 16, 8), ((1, 1, 1), 33, (1, 7, 8), 5, 5), ((1, (1, 2, 4), 1), 130, (2, 9, 11), 9, 9),
    (((1, 2, 4), (1, 2, 4, 8), 1), 12, (8, 16, 24), 3, 3),      # 23 parts over 24 segments (STPP alone has no segment limit)
    (PRODUCT, 64, (2, 7, 9), 1, 1),
]


@pytest.mark.parametrize("standalong", [True, False])
@pytest.mark.parametrize("cfg,d,split,p_gpu,p_emu", STPP_GRID)
def test_stpp_against_float64_and_the_oracle(backend, cfg, d, split, p_gpu, p_emu, standalong):
    """StructuredTemporalPyramidPooling (ssn_stpp_fwd / ssn_stpp_bwd): the part table equals the oracle's, values and the feature
    gradient equal the oracle's evaluated in float64 -- with and without the stand-alone classifier feature."""
    p = p_gpu if backend.is_gpu else p_emu
    g = torch.Generator().manual_seed(7 + d)
    mod = P.StructuredTemporalPyramidPooling(d, standalong, configs=cfg)
    assert mod.part_table(split) == O.stpp_part_table(split, cfg)
    ft, sc = torch.randn(p * split[2], d, generator=g), torch.rand(p, 2, generator=g)
    ga, gs = torch.randn(p, mod.activity_feat_dim(), generator=g), torch.randn(p, mod.completeness_feat_dim(), generator=g)
    f = backend.put(ft).clone().requires_grad_()
    act, st = mod(f, backend.put(sc), split)
    ((act * backend.put(ga)).sum() + (st * backend.put(gs)).sum()).backward()
    f64 = ft.double().requires_grad_()
    act64, st64 = O.stpp_forward(f64, sc.double(), split, cfg, standalone_classifier=standalong)
    ((act64 * ga.double()).sum() + (st64 * gs.double()).sum()).backward()
    figures = (err(act, act64), err(st, st64), err(f.grad, f64.grad))
    print("stpp", cfg, d, split, p, standalong, "act %.2e stpp %.2e d_ft %.2e" % figures)
    # one thread adds at most 24 fp32 segment values in order, then two divisions and one product: (24 + 3) * 2^-24 = 1.6e-6 at the
    # very worst, under the 2e-6 the heads hold against float64; the gradient is a sum of as many such terms
    assert max(figures) < 2e-6, (cfg, d, split, standalong, figures)


def completeness_inputs(videos, group, c, rounded, seed):
    """pred [videos * group, C] and 1-based labels with 0 among them (the reference's ``labels - 1`` then wraps to the last column);
    rounded: multiples of 0.5, so that hinge values tie inside a group and are exactly 0 where the prediction is +-1."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(videos * group, c, generator=g) * 1.5
    if rounded:
        pred = torch.round(pred * 2) / 2
    labels = torch.randint(0, c + 1, (videos * group,), generator=g)
    labels[::5] = 0
    return pred, labels


COMPLETENESS_SHAPES = [(32, 7, 1, 200), (64, 8, 2, 20), (300, 7, 1, 200), (5, 24, 4, 1), (3, 4, 1, 5)]      # videos, group, split, C


@pytest.mark.parametrize("rounded", [True, False])
@pytest.mark.parametrize("videos,group,split,c", COMPLETENESS_SHAPES)
def test_completeness_loss_against_the_oracle(backend, videos, group, split, c, rounded):
    """CompletenessLoss against oracle.completeness_loss: more than 256 and more than 2048 rows, label 0, tied and exactly-zero hinge
    values, a negative group of which int(n * 0.17) keeps nothing, and a data-parallel share of the denominator."""
    pred, labels = completeness_inputs(videos, group, c, rounded, seed=videos + c)
    if rounded:
        hinge = 1 - torch.where(torch.arange(pred.shape[0]) % group < split, 1.0, -1.0) * pred[torch.arange(pred.shape[0]), labels - 1]
        assert (hinge == 0).any() or pred.shape[0] < 30      # (the case exists in the data)
    want_loss, want_grad = O.completeness_loss(pred, labels.numpy(), split, group)
    for rows in (None, 4 * pred.shape[0]):
        leaf = backend.put(pred.clone()).requires_grad_()
        loss = P.CompletenessLoss()(leaf, backend.put(labels), split, group, global_rows=rows)
        loss.backward()
        # this rank's share of the gathered batch's denominator: (positives + int(negatives * 0.17) over all rows) / world
        n_groups, world = (rows or pred.shape[0]) // group, (rows or pred.shape[0]) / pred.shape[0]
        scale = (videos * split + int(videos * (group - split) * 0.17)) / ((n_groups * split + int(n_groups * (group - split) * 0.17)) / world)
        got, want = leaf.grad.cpu().numpy(), want_grad * np.float32(scale)
        print("completeness", (videos, group, split, c, rounded, rows), "loss %.9g oracle %.9g" % (loss.item(), float(want_loss) * scale),
              "equal" if np.array_equal(got, want) else "max grad diff %.3g" % np.abs(got - want).max())
        assert rel_err(loss, torch.tensor([float(want_loss) * scale])) < 1e-6
        assert np.array_equal(got != 0, want_grad != 0), "OHEM kept a different row set"
        np.testing.assert_allclose(got, want, rtol=1e-6)
    if (group - split) * 0.17 < 1:
        assert not want_grad.reshape(videos, group, c)[:, split:].any()      # (no negative row survives in this case)


@pytest.mark.parametrize("rows,group,ratio,positive,c", [(600, 6, 0.5, -1, 20), (600, 6, 0.5, 1, 20), (2100, 7, 0.17, -1, 200),
                                                         (2100, 7, 1.0, 1, 200), (9, 3, 0.17, -1, 4)])
def test_ohem_hinge_against_the_oracle(backend, rows, group, ratio, positive, c):
    """OHEMHingeLoss alone (the reference's Function signature): loss 1e-6, gradient and kept rows exact."""
    pred, labels = completeness_inputs(rows // group, group, c, True, seed=rows + group)
    want_loss, want_grad = O.ohem_hinge(pred, labels.numpy(), positive, ratio, group)
    leaf = backend.put(pred.clone()).requires_grad_()
    loss = P.OHEMHingeLoss.apply(leaf, backend.put(labels), positive, ratio, group)
    loss.backward()
    assert abs(loss.item() - float(want_loss)) <= 1e-6 * abs(float(want_loss))
    assert np.array_equal(leaf.grad.cpu().numpy(), want_grad)


@pytest.mark.parametrize("r,c,scale", [(32, 201, 1.0), (4096, 201, 1.0), (7, 1000, 1.0), (1, 21, 1.0), (32, 201, 30.0), (4096, 201, 30.0),
                                       (7, 1000, 30.0), (1, 201, 30.0)])
def test_activity_loss_against_float64(backend, r, c, scale):
    """ActivityLoss (ssn_ce_loss_*) against float64 F.cross_entropy; logits scaled by 30 overflow expf without the max subtraction."""
    g = torch.Generator().manual_seed(r + c)
    logits = torch.randn(r, c, generator=g) * scale
    target = torch.randint(0, c, (r,), generator=g)
    target[0], target[-1] = c - 1, 0 if r > 1 else c - 1
    leaf = backend.put(logits.clone()).requires_grad_()
    loss = P.ActivityLoss()(leaf, backend.put(target))
    loss.backward()
    l64 = logits.double().requires_grad_()
    want = F.cross_entropy(l64, target)
    want.backward()
    print("activity", (r, c, scale), "loss %.9g float64 %.9g gradient %.2e" % (loss.item(), want.item(), rel_err(leaf.grad, l64.grad)))
    assert torch.isfinite(leaf.grad).all()
    assert abs(loss.item() - want.item()) <= max(1e-6 * abs(want.item()), 1e-6)
    assert rel_err(leaf.grad, l64.grad) < 5e-6


def regression_inputs(n, c, dyadic, seed):
    """pred [n, C, 2], labels (1-based, with 0 = the last class among them), targets [n, 2].  The differences at the picked class lie on
    both sides of |d| = 1 and exactly on it; dyadic: all of them multiples of 1/4, so that every fp32 operation of the loss is exact."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(n, c, 2, generator=g) * 2
    labels = torch.randint(0, c + 1, (n,), generator=g)
    labels[0] = 0
    targets = torch.round(torch.randn(n, 2, generator=g) * 4) / 4
    marks = torch.tensor([1.0, -1.0, 0.0, 0.5, -0.75, 1.25, -3.0, 1.0 - 2.0 ** -20, -1.0 - 2.0 ** -20, 2.5])
    d = marks[torch.arange(2 * n) % marks.numel()].reshape(n, 2)
    if not dyadic:
        d = torch.where(torch.rand(n, 2, generator=g) < 0.5, d, torch.randn(n, 2, generator=g) * 1.5)
    pred[torch.arange(n), labels - 1] = targets + d
    return pred, labels, targets


@pytest.mark.parametrize("dyadic", [True, False])
@pytest.mark.parametrize("n,c", [(2, 1), (2, 200), (33, 1), (33, 200), (700, 1), (700, 200), (129, 20)])
def test_classwise_regression_loss_against_float64(backend, n, c, dyadic):
    """ClassWiseRegressionLoss against oracle.classwise_regression_loss in float64."""
    pred, labels, targets = regression_inputs(n, c, dyadic, seed=n + c)
    leaf = backend.put(pred.clone()).requires_grad_()
    loss = P.ClassWiseRegressionLoss()(leaf, backend.put(labels), backend.put(targets))
    loss.backward()
    p64 = pred.double().requires_grad_()
    want = O.classwise_regression_loss(p64, labels, targets.double())
    want.backward()
    # Loss: one fp32 subtraction and one smooth-L1 term per element (3 roundings, 2^-24 relative each), then ONE thread adds the 2n
    # non-negative terms in order: at most (2n + 3) * 2^-24 relative, and one more rounding each for the division and the factor 2.
    # With dyadic differences every one of these operations is exact but the final division.
    bound = 1e-6 if dyadic else max(1e-6, (2 * n + 5) * 2.0 ** -24)
    print("regression", (n, c, dyadic), "loss %.9g float64 %.9g gradient %.2e" % (loss.item(), want.item(), rel_err(leaf.grad, p64.grad)))
    assert abs(loss.item() - want.item()) <= bound * abs(want.item())
    assert np.array_equal(leaf.grad.cpu().numpy() != 0, p64.grad.numpy() != 0)      # only the picked class, and nothing where d == 0
    assert rel_err(leaf.grad, p64.grad) < 1e-6      # (d or +-1, times one fp32 constant)


# activity rows, (videos, group, split), regression rows, C
OBJECTIVE_SHAPES = [(64, (32, 7, 1), 33, 200), (600, (300, 7, 1), 700, 200), (128, (64, 8, 2), 2, 20), (4096, (5, 24, 4), 129, 1),
                    (1, (3, 4, 1), 2, 5)]


@pytest.mark.parametrize("ra,comp_shape,n_reg,c", OBJECTIVE_SHAPES)
def test_objective_parts_are_bit_identical_to_the_criterions(backend, ra, comp_shape, n_reg, c):
    """SSNObjective (one launch each way) at the shapes above: its three parts are bit-identical to ActivityLoss / CompletenessLoss /
    ClassWiseRegressionLoss run on their own, the total is the driver's mix, gradients those of the separate criterions -- with and
    without regression, with a data-parallel share of the denominator."""
    videos, group, split = comp_shape
    g = torch.Generator().manual_seed(ra + c)
    act = torch.randn(ra, c + 1, generator=g) * 3
    act_t = torch.randint(0, c + 1, (ra,), generator=g)
    comp, comp_t = completeness_inputs(videos, group, c, False, seed=ra)
    reg, reg_lbl, reg_t = regression_inputs(n_reg, c, False, seed=ra + 1)
    for with_reg, (wc, wr), rows in ((True, (0.1, 0.1), None), (False, (0.1, 0.1), None), (True, (0.3, 0.7), 4 * comp.shape[0])):
        leaves = [backend.put(t.clone()).requires_grad_() for t in (act, comp, reg)]
        obj = P.SSNObjective(wc, wr)
        args = [leaves[0], backend.put(act_t), leaves[1], backend.put(comp_t)]
        if with_reg:
            args += [leaves[2], backend.put(reg_lbl), backend.put(reg_t)]
        total = obj(*args, sample_split=split, sample_group_size=group, global_rows=rows)
        total.backward()
        sep = [backend.put(t.clone()).requires_grad_() for t in (act, comp, reg)]
        parts = [P.ActivityLoss()(sep[0], backend.put(act_t)), P.CompletenessLoss()(sep[1], backend.put(comp_t), split, group, global_rows=rows)]
        if with_reg:
            parts.append(P.ClassWiseRegressionLoss()(sep[2], backend.put(reg_lbl), backend.put(reg_t)))
        for k, part in enumerate(parts):
            assert obj.parts[k].item() == part.item(), (with_reg, rows, k, obj.parts[k].item(), part.item())
        if not with_reg:
            assert obj.parts[2].item() == 0.0
        mix = parts[0] + wc * parts[1].reshape(())
        if with_reg:
            mix = mix + wr * parts[2]
        assert abs(total.item() - mix.item()) <= 2e-7 * max(1.0, abs(mix.item()))
        mix.backward()
        for k in range(3 if with_reg else 2):
            assert rel_err(leaves[k].grad, sep[k].grad) < 1e-6, (with_reg, rows, k)
        assert torch.equal(leaves[0].grad, sep[0].grad)      # (the activity gradient has no weight in front: same arithmetic)
        assert leaves[2].grad is None or with_reg


REORG_WIDTHS = (201, 200, 400)      # ActivityNet: 200 classes + background, completeness, 2 regression values per class


@pytest.mark.parametrize("standalong", [True, False])
@pytest.mark.parametrize("cfg", [PRODUCT, (1, 1, 1)])
def test_reorganised_stpp_at_activitynet_size(backend, cfg, standalong):
    """STPPReorgainzed against oracle.stpp_reorganized: 600 score rows, 187 proposals with random sorted ticks, score widths of
    201 / 200 / 400 per part (the 400 regression columns take the kernel's column loop round a second time)."""
    a_len, c_len, r_len = REORG_WIDTHS
    t_rows, n_prop = 600, 187
    mod = P.STPPReorgainzed(0, a_len, c_len, r_len, standalong, True, stpp_cfg=cfg)
    width = mod.reg_slice.stop
    mod.feat_dim = width
    assert width == (a_len if standalong else a_len * mod.feat_multiplier) + (c_len + r_len) * mod.feat_multiplier
    rng = np.random.RandomState(11)
    scores = rng.standard_normal((t_rows, width)).astype(np.float32)
    ticks = np.sort(rng.randint(0, t_rows, size=(n_prop, 4)), axis=1)
    ticks[0], ticks[1], ticks[2] = (0, 0, 0, 0), (t_rows - 1,) * 4, (0, 0, t_rows - 1, t_rows - 1)
    scaling = rng.uniform(0.0, 1.0, size=(n_prop, 2)).astype(np.float32)
    want = O.stpp_reorganized(scores, ticks, scaling, a_len, c_len, r_len, stpp_cfg=cfg, standalone_classifier=standalong)
    for shift in (False, True):      # (and with score rows that do not start 16-byte aligned)
        dev = misaligned(torch.from_numpy(scores), backend) if shift else backend.put(torch.from_numpy(scores))
        got = mod.forward(dev, torch.from_numpy(ticks), scaling)
        for a, w, key in zip(got, want, ("act", "comp", "reg")):
            assert not np.isnan(w).any()
            print("reorg", cfg, standalong, shift, key, "%.2e" % rel_err(a, torch.from_numpy(w)))
            assert rel_err(a, torch.from_numpy(w)) < 1e-6, key
            np.testing.assert_allclose(a.cpu().numpy(), w, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("lengths", [(300, 0, 17), (0, 5, 0), (3, 700, 256), (257, 1, None), (0, 0, 0)])
def test_label_select_against_indexing(backend, lengths):
    """ssn_label_select: target[idx0], target[idx1], target[idx2], reg_target[idx2] in one launch, index lists of different and of
    zero length, with and without the regression list."""
    n_prop = 900
    g = torch.Generator().manual_seed(13)
    target = torch.randint(0, 201, (n_prop,), generator=g)
    reg_target = torch.randn(n_prop, 2, generator=g)
    idx = [None if n is None else torch.randperm(n_prop, generator=g)[:n].sort().values for n in lengths]
    d_idx = [backend.put(i) for i in idx]
    outs = [None if i is None else backend.put(torch.full((i.numel(),), -7, dtype=torch.int64)) for i in idx]
    out_reg = None if idx[2] is None else backend.put(torch.full((idx[2].numel(), 2), -7.0))
    K.label_select(backend.put(target), backend.put(reg_target), d_idx, outs, out_reg)
    for i, o in zip(idx, outs):
        if i is not None:
            assert torch.equal(o.cpu(), target[i])
    if idx[2] is not None:
        assert torch.equal(out_reg.cpu(), reg_target[idx[2]])


# ---- operands that are contiguous but do not start 16-byte aligned --------------------------------------------------------------
@pytest.mark.parametrize("r,o,d", [(8, 5, 64), (3, 21, 1024), (5, 3, 260), (4, 7, 33)])
def test_linear_with_operands_off_alignment(backend, r, o, d):
    """LinearFn with x, w and the output gradient (each alone, then all) handed over as ``buf[1:].view(shape)``: the results of the
    aligned call to 1e-6 (the 4-byte path adds in another order than the 16-byte path), float64 to 2e-6."""
    g = torch.Generator().manual_seed(d)
    x, w, b, go = torch.randn(r, d, generator=g), torch.randn(o, d, generator=g) * 0.1, torch.randn(o, generator=g), torch.randn(r, o, generator=g)
    x64, w64, b64 = [t.double().requires_grad_() for t in (x, w, b)]
    out64 = x64 @ w64.t() + b64
    out64.backward(go.double())
    ref = [out64.detach(), x64.grad, w64.grad, b64.grad]

    def run(shift):
        xl, wl, gl = [(misaligned(t, backend) if n in shift else backend.put(t).clone()) for n, t in (("x", x), ("w", w), ("go", go))]
        xl.requires_grad_(), wl.requires_grad_()
        bl = backend.put(b).clone().requires_grad_()
        out = FN.LinearFn.apply(xl, wl, bl)
        out.backward(gl)
        return [out.detach(), xl.grad, wl.grad, bl.grad]

    base = run(())
    for shift in (("x",), ("w",), ("go",), ("x", "w", "go")):
        got = run(shift)
        for k, (a, b0, r64) in enumerate(zip(got, base, ref)):
            assert err(a, b0) < 1e-6 and err(a, r64) < 2e-6, (shift, k, err(a, b0), err(a, r64))
        if shift == ("go",):      # (the backward kernels have one path only)
            assert all(torch.equal(a, b0) for a, b0 in zip(got, base))
    # the entry point itself, with the output off alignment too
    out = misaligned(torch.zeros(r, o), backend)
    K.linear_fwd(misaligned(x, backend), misaligned(w, backend), misaligned(b, backend), out)
    assert err(out, ref[0]) < 2e-6


@pytest.mark.parametrize("crops,t,d", [(10, 7, 1024), (10, 4, 201), (3, 2, 64), (1, 3, 33)])
def test_crop_mean_and_reg_denorm_off_alignment(backend, crops, t, d):
    """ssn_crop_mean with the input, the output or both off alignment, ssn_reg_denorm off its 8 bytes: bit-identical to the aligned call
    (either path adds the crops of an element in the same order), which holds the float64 mean to 1e-6."""
    g = torch.Generator().manual_seed(crops + d)
    x = torch.randn(crops * t, d, generator=g)
    base = backend.put(torch.empty(t, d))
    K.crop_mean(backend.put(x), crops, base)
    assert rel_err(base, x.double().view(crops, t, d).mean(dim=0)) < 1e-6
    for shift_x, shift_out in ((True, False), (False, True), (True, True)):
        out = misaligned(torch.zeros(t, d), backend) if shift_out else backend.put(torch.zeros(t, d))
        K.crop_mean(misaligned(x, backend) if shift_x else backend.put(x), crops, out)
        assert torch.equal(out, base), (shift_x, shift_out)
    reg = torch.randn(t, d, 2, generator=g)
    want = reg.double() * torch.tensor([1.7, 0.9], dtype=torch.double) + torch.tensor([0.3, -0.2], dtype=torch.double)
    a, m = backend.put(reg.clone()), misaligned(reg, backend)
    K.reg_denorm(a, 0.3, 1.7, -0.2, 0.9)
    K.reg_denorm(m, 0.3, 1.7, -0.2, 0.9)
    assert rel_err(a, want) < 1e-6 and torch.equal(a, m)


@pytest.mark.parametrize("cfg,d,c,split", [(PRODUCT, 1024, 20, (2, 7, 9)), (PRODUCT, 260, 5, (2, 7, 9)), (((1, 1), 1, 1), 6, 3, (2, 7, 9)),
                                           (WIDE, 64, 4, (4, 12, 16))])
def test_heads_and_stpp_with_operands_off_alignment(backend, cfg, d, c, split):
    """HeadsFn and the separate chain with the features, one weight, or all of them off alignment.  Features only: bit-identical (they
    are read 4 bytes at a time on either path).  Weights: the bounds of the aligned cases."""
    case = HeadsCase(cfg, d, c, split, 8, STD_TYPES, True, seed=3 * d)
    ref = case.float64()
    for fused in (True, False):
        base = case.run(backend, fused)
        got = case.run(backend, fused, shift=("ft",))
        assert all(torch.equal(a, b) for a, b in zip(got, base)), ("features", fused)
        for shift in (("w0",), ("w1",), ("w2",), ("ft", "w0", "w1", "w2")):
            got = case.run(backend, fused, shift=shift)
            for k, (a, b, r) in enumerate(zip(got, base, ref)):
                assert err(a, b) < 1e-6 and err(a, r) < 2e-6, (fused, shift, k, err(a, b), err(a, r))
    # STPP alone, output gradients off alignment as well
    g = torch.Generator().manual_seed(5)
    m = case.stpp.feat_multiplier
    ga, gs = torch.randn(8, d, generator=g), torch.randn(8, m * d, generator=g)
    res = []
    for shift in (False, True):
        f = (misaligned(case.ft, backend) if shift else backend.put(case.ft).clone()).requires_grad_()
        act, st = FN.StppFn.apply(f, misaligned(case.sc, backend) if shift else backend.put(case.sc), case.table, case.n_seg)
        torch.autograd.backward([act, st], [misaligned(ga, backend), misaligned(gs, backend)] if shift else [backend.put(ga), backend.put(gs)])
        res.append((act.detach(), st.detach(), f.grad))
    assert all(torch.equal(a, b) for a, b in zip(*res))
