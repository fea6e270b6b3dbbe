"""MiniMaskRCNN.heads_loss on detector.PaddedTargets, captured ONCE in a hipGraph and replayed on annotation sets with other box
counts: what the list form of the targets cannot do (its shapes are those of one batch).  Heads only, on random feature maps of a
2 x 128 x 256 image.  Asserted per replay: the losses agree with an eager heads_loss on the same annotations within the bound of the
existing replay test (tests/test_detector_gpu.py: 2e-3 relative; the heads' convolutions are not bit-stable from call to call), every
head gradient is finite, and no RoI handed to roi_align is a padding row."""
import pytest
import torch

from _util import TINY

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W, GMAX = 2, 128, 256, 16
SENTINEL = [1.25, 2.25, 250.25, 120.25]      # written into the padding rows after every copy: it would match half the image if it were read


def _fixed_keys():
    cache = {}

    def rand_like(t):
        n = t.numel()
        if n not in cache:
            cache[n] = torch.rand(n, generator=torch.Generator("cpu").manual_seed(1000 + n)).to(t.device)
        return cache[n].view_as(t).to(t.dtype)
    return rand_like


def _annotations(counts, seed):
    from panoswintransformerobjectdetection_amd.detector import synthetic_targets
    tg = next(t for t in (synthetic_targets(B, H, W, "cpu", seed=s) for s in range(seed, seed + 200))
              if all(i["boxes"].shape[0] >= n for i, n in zip(t, counts)))
    return [{k: v[:n] for k, v in t.items()} for t, n in zip(tg, counts)]


def test_one_captured_heads_step_is_replayed_on_annotations_with_other_box_counts():
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _body(side)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def _body(side):
    from panoswintransformerobjectdetection_amd import detector as det
    from panoswintransformerobjectdetection_amd.graph import GraphedCallable
    torch.manual_seed(0)
    m = det.MiniMaskRCNN(dict(TINY, compute_dtype=torch.float32), num_classes=80).to(DEV).train()
    m.rand_like = _fixed_keys()
    heads = m.head_parameters()
    feats = [torch.randn(B, c, H // s, W // s, device=DEV) for c, s in zip(m.backbone.num_features, (4, 8, 16, 32))]
    sets = [_annotations(c, seed) for c, seed in (((4, 9), 0), ((7, 2), 300), ((1, 5), 600))]
    T = det.PaddedTargets.allocate(B, GMAX, DEV, mask_hw=(H, W))
    pad = torch.tensor(SENTINEL, device=DEV)

    def load(tg):
        T.copy_from([t["boxes"] for t in tg], [t["labels"] for t in tg], [t["masks"] for t in tg])
        for b, n in enumerate(len(t["boxes"]) for t in tg):
            T.boxes[b, n:] = pad

    seen = []

    def roi_align(*a, **kw):
        seen.append(a[2])
        return det.roi_align(*a, **kw)

    m.roi_align = roi_align
    state = {}

    def step():
        for p in heads:
            p.grad = None
        ls = m.heads_loss(feats, T, (H, W))
        sum(ls.values()).backward()
        state["losses"] = torch.stack([ls[k] for k in sorted(ls)])
        return state["losses"]

    load(sets[0])
    g = GraphedCallable(step, warmup=2, stream=side, parameters=heads)
    captured_rois = seen[-2:]                                   # the two calls of the capture pass: static tensors of the graph's pool
    assert [tuple(r.shape) for r in captured_rois] == [(B, 512, 4), (B, 128, 4)]
    names = sorted(["loss_rpn_cls", "loss_rpn_bbox", "loss_cls", "loss_bbox", "loss_mask"])
    for replay, tg in enumerate(sets[1:] + sets[:1]):           # other counts than the captured ones first
        load(tg)
        g()
        side.synchronize()
        got = dict(zip(names, state["losses"].tolist()))
        grads_ok = all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in heads)
        rois = [r.clone() for r in captured_rois]
        with torch.no_grad():
            want = {k: float(v) for k, v in m.heads_loss(feats, T, (H, W)).items()}      # eager, same annotations and keys
        assert set(want) == set(names)
        for k in names:
            assert abs(got[k] - want[k]) <= 2e-3 * max(abs(want[k]), 1e-3), (replay, k, got[k], want[k])
        assert grads_ok, replay
        for r in rois:
            assert not bool((r == pad).all(-1).any()), replay
        # the RoIs are this replay's: every image's first gt box can only be drawn from its own annotations
        assert all(bool((rois[0][b] == T.boxes[b, 0]).all(-1).any()) or int(T.count[b]) == 0 for b in range(B)), replay


def _layout_keys(case, gmax):
    """rand_like stand-in that gives a candidate the same key whichever form draws it: the RPN's 8,184 keys by size; in the RoI stage a
    draw of n keys is the first n - R of `gmax` fixed gt keys, then R fixed proposal keys (lists draw G_b + R per image, a caller's
    PaddedTargets max_gt + R)"""
    g = torch.Generator("cpu").manual_seed(77)
    rpn, gt, prop = (torch.rand(n, generator=g).to(DEV) for n in (3 * sum(h * w for h, w in case.LEVELS), gmax, case.R))

    def rand_like(t):
        n = t.numel()
        return (rpn if n == rpn.numel() else torch.cat([gt[:n - case.R], prop])).view_as(t).to(t.dtype)
    return rand_like


@pytest.mark.parametrize("counts", [(5, 5), (3, 7)])
def test_lists_and_the_padded_targets_copied_from_them_run_the_same_kernels_on_the_same_buffers(counts):
    """The same random RPN outputs, feature maps, proposals and keys through _rpn_losses_and_proposals and _roi_losses, once as lists and
    once as a PaddedTargets filled by copy_from with max_gt = max(counts).  Bit-equal RPN losses and, for equal counts, bit-equal RoIs in
    both roi_align calls; for ragged counts the forms differ in the layout of the RoI stage's keys only (a list's padding rows hold a 0
    between the gt keys and the proposal keys), so the sampled RoIs that are proposals are bit-equal."""
    import _heads_list_case as case
    from panoswintransformerobjectdetection_amd import detector as det
    assert (case.B, case.H, case.W) == (B, H, W)
    torch.manual_seed(0)
    m = det.MiniMaskRCNN(dict(TINY, compute_dtype=torch.float32), num_classes=80).to(DEV).train()
    m.rand_like = _layout_keys(case, max(counts))
    rpn_outs, fpn, proposals = case.inputs()
    rpn_outs, fpn = [(c.to(DEV), r.to(DEV)) for c, r in rpn_outs], [f.to(DEV) for f in fpn]
    proposals = [p.to(DEV) for p in proposals]
    anchors = det.make_anchors(case.LEVELS, m.STRIDES, DEV)
    assert sum(a.shape[0] for a in anchors) == 8184
    tg = [{k: v.to(DEV) for k, v in t.items()} for t in _annotations(counts, 0)]
    T = det.PaddedTargets.allocate(B, max(counts), DEV, mask_hw=(H, W))
    T.copy_from([t["boxes"] for t in tg], [t["labels"] for t in tg], [t["masks"] for t in tg])
    seen = []

    def roi_align(*a, **kw):
        seen.append(a[2].clone())
        return det.roi_align(*a, **kw)

    m.roi_align = roi_align
    rpn_loss = []
    with torch.no_grad():
        for form in (det.PaddedTargets.of(tg), T):
            rpn_loss.append(torch.stack(m._rpn_losses_and_proposals(rpn_outs, anchors, form, (H, W))[:2]))
            m._roi_losses(fpn, proposals, form, (H, W))
    torch.cuda.synchronize()
    print("rpn losses", rpn_loss[0].tolist(), rpn_loss[1].tolist())
    assert torch.equal(rpn_loss[0], rpn_loss[1]) and bool(torch.isfinite(rpn_loss[0]).all())
    assert [tuple(r.shape) for r in seen] == [(B, 512, 4), (B, 128, 4)] * 2
    for got, want in zip(seen[:2], seen[2:]):
        if counts[0] == counts[1]:
            assert torch.equal(got, want)
            continue
        for b in range(B):
            is_gt = [(r[b][:, None] == T.boxes[b][None]).all(-1).any(1) for r in (got, want)]
            assert torch.equal(is_gt[0], is_gt[1]) and int((~is_gt[0]).sum()) >= got.shape[1] // 2
            assert torch.equal(got[b][~is_gt[0]], want[b][~is_gt[0]]), b
