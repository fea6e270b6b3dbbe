"""detector.sample_ranks / rpn_targets / roi_targets / mask_targets on the CPU: the definitions against the padded branch of
MiniMaskRCNN as it stood before them (restated in tests/_targets_cases.py), the tie rules, and the argument checks and workspace sizes
of the C entry points.  The kernels: tests/test_targets_gpu.py."""
import ctypes

import pytest
import torch

from panoswintransformerobjectdetection_amd import detector as det

import _targets_cases as tc


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- sample_ranks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pop", tc.POPULATIONS)
def test_sample_ranks_is_the_parents_rule_on_distinct_composed_keys(pop):
    B, N, n_pos, n_neg = 3, 700, 128, 256
    gt_inds, key = tc.population(pop, B, N, _gen(1)), tc.keys("distinct", B, N, _gen(2))
    assert tc.composed_keys_distinct(gt_inds, key)
    pos_rank, neg_rank = det.sample_ranks(gt_inds, key, n_pos, n_neg)
    assert pos_rank.dtype == torch.long and tuple(pos_rank.shape) == (B, n_pos) and tuple(neg_rank.shape) == (B, n_neg)
    anchors, gt = torch.zeros(N, 4), torch.zeros(B, 16, 4)
    for b in range(B):
        want = tc.parent_rpn_image(gt_inds[b], key[b], anchors, gt[b], n_pos, n_neg)
        assert torch.equal(pos_rank[b], want[0]) and torch.equal(neg_rank[b], want[1]), (pop, b)


def test_sample_ranks_breaks_ties_by_ascending_index():
    B, N = 2, 500
    gt_inds, key = tc.population("mix", B, N, _gen(3)), tc.keys("eighths", B, N, _gen(4))
    pos_rank, neg_rank = det.sample_ranks(gt_inds, key, N, N)
    for rank, comp in zip((pos_rank, neg_rank), tc.composed(gt_inds, key)):
        for b in range(B):
            c = comp[b][rank[b]]
            assert sorted(rank[b].tolist()) == list(range(N))
            assert bool((c[1:] >= c[:-1]).all())
            same = c[1:] == c[:-1]
            assert int(same.sum()) > N // 2 and bool((rank[b][1:] > rank[b][:-1])[same].all())


def test_sample_ranks_orders_by_the_composed_float32_key_then_the_index():
    """keys j * 2^-24 are all different, but fl(key + 2) keeps 2^-22: among the non-members the order is that of the COMPOSED key, and
    candidates whose composed keys tie come out by index even where their keys say otherwise"""
    N = 64
    key = (torch.arange(N).flip(0).float() * 2.0 ** -24)[None]      # descending keys: index order and key order disagree everywhere
    gt_inds = torch.zeros(1, N, dtype=torch.long)                   # no positive: the positive order is all "behind"
    comp = key + 2
    assert int(torch.unique(comp).numel()) < N // 2 and int(torch.unique(key).numel()) == N
    pos_rank, neg_rank = det.sample_ranks(gt_inds, key, N, N)
    want = sorted(range(N), key=lambda i: (float(comp[0, i]), i))
    assert pos_rank[0].tolist() == want
    assert want != sorted(range(N), key=lambda i: float(key[0, i]))
    assert neg_rank[0].tolist() == list(range(N - 1, -1, -1))      # the members keep their full-resolution keys
    with pytest.raises(ValueError):
        det.sample_ranks(gt_inds, key, N + 1, 1)


# ---- rpn_targets / roi_targets --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Gmax", [1, 16])
def test_rpn_targets_is_the_parents_per_image_branch(Gmax):
    n_pos_max, n_tot = 128, 256
    gt_inds, key, cand, gt, _, count = tc.stage_case(Gmax, 2100, False, seed=3)
    assert tc.composed_keys_distinct(gt_inds, key) and count.tolist() == [Gmax, 0, 1]
    anchors = cand[0]
    idx, valid, pos_valid, reg_t = det.rpn_targets(gt_inds, key, anchors, gt, n_pos_max, n_tot)
    assert idx.dtype == torch.long and valid.dtype == torch.float32 and pos_valid.dtype == torch.bool and reg_t.dtype == torch.float32
    assert bool(pos_valid[0].any()) and not bool(pos_valid[1].any())
    for b in range(3):
        _, _, w_idx, w_valid, w_pv, w_d = tc.parent_rpn_image(gt_inds[b], key[b], anchors, gt[b], n_pos_max, n_tot)
        assert torch.equal(idx[b], w_idx) and torch.equal(valid[b], w_valid) and torch.equal(pos_valid[b], w_pv), b
        assert torch.equal(reg_t[b], torch.where(w_pv[:, None], w_d, torch.zeros_like(w_d))), b
        assert not reg_t[b][~w_pv].any()


@pytest.mark.parametrize("Gmax", [1, 16])
def test_roi_targets_is_the_parents_per_image_branch(Gmax):
    n_pos_max, n_tot, C = 128, 512, 80
    gt_inds, key, cand, gt, labels, count = tc.stage_case(Gmax, 1000, True, seed=4)
    assert tc.composed_keys_distinct(gt_inds, key) and bool((gt_inds[1, :Gmax] == -1).all())
    got = det.roi_targets(gt_inds, key, cand, gt, labels, C, n_pos_max, n_tot, (0.1, 0.1, 0.2, 0.2))
    assert [t.dtype for t in got] == [torch.float32, torch.long, torch.float32, torch.bool, torch.long]
    pad = torch.tensor(tc.SENTINEL)
    assert not bool((got[0] == pad).all(-1).any()) and not bool((got[1] == tc.SENTINEL_LABEL).any())
    assert bool(got[3][0].any()) and not bool(got[3][0].all())                    # fewer positives than slots: the filler offset is active
    for b in range(3):
        w_rois, w_lab, w_reg, w_pv, w_gi = tc.parent_roi_image(gt_inds[b], key[b], cand[b], gt[b], labels[b], C, n_pos_max, n_tot)
        assert torch.equal(got[0][b], w_rois) and torch.equal(got[1][b], w_lab) and torch.equal(got[3][b], w_pv) and torch.equal(got[4][b], w_gi), b
        assert torch.equal(got[2][b], torch.where(w_pv[:, None], w_reg, torch.zeros_like(w_reg))), b
        assert len({tuple(r) for r in got[0][b].tolist()}) >= n_tot - 60       # no RoI twice, up to the cases' duplicate boxes


# ---- mask_targets ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(37, 53), (128, 256)])
def test_mask_targets_is_the_parents_all_channels_statement_bit_for_bit(H, W):
    masks, rois, gt_idx, pos_valid, count = tc.mask_case(H, W)
    got = det.mask_targets(masks, rois, gt_idx, pos_valid, 28)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2 * tc.MASK_P, 28, 28) and set(got.unique().tolist()) == {0.0, 1.0}
    for b in range(2):
        want = tc.parent_mask_image(masks[b], rois[b], gt_idx[b].clamp(0, tc.MASK_GMAX - 1), (H, W), 28)
        want = torch.where(pos_valid[b][:, None, None], want, torch.zeros_like(want))
        assert torch.equal(got[b * tc.MASK_P:(b + 1) * tc.MASK_P], want), b
    assert not got.view(2, tc.MASK_P, -1)[~pos_valid].any()
    assert bool((gt_idx[pos_valid] < count[:, None].expand(-1, tc.MASK_P)[pos_valid]).all())   # no valid row points at a plane of ones
    # float32 and float64 agree outside the near-threshold set, and that set is small
    near, truth = tc.near_threshold(masks, rois, gt_idx, pos_valid)
    share = float(near.float().mean())
    print(f"{H} x {W}: near-threshold share {share:.2e}")
    assert share <= tc.NEAR_SHARE
    assert torch.equal(got[~near], truth[~near])
    flt = det.mask_targets(masks, rois, gt_idx, pos_valid, 28, return_float=True)
    assert flt.dtype == torch.float32 and torch.equal((flt >= 0.5).float(), got)


def test_heads_hooks_are_the_dispatchers():
    assert det.MiniMaskRCNN.rpn_targets is det.rpn_targets_dispatch and det.MiniMaskRCNN.roi_targets is det.roi_targets_dispatch
    assert det.MiniMaskRCNN.mask_targets is det.mask_targets_dispatch


# ---- the C entry points without a GPU ------------------------------------------------------------------------------------------------------
ERR = -1


def _lib_and_pointer():
    from panoswintransformerobjectdetection_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    return lib, buf, (ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15


def _each_bad(fn, ok, bads):
    for i, v in bads:
        bad = list(ok)
        bad[i] = v
        assert fn(*bad) == ERR, (i, v)


def test_workspace_sizes_of_the_sampler():
    lib, _, _ = _lib_and_pointer()
    R = lib.pswin_sample_rows_per_workgroup()
    assert R > 0 and R % 64 == 0
    ws = lib.pswin_sample_workspace
    assert ws(3, R, 512) == 16 and ws(1, 1, 1) == 16                       # one chunk: the tree has one level, nothing is staged
    assert ws(3, R + 1, 512) == 3 * 2 * 2 * 512 * 8                       # two chunks keep 512 composites of 8 bytes each, per list and image
    c0 = -(-130944 // R)                                                  # the RPN at 512 x 1024: every level keeps k per chunk
    c1 = -(-c0 * 512 // R)
    assert ws(8, 130944, 512) == 8 * 2 * (c0 + c1) * 512 * 8
    assert ws(2, 4 * R + 1, 1) == 2 * 2 * 5 * 8                           # k = 1: five chunks leave five composites, one more level
    for B, N, k in ((0, 8, 4), (1, 0, 1), (1, 8, 0), (1, 8, 9), (1, 4 * R, R // 2 + 1)):
        assert ws(B, N, k) == ERR, (B, N, k)
    assert ws(1, 4 * R, R // 2) > 0


def test_argument_errors_of_the_sampler_and_target_entry_points_without_a_gpu():
    """Every new entry point validates before it touches the device: PSWIN_ERR_ARG (-1) on a CPU-only host."""
    lib, _buf, p = _lib_and_pointer()
    # gt_inds, key, B, N, n_pos, n_neg, pos_rank, neg_rank, workspace, stream
    _each_bad(lib.pswin_sample_ranks, [p, p, 2, 3000, 128, 256, p, p, p, None],
              ((0, None), (1, None), (6, None), (7, None), (8, None), (2, 0), (3, 0), (4, 0), (5, 0), (4, 3001), (5, 3001), (5, 1025),
               (0, p + 4), (1, p + 2), (6, p + 4), (8, p + 8)))
    # gt_inds, pos_rank, neg_rank, anchors, gt, B, N, Gmax, n_pos_max, n_tot, idx, valid, pos_valid, reg_t, stream
    _each_bad(lib.pswin_rpn_targets, [p, p, p, p, p, 2, 3000, 16, 128, 256, p, p, p, p, None],
              ((0, None), (1, None), (2, None), (3, None), (4, None), (10, None), (11, None), (12, None), (13, None), (5, 0), (6, 0), (7, 0),
               (7, 257), (8, 0), (8, 257), (9, 3001), (9, 1025), (3, p + 8), (4, p + 8), (13, p + 8), (10, p + 4), (11, p + 2)))
    # gt_inds, pos_rank, neg_order, cand, gt, gt_labels, B, N, Gmax, n_pos_max, n_tot, num_classes, stds, rois, labels, reg_t, pos_valid,
    # gt_idx, stream
    stds = (ctypes.c_float * 4)(0.1, 0.1, 0.2, 0.2)
    zero = (ctypes.c_float * 4)(0.1, 0.0, 0.2, 0.2)
    sp, zp = ctypes.cast(stds, ctypes.c_void_p), ctypes.cast(zero, ctypes.c_void_p)
    _each_bad(lib.pswin_roi_targets, [p, p, p, p, p, p, 2, 1016, 16, 128, 512, 80, sp, p, p, p, p, p, None],
              ((0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (12, None), (13, None), (14, None), (15, None), (16, None),
               (17, None), (6, 0), (7, 0), (8, 0), (8, 257), (9, 0), (9, 513), (10, 1017), (11, 0), (12, zp), (3, p + 8), (4, p + 8),
               (13, p + 8), (15, p + 8), (14, p + 4), (17, p + 4)))
    # masks, rois, gt_idx, pos_valid, B, P, Gmax, H, W, size, out, stream
    _each_bad(lib.pswin_mask_targets, [p, p, p, p, 2, 128, 16, 128, 256, 28, p, None],
              ((0, None), (1, None), (2, None), (3, None), (10, None), (4, 0), (5, 0), (6, 0), (6, 257), (7, 0), (8, 0), (9, 0), (9, 65),
               (1, p + 8), (2, p + 4), (10, p + 2)))
