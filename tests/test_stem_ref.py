"""The float64 mirror of the fused stem (tests/_stem_ref.py), checked on the CPU: its backward formulas against float64 autograd
of the plain module, the float32-against-float64 yardstick the GPU tolerances of test_stem_chain_gpu.py are derived from, and the
no-fragile-mask condition on every input the GPU test uses."""
import pytest
import torch
import torch.nn as nn

import _stem_ref as R


def _plain(p, state, momentum):
    m = nn.Sequential(nn.Conv2d(3, 32, 3, 1, 1), nn.BatchNorm2d(32, momentum=momentum), nn.ReLU(),
                      nn.Conv2d(32, 64, 3, 1, 1), nn.BatchNorm2d(64, momentum=momentum), nn.ReLU(),
                      nn.Conv2d(64, 96, 4, 4)).double()
    with torch.no_grad():
        for i, (c, b) in zip((1, 2), ((m[0], m[1]), (m[3], m[4]))):
            c.weight.copy_(p[f"w{i}"]); c.bias.copy_(p[f"b{i}"])
            b.weight.copy_(p[f"g{i}"]); b.bias.copy_(p[f"be{i}"])
            b.running_mean.copy_(state[f"rm{i}"]); b.running_var.copy_(state[f"rv{i}"]); b.num_batches_tracked.fill_(state[f"nbt{i}"])
        m[6].weight.copy_(p["w3"]); m[6].bias.copy_(p["b3"])
    return m


@pytest.mark.parametrize("momentum", [0.1, None])
@pytest.mark.parametrize("training", [True, False])
def test_mirror_equals_float64_autograd(training, momentum):
    """With the rounding replaced by the identity the mirror IS the module: tokens, the ten gradients, the running statistics and
    the counters equal float64 autograd of Conv-BN-ReLU-Conv-BN-ReLU-Conv (conv biases present) to 1e-10 relative."""
    B, H, W = 2, 12, 20
    x, p, state, dtok = R.make_case(B, H, W, 3)
    m = _plain(p, state, momentum).train(training)
    t = m(x.double())
    tok_ref = t.permute(0, 2, 3, 1).reshape(-1, 96)
    (tok_ref * dtok.double()).sum().backward()
    f = R.forward(x, p, state, training, rnd=R.identity, momentum=momentum)
    assert R.relerr(f.tok, tok_ref.detach()) < 1e-10
    g = R.backward(x, p, f.y2, f.prm1, f.prm2, dtok, training, rnd=R.identity)
    ref = dict(w1=m[0].weight.grad, b1=m[0].bias.grad, g1=m[1].weight.grad, be1=m[1].bias.grad, w2=m[3].weight.grad,
               b2=m[3].bias.grad, g2=m[4].weight.grad, be2=m[4].bias.grad, w3=m[6].weight.grad, b3=m[6].bias.grad)
    scale = {"b1": float(ref["be1"].norm()), "b2": float(ref["be2"].norm())}
    for k in R.GRADS:
        if training and k in ("b1", "b2"):       # a bias in front of a training-mode BatchNorm: exactly zero here, rounding noise in autograd
            assert float(g[k].abs().max()) == 0.0
            assert float(ref[k].norm()) < 1e-10 * scale[k]
            continue
        assert R.relerr(g[k], ref[k]) < 1e-10, k
    for i, bn in ((1, m[1]), (2, m[4])):
        assert R.relerr(f.state[f"rm{i}"], bn.running_mean) < 1e-10
        assert R.relerr(f.state[f"rv{i}"], bn.running_var) < 1e-10
        assert f.state[f"nbt{i}"] == int(bn.num_batches_tracked) == state[f"nbt{i}"] + int(training)
        if not training:
            assert torch.equal(f.state[f"rm{i}"], state[f"rm{i}"].double()) and torch.equal(f.state[f"rv{i}"], state[f"rv{i}"].double())


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,H,W,seed", R.CASES)
def test_no_fragile_masks(B, H, W, seed, training):
    """The condition of _stem_ref.py on every input of the GPU chain test, with the room the choice of seeds promises (24 x)."""
    x, p, state, _ = R.make_case(B, H, W, seed)
    lo, d = R.assert_no_fragile_mask(x, p, R.forward(x, p, state, training).prm1.float())
    assert lo > 24 * d, (lo, d)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,H,W", list(R.SEEDS))
def test_yardstick_table(B, H, W, training):
    """The float32-against-float64 gap of the anchored backward, per gradient: the largest over the shape's seeds is what
    test_stem_chain_gpu.py records (F32_GAP, and its docstring) and multiplies by 4.  The table must match what is computed here:
    within a factor of two either way above the floor of 1e-6, since the convolutions' summation order may differ between CPUs."""
    import test_stem_chain_gpu as T
    worst = {}
    for seed in R.SEEDS[(B, H, W)]:
        for k, v in R.f32_gaps(B, H, W, seed, training).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print((B, H, W, training), " ".join(f"{k}={v:.1e}" for k, v in worst.items()))
    table = T.F32_GAP[(B, H, W, training)]
    assert set(table) == set(worst)
    for k, v in worst.items():
        lo, hi = max(v, T.GAP_FLOOR), max(table[k], T.GAP_FLOOR)
        assert hi <= 2 * lo and lo <= 2 * hi, (k, v, table[k])
        assert T.tolerance(B, H, W, training, k) <= 2e-3
