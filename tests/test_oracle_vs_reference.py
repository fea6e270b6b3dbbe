"""The CPU oracle against the reference, through what the reference computed on the same models and inputs (fixtures written by
oracle/gen_golden.py oracle_vs_reference: tests/golden/oracle_vs_reference.npz and reference_interface.json; the inputs whose last
stage is 3 x 6 and 5 x 10 tokens lie in oracle_vs_reference_small.npz, written by oracle_vs_reference_small)."""
import json
import os

import pytest
import torch

import panoswin_oracle as po
from _util import GOLDEN, TINY, TINY_PITCH, ZERO_GRAD_KEYS, build_filled, golden
from detfill import det_uniform


def _case(gold, cfg, pano, shape):
    """The fixture's key prefix of the case stored with this configuration."""
    want = json.dumps(dict(cfg=cfg, pano=pano, shape=list(shape)), sort_keys=True)
    keys = [k[:-len(":config")] for k in gold.files if k.endswith(":config") and str(gold[k]) == want]
    assert len(keys) == 1, want
    return keys[0]


def _check(ref_sample, step, ref_norm, got, rtol, atol, what):
    """allclose(ref, got, rtol, atol) on the stored elements (every step-th one of the flattened tensor, from the first), and on the
    whole tensor the bound that the element-wise one implies: | ||ref|| - ||got|| | <= ||ref - got|| <= rtol ||got|| + atol sqrt(n)."""
    ref = torch.from_numpy(ref_sample)
    assert torch.allclose(ref, got.reshape(-1)[::int(step)][:ref.numel()], rtol=rtol, atol=atol), what
    got_norm = got.double().norm().item()
    assert abs(got_norm - ref_norm) <= rtol * got_norm + atol * got.numel() ** 0.5, what


def _interface():
    with open(os.path.join(GOLDEN, "reference_interface.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("cfg,pano,shape", [(TINY, True, (2, 3, 64, 128)), (TINY, False, (1, 3, 60, 100)),
                                            (TINY_PITCH, True, (2, 3, 64, 128)), (TINY, True, (1, 3, 100, 196)),
                                            (TINY, True, (1, 3, 96, 192)), (TINY, True, (1, 3, 160, 320))])
def test_same_outputs_and_grads(cfg, pano, shape):
    gold = golden("oracle_vs_reference_small" if shape[2] in (96, 160) else "oracle_vs_reference")
    c = _case(gold, cfg, pano, shape)
    # the reference ran with the weights det_fill_module(.., "live") gives the oracle (the generator checks the state dicts are equal)
    ora = build_filled(po.SimplePanoSwinTransformerOracle, cfg, pano, "live")
    x = det_uniform(shape, "live:x", 1.0).requires_grad_(True)
    outs = ora(x)
    assert sum(k.startswith(c + ":out") and k.count(":") == 1 for k in gold.files) == len(outs)
    for i, o in enumerate(outs):
        _check(gold[f"{c}:out{i}"], gold[f"{c}:out{i}:step"], float(gold[f"{c}:out{i}:norm"]), o.detach(), 1e-5, 1e-6, f"out{i}")
    ws = [det_uniform(tuple(o.shape), f"live:w{i}") for i, o in enumerate(outs)]
    sum((a * w).sum() for a, w in zip(outs, ws)).backward()
    _check(gold[f"{c}:dx"], gold[f"{c}:dx:step"], float(gold[f"{c}:dx:norm"]), x.grad, 1e-4, 1e-5 * float(gold[f"{c}:dx:max"]), "dx")
    names = [str(k) for k in gold[f"{c}:grad_names"]]
    params = dict(ora.named_parameters())
    assert names == list(params)
    ends = gold[f"{c}:grad_len"].cumsum()
    for j, k in enumerate(names):
        p = params[k]
        if gold[f"{c}:grad_none"][j]:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert p.grad is not None, k
        if any(z in k for z in ZERO_GRAD_KEYS):
            continue
        ref = gold[f"{c}:grad"][ends[j] - gold[f"{c}:grad_len"][j]:ends[j]]
        scale = float(gold[f"{c}:grad_max"][j])
        _check(ref, gold[f"{c}:grad_step"][j], float(gold[f"{c}:grad_norm"][j]), p.grad, 1e-4, 1e-5 * max(scale, 1e-6), k)


def test_reference_registry_name_and_kwargs():
    import inspect
    ref = _interface()
    assert "SimplePanoSwinTransformer" in ref["registry"]
    ora_sig = inspect.signature(po.SimplePanoSwinTransformerOracle.__init__)
    assert ref["init_parameters"] == list(ora_sig.parameters)
    for k, d in ref["init_defaults"].items():
        assert d == repr(ora_sig.parameters[k].default), k


def test_product_class_matches_the_reference_interface():
    """The PRODUCT class (not only the oracle): same constructor parameters and defaults as the reference (HOT:781-801)
    plus the single keyword ``compute_dtype``, and identical state-dict keys and shapes for pano / planar / pitch-block
    configurations, so reference checkpoints load with strict=True.  Construction needs no GPU."""
    import inspect
    from panoswintransformerobjectdetection_amd import SimplePanoSwinTransformer
    ref = _interface()
    got_sig = inspect.signature(SimplePanoSwinTransformer.__init__).parameters
    assert list(got_sig) == ref["init_parameters"] + ["compute_dtype"]
    for k, d in ref["init_defaults"].items():
        assert d == repr(got_sig[k].default), k
    cfgs = {"tiny": TINY, "tiny_pitch": TINY_PITCH, "tiny_planar_noape": dict(TINY, ape=False, pano_mode=False),
            "tiny_out13": dict(TINY, out_indices=(1, 3)), "T": dict(embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], ape=True)}
    assert set(cfgs) == set(ref["state_dicts"])
    for name, cfg in cfgs.items():
        want = ref["state_dicts"][name]
        got = SimplePanoSwinTransformer(**cfg).state_dict()
        assert [k for k, _, _ in want] == list(got.keys()), name
        for k, shape, dtype in want:
            assert list(got[k].shape) == shape and str(got[k].dtype) == dtype, k
    # loading a state dict with the reference's keys, shapes and dtypes into the product is strict-clean
    m = SimplePanoSwinTransformer(**TINY_PITCH)
    m.load_state_dict({k: torch.zeros(shape, dtype=getattr(torch, dtype.split(".")[1])) for k, shape, dtype in ref["state_dicts"]["tiny_pitch"]},
                      strict=True)
