"""The row movers, column sums and grouped reductions of csrc/pswin_move.hip and the table-gradient stages of csrc/pswin_attn.hip against
their float64 definitions (tests/_move_cases.py, checked on the CPU by tests/test_move_cases.py) on operands with ONE right answer: every
comparison is an equality of bits, of values (torch.equal against the definition cast once to the output dtype) or of isnan / isinf masks.

Which parametrization reaches which kernel:
  window_gather_kernel<x, w>, window_scatter_add_kernel<w, x>   the four dtype pairs of test_window_gather / test_window_scatter_add at
                                                                 C = 2056 (every pair), and all but f32 -> bf16 / bf16 -> f32 below it
  window_gather8_kernel<false / true>                           f32-bf16-plain / f32-bf16-scaled at C <= 2048
  window_scatter_add8_kernel<S, R, B>                           bf16-f32 with the eight flag ids (---, --B, ... SRB) at C = 96 and 768
  the B > 65535 fallback                                        test_more_images_than_a_grid_has_rows
  rowsum_direct_kernel<bf16 / f32>                              test_colsum_abi at N = 16384, 16392 / 8192, 8200 with M <= 1024
  rowsum_partial_kernel<bf16 / f32> + colsum_kernel             test_colsum_abi at every other (N, M); with a skip range: test_colsum_skip
  reduce_jobs_kernel, lane shapes 1024 x 1, 128 x 8, 16 x 64    test_reduce_jobs (rows <= 16, <= 128, beyond), test_colsum_through_ops
  dtab_partial_kernel, colsum_kernel, dtab_final_kernel         test_table_gradients, ids ...-nd0 (no distance table) and ...-nd1 / 4 / 5 / 15
rowsum_direct_kernel is unreachable from every Python caller (ops.colsum never passes an output); it is reached here through the C ABI.
"""
import ctypes

import pytest
import torch

import _move_cases as mc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16, F64 = mc.F32, mc.BF16, mc.F64
_MAPS = {}


def _lib():
    from panoswintransformerobjectdetection_amd import _lib as lib
    return lib


def _dev(t, dtype):
    return None if t is None else t.to(dtype).to(DEV)


def _maps(ops, geom):
    """the device's (map, inv) as int32, compared with the oracle's first; the identity map from torch.arange"""
    if geom not in _MAPS:
        wmap, inv = mc.maps(geom)
        if geom.startswith("ident"):
            a = torch.arange(len(wmap), dtype=torch.int32, device=DEV)
            _MAPS[geom] = (a, a)
        else:
            pano, H, W, s = mc.GEOMS[geom]
            dmap, dinv, nW = ops.window_maps(pano, H, W, s, DEV)
            assert nW * 49 == len(wmap) and torch.equal(dmap.cpu().long(), wmap) and torch.equal(dinv.cpu().long(), inv), geom
            _MAPS[geom] = (dmap, dinv)
    return _MAPS[geom]


def _row_ptr(buf):
    """the address of row GUARD of a guarded buffer"""
    return ctypes.c_void_p(buf.data_ptr() + mc.GUARD * buf.shape[1] * buf.element_size())


def _scale(c):
    return None if c["scale"] is None else c["scale"].float().to(DEV)


def _gather(ops, c, geom, x64=None, guarded=False):
    lib = _lib()
    x = _dev(c["x"] if x64 is None else x64, c["xdt"])
    wmap, sc = _maps(ops, geom)[0], _scale(c)
    if not guarded:
        return ops._gather_raw(x, wmap, sc, c["n_slots"], c["wdt"]).cpu()
    buf = mc.guarded(c["B"] * c["n_slots"], c["C"], c["wdt"]).to(DEV)
    lib.call("pswin_window_gather", x, lib.ptr(x), lib.dtype_code(x), lib.ptr(wmap), lib.ptr(sc), _row_ptr(buf), lib.dtype_code(buf),
             c["B"], c["S"], c["n_slots"], c["C"])
    return buf.cpu()


def _scatter(ops, c, geom, win64=None, guarded=False):
    lib = _lib()
    win = _dev(c["win"] if win64 is None else win64, c["wdt"])
    inv, sc, resid, bias = _maps(ops, geom)[1], _scale(c), _dev(c["resid"], c["xdt"]), _dev(c["bias"], F32)
    if not guarded:
        return ops._scatter_raw(win, inv, resid, sc, c["S"], c["xdt"], bias=bias).cpu()
    buf = mc.guarded(c["B"] * c["S"], c["C"], c["xdt"]).to(DEV)
    lib.call("pswin_window_scatter_add", win, lib.ptr(win), lib.dtype_code(win), lib.ptr(inv), lib.ptr(resid), lib.ptr(sc), lib.ptr(bias),
             _row_ptr(buf), lib.dtype_code(buf), c["B"], c["S"], c["n_slots"], c["C"])
    return buf.cpu()


# ---------------------------------------------------------------------------------------------------------------------
# A. window gather and scatter-add
# ---------------------------------------------------------------------------------------------------------------------
def test_device_maps_equal_the_oracle(ops):
    for geom in mc.PADDED_GEOMS:
        dmap, dinv = _maps(ops, geom)
        assert (len(dinv), len(dmap), int((dmap < 0).sum())) == mc.GEOM_COUNTS[geom]


@pytest.mark.parametrize("p", mc.gather_params(), ids=mc.mover_id)
def test_window_gather(ops, p):
    """win[b, slot] = scale_b * x[b, map[slot]], +0 where map[slot] < 0, cast once"""
    c = mc.gather_case(*p)
    got = _gather(ops, c, p[1])
    assert got.dtype == c["wdt"] and not mc.judge_values(got, mc.gather_def(c))
    assert not bool((mc.bits(got[:, c["wmap"] < 0]) != 0).any())


@pytest.mark.parametrize("p", mc.scatter_params(), ids=mc.mover_id)
def test_window_scatter_add(ops, p):
    """out[b, t] = resid[b, t] + scale_b * (win[b, inv[t]] + bias), cast once: the bias BEFORE the scale in both kernel families
    (window_scatter_add8_kernel: `a = a + b0` ahead of `a = a * sc`; window_scatter_add_kernel: `val + bias` ahead of `val * sc`)"""
    c = mc.scatter_case(*p)
    got = _scatter(ops, c, p[1])
    assert got.dtype == c["xdt"] and not mc.judge_values(got, mc.scatter_def(c))


@pytest.mark.parametrize("C", mc.WIDTHS + (96,), ids=[f"C{C}-8wide" for C in mc.PATH8_WIDTHS] + ["C2056-generic", "C96-generic"])
def test_guard_bands(ops, C, request):
    """the entry points write their rows and nothing else: the output sits 4 rows into a buffer of a sentinel bit pattern, over every
    geometry of the width (all tails of the 8-wide kernels), with and without a scale"""
    generic = request.node.callspec.id.endswith("generic")
    gpair, spair = ((F32, F32), (F32, F32)) if generic and C == 96 else ((F32, BF16), (BF16, F32))
    assert mc.takes_8wide(C, *gpair, "gather") == (not generic) and mc.takes_8wide(C, *spair, "scatter") == (not generic)
    for geom in mc.PADDED_GEOMS + (mc.extra_geoms(C) if C in mc.PATH8_WIDTHS else ("ident333",)):
        for scaled in (False, True):
            c = mc.gather_case(C, geom, *gpair, scaled)
            assert not mc.judge_guard(_gather(ops, c, geom, guarded=True), mc.gather_def(c), f"gather {geom} scaled={scaled}")
        for flags in ((True, True, True), (False, False, False)):
            c = mc.scatter_case(C, geom, *spair, flags)
            assert not mc.judge_guard(_scatter(ops, c, geom, guarded=True), mc.scatter_def(c), f"scatter {geom} {flags}")


def test_more_images_than_a_grid_has_rows(ops):
    """B = 65536 fails the `B <= 65535` test of both entry points (blockIdx.y is the image on the 8-wide path): the generic kernels run"""
    g = mc.gather_case(8, "ident3", F32, BF16, True, B=mc.BIG_B)
    assert not mc.judge_guard(_gather(ops, g, "ident3", guarded=True), mc.gather_def(g))
    s = mc.scatter_case(8, "ident3", BF16, F32, B=mc.BIG_B)
    assert not mc.judge_guard(_scatter(ops, s, "ident3", guarded=True), mc.scatter_def(s))


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("wdt", [BF16, F32], ids=["8wide", "generic"])
@pytest.mark.parametrize("geom", mc.PADDED_GEOMS)
def test_gather_beside_a_non_finite_row(ops, geom, wdt, scaled):
    """row 0 of image 0 = +inf, of image 1 = NaN (the row the 8-wide kernel loads for a padding slot): padding slots stay +0, the slots of
    row 0 carry inf / NaN, every other slot is what the finite run gave"""
    for C in (96, 768):
        c = mc.gather_case(C, geom, F32, wdt, scaled, scale=(0.5, 2.0))
        finite = _gather(ops, c, geom)
        assert not mc.judge_values(finite, mc.gather_def(c))
        assert not mc.judge_poisoned_gather(_gather(ops, c, geom, x64=mc.poison_row0(c)), finite, c)


@pytest.mark.parametrize("wdt", [BF16, F32], ids=["8wide", "generic"])
def test_scatter_beside_a_non_finite_slot(ops, wdt):
    """one slot row of win = inf that inv points to from exactly one token, and NaN in every padding slot (no token reads one): only that
    token's row is non-finite"""
    geom = "pano13x25s3"
    for C in (96, 768):
        c = mc.scatter_case(C, geom, wdt, F32)
        t0 = c["S"] - 1
        slot = int(c["inv"][t0])
        assert int((c["inv"] == slot).sum()) == 1
        win = c["win"].clone()
        win[0, slot] = float("inf")
        win[:, c["wmap"] < 0] = float("nan")
        got, want = _scatter(ops, c, geom, win64=win), mc.scatter_def(c).float()
        bad = torch.zeros(c["B"], c["S"], dtype=torch.bool)
        bad[0, t0] = True
        assert torch.equal((~torch.isfinite(got)).any(2), bad) and not bool(torch.isfinite(got[0, t0]).any())
        assert torch.equal(got[~bad], want[~bad])


@pytest.mark.parametrize("C", [96, 768])
def test_adjoints_through_autograd(ops, C):
    """window_gather's backward is the scatter definition; window_scatter_add's backward returns the scaled gather, dout itself and the
    exact column sum of scale_b * dout as the bias gradient"""
    geom = "pano13x25s3"
    wmap, inv = _maps(ops, geom)
    a = mc.scatter_case(C, geom, BF16, F32, (False, False, False))              # win = the upstream gradient of a gather
    x = torch.zeros(a["B"], a["S"], C, device=DEV, requires_grad=True)
    win = ops.window_gather(x, wmap, inv, BF16)
    win.backward(_dev(a["win"], BF16))
    assert not mc.judge_values(x.grad.cpu(), mc.scatter_def(a), "gather backward")
    for cls in ("exact", "ties"):
        b = mc.gather_case(C, geom, F32, BF16, True, cls)                         # x = the upstream gradient of a scatter-add
        w = torch.zeros(b["B"], b["n_slots"], C, dtype=BF16, device=DEV, requires_grad=True)
        resid = torch.zeros(b["B"], b["S"], C, device=DEV, requires_grad=True)
        bias = torch.zeros(C, device=DEV, requires_grad=True)
        dout = _dev(b["x"], F32)
        ops.window_scatter_add(w, resid, wmap, inv, _scale(b), bias, bias_grad_elsewhere=False).backward(dout)
        assert w.grad.dtype == BF16 and not mc.judge_values(w.grad.cpu(), mc.gather_def(b), f"dwin ({cls})")
        assert torch.equal(resid.grad, dout)
        want_db = (b["x"] * b["scale"][:, None, None]).sum((0, 1))
        assert float((b["x"].abs() * b["scale"][:, None, None]).sum((0, 1)).max()) * 2 < mc.LIMIT
        assert not mc.judge_values(bias.grad.cpu(), want_db, f"dbias ({cls})")


# ---------------------------------------------------------------------------------------------------------------------
# B. interp_rows and its adjoint
# ---------------------------------------------------------------------------------------------------------------------
INTERP = [(k, P, C) for k in ("random", "row7") for P in mc.INTERP_P for C in mc.INTERP_C] + [("identity", mc.INTERP_S, C) for C in mc.INTERP_C]


@pytest.mark.parametrize("kind,P,C", INTERP)
def test_interp_rows_and_its_adjoint(ops, kind, P, C):
    """out = T x and dx = T^T dout for the dense float64 T of the taps; every sum is exact, so the order of the adjoint's atomics is free"""
    c = mc.interp_case(kind, P, C)
    x = _dev(c["x"], F32).requires_grad_(True)
    out = ops.interp_rows(x, c["idx"].to(torch.int32).to(DEV), _dev(c["w"], F32))
    out.backward(_dev(c["dout"], F32))
    assert not mc.judge_interp(out.detach().cpu(), x.grad.cpu(), c)


# ---------------------------------------------------------------------------------------------------------------------
# C. column sums
# ---------------------------------------------------------------------------------------------------------------------
def _cid(p):
    return f"{mc.DT_NAME[p[0]]}-N{p[1]}-M{p[2]}" + ("-" + p[3] if len(p) > 3 else "")


def _blocks(c):
    lib = _lib()
    R = lib.load().pswin_colsum_workspace(c["M"], c["N"], lib.BF16 if c["dt"] == BF16 else lib.F32) // c["N"]
    assert R == c["R"]
    return R


@pytest.mark.parametrize("p", mc.colsum_cases(), ids=_cid)
def test_colsum_abi(ops, p):
    """pswin_colsum with an output: NaN-filled, inside guard bands; the workspace NaN-filled and guarded as well.  One pass
    (rowsum_direct_kernel: the workspace stays untouched) or partial rows (each the exact sum of its own rows) + colsum_kernel"""
    lib = _lib()
    c = mc.colsum_case(*p)
    R = _blocks(c)
    x = _dev(c["x"], c["dt"])
    out = mc.guarded(1, c["N"], F32, fill=float("nan")).to(DEV)
    ws = mc.guarded(R, c["N"], F32, fill=float("nan")).to(DEV)
    lib.call("pswin_colsum", x, lib.ptr(x), lib.dtype_code(x), c["M"], c["N"], _row_ptr(out), _row_ptr(ws))
    assert not mc.judge_guard(out.cpu(), mc.colsum_def(c)[None], "column sums")
    ws = ws.cpu()
    if mc.takes_direct(c["M"], c["N"], c["dt"]):
        fresh = mc.guarded(R, c["N"], F32, fill=float("nan"))
        assert torch.equal(mc.bits(ws), mc.bits(fresh))
    elif c["M"] <= 4097:
        assert not mc.judge_guard(ws, mc.partial_def(c), "partial rows")
    else:                                                     # the capped grid: every partial row written, their sum the column sums
        inner = ws[mc.GUARD:mc.GUARD + R]
        assert torch.equal(mc.bits(ws[:mc.GUARD]), mc.bits(mc.guarded(R, c["N"], F32)[:mc.GUARD])) and torch.equal(mc.bits(ws[mc.GUARD + R:]), mc.bits(mc.guarded(R, c["N"], F32)[:mc.GUARD]))
        assert not bool(torch.isnan(inner).any()) and torch.equal(inner.double().sum(0), mc.colsum_def(c))


@pytest.mark.parametrize("M", [4096, 4097])
@pytest.mark.parametrize("dt,N", mc.OPS_COLSUM, ids=lambda v: mc.DT_NAME.get(v, f"N{v}"))
def test_colsum_through_ops(ops, dt, N, M):
    """ops.colsum: pswin_reduce_jobs alone up to 4096 rows, partial rows + pswin_reduce_jobs beyond"""
    c = mc.colsum_case(dt, N, M)
    assert not mc.judge_values(ops.colsum(_dev(c["x"], dt)).cpu(), mc.colsum_def(c))


@pytest.mark.parametrize("which", range(5), ids=["empty", "everything", "first-chunk", "across-group-256", "last-group"])
@pytest.mark.parametrize("dt,N,M", mc.SKIP_CASES, ids=lambda v: mc.DT_NAME.get(v, str(v)))
def test_colsum_skip(ops, dt, N, M, which):
    """the skipped columns of x hold NaN: not read.  Every partial row holds +0 there and the exact sums elsewhere"""
    lib = _lib()
    c = mc.colsum_case(dt, N, M)
    lo, hi = mc.skip_ranges(N, dt)[which]
    R = _blocks(c)
    xf = c["x"].to(dt)
    xf[:, lo:hi] = float("nan")
    x = xf.to(DEV)
    ws = mc.guarded(R, N, F32, fill=float("nan")).to(DEV)
    lib.call("pswin_colsum_skip", x, lib.ptr(x), lib.dtype_code(x), M, N, lo, hi, _row_ptr(ws))
    ws = ws.cpu()
    assert not mc.judge_guard(ws, mc.partial_def(c, skip=(lo, hi)), "partial rows")
    assert not mc.judge_partials(ws[mc.GUARD:mc.GUARD + R], c, (lo, hi))
    want = mc.colsum_def(c)
    want[lo:hi] = 0.0
    assert not mc.judge_values(ops.colsum(x, zero_cols=(lo, hi)).cpu(), want)


# ---------------------------------------------------------------------------------------------------------------------
# D. pswin_reduce_jobs
# ---------------------------------------------------------------------------------------------------------------------
def _reduction(src, spec):
    """(job, its guarded destination buffer): the destination NaN-filled between rows of sentinel"""
    from panoswintransformerobjectdetection_amd import grad_queue
    rows, dt, cols, ld, off = spec
    buf = mc.guarded(1, cols, F32, fill=float("nan")).to(DEV)
    return grad_queue.Reduction(src, off * src.element_size(), _lib().dtype_code(src), rows, cols, ld, buf[mc.GUARD]), buf


@pytest.fixture(scope="module")
def reduce_jobs():
    """per spec: (spec, source on the device, float64 sums, the result of the job launched ALONE)"""
    from panoswintransformerobjectdetection_amd import grad_queue
    out = []
    for i, spec in enumerate(mc.reduce_specs()):
        src64 = mc.reduce_src(spec, i)
        src = _dev(src64, spec[1])
        job, buf = _reduction(src, spec)
        grad_queue._launch_reductions([job])
        out.append((spec, src, mc.reduce_def(src64, spec), buf))
    torch.cuda.synchronize()
    return [(spec, src, want, buf.cpu()) for spec, src, want, buf in out]


@pytest.mark.parametrize("n", [1, 96, 97, 193, 0], ids=lambda n: f"{n}-jobs" if n else "every-job")
def test_reduce_jobs(ops, reduce_jobs, n):
    """one grouped launch (n jobs: the list trimmed or cycled; 97 and beyond split at the job table's 96 entries): every job equals its
    float64 sum and what it returned when launched alone, and writes nothing around its destination"""
    from panoswintransformerobjectdetection_amd import grad_queue
    picked = mc.cycled(reduce_jobs, n or len(reduce_jobs))
    made = [_reduction(src, spec) for spec, src, _, _ in picked]
    grad_queue._launch_reductions([job for job, _ in made])
    torch.cuda.synchronize()
    for (spec, _, want, alone), (_, buf) in zip(picked, made):
        buf = buf.cpu()
        assert not mc.judge_guard(alone, want[None], f"alone {spec}")
        assert not mc.judge_guard(buf, want[None], f"grouped {spec}")
        assert torch.equal(mc.bits(buf), mc.bits(alone))


# ---------------------------------------------------------------------------------------------------------------------
# E. table gradients
# ---------------------------------------------------------------------------------------------------------------------
def _table_job(c):
    from panoswintransformerobjectdetection_amd import grad_queue
    lib = _lib().load()
    heads = c["heads"]
    g = mc.pad64(c["g"]).float().to(DEV)
    dist = None if c["dist"] is None else mc.pad64(c["dist"]).float().to(DEV)
    dbeta = mc.guarded(mc.NBINS, heads, F32, fill=float("nan")).to(DEV)
    dalpha = mc.guarded(mc.NBINS, heads, F32, fill=float("nan")).to(DEV) if dist is not None else None
    ws = torch.full((lib.pswin_attn_table_grads_workspace(heads),), float("nan"), device=DEV)
    rows = slice(mc.GUARD, mc.GUARD + mc.NBINS)
    job = grad_queue.TableGrad(g, dist, None if dalpha is None else dalpha[rows], dbeta[rows], ws, c["n_tiles"], c["nb"], c["n_dist"], heads)
    return job, dalpha, dbeta


def _judge_table_buffers(dalpha, dbeta, c):
    wa, wb = mc.table_def(c)
    return mc.judge_guard(dbeta.cpu(), wb, "dbeta") + ([] if wa is None else mc.judge_guard(dalpha.cpu(), wa, "dalpha"))


def _queued_stages(job):
    """the three steps as grad_queue.table_gradients issues them: stage 1, the row sum of the partials as a reduction, stage 4"""
    from panoswintransformerobjectdetection_amd import grad_queue
    lib = _lib()
    ld = job.workspace.numel() // 129
    blocks = lib.load().pswin_attn_table_grads_partial_rows(job.n_tiles, job.heads)
    grad_queue._launch_table_grads([job], 1)
    grad_queue._launch_reductions([grad_queue.Reduction(job.workspace, 0, lib.F32, blocks, ld, ld, job.workspace[128 * ld:])])
    grad_queue._launch_table_grads([job], 4)
    return blocks


@pytest.mark.parametrize("shape", mc.table_shapes(), ids=lambda s: "h%d-t%d-nb%d-nd%d" % s)
def test_table_gradients(ops, shape):
    """dbeta, and dalpha where there is a distance table, from the one-call form (stages 1 + colsum_kernel + final) and from the queued
    form (stage 1, pswin_reduce_jobs, stage 4): both equal the float64 index_add_ over the 169 bins, NaN-filled outputs inside guard bands"""
    from panoswintransformerobjectdetection_amd import grad_queue
    c = mc.table_case(*shape)
    job, dalpha, dbeta = _table_job(c)
    grad_queue._launch_table_grads([job])
    assert not _judge_table_buffers(dalpha, dbeta, c)
    job, dalpha, dbeta = _table_job(c)
    assert _queued_stages(job) == mc.dtab_blocks(c["n_tiles"], c["heads"])
    assert not _judge_table_buffers(dalpha, dbeta, c)


def test_table_gradient_batch_equals_the_single_launches(ops):
    from panoswintransformerobjectdetection_amd import grad_queue
    cases = [mc.table_case(*s) for s in ((1, 129, 129, 1), (24, 24, 12, 4), (3, 127, 127, 0))]
    made = [_table_job(c) for c in cases]
    grad_queue._launch_table_grads([m[0] for m in made])
    for c, (_, dalpha, dbeta) in zip(cases, made):
        assert not _judge_table_buffers(dalpha, dbeta, c)
        job, a1, b1 = _table_job(c)
        grad_queue._launch_table_grads([job])
        assert torch.equal(mc.bits(b1.cpu()), mc.bits(dbeta.cpu())) and (a1 is None or torch.equal(mc.bits(a1.cpu()), mc.bits(dalpha.cpu())))


def test_padded_tiles_are_bit_copies(ops):
    """Tiles(table, symmetric=False): pswin_attn_pad_tiles gives the padded copy and the padded transpose of any bit pattern, NaN payloads
    included"""
    t = mc.random_bit_table(5)
    tiles = ops.Tiles(t.view(F32).to(DEV), symmetric=False)
    assert torch.equal(tiles.fwd.cpu().view(torch.int32), mc.pad64(t))
    assert torch.equal(tiles.bwd.cpu().view(torch.int32), mc.pad64(t.transpose(1, 2).contiguous()))
