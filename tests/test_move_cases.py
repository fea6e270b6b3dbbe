"""tests/_move_cases.py checked on the CPU before anything goes to a GPU: the conditions the exact assertions of
tests/test_move_exact_gpu.py rest on (bounded sums, ties that are ties, injective maps, the four tail configurations of the 8-wide row
movers per width, the block counts the column-sum cases aim for), the float32 evaluation of every definition equal to the float64 one bit
for bit, and every judge applied to the definition's own output with one planted defect at a time.  The last test prints which judge caught
each defect."""
import pytest
import torch

import _move_cases as mc
from _gemm_exact_cases import is_tie, rne_bf16

F32, BF16, F64 = mc.F32, mc.BF16, mc.F64

GATHER, SCATTER = mc.gather_params(), mc.scatter_params()


def test_maps_are_injective_with_the_padding_slots_counted():
    for geom, (S, slots, pads) in mc.GEOM_COUNTS.items():
        wmap, inv = mc.maps(geom)
        assert (len(inv), len(wmap), int((wmap < 0).sum())) == (S, slots, pads), geom
        real = wmap[wmap >= 0]
        assert len(torch.unique(real)) == len(real) == S and torch.equal(torch.sort(real).values, torch.arange(S))
        assert torch.equal(wmap[inv], torch.arange(S)) and len(torch.unique(inv)) == S
    wmap, inv = mc.maps("ident333")
    assert torch.equal(wmap, torch.arange(333)) and inv is wmap


def test_odd_integers_from_257_to_511_are_bf16_ties_and_round_to_even():
    odd = torch.arange(257, 512, 2, dtype=F64)
    for v in (odd, -odd):
        assert bool(is_tie(v).all())
        lo, hi = v - 1, v + 1                                     # the two bf16 neighbours
        assert mc.fits(lo, BF16) and mc.fits(hi, BF16)
        even = torch.where((lo / 2) % 2 == 0, lo, hi)             # the one whose last kept bit is 0 (a bf16 ulp is 2 in [256, 512))
        assert torch.equal(rne_bf16(v).double(), even)
        assert bool((mc.round_ties_away(v).double() == v + v.sign()).all())
    assert not bool(is_tie(torch.arange(-256, 257, dtype=F64)).any())


@pytest.mark.parametrize("C", mc.PATH8_WIDTHS)
def test_every_tail_of_the_8_wide_kernels_is_in_the_case_list(C):
    rpb = 256 // (C // 8)
    assert mc.rpb8(C) == rpb
    for kind, params, rows_of in (("gather", GATHER, lambda geom: len(mc.maps(geom)[0])), ("scatter", SCATTER, lambda geom: len(mc.maps(geom)[1]))):
        seen = set()
        for p in params:
            if p[0] == C and mc.takes_8wide(C, p[2], p[3], kind):
                seen |= mc.tail_kinds(rows_of(p[1]), C)
        assert seen >= mc.required_tails(C), (kind, C, seen)
    assert mc.required_tails(C) == ({"u1_past", "u1_cut", "u0_cut", "single"} if rpb >= 2 else {"u1_past", "single"})
    assert rpb >= 2 or C == 2048                                  # the one width whose row groups are single rows
    if C == 8:
        assert mc.tail_kinds(98, 8) >= {"single", "u1_past"}      # rpb = 256: one block, every u = 1 row clamped


def test_idle_threads_and_the_dispatch_of_the_widths():
    assert [(mc.rpb8(C), 256 - mc.rpb8(C) * (C // 8)) for C in (192, 384, 768)] == [(10, 16), (5, 16), (2, 64)]
    assert mc.takes_8wide(2048, F32, BF16, "gather") and not mc.takes_8wide(2056, F32, BF16, "gather")
    assert not mc.takes_8wide(8, F32, BF16, "gather", B=mc.BIG_B) and not mc.takes_8wide(96, F32, F32, "scatter")
    assert {p[4] for p in SCATTER if p[0] in mc.FLAG_WIDTHS_8 and (p[2], p[3]) == (BF16, F32)} == set(mc.FLAGS)
    assert {p[4] for p in SCATTER if p[0] == 96 and (p[2], p[3]) == (F32, F32)} == set(mc.FLAGS)
    for pair in mc.DT_PAIRS:
        assert {p[0] for p in GATHER if (p[2], p[3]) == pair} == set(mc.WIDTHS) == {p[0] for p in SCATTER if (p[2], p[3]) == pair}
    assert {(p[4], p[5]) for p in GATHER if (p[2], p[3]) == (F32, BF16)} == {(s, k) for s in (False, True) for k in ("exact", "ties")}


@pytest.mark.parametrize("p", GATHER, ids=mc.mover_id)
def test_gather_case_is_exact(p):
    c = mc.gather_case(*p)
    assert not mc.mover_conditions(c)
    assert torch.equal(mc.gather_def(c, F32).double(), mc.gather_def(c))
    if c["scale"] is not None and p[5] == "exact":
        assert float(c["scale"][0]) in (0.0, 0.5) and float(c["scale"][1]) == 2.0


@pytest.mark.parametrize("p", SCATTER, ids=mc.mover_id)
def test_scatter_case_is_exact(p):
    c = mc.scatter_case(*p)
    assert not mc.mover_conditions(c)
    assert torch.equal(mc.scatter_def(c, F32).double(), mc.scatter_def(c))
    assert [c["scale"] is not None, c["resid"] is not None, c["bias"] is not None] == list(p[4])


def test_the_many_images_case_is_small_and_exact():
    c = mc.gather_case(8, "ident3", F32, BF16, True, B=mc.BIG_B)
    assert not mc.mover_conditions(c) and c["x"].numel() * 4 < 10 * 2 ** 20
    assert set(c["scale"].tolist()) <= {0.0, 0.5, 2.0}
    s = mc.scatter_case(8, "ident3", BF16, F32, B=mc.BIG_B)
    assert not mc.mover_conditions(s) and torch.equal(mc.scatter_def(s, F32).double(), mc.scatter_def(s))


INTERP = [(k, P, C) for k in ("random", "row7") for P in mc.INTERP_P for C in mc.INTERP_C] + [("identity", mc.INTERP_S, C) for C in mc.INTERP_C]


@pytest.mark.parametrize("kind,P,C", INTERP)
def test_interp_case_is_exact(kind, P, C):
    c = mc.interp_case(kind, P, C)
    assert not mc.interp_conditions(c)
    for a, b in zip(mc.interp_def(c, F32), mc.interp_def(c)):
        assert torch.equal(a.double(), b)
    assert not mc.judge_interp(*[t.float() for t in mc.interp_def(c)], c)
    reached = mc.reached_rows(c)
    if kind == "row7":
        assert reached.tolist() == [i == 7 for i in range(mc.INTERP_S)]
    if kind == "random":
        assert not bool(reached[0]) and bool((c["idx"][c["w"] == 0] == 0).all()) and bool((c["w"] == 0).any() or P == 1)
    if kind == "identity":
        assert bool(reached.all())


COLSUM = mc.colsum_cases()


def _cid(p):
    return f"{mc.DT_NAME[p[0]]}-N{p[1]}-M{p[2]}" + ("-" + p[3] if len(p) > 3 else "")


@pytest.mark.parametrize("p", COLSUM + [(dt, N, M, "ints") for dt, N in mc.OPS_COLSUM for M in (4096, 4097)] + [p + ("ints",) for p in mc.SKIP_CASES], ids=_cid)
def test_colsum_case_is_exact(p):
    c = mc.colsum_case(*p)
    assert not mc.colsum_conditions(c)
    assert torch.equal(mc.colsum_def(c, F32).double(), mc.colsum_def(c))
    if c["M"] <= 4097:
        part = mc.partial_def(c)
        assert torch.equal(part.sum(0), mc.colsum_def(c)) and torch.equal(mc.partial_def(c, F32).double(), part)


def test_the_column_sum_cases_reach_the_block_counts_they_aim_for():
    geom = lambda dt, N, M: mc.rowsum_geom(M, N, dt)
    assert [geom(BF16, 2048, 8 * R - 3)["R"] for R in mc.STAGE2_R] == list(mc.STAGE2_R) and geom(BF16, 2048, 5)["rpi"] == 1
    for dt in (BF16, F32):
        # N % 8 == 0 makes the f32 group count even: 8200 columns are 2050 groups, a last block of 32 with TWO live groups (bf16: one)
        assert [N // mc.ve_of(dt) for N in mc.DIRECT_N[dt]] == [2048, 2049 if dt == BF16 else 2050]
        assert all(mc.takes_direct(M, N, dt) == (M <= 1024) for N in mc.DIRECT_N[dt] for M in mc.DIRECT_M)
    g = geom(BF16, 288, 1003)
    assert (g["vpr"], g["rpi"], 256 - g["rpi"] * g["vprb"]) == (36, 7, 4)
    g = geom(BF16, 3072, 4097)
    assert (g["vpr"], g["ychunks"], g["R"]) == (384, 2, 513)
    assert geom(BF16, 8, 4097)["rpi"] == 256 and geom(F32, 8, 4097)["rpi"] == 128
    assert all(M % (geom(dt, N, M)["rpi"] * 8) for dt, N in mc.TWO_STAGE for M in (1003,))
    for dt, N, M in mc.CAPPED:                                   # the grid is capped and blocks 0 .. 4 make a ninth trip
        g = geom(dt, N, M)
        assert g["R"] == 2048 and g["rpi"] == 1 and M - 8 * 2048 == 5
    for dt, N, M in mc.SKIP_CASES:
        assert geom(dt, N, M)["vpr"] == 384 and all(lo % mc.ve_of(dt) == 0 and hi % mc.ve_of(dt) == 0 and 0 <= lo <= hi <= N for lo, hi in mc.skip_ranges(N, dt))
    big = [p for p in COLSUM if p[1] * p[2] * (2 if p[0] == BF16 else 4) > 60 * 2 ** 20]          # the two largest operands of the file, 67 MB
    assert sorted(p[2] for p in big) == [16389, 16389]


SPECS = mc.reduce_specs()


def test_reduce_jobs_cover_the_lane_shapes_and_are_exact():
    assert {mc.rj_groups_per_block(r) for r in mc.RJ_ROWS} == {1024, 128, 16}
    assert [mc.rj_groups_per_block(r) for r in (16, 17, 128, 129)] == [1024, 128, 128, 16]
    for rows in mc.RJ_ROWS:
        G = mc.rj_groups_per_block(rows)
        for dt in (F32, BF16):
            groups = {s[2] // mc.ve_of(dt) for s in SPECS if s[0] == rows and s[1] == dt}
            assert groups == {1, G - 1, G, G + 1, 2 * G + 1}
            assert {s[3] > s[2] for s in SPECS if s[0] == rows and s[1] == dt} == {False, True}
    assert len(SPECS) > 97 and mc.RJ_MAX == 96
    for n in (96, 97, 193):                                      # the trimmed and the cycled lists keep every lane shape and both dtypes
        picked = mc.cycled(SPECS, n)
        assert len(picked) == n and {(mc.rj_groups_per_block(s[0]), s[1]) for s in picked} == {(G, dt) for G in (1024, 128, 16) for dt in (F32, BF16)}
    assert mc.cycled(SPECS, len(SPECS)) == SPECS and len(mc.cycled(SPECS, 1)) == 1
    for i, s in enumerate(SPECS):
        src = mc.reduce_src(s, i)
        assert float(src.abs().sum(0).max()) < mc.LIMIT and mc.fits(src, s[1])
        assert torch.equal(mc.reduce_def(src, s, F32).double(), mc.reduce_def(src, s))


TABLES = mc.table_shapes()


def test_table_shapes_walk_the_block_cap_and_the_distance_indexing():
    assert (mc.dtab_cap(1), mc.dtab_cap(3), mc.dtab_cap(24)) == (128, 128, 22)
    for heads, wanted in ((1, {1, 15, 16, 17, 127, 128, 129, 257}), (3, {127, 129}), (24, {21, 22, 23, 45})):
        for nd in (0, 1):
            assert {n for h, n, nb, d in TABLES if h == heads and nb == n and d == nd} == wanted
    assert {(nb, nd) for h, n, nb, nd in TABLES if nb != n} == {(12, 4), (15, 15), (20, 5)}
    assert all(n % nb == 0 and (nd == 0 or nb % nd == 0) for h, n, nb, nd in TABLES)
    assert all(n > mc.dtab_cap(h) for h, n, nb, nd in TABLES if nb != n)


@pytest.mark.parametrize("shape", TABLES, ids=lambda s: "h%d-t%d-nb%d-nd%d" % s)
def test_table_case_is_exact(shape):
    c = mc.table_case(*shape)
    assert not mc.table_conditions(c)
    for a, b in zip(mc.table_def(c, F32), mc.table_def(c)):
        assert (a is None and b is None) or torch.equal(a.double(), b)


def test_guarded_buffers_and_bit_tables():
    for dt in (F32, BF16):
        buf = mc.guarded(3, 8, dt, fill=float("nan"))
        assert buf.shape == (3 + 2 * mc.GUARD, 8) and bool(torch.isnan(buf[mc.GUARD:-mc.GUARD]).all())
        v = float(buf[0, 0])                                     # the sentinel is finite and no result of any case: far too large, or no half-integer
        assert bool(torch.isfinite(buf[:mc.GUARD]).all()) and (abs(v) > 2.0 ** 24 or 2 * v != round(2 * v))
    t = mc.random_bit_table(3)
    f = t.view(F32)
    assert bool(torch.isnan(f).any()) and bool(torch.isinf(f).any()) and torch.equal(mc.pad64(t)[:, :49, :49], t)


# ---------------------------------------------------------------------------------------------------------------------
# every judge sees every planted defect (and passes the definition's own output)
# ---------------------------------------------------------------------------------------------------------------------
def _in_guard(out64, dtype):
    rows = out64.reshape(-1, out64.shape[-1])
    buf = mc.guarded(rows.shape[0], rows.shape[1], dtype)
    buf[mc.GUARD:mc.GUARD + rows.shape[0]] = mc.cast(rows, dtype)
    return buf


def _defects():
    """name -> (complaints on the clean output, complaints on the output with the defect)"""
    found = {}
    g8 = mc.gather_case(96, "pano5x9s3", F32, BF16, True)
    want = mc.gather_def(g8)
    buf = _in_guard(want, BF16)
    clean = mc.judge_guard(buf, want)
    bad = buf.clone()
    mc.bits(bad)[mc.GUARD + want.shape[0] * want.shape[1] - 1] = mc.SENTINEL[BF16]
    found["the last row not written"] = (clean, mc.judge_guard(bad, want))
    bad = buf.clone()
    bad[mc.GUARD + want.shape[0] * want.shape[1], 5] = 1.0
    found["the first row of the trailing guard band written"] = (clean, mc.judge_guard(bad, want))

    for scaled in (False, True):
        c = mc.gather_case(96, "planar8x9s3", F32, BF16, scaled, scale=(0.5, 2.0))
        fin, x = mc.cast(mc.gather_def(c), BF16), mc.poison_row0(c)
        got = mc.cast(mc.gather_def(c, x=x), BF16)
        bad = got.clone()
        bad[:, c["wmap"] < 0] = mc.cast(0.0 * x[:, 0:1], BF16)
        found[f"a padding slot holding 0 * row 0 with row 0 = inf ({'scaled' if scaled else 'plain'})"] = (
            mc.judge_poisoned_gather(got, fin, c), mc.judge_poisoned_gather(bad, fin, c))

    s8 = mc.scatter_case(96, "pano13x25s3", BF16, F32)
    clean = mc.judge_values(mc.scatter_def(s8).float(), mc.scatter_def(s8))
    found["the scale of image 0 used for image 1 (gather)"] = (mc.judge_values(mc.cast(want, BF16), want), mc.judge_values(mc.cast(mc.gather_def(g8, swap_scale=True), BF16), want))
    found["the scale of image 0 used for image 1 (scatter)"] = (clean, mc.judge_values(mc.scatter_def(s8, swap_scale=True).float(), mc.scatter_def(s8)))
    found["bias added after the scale instead of before"] = (clean, mc.judge_values(mc.scatter_def(s8, bias_after_scale=True).float(), mc.scatter_def(s8)))
    for name, c, d in (("gather", mc.gather_case(96, "pano5x9s3", F32, BF16, True, "ties"), mc.gather_def),
                       ("scatter", mc.scatter_case(96, "pano5x9s3", F32, BF16, cls="ties"), mc.scatter_def)):
        found[f"a tie rounded away from even ({name})"] = (mc.judge_values(mc.cast(d(c), BF16), d(c)), mc.judge_values(mc.round_ties_away(d(c)), d(c)))

    for cls in ("ints", "big"):
        c = mc.colsum_case(BF16, 2048, 8 * 257 - 3, cls)
        clean = mc.judge_values(mc.colsum_def(c).float(), mc.colsum_def(c))
        r = c["M"] // 2
        found[f"one column-sum row dropped ({cls})"] = (clean, mc.judge_values(mc.colsum_def(c, drop=r).float(), mc.colsum_def(c)))
        found[f"one column-sum row doubled ({cls})"] = (clean, mc.judge_values(mc.colsum_def(c, double=r).float(), mc.colsum_def(c)))
    found["the partial rows of the last block left unsummed in the second stage"] = (clean, mc.judge_values(mc.partial_def(c)[:-1].sum(0).float(), mc.colsum_def(c)))
    c = mc.colsum_case(*mc.SKIP_CASES[1])
    for lo, hi in mc.skip_ranges(c["N"], c["dt"])[1:]:
        found[f"a skipped column summed instead of zeroed (columns {lo} .. {hi})"] = (
            mc.judge_partials(mc.partial_def(c, skip=(lo, hi)).float(), c, (lo, hi)), mc.judge_partials(mc.partial_def(c, skip=(lo, hi), sum_skipped=True).float(), c, (lo, hi)))

    spec = next(s for s in SPECS if s[0] == 17 and s[3] > s[2])
    src = mc.reduce_src(spec)
    found["a reduce job reading ld = cols when ld > cols"] = (mc.judge_values(mc.reduce_def(src, spec).float(), mc.reduce_def(src, spec)),
                                                             mc.judge_values(mc.reduce_def(src, spec, ld_is_cols=True).float(), mc.reduce_def(src, spec)))

    c = mc.interp_case("random", 98, 8)
    found["an interp_rows tap with weight 0 still contributing"] = (mc.judge_interp(*[t.float() for t in mc.interp_def(c)], c),
                                                                   mc.judge_interp(*[t.float() for t in mc.interp_def(c, zero_tap_weight=1 / 16)], c))
    dx_only = [mc.interp_def(c)[0].float(), mc.interp_def(c, zero_tap_weight=1 / 16)[1].float()]
    found["... in the adjoint alone: an unreached row is not 0"] = ([], [m for m in mc.judge_interp(*dx_only, c) if "no non-zero tap" in m])

    c = mc.table_case(3, 30, 15, 15)
    clean = mc.judge_table(*[t.float() for t in mc.table_def(c)], c)
    found["a table-gradient bin built from (j, i) instead of (i, j)"] = (clean, mc.judge_table(*[t.float() for t in mc.table_def(c, transposed_bins=True)], c))
    c = mc.table_case(1, 30, 15, 4)                              # n_dist does not divide nb: for this check only, the entry points refuse it
    assert 15 % 4
    found["the distance tile taken as tile % n_dist"] = (mc.judge_table(*[t.float() for t in mc.table_def(c)], c),
                                                        mc.judge_table(*[t.float() for t in mc.table_def(c, plain_modulo=True)], c))
    return found


PLANTED = ("the last row not written", "the first row of the trailing guard band written", "a padding slot holding 0 * row 0", "the scale of image 0 used for image 1",
           "a tie rounded away from even", "bias added after the scale", "one column-sum row dropped", "one column-sum row doubled",
           "a skipped column summed instead of zeroed", "the partial rows of the last block left unsummed", "a reduce job reading ld = cols",
           "an interp_rows tap with weight 0 still contributing", "a table-gradient bin built from (j, i)", "the distance tile taken as tile % n_dist")


def test_every_judge_flags_every_planted_defect(capsys):
    found = _defects()
    with capsys.disabled():
        print()
        for name, (clean, bad) in found.items():
            print(f"  planted defect caught: {name}: {bad[0] if bad else 'NOT CAUGHT'}")
    for name, (clean, bad) in found.items():
        assert not clean, (name, clean)
        assert bad, name
    assert len(PLANTED) == 14
    for p in PLANTED:
        assert any(name.startswith(p) for name in found), p
