"""LightGlue's head and tail one launcher at a time (airfe_debug_lg_prepare / airfe_debug_lg_assign, include/airfe_debug.h) against the float64 references and
derived bounds of tests/lg_tail_ref.py: lg_prepare_kernel; rowdot256_kernel; sim_kernel; the matrix-form assignment (form 0: lg_lse_kernel / lg_arg_kernel for
B <= 8, lg_rowlse / lg_collse / lg_rowarg / lg_colarg above) and the fused one (form 1: lg_sim_lse_kernel / lg_sim_arg_kernel / lg_filter_fused_kernel), with
lg_filter_kernel behind form 0.  tests/test_gpu_lightglue.py reaches these kernels only behind a whole 2-byte network (gate 0.05 on the scores).  Here z and sim
are held to float64 of the host inputs, the log-sum-exps and the scores to float64 of the DEVICE's own float32 sim and z, and every decision (row / column first
maximum, the match list) to the scan of the device's own scores, exactly — and to the float64 decisions wherever the bounds settle them.  The hooks start every
launch with NaN in all padding rows and in every output, and ZERO in rowarg / colarg / idx (the value that passes for a valid index), so "finite" means "written,
and from inside lens only".  Measured error-to-bound ratios: DESIGN.md §2a.

Mutations applied to kernels_lg.hip one at a time (scratch builds, never committed), and the tests of this file that failed on each on the MI355X:
  reduce_rows16 without reduce_step<1>                          52 tests, the first test_lengths_vs_float64[400-400-400-fp16]
  lg_sim_lse_kernel's row maximum taken without the cv mask     test_finite_padding_stays_out_of_every_reduction[fp16], [bf16] and no other: with NaN padding
                                                                fmaxf drops the padded column on its own, which is why the hook takes a finite `pad`
  ba_merge preferring the HIGHER index on ties (b.i > a.i)      test_families_vs_float64[constant-*] (4): ba_merge folds lanes WITHIN a tile, where only the
                                                                constant family ties; dup's ties lie across tiles (the filters' fold)
"""
import numpy as np
import pytest

import lg_tail_ref as R
from airslam_amd import api, weights
from gpu_common import diag

pytestmark = pytest.mark.gpu
PRECS = pytest.mark.parametrize("prec", [1, 0], ids=["fp16", "bf16"])
CONTEXTS = {400: dict(max_keypoints=400, max_batch=16), 1024: dict(max_keypoints=1024, max_batch=2)}
W, BIAS = R.matchability()
THR = 0.1
_C, _IN, _ALONE = {}, {}, {}


def _ctx(k):
    if k not in _C:
        _C[k] = api.Context(lightglue=weights.synthetic_lightglue(1234, n_layers=1), **CONTEXTS[k])       # only the arena matters
    return _C[k]


def _inputs(kind, n0, n1):
    key = (kind, n0, n1)
    if key not in _IN:
        _IN[key] = R.family(kind, n0, n1, R.case_seed(kind, n0, n1))
    return _IN[key]


def _launch(k, cases, prec, form, cap=None, pad=None):
    """one hook call on the batch `cases` [(kind, n0, n1), ...] -> the hook's dict"""
    n = max(1, max(max(c[1], c[2]) for c in cases))
    md, x = np.zeros((2 * len(cases), n, 256), np.float32), np.zeros((2 * len(cases), n, 256), np.float32)
    lens = []
    for b, (kind, n0, n1) in enumerate(cases):
        md0, md1, x0, x1 = _inputs(kind, n0, n1)
        md[2 * b, :n0], md[2 * b + 1, :n1], x[2 * b, :n0], x[2 * b + 1, :n1] = md0, md1, x0, x1
        lens += [n0, n1]
    return _ctx(k).debug_lg_assign(md, x, lens, W, BIAS, prec, form, cap=cap, thr=THR, pad=pad)


def _pair(out, b, n0, n1):
    """pair b's outputs cut to its lengths (idx / score whole)"""
    cut = {"z0": out["z"][2 * b, :n0], "z1": out["z"][2 * b + 1, :n1], "sim": out["sim"][b, :n0, :n1], "scores": out["scores"][b, :n0, :n1],
           "rowlse": out["rowlse"][b, :n0], "collse": out["collse"][b, :n1], "rowarg": out["rowarg"][b, :n0], "rowval": out["rowval"][b, :n0],
           "colarg": out["colarg"][b, :n1], "idx": out["idx"][b], "score": out["score"][b], "nmatch": int(out["nmatch"][b])}
    return cut


def _ratio(name, got, ref, bound, bad):
    """max |got - ref| / bound (inf where got is not finite); -inf entries of ref must be met exactly"""
    got, ref, bound = (np.asarray(t, np.float64) for t in (got, ref, bound))
    if got.size == 0:
        return 0.0
    inf = np.isinf(ref)
    if inf.any() and not np.array_equal(got[inf], ref[inf]):
        bad.append((name, "expected -inf"))
    g, r, d = got[~inf], ref[~inf], bound[~inf]
    if g.size == 0:
        return 0.0
    if not np.isfinite(g).all():
        bad.append((name, "not finite", int((~np.isfinite(g)).sum())))
        return float("inf")
    ratio = float((np.abs(g - r) / d).max())
    if ratio > 1.0:
        k = int(np.argmax(np.abs(g - r) / d))
        bad.append((name, "ratio", ratio, "at", k, "got", float(g.flat[k]), "ref", float(r.flat[k]), "bound", float(d.flat[k])))
    return ratio


def _check(tag, p, case, prec, cap, against64=True):
    """one pair's outputs against everything the reference states -> the error-to-bound ratios"""
    kind, n0, n1 = case
    md0, md1, x0, x1 = _inputs(kind, n0, n1)
    bad, ratios = [], {}
    for side, x in (("z0", x0), ("z1", x1)):
        z, dz = R.z_ref(x, W, BIAS)
        ratios[side] = _ratio(side, p[side], z, dz, bad)
    s64, ds = R.sim_ref(md0, md1, prec)
    ratios["sim"] = _ratio("sim", p["sim"], s64, ds, bad)
    if not bad:                                     # (the references below are taken on the device's own sim and z: they must be finite)
        r = R.scores_ref(p["sim"], p["z0"], p["z1"])
        ratios["rowlse"] = _ratio("rowlse", p["rowlse"], r["rowlse"], r["d_rowlse"], bad)
        ratios["collse"] = _ratio("collse", p["collse"], r["collse"], r["d_collse"], bad)
        ratios["scores"] = _ratio("scores", p["scores"], r["scores"], r["d_scores"], bad)
    if not bad:
        d = R.scan(p["scores"], THR, cap)
        nm = p["nmatch"]
        for k in ("rowarg", "rowval", "colarg"):
            if not np.array_equal(p[k], d[k]):
                bad.append((k, "differs from the scan of the device's scores at", np.flatnonzero(p[k] != d[k])[:5].tolist()))
        if nm != d["nmatch"] or not np.array_equal(p["idx"][:nm], d["idx"]) or not np.array_equal(p["score"][:nm], d["score"]):
            bad.append(("match list", nm, d["nmatch"]))
        if np.any(p["idx"][nm:] != 0) or not np.isnan(p["score"][nm:]).all():
            bad.append(("written past the match count", nm))
        if against64 and n0 and n1:
            sr, sc = R.safe(r["scores"], r["d_scores"], 1), R.safe(r["scores"], r["d_scores"], 0)
            a1, a0 = np.argmax(r["scores"], 1), np.argmax(r["scores"], 0)
            if not np.array_equal(p["rowarg"][sr], a1[sr]) or not np.array_equal(p["colarg"][sc], a0[sc]):
                bad.append(("float64 decisions differ on settled rows / columns", np.flatnonzero(sr & (p["rowarg"] != a1))[:5].tolist(),
                            np.flatnonzero(sc & (p["colarg"] != a0))[:5].tolist()))
            ratios["fragile"] = int((~sr).sum() + (~sc).sum())
    diag(f"lgtail_{tag}_{kind}_{n0}x{n1}_{'fp16' if prec else 'bf16'}", nmatch=p["nmatch"], **ratios)
    assert not bad, (tag, case, prec, bad)
    return ratios


def _untouched(out, b, n0, n1):
    """pair b's outputs beyond its lengths are still the hook's poison"""
    assert np.isnan(out["rowlse"][b, n0:]).all() and np.isnan(out["rowval"][b, n0:]).all() and np.isnan(out["collse"][b, n1:]).all()
    assert not out["rowarg"][b, n0:].any() and not out["colarg"][b, n1:].any()
    assert np.isnan(out["scores"][b, n0:]).all() and np.isnan(out["scores"][b, :, n1:]).all()


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _alone(k, case, prec, form):
    """a pair's B = 1 outputs, launched once"""
    key = (k, case, prec, form)
    if key not in _ALONE:
        _ALONE[key] = _pair(_launch(k, [case], prec, form), 0, case[1], case[2])
    return _ALONE[key]


# ------------------------------------------------------------------ prepare
PREP = {  # lens per pair, ld, normalize, slack_rows, second pair
    "full_ragged": dict(lens=[(400, 317)], ld=259, norm=True, slack=0, second=None),
    "tiny_ld258": dict(lens=[(1, 5)], ld=258, norm=False, slack=37, second=None),
    "tile_edge_big_slack": dict(lens=[(64, 65)], ld=259, norm=False, slack=437, second=None),
    "batch_of_three": dict(lens=[(400, 317), (1, 5), (64, 65)], ld=258, norm=True, slack=37, second=None),
    "second_pair": dict(lens=[(400, 317)], ld=259, norm=True, slack=37, second=(64, 65)),
    "second_pair_empty_side": dict(lens=[(1, 5)], ld=259, norm=False, slack=0, second=(0, 33)),
}


@PRECS
@pytest.mark.parametrize("name", list(PREP))
def test_prepare_vs_float64(name, prec):
    """Token rows, their 2-byte shadow and lens exactly; the rotary tables within the argument's and the result's ulps at |argument| up to ~60 rad (wr up to
    +-30); padded rows exactly 0 / cos 1 / sin 0, slack rows exactly 0; every row finite (the arena started as NaN: every row was written) and no row beyond
    2 Bt Np + slack_rows touched."""
    c = PREP[name]
    ctx = _ctx(400)
    rng = np.random.default_rng(len(name) + 10 * c["ld"])
    kp = 1 if c["ld"] == 259 else 0
    norm = (376.0, 240.0, float(np.float32(1.0 / 752 * 0.5))) if c["norm"] else None

    def rows(n, cap):
        f = rng.normal(size=(cap, c["ld"])).astype(np.float32)
        f[:, kp], f[:, kp + 1] = (rng.uniform(0, 752, cap), rng.uniform(0, 480, cap)) if c["norm"] else (rng.uniform(-1, 1, cap), rng.uniform(-1, 1, cap))
        f[n:] = np.nan                                # rows beyond the count must not be read
        return f
    B = len(c["lens"])
    f0, f1 = np.stack([rows(n0, 400) for n0, _ in c["lens"]]), np.stack([rows(n1, 400) for _, n1 in c["lens"]])
    n0, n1 = [l[0] for l in c["lens"]], [l[1] for l in c["lens"]]
    wr = rng.uniform(-30, 30, size=(32, 2)).astype(np.float32)
    second = None if c["second"] is None else (rows(c["second"][0], c["second"][0]), rows(c["second"][1], c["second"][1]))
    out = ctx.debug_lg_prepare(f0, f1, n0, n1, wr, prec, kp_off=kp, normalize=norm, second=second, slack_rows=c["slack"])
    ref = R.prepare(f0, f1, n0, n1, wr, prec, out["Np"], kp_off=kp, normalize=norm, second=second, slack_rows=c["slack"])
    T = 2 * (2 if second else B) * out["Np"]
    assert out["rows_past"] == 0
    assert np.array_equal(out["lens"], ref["lens"])
    assert np.isfinite(out["x32"]).all() and np.isfinite(out["xb"]).all() and np.isfinite(out["rot_cos"][:T]).all() and np.isfinite(out["rot_sin"][:T]).all()
    assert np.array_equal(out["x32"], ref["x32"]) and np.array_equal(out["xb"], ref["xb"])
    pad = ref["valid"][:T] == 0
    assert (out["rot_cos"][:T][pad] == 1).all() and (out["rot_sin"][:T][pad] == 0).all() and (out["x32"][ref["valid"] != 1] == 0).all()
    ec, es = np.abs(out["rot_cos"][:T] - ref["cos"][:T]), np.abs(out["rot_sin"][:T] - ref["sin"][:T])
    tok = ref["valid"][:T] == 1
    rc, rs = float((ec[tok] / ref["dcos"][:T][tok]).max()), float((es[tok] / ref["dsin"][:T][tok]).max())
    diag(f"lgtail_prepare_{name}_{'fp16' if prec else 'bf16'}", cos=rc, sin=rs)
    assert np.all(ec <= ref["dcos"][:T]) and np.all(es <= ref["dsin"][:T]), (rc, rs)


# ------------------------------------------------------------------ assignment
@PRECS
@pytest.mark.parametrize("k,n0,n1", [(k, n0, n1) for k in R.LENGTHS for n0, n1 in R.LENGTHS[k]])
def test_lengths_vs_float64(k, n0, n1, prec):
    """full, ragged and degenerate lengths, both forms: one row / column against a full other side, lengths one below, at and one above the 64-wide tile, more
    workgroups than one per side; the two forms' similarity matrices are the same bits"""
    case = ("planted", n0, n1)
    outs = []
    for form in (0, 1):
        out = _launch(k, [case], prec, form)
        _untouched(out, 0, n0, n1)
        p = _pair(out, 0, n0, n1)
        _ALONE[(k, case, prec, form)] = p
        _check(f"len_f{form}_{k}", p, case, prec, _ctx(k).np_rows)
        outs.append(p)
    assert np.array_equal(outs[0]["sim"], outs[1]["sim"]) and np.array_equal(outs[0]["z0"], outs[1]["z0"]) and np.array_equal(outs[0]["z1"], outs[1]["z1"])


@PRECS
@pytest.mark.parametrize("B", [8, 9])
def test_pairs_of_a_batch_are_their_single_launches_bit_for_bit(B, prec):
    """B = 8: lg_lse_kernel / lg_arg_kernel (rows and columns in one launch); B = 9: the four separate kernels with four-row workgroups.  Ragged pairs; every
    pair's outputs are its B = 1 outputs in both forms (a pair's order of summation depends neither on the batch nor on the launch form)."""
    cases = [("planted", n0, n1) for n0, n1 in R.BATCH[:B]]
    for form in (0, 1):
        out = _launch(400, cases, prec, form)
        for b, c in enumerate(cases):
            _untouched(out, b, c[1], c[2])
            p = _pair(out, b, c[1], c[2])
            _check(f"B{B}_f{form}_p{b}", p, c, prec, 400)
            _same(p, _alone(400, c, prec, form), (B, form, b, c))


@PRECS
@pytest.mark.parametrize("n0,n1", R.FAMILY_SHAPES)
@pytest.mark.parametrize("kind", [f for f in R.FAMILIES if f != "planted"])
def test_families_vs_float64(kind, n0, n1, prec):
    """wide: |sim| to ~200; ramp / ramp_down: every fold of tile partials re-scales one side by more than e^40; constant: every entry ties, the first index wins
    everywhere and lse = v + log n; dup: exact ties across tile boundaries, the lowest index wins"""
    case = (kind, n0, n1)
    for form in (0, 1):
        out = _launch(400, [case], prec, form)
        p = _pair(out, 0, n0, n1)
        r = _check(f"fam_f{form}", p, case, prec, 400, against64=kind != "constant")
        if kind == "constant":
            assert not p["rowarg"].any() and not p["colarg"].any()
            v = np.float64(p["sim"][0, 0])
            assert (p["sim"] == p["sim"][0, 0]).all() and v == 4.0
            assert np.abs(p["rowlse"] - (v + np.log(n1))).max() <= (3 + np.log2(n1)) * 2.0 ** -23 + 2 * R.ulp32(v + np.log(n1))
            assert np.abs(p["collse"] - (v + np.log(n0))).max() <= (3 + np.log2(n0)) * 2.0 ** -23 + 2 * R.ulp32(v + np.log(n0))
            assert p["nmatch"] == (1 if np.float32(p["rowval"][0]) > np.log(THR) else 0)
        if kind == "dup":
            i0, i1 = R.dup_indices(n0), R.dup_indices(n1)
            assert len(i0) == 3 and len(i1) == 3
            sc = p["scores"]
            assert np.array_equal(sc[i0[0]], sc[i0[1]]) and np.array_equal(sc[i0[0]], sc[i0[2]]), "duplicate rows must score the same bits"
            assert np.array_equal(sc[:, i1[0]], sc[:, i1[1]]) and np.array_equal(sc[:, i1[0]], sc[:, i1[2]])
            cols = np.flatnonzero(np.isin(p["colarg"], i0))         # columns whose best row is a duplicate: the first of the three
            rows = np.flatnonzero(np.isin(p["rowarg"], i1))
            assert len(cols) >= 1 and len(rows) >= 1, "the planted partner of the duplicates must pick one of them"
            assert (p["colarg"][cols] == i0[0]).all() and (p["rowarg"][rows] == i1[0]).all()
        assert r["scores"] <= 1.0


@PRECS
def test_cap_below_the_number_of_matches(prec):
    """nmatch = cap, the first cap matches in row order, nothing behind them — neither in the pair's own slots nor in the next pair's"""
    cases = [("planted", 400, 400), ("planted", 5, 5)]
    for form in (0, 1):
        full = _alone(400, cases[0], prec, form)
        assert full["nmatch"] > 150
        out = _launch(400, cases, prec, form, cap=50)
        p = _pair(out, 0, 400, 400)
        assert p["nmatch"] == 50 and np.array_equal(p["idx"], full["idx"][:50]) and np.array_equal(p["score"], full["score"][:50])
        _check(f"cap_f{form}_p0", p, cases[0], prec, 50)
        _check(f"cap_f{form}_p1", _pair(out, 1, 5, 5), cases[1], prec, 50)          # (its slots behind its own count are still poison: _check)


@PRECS
@pytest.mark.parametrize("B", [5, 10])
def test_empty_sides_have_no_matches(B, prec):
    """(n0, 0), (0, n1) and (0, 0) between normal pairs (B = 5: merged launches, B = 10: the four kernels): no match, whatever an earlier call left in colarg (the
    hook leaves zeros: row 0 with colarg[0] = 0 and exp(0) = 1 > thr would pass for a match); the neighbours are their single launches bit for bit"""
    cases = [("planted", 129, 200), ("planted", 200, 0), ("planted", 0, 150), ("planted", 0, 0), ("planted", 65, 97)] * (B // 5)
    for form in (0, 1):
        out = _launch(400, cases, prec, form)
        for b, c in enumerate(cases):
            p = _pair(out, b, c[1], c[2])
            if c[1] and c[2]:
                _same(p, _alone(400, c, prec, form), (B, form, b, c))
                continue
            assert p["nmatch"] == 0, (form, b, c, p["nmatch"], p["idx"][:2].tolist(), p["score"][:2].tolist())
            assert not p["idx"].any() and np.isnan(p["score"]).all()
            assert not p["rowarg"].any() and (p["rowval"] == 0).all()                # a row without a column keeps (0, 0.0f): light_glue.cpp:217
            assert (p["rowlse"] == -np.inf).all() and (p["collse"] == -np.inf).all()
            _untouched(out, b, c[1], c[2])


@PRECS
def test_finite_padding_stays_out_of_every_reduction(prec):
    """The padding rows of the descriptors hold a FINITE row (8 x a valid descriptor of the other side: similarities far above every valid one) instead of NaN,
    which fmaxf drops on its own: a maximum, a sum or an arg-max that lets a padded row or column in shows at once"""
    for n0, n1 in ((33, 400), (129, 63), (400, 317)):
        case = ("planted", n0, n1)
        md0, md1, _, _ = _inputs(*case)
        for form in (0, 1):
            for pad in (8 * md0[0], 8 * md1[0]):
                p = _pair(_launch(400, [case], prec, form, pad=pad), 0, n0, n1)
                _same(p, _alone(400, case, prec, form), (case, form))


def test_hooks_reject_bad_arguments():
    ctx = _ctx(1024)
    md = np.zeros((2, 8, 256), np.float32)
    for lens, kw in (([9, 3], {}), ([3, -1], {}), ([3, 3], {"cap": 0}), ([3, 3], {"cap": 2000})):
        with pytest.raises(api.AirfeError):
            ctx.debug_lg_assign(md, md, lens, W, BIAS, 1, 0, **kw)
    with pytest.raises(api.AirfeError):
        ctx.debug_lg_assign(md, md, [3, 3], W, BIAS, 1, 2)
    with pytest.raises(api.AirfeError):
        ctx.debug_lg_assign(np.zeros((6, 8, 256), np.float32), np.zeros((6, 8, 256), np.float32), [3] * 6, W, BIAS, 1, 0)        # B = 3 > max_batch = 2
    f = np.zeros((1, 8, 259), np.float32)
    with pytest.raises(api.AirfeError):
        ctx.debug_lg_prepare(f, f, [9], [1], np.zeros((32, 2)), 1)
    with pytest.raises(api.AirfeError):
        ctx.debug_lg_prepare(f, f, [1], [1], np.zeros((32, 2)), 1, slack_rows=5000)             # beyond the arena's rows
    out = ctx.debug_lg_assign(md, md, [3, 3], W, BIAS, 1, 0)
    assert out["nmatch"][0] >= 0 and np.isfinite(out["scores"][0, :3, :3]).all()
