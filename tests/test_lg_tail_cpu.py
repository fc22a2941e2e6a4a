"""Keeps tests/lg_tail_ref.py honest without a GPU: its float64 tail is the tail of oracle/ref_nets.lightglue_forward, a numpy float32 run of every formula stays
inside the bound the reference states for it, on every family and length tests/test_gpu_lg_tail.py runs, and the inputs leave almost no row whose float64 decision
the bounds cannot settle."""
import numpy as np
import pytest
import torch

import lg_tail_ref as R
from kernel_ref import r2
from oracle import ref_nets, ref_post

W, BIAS = R.matchability()
_IN = {}


def _inputs(kind, n0, n1):
    key = (kind, n0, n1)
    if key not in _IN:
        _IN[key] = R.family(kind, n0, n1, R.case_seed(kind, n0, n1))
    return _IN[key]


def _sim32(md0, md1, prec):
    return (r2(md0, prec).astype(np.float32) @ r2(md1, prec).astype(np.float32).T).astype(np.float32)


@pytest.mark.parametrize("kind,n0,n1", [("planted", 65, 97), ("wide", 129, 200), ("dup", 129, 200), ("ramp", 129, 200)])
def test_reference_tail_is_the_oracles_tail(kind, n0, n1, monkeypatch):
    """lightglue_forward with no layer, final_proj = 4 I (its d^-1/4 = 1 / 4 undoes it exactly) and a zero positional projection IS its tail on the descriptors; run in
    float64 (the oracle's tensor factory patched), it must agree with the reference to float64 rounding.  The oracle takes md and the token row from ONE tensor, so
    the descriptors serve as both here."""
    monkeypatch.setattr(ref_nets, "_t", lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))
    md0, md1, _, _ = _inputs(kind, n0, n1)
    md0, md1 = r2(md0, 1), r2(md1, 1)
    w = {"posenc.Wr.weight": np.zeros((32, 2)), "log_assignment.-1.final_proj.weight": 4.0 * np.eye(256), "log_assignment.-1.final_proj.bias": np.zeros(256),
         "log_assignment.-1.matchability.weight": W.astype(np.float64)[None, :], "log_assignment.-1.matchability.bias": np.array([float(BIAS)])}
    want = ref_nets.lightglue_forward(w, np.zeros((n0, 2)), md0, np.zeros((n1, 2)), md1, n_layers=0)
    got = R.tail(md0, md1, md0, md1, W, BIAS, 1)
    assert want.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # ... and the scan is filter_matches
    s32 = want.astype(np.float32)
    idx, sc = ref_post.filter_matches(s32, 0.1)
    mine = R.scan(s32, 0.1)
    assert np.array_equal(mine["idx"], idx) and np.array_equal(mine["score"], sc) and mine["nmatch"] == len(idx)
    assert np.array_equal(mine["rowarg"], np.argmax(s32, 1)) and np.array_equal(mine["colarg"], np.argmax(s32, 0))


@pytest.mark.parametrize("prec", [1, 0], ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind,n0,n1", R.gpu_cases())
def test_float32_run_stays_inside_the_bounds_and_few_rows_are_fragile(kind, n0, n1, prec):
    """Every bound against a plain numpy float32 evaluation of the same formula; then the share of rows and columns that `safe` cannot settle: at most 2 %, the
    share tests/test_gpu_lightglue.py allows.  `constant` ties every entry by construction (its decisions are pinned by the closed form instead)."""
    md0, md1, x0, x1 = _inputs(kind, n0, n1)
    sim64, dsim = R.sim_ref(md0, md1, prec)
    sim = _sim32(md0, md1, prec)
    assert np.all(np.abs(sim - sim64) <= dsim)
    zs = []
    for x in (x0, x1):
        z, dz = R.z_ref(x, W, BIAS)
        z32 = R.z32(x, W, BIAS)
        assert np.all(np.abs(z32 - z) <= dz)
        zs.append(z32)
    r = R.scores_ref(sim, zs[0], zs[1])
    rl, cl = R.lse32(sim, 1), R.lse32(sim, 0)
    assert np.all(np.abs(rl - r["rowlse"]) <= r["d_rowlse"]), float((np.abs(rl - r["rowlse"]) / r["d_rowlse"]).max())
    assert np.all(np.abs(cl - r["collse"]) <= r["d_collse"]), float((np.abs(cl - r["collse"]) / r["d_collse"]).max())
    s32 = R.scores32(sim, rl, cl, zs[0], zs[1])
    assert np.all(np.abs(s32 - r["scores"]) <= r["d_scores"]), float((np.abs(s32 - r["scores"]) / r["d_scores"]).max())
    if kind == "constant":
        assert np.abs(r["rowlse"] - (4.0 + np.log(n1))).max() < 1e-12 and np.abs(r["collse"] - (4.0 + np.log(n0))).max() < 1e-12
        return
    sr, sc = R.safe(r["scores"], r["d_scores"], 1), R.safe(r["scores"], r["d_scores"], 0)
    fragile = int((~sr).sum() + (~sc).sum())
    assert fragile <= 0.02 * (n0 + n1), (fragile, n0 + n1)
    # on the safe rows the float32 run decides as float64 does
    d = R.scan(s32)
    assert np.array_equal(d["rowarg"][sr], np.argmax(r["scores"], 1)[sr]) and np.array_equal(d["colarg"][sc], np.argmax(r["scores"], 0)[sc])


def test_families_do_what_they_are_for():
    md0, md1, _, _ = _inputs("ramp", 400, 400)
    s, _ = R.sim_ref(md0, md1, 1)
    tmax = np.array([s[:, t * 64:(t + 1) * 64].max(1) for t in range(7)])
    assert (np.diff(tmax, axis=0) > 40).all()
    tmax = np.array([s[t * 64:(t + 1) * 64].max(0) for t in range(7)])
    assert (np.diff(tmax, axis=0) > 40).all()
    md0, md1, _, _ = _inputs("ramp_down", 129, 200)
    s, _ = R.sim_ref(md0, md1, 0)
    assert (np.diff(np.array([s[:, t * 64:(t + 1) * 64].max(1) for t in range(4)]), axis=0) < -40).all()
    s, _ = R.sim_ref(*_inputs("wide", 400, 400)[:2], 1)
    assert s.max() > 180 and s.min() < -180
    md0, md1, x0, _ = _inputs("dup", 400, 400)
    assert R.dup_indices(400) == [5, 70, 399] and np.array_equal(md0[5], md0[70]) and np.array_equal(md0[5], md0[399]) and np.array_equal(x0[5], x0[399])
    assert R.dup_indices(129) == [5, 70, 128] and R.dup_indices(63) == [5]


def test_prepare_argument_bound_covers_either_contraction():
    rng = np.random.default_rng(3)
    f = rng.uniform(-1, 1, size=(1, 300, 259)).astype(np.float32)
    wr = rng.uniform(-30, 30, size=(32, 2)).astype(np.float32)
    ref = R.prepare(f, f, [300], [0], wr, 1, 304)
    a32 = R.prepare_arg32(f[0, :, 1], f[0, :, 2], wr)
    fused = (wr[None, :, 0].astype(np.float64) * f[0, :, 1, None] + (wr[None, :, 1] * f[0, :, 2, None]).astype(np.float32)).astype(np.float32)      # one product kept exact
    for a in (a32, fused):
        assert np.all(np.abs(np.cos(a.astype(np.float64)) - ref["cos"][:300]) <= ref["dcos"][:300])
        assert np.all(np.abs(np.sin(a.astype(np.float64)) - ref["sin"][:300]) <= ref["dsin"][:300])
    assert np.abs(a32).max() > 40 and np.array_equal(ref["lens"], [300, 0]) and (ref["x32"][300:] == 0).all()
