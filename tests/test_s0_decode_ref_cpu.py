"""The reference, envelope and cases of tests/s0_decode_ref.py, proved without a device: the envelope is not too tight (the float32 restatement of the same expressions
lies inside it at every element of every bounded case), not too loose (ten wrong decodes each leave it by a factor > 10 at >= 100 elements), the float64 reference agrees
with the decode inside oracle/ref_nets.py::plnet_s0_lines, and every case holds what tests/test_gpu_s0_decode_pin.py relies on."""
import numpy as np
import pytest
import torch

import s0_decode_ref as R
from oracle import ref_nets

F = np.float32
OUTPUTS = ("lines", "jloc", "joff")


def _oracle(h):
    """oracle/ref_nets.py's float32 decode of one image h [17, 128, 128] -> lines [49152, 4], jloc, joff, thin, aux as numpy"""
    with torch.no_grad():
        return [t.numpy() for t in ref_nets.plnet_s0_decode(torch.from_numpy(np.array(h, F)))]          # (a copy: the cases are read-only)


@pytest.mark.parametrize("name", R.BOUNDED)
def test_float32_restatement_lies_inside_the_envelope(name):
    ref, env, f32 = R.expected(name)
    for k in OUTPUTS:
        err = np.abs(f32[k].astype(np.float64) - ref[k])
        share = float((err / np.maximum(env[k], 1e-300))[err > 0].max()) if (err > 0).any() else 0.0
        print(f"{name} {k}: float32 restatement at {share:.3f} of the envelope (max |err| {err.max():.3e}, envelope {env[k].min():.3e} .. {env[k].max():.3e})")
        assert np.isfinite(env[k]).all() and (err <= env[k]).all(), (name, k, int((err > env[k]).sum()))


def test_reference_agrees_with_the_oracle_decode_on_benign():
    ref, env, _ = R.expected("benign")
    h = R.case("benign")
    for b in range(2):
        lines, jloc, joff, thin, aux = _oracle(h[b])
        for k, got in (("lines", lines), ("jloc", jloc), ("joff", joff)):
            err = np.abs(got.astype(np.float64) - ref[k][b])
            assert (err <= env[k][b]).all(), (k, b, float((err - env[k][b]).max()))
        assert np.array_equal(thin, h[b, 9:13]) and np.array_equal(aux, h[b, 13:17])


@pytest.mark.parametrize("name", ["benign", "steep"])
def test_benign_and_steep_are_not_decided_by_the_clamps(name):
    v = R.expected(name)[0]["lines"]
    inside = float(((v > 0) & (v < 127)).mean())
    print(f"{name}: {inside:.3f} of the endpoint coordinates lie strictly inside (0, 127)")
    assert inside >= 0.5


def test_steep_stays_hundreds_of_ulps_from_the_pole_and_reaches_it_closer_than_benign():
    h = R.case("steep").astype(np.float64)
    s = 1 / (1 + np.exp(-h[:, 1:3]))
    gap = (np.pi / 2 - s * np.pi / 2) / 2.0 ** -23             # (1 ulp of a float32 in [1, 2) is 2^-23)
    print(f"steep: the angle comes within {gap.min():.0f} float32 ulps of the pole, md1 / md2 logits in [{h[:, 1:3].min()}, {h[:, 1:3].max()}]")
    assert 300 < gap.min() < 2000 and np.abs(h[:, 1:3]).max() <= 10
    assert np.abs(R.case("benign")[:, 1:3]).max() <= 3


def test_clamps_reaches_all_six_sides_and_the_border_pixels():
    n = R.clamp_sides(R.case("clamps"))
    print("clamps:", n)
    assert set(n) == {"d_lo", "d_hi", "x_lo", "x_hi", "y_lo", "y_hi"} and min(n.values()) >= 100
    v = R.decode(R.case("clamps"), np.float64, clamp=False)["lines"].reshape(2, 3, R.FH, R.FH, 4)
    for sl in (np.s_[:, :, 0], np.s_[:, :, 127], np.s_[:, :, :, 0], np.s_[:, :, :, 127]):      # rows / columns 0 and 127 are clamped AND unclamped
        e = v[sl]
        assert ((e < 0) | (e > 127)).sum() >= 100 and ((e > 0) & (e < 127)).sum() >= 100


def test_saturated_sigmoid_is_exact_in_float32():
    h = R.case("saturated_sigmoid")
    for i in (0, 1, 2, 3, 4, 7, 8):
        assert set(np.unique(h[:, i])) == {-90.0, 90.0}, i
    s = R._sigmoid(h[:, [0, 1, 2, 3, 4, 7, 8]].astype(F))
    assert set(np.unique(s)) == {0.0, 1.0}
    assert (np.abs(h[:, 6] - h[:, 5]) == 200).all()
    _, _, f32 = R.expected("saturated_sigmoid")
    assert set(np.unique(f32["jloc"])) == {0.0, 1.0} and set(np.unique(f32["joff"])) == {-0.5, 0.5}
    # md1 / md2 = +90 only where all three d_r are 0 (the pole is the next case's)
    dz = (h[:, 3] < 0) & (h[:, 4] < 0)
    assert ((h[:, 1] < 0) | dz).all() and ((h[:, 2] < 0) | dz).all() and (h[:, 1] > 0).sum() >= 100 and (h[:, 2] > 0).sum() >= 100


def test_pole_is_decided_by_the_sign_of_tan_in_float32():
    h = R.case("pole")
    assert ((h[:, 1] >= 17) | (h[:, 2] >= 17)).all() and ((h[:, 1] >= 17) & (h[:, 2] >= 17)).sum() >= 1000
    s = R._sigmoid(h[:, 1:3].astype(F))
    assert (s[h[:, 1:3] >= 17] == 1).all() and (s[h[:, 1:3] < 17] <= F(1) - F(2.0 ** -23)).all()
    raw = R.decode(h, F, clamp=False)["lines"]
    assert np.isfinite(raw).all()
    out = np.minimum(np.abs(raw - 0), np.abs(raw - 127))
    outside = (raw < -1) | (raw > 128)
    print(f"pole: the unclamped float32 coordinates come within {out[outside].min():.1f} px of [0, 127] at the nearest")
    assert outside.all()
    # float32 takes the far side of the pole, float64 the near side: the two clamped results differ at the coordinates a logit >= 17 drives
    ref, _, f32 = R.expected("pole")
    differ = int((f32["lines"] != ref["lines"]).sum())
    print(f"pole: float32 and float64 disagree at {differ} of {raw.size} clamped coordinates")
    assert differ >= raw.size // 4 and set(np.unique(f32["lines"])) == {0.0, 127.0}
    # the oracle's own float32 decode (torch) gives the same clamped lines
    for b in range(2):
        assert np.array_equal(_oracle(h[b])[0], f32["lines"][b])


def test_copies_has_plateaus_and_ties_and_identifying_values():
    h = R.case("copies")
    a = R.expected("copies")[2]["jloc"]
    kept = R.jnms_ref(a) > 0
    assert len(np.unique(a)) == 5
    pad = np.pad(kept, ((0, 0), (1, 1), (1, 1)))
    ties = sum(int((kept & pad[:, 1 + dy:1 + dy + R.FH, 1 + dx:1 + dx + R.FH]).sum()) for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)))
    print(f"copies: {int(kept.sum())} of {a.size} pixels survive the 3x3 suppression, {ties} neighbouring pairs of survivors (exact ties)")
    assert ties >= 1000 and 0.05 < kept.mean() < 0.95
    for name in R.CASES:                                       # every case carries the identifying planes
        ta = R.case(name)[:, 9:17]
        assert len(np.unique(ta)) == ta.size
    assert len(np.unique(np.stack([R.ids_loi(0), R.ids_loi(1)]))) == 2 * R.NPX * 128


def test_cases_are_exact_in_both_two_byte_types_and_the_one_hot_head_reproduces_them():
    for name in R.CASES:
        h = R.case(name)
        lg = h[:, :9]
        assert np.array_equal(lg.astype(np.float16).astype(F), lg), name
        assert np.array_equal((lg.view(np.uint32) & 0xFFFF), np.zeros(lg.shape, np.uint32)), name      # bf16: the low 16 bits of the float32 are zero
        assert not np.array_equal(h[0], h[1])
    x, w, b = R.features_for(R.case("copies"))                 # (features_for asserts x w^T = h in float64 itself)
    for t in (x, w):
        assert np.array_equal(t.astype(np.float16).astype(F), t) and not (t.view(np.uint32) & 0xFFFF).any()
    assert (b == 0).all() and sorted(np.unique(w)) == [0.0, 1.0, 32.0, 1024.0, 32768.0]


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_envelope_is_not_too_loose(mutant):
    """every wrong decode moves at least 100 elements of some bounded case beyond 10 x their own envelope"""
    best = {}
    for name in R.BOUNDED:
        ref, env, _ = R.expected(name)
        bad = R.decode(R.case(name), np.float64, mutant)
        best[name] = sum(int((np.abs(bad[k] - ref[k]) > 10 * env[k]).sum()) for k in OUTPUTS)
    print(f"{mutant}: elements beyond 10 x the envelope per case: {best}")
    assert max(best.values()) >= 100
