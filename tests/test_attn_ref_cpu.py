"""No-GPU proof of tests/attn_ref.py, the yardstick of tests/test_gpu_attention.py: the reference against a plain float64 soft-max attention in torch, the bound
against a numpy emulation of attention32_kernel's rounding (it must hold on every element, with and without a flush of subnormal fp16 P), and the teeth — the same
emulation with a defect planted (a mask bound off by one either way, two keys swapped on the V side of one 16-key group) must be REJECTED by the checks the GPU tests
apply."""
import numpy as np
import pytest

import attn_ref
from gpu_common import to_2byte


def emulate(q, k, v, lens, cross, prec, flush=False, defect=None):
    """attention32_kernel's arithmetic in numpy (csrc/kernels_attn.hip), one (sequence, head) at a time: 64-key tiles (a 32-key sub-tile when that is all that is left), fp32
    scores minus a shift that the FIRST tile fixes from its row maximum, p = 2^(s - shift) in fp32; a later tile in which some row of a 32-query wave has a
    half-row sum (the keys a lane holds: bit 3 of the key index) beyond 2^14 is re-centred for that wave by the tile's own row maximum, accumulators rescaled.  P is rounded
    to `prec` for the P V product (flush: fp16 P below 2^-14 become 0), the row sum l adds the unrounded p, the output o / l is rounded to `prec`.
    defect: "drop" — the last valid key is masked; "leak" — the first padding key is not; "swap" — keys 2 and 5 of every 16-key group change places on the V side only."""
    S, H, n, _ = q.shape
    r2 = lambda x: attn_ref.to_2byte(x, prec)
    q, k, v = r2(q), r2(k), r2(v)
    out = np.zeros((S, n, H * 64))
    for s in range(S):
        skv = s ^ 1 if cross else s
        lq = int(lens[s])
        lk = int(lens[skv]) + {"drop": -1, "leak": 1}.get(defect, 0)
        assert 0 <= lk <= n
        for h in range(H):
            vv = v[skv, h].copy()
            if defect == "swap":
                a = np.arange(2, n - 3, 16)
                vv[a], vv[a + 3] = v[skv, h][a + 3], v[skv, h][a]
            sc = (q[s, h, :lq] @ k[skv, h].T).astype(np.float32)
            m = np.zeros(lq, np.float32); l = np.zeros(lq, np.float32); o = np.zeros((lq, 64), np.float32)
            wave = np.arange(lq) // 32
            for j0 in range(0, lk, 64):
                j1 = min(j0 + (64 if lk - j0 > 32 else 32), n)
                valid = np.arange(j0, j1) < lk
                hi = ((np.arange(j0, j1) - j0) & 8) != 0
                st = np.where(valid[None, :], sc[:, j0:j1] - m[:, None], -np.inf).astype(np.float32)
                if j0 == 0:
                    redo = np.ones(lq, bool)
                else:
                    p = np.exp2(st)
                    over = ~((p[:, ~hi].sum(1, dtype=np.float32) <= 16384) & (p[:, hi].sum(1, dtype=np.float32) <= 16384))
                    redo = np.isin(wave, wave[over])
                if redo.any():
                    mx = st[redo].max(1)
                    if j0:
                        alpha = np.exp2(-mx).astype(np.float32)
                        l[redo] *= alpha; o[redo] *= alpha[:, None]
                    m[redo] += mx
                    st[redo] -= mx[:, None]
                p = np.exp2(st).astype(np.float32)
                l += p[:, ~hi].sum(1, dtype=np.float32) + p[:, hi].sum(1, dtype=np.float32)
                pr = r2(p)
                if flush and prec == 1:
                    pr[pr < 2.0 ** -14] = 0.0
                o += (pr @ vv[j0:j1]).astype(np.float32)
            with np.errstate(divide="ignore"):
                inv = np.where(l > 0, np.float32(1) / l, np.float32(0)).astype(np.float32)
            out[s, :lq, h * 64:(h + 1) * 64] = r2(o * inv[:, None])
    return out


def _random(n, lens, scale, seed, H=1):
    rng = np.random.default_rng(seed)
    S = len(lens)
    return (rng.standard_normal((S, H, n, 64)) * scale, rng.standard_normal((S, H, n, 64)) * scale, rng.standard_normal((S, H, n, 64)))


@pytest.mark.parametrize("prec", [0, 1])
def test_rounding_is_the_hooks(prec):
    x = np.random.default_rng(1).standard_normal(100000).astype(np.float32) * np.float32(10.0) ** np.random.default_rng(2).integers(-9, 5, 100000).astype(np.float32)
    x = np.concatenate([x, np.float32([0, -0.0, attn_ref.MAXV[prec], -attn_ref.MAXV[prec], 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 1 + 2.0 ** -8, 1 + 2.0 ** -9, 1 + 3 * 2.0 ** -9])])
    assert np.array_equal(attn_ref.to_2byte(x, prec), to_2byte(x, prec).astype(np.float64))
    assert np.isfinite(attn_ref.to_2byte(np.float32([attn_ref.MAXV[prec]]), prec)).all()


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("lens", [(48, 48), (33, 48), (1, 17), (0, 37), (0, 0)])
def test_reference_is_float64_softmax_attention(lens, cross, prec):
    import torch
    q, k, v = _random(48, lens, 0.6, 3, H=2)
    ref = attn_ref.reference(q, k, v, lens, cross, prec)
    tq, tk, tv = (torch.from_numpy(to_2byte(x, prec)).double() for x in (q, k, v))
    want = np.zeros_like(ref)
    for s in range(2):
        skv = s ^ 1 if cross else s
        if lens[s] and lens[skv]:
            for h in range(2):
                p = torch.softmax(tq[s, h, :lens[s]] @ tk[skv, h, :lens[skv]].T * np.log(2.0), dim=1)
                want[s, :lens[s], h * 64:(h + 1) * 64] = (p @ tv[skv, h, :lens[skv]]).numpy()
    assert np.abs(ref - want).max() <= 1e-12
    assert not ref[0, lens[0]:].any() and not ref[1, lens[1]:].any()


@pytest.mark.parametrize("shape", [(400, 400), (400, 317), (1024, 1000), (48, 33)])
@pytest.mark.parametrize("scale", [0.05, 0.6, 1.2])
@pytest.mark.parametrize("prec", [0, 1])
def test_emulated_kernel_stays_within_the_bound(prec, scale, shape):
    n, lk = shape
    lens = (n, lk)
    q, k, v = _random(n, lens, scale, n + lk)
    ref = attn_ref.reference(q, k, v, lens, True, prec)
    bnd = attn_ref.bound(q, k, v, lens, True, prec)
    for flush in (False, True):
        w = attn_ref.worst_ratio(emulate(q, k, v, lens, True, prec, flush), ref, bnd, lens)      # cross: sequence 0's n queries see lk keys, sequence 1's lk queries n
        print(f"prec {prec} scale {scale} {shape} flush {flush}: worst err / bound {w:.3f}")
        assert w <= 1.0, (flush, w)


@pytest.mark.parametrize("prec", [0, 1])
def test_emulated_kernel_recentres_within_the_bound(prec):
    """the re-centring path of the emulation itself (logits that grow by 2^19 per tile), so that the bound is also proven where the shift moves"""
    rng = np.random.default_rng(5)
    n, lens = 400, (400, 389)
    q = np.zeros((2, 1, n, 64)); k = np.zeros((2, 1, n, 64))
    q[..., 0] = 1.0
    k[..., 0] = np.linspace(-60.0, 60.0, n)[None, None, :]
    q[..., 1:] = rng.standard_normal((2, 1, n, 63)) * 0.2
    k[..., 1:] = rng.standard_normal((2, 1, n, 63)) * 0.2
    v = rng.standard_normal((2, 1, n, 64))
    ref, bnd = attn_ref.reference(q, k, v, lens, False, prec), attn_ref.bound(q, k, v, lens, False, prec)
    for flush in (False, True):
        assert attn_ref.worst_ratio(emulate(q, k, v, lens, False, prec, flush), ref, bnd, lens) <= 1.0


PROBE_CASES = [(144, (129, 97)), (48, (33, 47)), (400, (399, 317)), (80, (65, 79))]


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("case", PROBE_CASES)
def test_probe_accepts_the_emulation_and_rejects_every_planted_defect(case, cross, prec):
    n, lens = case
    q, k, v = attn_ref.probe(n, lens, 7, H=1)
    exp = attn_ref.probe_expected(k, lens, cross)
    for s in range(2):
        lk = lens[s ^ 1 if cross else s]
        assert abs(exp[s, :lens[s]].sum(1) - 1).max() < 1e-12 and not exp[s, lens[s]:].any()
        if lk < 64:
            assert not exp[s, :, lk:64].any()
    for flush in (False, True):
        assert attn_ref.probe_check(emulate(q, k, v, lens, cross, prec, flush), k, lens, cross, prec) is None
    for defect in ("drop", "leak", "swap"):
        why = attn_ref.probe_check(emulate(q, k, v, lens, cross, prec, False, defect), k, lens, cross, prec)
        assert why is not None, f"the probe accepts the planted defect {defect}"


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("case", PROBE_CASES)
def test_bound_rejects_a_mask_off_by_one_on_random_data(case, prec):
    n, lens = case
    q, k, v = _random(n, lens, 0.05, 9)
    ref, bnd = attn_ref.reference(q, k, v, lens, False, prec), attn_ref.bound(q, k, v, lens, False, prec)
    assert attn_ref.worst_ratio(emulate(q, k, v, lens, False, prec), ref, bnd, lens) <= 1.0
    for defect in ("drop", "leak"):
        w = attn_ref.worst_ratio(emulate(q, k, v, lens, False, prec, False, defect), ref, bnd, lens)
        assert w > 1.0, f"the bound accepts the planted defect {defect}: worst err / bound {w:.3f}"
    print("swap:", attn_ref.worst_ratio(emulate(q, k, v, lens, False, prec, False, "swap"), ref, bnd, lens))
