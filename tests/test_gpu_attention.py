"""The matcher's flash attention alone (kernels_attn.hip through airfe_debug_attention) against a float64 soft-max attention on the SAME 2-byte inputs: ragged lengths, the
32-key tail sub-tile, cross attention — and logits built to drive the kernel's RE-CENTRING path (its running shift is stale by design: a later tile whose partial row sums
leave the 2-byte range is recomputed with a fresh row maximum), which the LightGlue / SuperGlue parity tests never reach (0 re-centred tiles in 5 forwards of the bench
workload, profiles/r06_att_attention.txt).

Every comparison is also made PER ELEMENT against attn_ref.bound (tests/attn_ref.py: derived from the reference alone, proven on the CPU by tests/test_attn_ref_cpu.py),
in both 2-byte types through airfe_debug_attention_args, whose output buffer starts as NaN: more than eight (sequence, head) groups and H = 8 (the workgroup -> group
decode, cross attention beyond pair 0), row counts from 16 to 1024 with every key-tail residue, an exact probe (a leaked or dropped key shows as a non-zero where the
answer is 0, or as more than one unit in the last place), hostile key padding, zero lengths, which rows a launch writes, and determinism.  Each group of cases records
its largest err / bound per type through gpu_common.diag (DESIGN.md section 2a keeps the numbers)."""
import numpy as np
import pytest

import attn_ref
from airslam_amd import api, weights
from gpu_common import diag

pytestmark = pytest.mark.gpu
_C = {}
PRECS = [0, 1]
PNAME = {0: "bf16", 1: "fp16"}
CTX_PREC = 1                                                 # the shared context's matcher_precision (the default, fp16): what the old entry runs
_WORST = {}


def _ctx():
    if "c" not in _C:
        _C["c"] = api.Context(lightglue=weights.synthetic_lightglue(1234, n_layers=1), max_batch=4, max_keypoints=400)
    return _C["c"]


def _half(x):
    return x.astype(np.float16).astype(np.float64)


def _reference(q, k, v, lens, cross):
    """p = 2^(q.k - max) over the valid keys, out = sum p v / sum p; inputs rounded to fp16 like the kernel's operands (P itself is NOT rounded here: the tolerance covers it)"""
    S, H, n, _ = q.shape
    out = np.zeros((S, n, H * 64))
    q, k, v = _half(q), _half(k), _half(v)
    for s in range(S):
        skv = s ^ 1 if cross else s
        lq, lk = int(lens[s]), int(lens[skv])
        for h in range(H):
            sc = q[s, h, :lq] @ k[skv, h, :lk].T
            p = np.exp2(sc - sc.max(1, keepdims=True))
            out[s, :lq, h * 64:(h + 1) * 64] = (p @ v[skv, h, :lk]) / p.sum(1, keepdims=True)
    return out


def _record(group, prec, w):
    """the largest err / bound a group of cases saw, per type (gpu_common.diag: attention_<group>)"""
    d = _WORST.setdefault(group, {})
    d[PNAME[prec]] = max(d.get(PNAME[prec], 0.0), w)
    diag("attention_" + group, **d)


def _within_bound(group, name, got, q, k, v, lens, cross, prec):
    """every element of the valid rows of every sequence within attn_ref.bound of the float64 reference"""
    ref = attn_ref.reference(q, k, v, lens, cross, prec)
    w = attn_ref.worst_ratio(got, ref, attn_ref.bound(q, k, v, lens, cross, prec), lens)
    print(f"{name} {PNAME[prec]}: worst err / bound {w:.3f}")
    _record(group, prec, w)
    assert w <= 1.0, (name, PNAME[prec], w)


def _run(group, name, q, k, v, lens, cross, prec):
    lens = np.asarray(lens, np.int32)
    got = _ctx().debug_attention(q, k, v, lens, cross=cross, prec=prec)
    _within_bound(group, name, got, q, k, v, lens, cross, prec)
    return got


def _check(name, q, k, v, lens, cross, tol, also=PRECS):
    got = _ctx().debug_attention(q, k, v, lens, cross=cross)
    ref = _reference(q, k, v, lens, cross)
    assert np.isfinite(got).all(), name
    for s in range(q.shape[0]):
        err = np.abs(got[s, :lens[s]] - ref[s, :lens[s]]).max()
        assert err <= tol * max(1.0, np.abs(ref[s, :lens[s]]).max()), (name, s, err)
    _within_bound("existing", name, got, q, k, v, lens, cross, CTX_PREC)
    for prec in also:                                        # the same inputs in each type through the entry whose output buffer starts as NaN
        _run("existing", name, q, k, v, lens, cross, prec)
    return got


def _random(S, H, n, seed, scale=0.6):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((S, H, n, 64)) * scale, rng.standard_normal((S, H, n, 64)) * scale, rng.standard_normal((S, H, n, 64))


GROUPS = [(2, 4), (4, 4), (6, 4), (8, 4), (1, 8), (2, 8), (3, 8)]
GROUP_LENS = (144, 129, 97, 33, 65, 1, 128, 96)
ROWS = [(16, (16, 1)), (48, (33, 48)), (64, (64, 32)), (80, (65, 80)), (128, (128, 96)), (144, (129, 97)), (400, (400, 317)), (1024, (1024, 1000)), (1024, (897, 959))]
# (S, H, n, lens) of both lists: what the exact probe runs
SHAPES = [(S, H, 144, GROUP_LENS[:S]) for S, H in GROUPS] + [(2, 4, n, lens) for n, lens in ROWS]


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("lens", [(400, 400), (400, 317), (33, 400), (1, 64), (65, 97)])
def test_attention_vs_float64_softmax(lens, cross):
    rng = np.random.default_rng(sum(lens) + int(cross))
    S, H, n = 2, 4, 400
    q = rng.standard_normal((S, H, n, 64)) * 0.6           # logits ~ N(0, 0.36 * 64 = 23): a range of +-20 in log2 units, like a trained layer's sharpest heads
    k = rng.standard_normal((S, H, n, 64)) * 0.6
    v = rng.standard_normal((S, H, n, 64))
    _check(f"attn_{lens}_{cross}", q, k, v, np.array(lens, np.int32), cross, 4e-3)


@pytest.mark.parametrize("cross", [False, True])
def test_attention_recentres_when_later_tiles_dominate(cross):
    """Keys sorted so that the row maximum GROWS from tile to tile by far more than the 2^14 a partial row sum may reach under the stale shift: every tile behind the first
    must take the re-centring path (accumulators rescaled, shift updated), and early keys must underflow to exactly the weight float64 gives them (~0)."""
    rng = np.random.default_rng(5 + int(cross))
    S, H, n = 2, 4, 400
    q = np.zeros((S, H, n, 64)); k = np.zeros((S, H, n, 64))
    q[..., 0] = 1.0                                          # logit of (query i, key j) = k[j, 0] + noise
    k[..., 0] = np.linspace(-60.0, 60.0, n)[None, None, :]   # +19 per 64-key tile in log2 units: 2^19 >> 2^14
    q[..., 1:] = rng.standard_normal((S, H, n, 63)) * 0.2
    k[..., 1:] = rng.standard_normal((S, H, n, 63)) * 0.2
    v = rng.standard_normal((S, H, n, 64))
    lens = np.array([400, 389], np.int32)
    got = _check(f"attn_recentre_{cross}", q, k, v, lens, cross, 4e-3)
    # the answer is dominated by the last few keys: a kernel that skipped the re-centring would return inf / NaN or the first tile's average
    ref = _reference(q, k, v, lens, cross)
    assert np.abs(got[0, :lens[0]] - ref[0, :lens[0]]).max() < 0.02 and np.abs(ref[0, :10]).max() > 0.1


def test_attention_recentres_on_an_isolated_spike():
    """one key in the LAST tile beats everything before it by 2^40 for half of the queries only: lanes of one wave disagree about the need to re-centre (the kernel decides per
    wave with __any), rows without the spike must come out unchanged"""
    rng = np.random.default_rng(11)
    S, H, n = 2, 4, 400
    q = rng.standard_normal((S, H, n, 64)) * 0.3
    k = rng.standard_normal((S, H, n, 64)) * 0.3
    v = rng.standard_normal((S, H, n, 64))
    q[:, :, ::2, 7] = 8.0
    k[:, :, :, 7] = 0.0
    k[:, :, 390, 7] = 5.0                                    # +40 for the even queries at key 390
    lens = np.array([400, 400], np.int32)
    got = _check("attn_spike", q, k, v, lens, False, 4e-3)
    vh = v.astype(np.float16).astype(np.float64)
    assert np.abs(got[0, 0, :64] - vh[0, 0, 390]).max() < 2e-3       # an even query returns (almost exactly) the spike key's value row


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("SH", GROUPS)
def test_group_decode_beyond_eight_groups(SH, prec):
    """S * H from 8 to 32 and H = 8: the workgroup -> (sequence, head, query block) map with li / nqb > 0, s = grp / H with H != 4, cross attention beyond pair 0.  n = 144: two
    query blocks, the second holding one wave.  Random data and a different length per sequence: a group routed to another sequence or head cannot pass."""
    S, H = SH
    q, k, v = _random(S, H, 144, 100 * S + H)
    for cross in ([False, True] if S % 2 == 0 else [False]):
        _run("groups", f"groups_S{S}_H{H}_{cross}", q, k, v, GROUP_LENS[:S], cross, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("case", ROWS)
def test_row_counts_and_key_tails(case, cross, prec):
    """Np from 16 (one sub-tile, one block) to 1024 (nqb = 8), len_kv % 64 in {0, 1, 31, 32, 33, 63}, both sides of every 32- and 128-query boundary"""
    n, lens = case
    q, k, v = _random(2, 4, n, n + sum(lens))
    _run("rows", f"rows_{n}_{lens}_{cross}", q, k, v, lens, cross, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", SHAPES)
def test_exact_probe(shape, prec):
    """attn_ref.probe: every p a power of two, every sum exact — 0 where the answer is 0, one unit in the last place elsewhere"""
    S, H, n, lens = shape
    q, k, v = attn_ref.probe(n, lens, 17 * S + H + n, H=H)
    for cross in ([False, True] if S % 2 == 0 else [False]):
        got = _ctx().debug_attention(q, k, v, np.asarray(lens, np.int32), cross=cross, prec=prec)
        assert attn_ref.probe_check(got, k, lens, cross, prec) is None, (shape, cross, PNAME[prec], attn_ref.probe_check(got, k, lens, cross, prec))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("case", [(48, (33, 48)), (144, (129, 97)), (400, (400, 317))])
def test_hostile_key_padding(case, cross, prec):
    """the type's largest finite value, sign alternating, in every K and V row at or beyond lens[s] (bf16: the padded scores overflow to inf and NaN): the tail mask is a
    select, so the valid rows must still meet the bound"""
    n, lens = case
    q, k, v = _random(2, 4, n, 7 * n + sum(lens))
    sign = np.where((np.arange(n)[:, None] + np.arange(64)[None, :]) % 2 == 0, 1.0, -1.0)
    for s in range(2):
        k[s, :, lens[s]:] = (attn_ref.MAXV[prec] * sign)[lens[s]:]
        v[s, :, lens[s]:] = (attn_ref.MAXV[prec] * sign)[lens[s]:]
    _run("hostile", f"hostile_{n}_{lens}_{cross}", q, k, v, lens, cross, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_zero_lengths(prec):
    """len_q = 0: the sequence's workgroups leave before they write (the canary is intact); len_kv = 0: no tile runs and the rows are exactly zero"""
    n = 48
    q, k, v = _random(2, 4, n, 48)
    lens = np.array([0, 37], np.int32)
    got, past = _ctx().debug_attention(q, k, v, lens, cross=False, prec=prec, raw=True)
    assert past == 0 and np.isnan(got[0]).all()
    _within_bound("zero_len", "zero_len_self", got[:, :n], q, k, v, lens, False, prec)
    got, past = _ctx().debug_attention(q, k, v, lens, cross=True, prec=prec, raw=True)
    assert past == 0 and np.isnan(got[0]).all()
    assert not got[1, :37].any() and np.isfinite(got[1, :37]).all()
    got, past = _ctx().debug_attention(q, k, v, np.zeros(2, np.int32), cross=False, prec=prec, raw=True)
    assert past == 0 and np.isnan(got).all()
    got, past = _ctx().debug_attention(q, k, v, np.zeros(2, np.int32), cross=True, prec=prec, raw=True)
    assert past == 0 and np.isnan(got).all()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cross", [False, True])
def test_written_rows(cross, prec):
    """every row below lens[s] is written; waves that are entirely padding neither compute nor store: rows from 32 ceil(lens[s] / 32) up to Np keep the canary, and so do the
    slack rows behind the last sequence"""
    n, lens = 400, np.array([33, 400], np.int32)
    q, k, v = _random(2, 4, n, 433)
    got, past = _ctx().debug_attention(q, k, v, lens, cross=cross, prec=prec, raw=True)
    assert past == 0 and got.shape[1] == 400
    for s in range(2):
        assert np.isfinite(got[s, :lens[s]]).all()
        assert np.isnan(got[s, 32 * ((lens[s] + 31) // 32):]).all()
    _within_bound("written", f"written_{cross}", got, q, k, v, lens, cross, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_same_bits_twice(prec):
    n, lens = 144, np.array([129, 97], np.int32)
    q, k, v = _random(2, 4, n, 77)
    a, _ = _ctx().debug_attention(q, k, v, lens, cross=True, prec=prec, raw=True)
    b, _ = _ctx().debug_attention(q, k, v, lens, cross=True, prec=prec, raw=True)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
