"""Plain reference, per-element envelope and hand-built cases for the PLNet stage-0 decode (airfe_debug_s0_decode, include/airfe_debug.h; kernels_s0.hip: s0_hafm / s0_jloc
in s0_decode_kernel and s0_head_decode_kernel, s0_jnms_kernel, s0_loi_chw_kernel).  numpy only, no device code.

REFERENCE (decode): HAWP's hafm_decoding and the contract of SURVEY.md Appendix A.1, per pixel p = (y0, x0) of the 128 x 128 map, from the 17 head channels
md0 md1 md2 dis res | jloc0 jloc1 | joffx joffy | thin0..3 | aux0..3:
    s_k = sigmoid of md0, md1, md2, dis, res;  md_un = (s_md0 - 1/2) 2 pi,  st_un = s_md1 pi / 2,  ed_un = -s_md2 pi / 2
    d_r = clamp(s_dis + r s_res, 0, 1) for the three proposals r = -1, 0, +1
    start = (cos md_un - sin md_un tan st_un, sin md_un + cos md_un tan st_un) 5 d_r + (x0, y0), end = the same with ed_un; every coordinate clamped to [0, 127]
    lines_pred[r * 16384 + p] = (x_start, y_start, x_end, y_end);  jloc = softmax(jloc0, jloc1)[1];  joff = sigmoid(joffx, joffy) - 1/2
and the pure copies: thin / aux as CHW planes, ta8 = thin0..3 | aux0..3 pixel-major, loi CHW, jnms = a * (a == max3x3(a)).  decode(h, float64) is the reference;
decode(h, float32) is the same expressions in float32 (pi rounded to float32 first, as the kernel and the oracle have it) and serves only to validate the envelope and
as the expected value of the `pole` case.

ENVELOPE (envelope): the gate for computed values, per element, derived and not measured.  u = 2^-24 is float32's unit roundoff, 1 ulp <= 2 u relative.
  sigmoid = 1 / (1 + expf(-x)): expf <= 1 ulp (2 u; it enters 1 + e with weight e / (1 + e) <= 1), the sum u, the division u: 4 u.
  angles: (s - 1/2) * fl32(pi) * 2 — the difference u, fl32(pi) itself 0.47 u off pi, the product u, * 2 exact: 2.5 u on top of the sigmoid's error IN s (which the
    difference can amplify without bound near s = 1/2: hence s is perturbed first and the angle computed from it).  s * fl32(pi) / 2: 1.5 u.  tanf <= 1 ulp of its
    result, which is an angle error of at most 2 u relative (d tan / tan = d theta / (sin theta cos theta) >= d theta / theta): 3.5 u.
  d: the sum u, then the two products d * 5 of the coordinate, u each: 3 u on top of the sigmoids' errors (again amplified by the cancellation in s_dis - s_res:
    the sigmoids are perturbed first).
  The largest of these is 4 u; E = 4 x 4 u = 2^-20 gives it the factor 4 of head-room the sibling pins use (a different but valid order of the same float32
  operations, a fused multiply-add where the statement has two roundings).
  What no relative change of s, the angles or d expresses — cosf / sinf <= 1 ulp of their own results (2 u each), the product sin * tan (u), the difference (u), the
  final sum with the pixel coordinate (u, which also covers the stored result's rounding) — is at most 5 u of T = (|cos| + |sin tan|) 5 d + |x0|, the magnitudes of the
  terms: the floor is 4 x 5 u T = 10 ulp of T, plus 2^-126 absolute (a sigmoid below float32's normal range may come out as 0).
  The interval of every quantity is followed through the expression: s (1 +- E), the angle from it (1 +- E), d from the perturbed sigmoids, clamped, (1 +- E); the
  unclamped coordinate is evaluated at the 8 corners (md_un, st_un or ed_un, d) — it is linear in tan and in d, and over 2^-20 of an angle cos and sin are monotone
  up to a second-order term far below the floor — widened by the floor, and only THEN clamped: env = the larger distance of the two clamped ends from the clamped
  reference.  Clamps are continuous, so no element is left out; a coordinate that is clamped with the whole interval has envelope 0 and must be 0 or 127 exactly.
  joff: E s + 4 u |s - 1/2|.  jloc = e1 / (e0 + e1) with the larger exponent 0: the other's argument is a rounded difference (u |D|, D = jloc1 - jloc0) under expf
  (2 u; allowed for both), which reaches jloc with weight 1 - jloc; the sum and the division u each: 4 x ((1 - jloc)(4 + |D|) + 2) u jloc + 2^-126.
  The envelope says nothing where the angle's interval reaches the pole of tan (a sigmoid within 2 E of 1: logits above ~13): such inputs belong to `pole`.

CASES (case): each a full [2, 17, 128, 128] float32 tensor of head channels (the kernels hard-wire the map size), image 1 drawn with another seed.  EVERY logit has
at most 8 significant bits and magnitude in [2^-14, 2^15] or is 0, so it is exact in bf16 and in fp16: features_for turns a case into line features and a one-hot head
that reproduce it exactly through the MFMA (thin / aux are integers below 2^18 — 2^17 image + 8 pixel + channel — split into four 5-bit digits on feature blocks 0 .. 3
under head entries 1, 2^5, 2^10, 2^15), so the same reference and envelope apply to the fused kernel.
  benign             md1 / md2 logits in [-3, 3]
  steep              md1 / md2 logits up to +-10 (the float64 angle stays > 500 float32 ulps from the pole), small d so that the steep tan shows unclamped
  clamps             both clamps of d and the endpoint clamps on all four sides, pixel rows / columns 0 and 127 included
  saturated_sigmoid  logits +-90 in every decoded channel (expf overflows: the sigmoid is exactly 0 or 1), jloc logits 200 apart (jloc exactly 0 or 1); md1 / md2 are
                     +90 only where d = 0 for all three proposals — elsewhere +90 is the pole, which the next case owns
  pole               md1 and / or md2 logits >= 17: the float32 sigmoid is 1.0f, st_un = fl32(pi) / 2 lies PAST the pole and tan is negative; float64 stays before it.
                     The case pins the float32 contract: expected is decode(h, float32), every unclamped float32 coordinate lies more than 1 px outside [0, 127], so the
                     clamped result is decided by the sign of tan alone and is compared for equality.  (A pixel has both logits at the pole, or one at the pole and the
                     other at 11 .. 13, steep enough for the same to hold on the regular side.)
  copies             benign logits; jloc logits on five levels in blocks, so that jloc has plateaus and exact ties for jnms
thin / aux / LOI hold values that identify (image, pixel, channel) in EVERY case, so any permutation shows."""
from __future__ import annotations

import functools
import zlib

import numpy as np

F = np.float32
FH, NPX, NP = 128, 128 * 128, 3 * 128 * 128
U = 2.0 ** -24
E = 16 * U                                   # 4 x the 4 u derived above
FLOOR_U = 20                                 # 4 x the 5 u derived above, in units of u
TINY = 2.0 ** -126
MUTANTS = ("residual_order", "swap_st_ed", "ed_sign", "scale_4", "no_d_clamp", "clamp_128", "swap_x0_y0", "jloc_ch0", "joff_swap", "joff_no_half")
BOUNDED = ("benign", "steep", "clamps", "saturated_sigmoid", "copies")
CASES = BOUNDED + ("pole",)
POLE_LOGITS = (17.0, 17.5, 18.0, 20.0, 30.0, 60.0, 90.0)


# ================================================================================================================ reference
def _sigmoid(x):
    with np.errstate(over="ignore"):
        return x.dtype.type(1) / (x.dtype.type(1) + np.exp(-x))


def _grid(dt):
    y0, x0 = np.meshgrid(np.arange(FH, dtype=dt), np.arange(FH, dtype=dt), indexing="ij")
    return x0, y0


def _hafm(md_un, st_un, ed_un, d, x0, y0, scale):
    """unclamped [..., 3, 128, 128, 4] from angles [..., 128, 128] and d [..., 3, 128, 128]"""
    cs, ss, yst, yed = (v[..., None, :, :] for v in (np.cos(md_un), np.sin(md_un), np.tan(st_un), np.tan(ed_un)))
    return np.stack([(cs - ss * yst) * d * scale + x0, (ss + cs * yst) * d * scale + y0, (cs - ss * yed) * d * scale + x0, (ss + cs * yed) * d * scale + y0], -1)


def decode(h: np.ndarray, dt=np.float64, mutant: str = None, clamp: bool = True):
    """h [..., 17, 128, 128] -> dict lines [..., 49152, 4], jloc [..., 128, 128], joff [..., 2, 128, 128] in dtype dt.  mutant: one of MUTANTS (a wrong decode, for
    tests/test_s0_decode_ref_cpu.py).  clamp = False: the endpoint coordinates before their clamp."""
    assert mutant is None or mutant in MUTANTS
    h = np.asarray(h).astype(dt)
    c = lambda i: h[..., i, :, :]
    pi = dt(F(np.pi)) if dt is F else dt(np.pi)
    one, half, two = dt(1), dt(0.5), dt(2)
    s = _sigmoid(h[..., 0:5, :, :])
    md0, md1, md2, dis, res = (s[..., i, :, :] for i in range(5))
    md_un, st_un, ed_un = (md0 - half) * pi * two, md1 * pi / two, -md2 * pi / two
    if mutant == "ed_sign":
        ed_un = -ed_un
    sign = np.array([1, 0, -1] if mutant == "residual_order" else [-1, 0, 1], dt).reshape(3, 1, 1)
    d = dis[..., None, :, :] + res[..., None, :, :] * sign
    if mutant != "no_d_clamp":
        d = np.clip(d, dt(0), one)
    x0, y0 = _grid(dt)
    if mutant == "swap_x0_y0":
        x0, y0 = y0, x0
    v = _hafm(md_un, st_un, ed_un, d, x0, y0, dt(4 if mutant == "scale_4" else 5))
    if mutant == "swap_st_ed":
        v = v[..., [2, 3, 0, 1]]
    if clamp:
        v = np.clip(v, dt(0), dt(128 if mutant == "clamp_128" else 127))
    o5, o6 = (c(6), c(5)) if mutant == "jloc_ch0" else (c(5), c(6))
    mx = np.maximum(o5, o6)
    e0, e1 = np.exp(o5 - mx), np.exp(o6 - mx)
    jx, jy = (c(8), c(7)) if mutant == "joff_swap" else (c(7), c(8))
    joff = _sigmoid(np.stack([jx, jy], -3)) - (dt(0) if mutant == "joff_no_half" else half)
    return {"lines": v.reshape(h.shape[:-3] + (NP, 4)), "jloc": e1 / (e0 + e1), "joff": joff}


def envelope(h: np.ndarray):
    """the per-element gate of the module docstring around decode(h, float64): dict lines / jloc / joff, float64, shaped like decode's"""
    h = np.asarray(h).astype(np.float64)
    s = _sigmoid(h[..., 0:5, :, :])
    lo, hi = s * (1 - E), s * (1 + E)
    pm = ((lo, 1 - E), (lo, 1 + E), (hi, 1 - E), (hi, 1 + E))
    md = np.stack([(a[..., 0, :, :] - 0.5) * np.pi * 2 * f for a, f in pm])
    md_b = (md.min(0), md.max(0))
    st_b = (lo[..., 1, :, :] * (1 - E) * np.pi / 2, hi[..., 1, :, :] * (1 + E) * np.pi / 2)
    ed_b = (-hi[..., 2, :, :] * (1 + E) * np.pi / 2, -lo[..., 2, :, :] * (1 - E) * np.pi / 2)
    sign = np.array([-1.0, 0.0, 1.0]).reshape(3, 1, 1)
    r_lo, r_hi = lo[..., 4, :, :][..., None, :, :] * sign, hi[..., 4, :, :][..., None, :, :] * sign
    d_b = (np.clip(lo[..., 3, :, :][..., None, :, :] + np.minimum(r_lo, r_hi), 0, 1) * (1 - E), np.clip(hi[..., 3, :, :][..., None, :, :] + np.maximum(r_lo, r_hi), 0, 1) * (1 + E))
    x0, y0 = _grid(np.float64)
    vmin = vmax = tmax = None
    for i in range(8):
        a, t, d = md_b[i & 1], (i >> 1) & 1, d_b[i >> 2]
        v = _hafm(a, st_b[t], ed_b[t], d, x0, y0, 5.0)
        cs, ss = np.abs(np.cos(a))[..., None, :, :], np.abs(np.sin(a))[..., None, :, :]
        yst, yed = np.abs(np.tan(st_b[t]))[..., None, :, :], np.abs(np.tan(ed_b[t]))[..., None, :, :]
        T = np.stack([(cs + ss * yst) * d * 5 + x0, (ss + cs * yst) * d * 5 + y0, (cs + ss * yed) * d * 5 + x0, (ss + cs * yed) * d * 5 + y0], -1)
        vmin, vmax, tmax = (v, v, T) if vmin is None else (np.minimum(vmin, v), np.maximum(vmax, v), np.maximum(tmax, T))
    floor = FLOOR_U * U * tmax + TINY
    ref = decode(h, np.float64)
    r = ref["lines"].reshape(vmin.shape)
    env = np.maximum(np.abs(np.clip(vmax + floor, 0, 127) - r), np.abs(np.clip(vmin - floor, 0, 127) - r))
    sj = _sigmoid(h[..., 7:9, :, :])
    D = np.abs(h[..., 6, :, :] - h[..., 5, :, :])
    j = ref["jloc"]
    return {"lines": env.reshape(ref["lines"].shape), "joff": E * sj + 4 * U * np.abs(sj - 0.5) + TINY, "jloc": 4 * ((1 - j) * (4 + D) + 2) * U * j + TINY}


def jnms_ref(a: np.ndarray) -> np.ndarray:
    """a [..., 128, 128] -> a * (a == max_pool2d(a, 3, 1, 1)), the dtype kept"""
    pad = np.full(a.shape[:-2] + (FH + 2, FH + 2), -np.inf, a.dtype)
    pad[..., 1:-1, 1:-1] = a
    mp = np.max(np.stack([pad[..., dy:dy + FH, dx:dx + FH] for dy in range(3) for dx in range(3)]), 0)
    return np.where(a == mp, a, a.dtype.type(0))


# ================================================================================================================ cases
def q8(v: np.ndarray) -> np.ndarray:
    """the nearest value with at most 8 significant bits, 0 below 2^-14: exact in float32, bf16 and fp16"""
    m, e = np.frexp(np.asarray(v, np.float64))
    out = np.ldexp(np.round(m * 256) / 256, e)
    out[np.abs(out) < 2.0 ** -14] = 0.0
    assert np.abs(out).max() <= 2.0 ** 15
    return out.astype(F)


def ids_ta(b: int) -> np.ndarray:
    """thin0..3 | aux0..3 of image b as [8, 128, 128]: 2^17 b + 8 p + channel"""
    return (b * 2 ** 17 + 8 * np.arange(NPX)[None, :] + np.arange(8)[:, None]).reshape(8, FH, FH).astype(F)


def ids_loi(b: int) -> np.ndarray:
    """the 128 LOI channels of image b pixel-major [16384, 128]: 2^21 b + 128 p + channel"""
    return (b * 2 ** 21 + 128 * np.arange(NPX)[:, None] + np.arange(128)[None, :]).astype(F)


def _image(name: str, b: int) -> np.ndarray:
    g = np.random.default_rng(zlib.crc32(f"{name}/{b}".encode()))
    u = lambda lo, hi: g.uniform(lo, hi, (FH, FH))
    pick = lambda vals: g.choice(np.asarray(vals, np.float64), (FH, FH))
    h = np.zeros((17, FH, FH))
    h[0], h[1], h[2], h[3], h[4] = u(-3, 3), u(-3, 3), u(-3, 3), u(-2, 2), u(-3, 0)          # benign; the cases below replace what they are about
    h[5], h[6], h[7], h[8] = u(-4, 4), u(-4, 4), u(-4, 4), u(-4, 4)
    if name == "steep":
        kind = g.integers(0, 4, (FH, FH))                      # 0: md1 steep towards the pole, 1: md2, 2: both steep away from it, 3: benign
        steep = u(6, 10)
        h[1] = np.where(kind == 0, steep, np.where(kind == 2, -steep, h[1]))
        h[2] = np.where(kind == 1, steep, np.where(kind == 2, -steep, h[2]))
        h[3], h[4] = u(-10, -6), u(-12, -8)
    elif name == "clamps":
        h[1], h[2], h[3], h[4] = u(-1, 4), u(-1, 4), u(-2, 3), u(-2, 3)
    elif name == "saturated_sigmoid":
        for i in (0, 1, 2, 3, 4, 7, 8):
            h[i] = pick([-90, 90])
        nz = (h[3] > 0) | (h[4] > 0)                           # some d_r > 0: +90 in md1 / md2 would be the pole
        h[1], h[2] = np.where(nz, -90, h[1]), np.where(nz, -90, h[2])
        h[5] = pick([-100, 100])
        h[6] = -h[5]
    elif name == "pole":
        # md_un with |cos|, |sin| >= 0.3 (0.3047 .. pi/2 - 0.3047 in every quadrant), d_r in [0.5, 0.9]: |5 d sin tan|, |5 d cos tan| > 127 + 1 by orders of magnitude
        th = (u(0.32, np.pi / 2 - 0.32) + pick([0, 1, 2, 3]) * np.pi / 2) - np.pi
        sm = th / (2 * np.pi) + 0.5
        h[0] = np.log(sm / (1 - sm))
        grp = np.arange(NPX).reshape(FH, FH) % 3               # 0: both at the pole, 1: md1 at the pole, md2 steep, 2: the reverse
        pole, steep = pick(POLE_LOGITS), pick([11.0, 12.0, 13.0])
        h[1], h[2] = np.where(grp == 2, steep, pole), np.where(grp == 1, steep, pole)
        h[3], h[4] = u(1.0, 2.0), u(-3.0, -1.5)
    elif name == "copies":
        lv = g.choice(np.array([-2.0, -1.0, 0.0, 1.0, 2.0]), (FH // 4, FH // 2))
        h[5], h[6] = 0.0, np.repeat(np.repeat(lv, 4, 0), 2, 1)      # 4 x 2 blocks of one level: plateaus, and ties between blocks of the same level
    else:
        assert name == "benign", name
    out = np.concatenate([q8(h[:9]), ids_ta(b)])
    return out


@functools.lru_cache(maxsize=None)
def case(name: str) -> np.ndarray:
    """[2, 17, 128, 128] float32, read-only"""
    h = np.stack([_image(name, b) for b in range(2)])
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """(reference, envelope, float32 restatement) of a case, each a dict of read-only [2, ...] arrays; thin / aux / ta8 / loi come from the case itself (expected_copies)"""
    out = (decode(case(name), np.float64), envelope(case(name)), decode(case(name), F))
    for d in out:
        for v in d.values():
            v.setflags(write=False)
    return out


def rows_for(h: np.ndarray, ld: int, off: int) -> np.ndarray:
    """head rows [B, 16384, ld] of one of the two production layouts: the 17 channels from column off, the LOI ids in columns 0 .. 127 of the (160, 128) layout, NaN in
    every column nothing may read"""
    B = h.shape[0]
    rows = np.full((B, NPX, ld), np.nan, F)
    rows[:, :, off:off + 17] = h.reshape(B, 17, NPX).transpose(0, 2, 1)
    if off == 128:
        for b in range(B):
            rows[b, :, :128] = ids_loi(b)
    return rows


def features_for(h: np.ndarray):
    """-> x [B * 16384, 128], w [17, 128], b [17]: line features and a one-hot head whose rows x w^T + b equal h exactly in bf16 and fp16 storage with fp32 accumulation.
    Logit channel c: feature c under w[c][c] = 1.  thin / aux channel c (an integer below 2^20): four 5-bit digits in features c, 32 + c, 64 + c, 96 + c under
    w = 1, 2^5, 2^10, 2^15."""
    B = h.shape[0]
    hp = h.reshape(B, 17, NPX).transpose(0, 2, 1).reshape(B * NPX, 17)
    x, w = np.zeros((B * NPX, 128), F), np.zeros((17, 128), F)
    x[:, :9] = hp[:, :9]
    w[np.arange(9), np.arange(9)] = 1
    v = hp[:, 9:].astype(np.int64)
    assert (v == hp[:, 9:]).all() and v.min() >= 0 and v.max() < 2 ** 20
    for k in range(4):
        x[:, 32 * k + 9:32 * k + 17] = (v >> (5 * k)) & 31
        w[np.arange(9, 17), 32 * k + np.arange(9, 17)] = 2.0 ** (5 * k)
    assert np.array_equal(x.astype(np.float64) @ w.astype(np.float64).T, hp.astype(np.float64))
    return x, w, np.zeros(17, F)


def expected_copies(h: np.ndarray):
    """the pure copies of h [B, 17, 128, 128]: thin, aux [B, 4, 128, 128], ta8 [B, 16384, 8], loi [128, 128, 128] (CHW, image 0: what rows_for's LOI columns hold)"""
    B = h.shape[0]
    return {"thin": h[:, 9:13], "aux": h[:, 13:17], "ta8": np.ascontiguousarray(h[:, 9:17].reshape(B, 8, NPX).transpose(0, 2, 1)),
            "loi": np.ascontiguousarray(ids_loi(0).T).reshape(128, FH, FH)}


def clamp_sides(h: np.ndarray):
    """how many elements of a case reach each of the six clamp sides in float64: d below 0 / above 1, x below 0 / above 127, y below 0 / above 127"""
    s = _sigmoid(np.asarray(h, np.float64)[..., 0:5, :, :])
    d = s[..., 3, :, :][..., None, :, :] + s[..., 4, :, :][..., None, :, :] * np.array([-1.0, 0.0, 1.0]).reshape(3, 1, 1)
    v = decode(h, np.float64, clamp=False)["lines"]
    x, y = v[..., [0, 2]], v[..., [1, 3]]
    return {"d_lo": int((d < 0).sum()), "d_hi": int((d > 1).sum()), "x_lo": int((x < 0).sum()), "x_hi": int((x > 127).sum()), "y_lo": int((y < 0).sum()),
            "y_hi": int((y > 127).sum())}
