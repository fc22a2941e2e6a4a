"""float64 reference of SuperGlue's front (sg_front_dev in airslam_amd/csrc/airfe_match.hip: sg_prepare_kernel in both forms and, split, the two MFMA GEMMs of the
keypoint encoder's large layers) with DERIVED bounds, and the weights, cases and planted mistakes that tests/test_gpu_sg_front.py (on the device) and
tests/test_sg_front_ref_cpu.py (which keeps this file honest) share.  numpy only; nothing here is fitted to a measurement.

Layers are numbered as the pack numbers them: kenc.encoder.i, i = 0 .. 4, sizes 3 -> 32 -> 64 -> 128 -> 256 -> 256, ReLU behind 0 .. 3.

  input      (x, y, score) in float32.  normalize: (v - c) * linv in float32 exactly as oracle/ref_post.normalize_keypoints does it (integer width // 2): the device's
             __fsub_rn / __fmul_rn give the same bits, so the input carries no error.
  fp32 layers  (the three small ones; unsplit: all five) are FMA loops from the bias: the reference is float64 on the float32 inputs and weights, and the bound goes
             layer by layer, e_out = |W| e_in + (K + 2) 2^-24 (|W| |h| + |b|).  ReLU is 1-Lipschitz: it does not enlarge it.
  unsplit    x32 = descriptor + y: e_4 and one more float32 rounding, ulp32(x).  xb is the device's own x32 rounded to the 2-byte type, bit for bit.
  split      every stage from the device's own previous output, so each bound is a one-stage bound:
               h128  the reference layer 2, rounded to the 2-byte type: e_2 + ulp2
               hb    relu(r2(W3) h128_dev + b3): kernel_ref.acc_bound + ulp2
               x32   descriptor + r2(W4) hb_dev + b4: kernel_ref.acc_bound + ulp32
               xb    the device's x32 rounded, bit for bit
  padding    rows at or past a sequence's length (the contract stated at sg_prepare_kernel and in DESIGN.md).  Unsplit: x32 and xb exactly zero.  Split: h128 exactly
             zero, hb exactly r2(relu(b3)) (a sum of exact zeros on the bias), x32 the constant row r2(W4) r2(relu(b3)) + b4 within acc_bound + ulp32, and every
             such row the same bits.
"""
from __future__ import annotations

import numpy as np

from airslam_amd import weights
from kernel_ref import EPS32, acc_bound, check, linear, r2, ulp2, ulp32      # noqa: F401  (check: re-exported for the two test files)
from oracle import ref_post

F = np.float32
SIZES = (3, 32, 64, 128, 256, 256)
SCALE = 0.7                       # PointMatcher's scale for SuperGlue (0.5 is LightGlue's)
MISTAKES = ("xy_swapped", "score_from_column_1", "no_relu_after_layer_1", "layer_4_bias_dropped", "centre_width_over_2.0", "scale_0.5")


def pack():
    """the pack both test files use: no 0.1 gain on kenc.encoder.4 (structured = False), so the encoder is not attenuated against the descriptor"""
    return weights.synthetic_superglue(1234, n_layers=2, structured=False)


# ------------------------------------------------------------------ cases (section "cases" of the test files' docstrings)
#   name: (context key, B, cap, n0 [B], n1 [B], normalize)
# lengths 1, 3, 4, 5, cap - 1, cap (the 4-keypoint groups of KE_LT and their tails), 0, unequal per side and pair, cap < Np, and Np = 400 with B = 1 (M = 800, Mg = 896)
CONTEXTS = {"np64": dict(max_keypoints=64, max_batch=2, image_width=752, image_height=480), "np400": dict(max_keypoints=400, max_batch=1, image_width=752, image_height=480),
            "odd": dict(max_keypoints=64, max_batch=2, image_width=753, image_height=481)}
CASES = {
    "b2_tails": ("np64", 2, 64, (1, 4), (3, 5), 0),
    "b2_full_and_empty": ("np64", 2, 64, (63, 64), (64, 0), 1),
    "b1_ragged": ("np64", 1, 64, (5,), (63,), 1),
    "b2_cap40": ("np64", 2, 40, (40, 1), (3, 39), 0),
    "b1_np400_surplus": ("np400", 1, 400, (400,), (317,), 1),
    "b1_np400_cap100": ("np400", 1, 100, (99,), (4,), 0),
    "b2_odd_size": ("odd", 2, 64, (64, 5), (33, 64), 1),
}


def features(seed: int, B: int, cap: int, width: int, height: int, raw: bool):
    """f [B, cap, 259] rows (score, x, y, unit descriptor): raw pixel coordinates, or normalised ones.  Row 0 holds score 0 at the image's origin, row 1 the far
    corner, row 2 a negative coordinate and a zero, row 3 the centre; every row is finite (the counts decide what is read)."""
    rng = np.random.default_rng(seed)
    f = np.empty((B, cap, 259), F)
    f[..., 0] = rng.uniform(0.0, 1.0, (B, cap))
    f[..., 1] = rng.uniform(0.0, width - 1, (B, cap))
    f[..., 2] = rng.uniform(0.0, height - 1, (B, cap))
    d = rng.normal(size=(B, cap, 256))
    f[..., 3:] = d / np.linalg.norm(d, axis=-1, keepdims=True)
    special = [(0.0, 0.0, 0.0), (1.0, width - 1.0, height - 1.0), (0.25, -3.5, 0.0), (0.5, float(width // 2), float(height // 2))]
    for r, (s, x, y) in enumerate(special[:cap]):
        f[:, r, 0], f[:, r, 1], f[:, r, 2] = s, x, y
    if not raw:
        for b in range(B):
            f[b] = ref_post.normalize_keypoints(f[b], width, height, SCALE)
    return f


def case_inputs(name: str):
    """-> (context key, f0, f1, n0, n1, normalize, width, height)"""
    key, B, cap, n0, n1, norm = CASES[name]
    c = CONTEXTS[key]
    seed = 100 + sorted(CASES).index(name)
    f0, f1 = features(seed, B, cap, c["image_width"], c["image_height"], bool(norm)), features(seed + 50, B, cap, c["image_width"], c["image_height"], bool(norm))
    return key, f0, f1, list(n0), list(n1), norm, c["image_width"], c["image_height"]


# ------------------------------------------------------------------ the encoder
def encoder_input(rows, normalize, width, height, mistake=None):
    """rows [n, 259] float32 -> (x, y, score) [n, 3] float32, as the kernel's first twelve threads build it"""
    rows = np.asarray(rows, F)
    if normalize:
        if mistake == "centre_width_over_2.0":
            l_inv = F(1.0 / max(width, height) * float(F(SCALE)))
            rows = rows.copy()
            rows[:, 1] = ((rows[:, 1] - F(width / 2.0)) * l_inv).astype(F)
            rows[:, 2] = ((rows[:, 2] - F(height / 2.0)) * l_inv).astype(F)
        else:
            rows = ref_post.normalize_keypoints(rows, width, height, 0.5 if mistake == "scale_0.5" else SCALE)
    x, y, s = rows[:, 1], rows[:, 2], rows[:, 1 if mistake == "score_from_column_1" else 0]
    if mistake == "xy_swapped":
        x, y = y, x
    return np.stack([x, y, s], 1).astype(F)


def fp32_layers(w, h, first, last, mistake=None):
    """layers first .. last as fp32 FMA loops on h (exact float32 values) -> (float64 output, bound)"""
    h = np.asarray(h, np.float64)
    e = np.zeros_like(h)
    for i in range(first, last + 1):
        W, b = w[f"kenc.encoder.{i}.weight"].astype(np.float64), w[f"kenc.encoder.{i}.bias"].astype(np.float64)
        if mistake == "layer_4_bias_dropped" and i == 4:
            b = np.zeros_like(b)
        e = e @ np.abs(W).T + (W.shape[1] + 2) * EPS32 * (np.abs(h) @ np.abs(W).T + np.abs(b))
        h = h @ W.T + b
        if i < 4 and not (mistake == "no_relu_after_layer_1" and i == 1):
            h = np.maximum(h, 0.0)
    return h, e


def front(w, f0, f1, n0, n1, Np, normalize, width, height, mistake=None):
    """The front of one call, sequence s = 2 b + side at rows s Np ..: dict lens [2B], valid [M] bool, desc [M, 256], h2 / e2 [M, 128] (layer 2's output), x / ex
    [M, 256] (the unsplit form's x32 and its bound, the final rounding included).  Padding rows are zero with a zero bound."""
    B = f0.shape[0]
    M = 2 * B * Np
    out = {"lens": np.array([n for b in range(B) for n in (n0[b], n1[b])], np.int32), "valid": np.zeros(M, bool), "desc": np.zeros((M, 256)),
           "h2": np.zeros((M, 128)), "e2": np.zeros((M, 128)), "x": np.zeros((M, 256)), "ex": np.zeros((M, 256))}
    for s, n in enumerate(out["lens"]):
        if n == 0:
            continue
        rows = np.asarray((f1 if s & 1 else f0)[s >> 1, :n], F)
        r = slice(s * Np, s * Np + n)
        k = encoder_input(rows, normalize, width, height, mistake)
        h2, e2 = fp32_layers(w, k, 0, 2, mistake)
        y, e4 = fp32_layers(w, k, 0, 4, mistake)
        x = rows[:, 3:].astype(np.float64) + y
        out["valid"][r], out["desc"][r], out["h2"][r], out["e2"][r], out["x"][r], out["ex"][r] = True, rows[:, 3:], h2, e2, x, e4 + ulp32(x)
    return out


# ------------------------------------------------------------------ the split form, stage by stage on the device's own outputs
def split_h128(ref, prec):
    """-> (reference h128 [M, 128], bound)"""
    return r2(ref["h2"], prec), ref["e2"] + ulp2(ref["h2"], prec) * ref["valid"][:, None]


def split_hb(w, h128_dev, prec):
    """hb [rows, 256] from the device's h128 (2-byte values, widened) -> (reference, bound)"""
    y, d = linear(h128_dev, r2(w["kenc.encoder.3.weight"], prec), w["kenc.encoder.3.bias"], relu=True)
    return r2(y, prec), d + ulp2(y, prec)


def split_x32(w, x_in, hb_dev, prec):
    """x32 [rows, 256] = x_in (what the prepare kernel left there: the descriptor, zero in padding and surplus rows) + r2(W4) hb_dev + b4 -> (reference, bound)"""
    y, d = linear(hb_dev, r2(w["kenc.encoder.4.weight"], prec), w["kenc.encoder.4.bias"])
    x = np.asarray(x_in, np.float64) + y
    return x, d + ulp32(x)


def split_padding_row(w, prec):
    """-> (hb [256] exactly, x32 [256], bound [256]) of a row whose h128 and descriptor are zero"""
    hb = r2(np.maximum(w["kenc.encoder.3.bias"].astype(np.float64), 0.0), prec)
    x, d = split_x32(w, np.zeros((1, 256)), hb[None], prec)
    return hb, x[0], d[0]


def same_bits(a, b) -> bool:
    """bit for bit, NaN patterns and the sign of zero included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
