"""Cost of stereo line triangulation on the device (kernels_stereoline.hip; include/airfe.h "Stereo lines"), timed between device events: medians over
--reps timed calls after 3 warm-ups, with min / max.
  Scene     16 synthetic stereo pairs (752x480) through airfe_stereo_plnet_batch_dev once; B = 1 takes the first pair, B = 64 the 16 pairs four times over.
            capL = 512 line slots, 400 keypoints, 8192 relation entries per frame; one random pose per frame.
  Timed     (a) airfe_stereo_lines_batch_dev alone on the lines and the line matches of the scene;
            (b) the composite airfe_stereo_line_landmarks_batch_dev: association left, association right, MatchLines with the band, triangulation;
            (c) the same chain by hand, in the same run: the three existing entries, then the line lists, their counts and the line matches
                downloaded (the whole [2B][capL][4] buffer: the counts are not known on the host before), selection and triangulation by the host core
                (the C entry airfe_stereo_lines per frame, writing straight into the upload buffers), and the six results uploaded at their capacity.
                Pinned host buffers on both ways, allocated once outside the clock, asynchronous copies, ONE synchronisation.  The baseline is existing
                entries plus the host core, not the code under test.
  Checked   before anything is timed: (a), (b) and (c) give the same bytes, every output.
  Condition ratio (b) / (c) <= 1.0.
    python tools/stereolines_timing.py [--reps R] [--quick] [--out FILE]        (on an MI355X; one JSON line per batch size)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from airslam_amd import api, synth, weights  # noqa: E402
from bowdb_timing import timed  # noqa: E402

CAM = (2.0, 60.0, 3.0, 47.90639384423901, 458.654, 457.296, 367.215, 248.375)
KEYS = ("lines_right_sel", "right_valid", "status", "endpoints", "plucker", "count")
H, W, K, CL, CJ, CE, B0 = 480, 752, 400, 512, 1024, 8192, 16


def scene(ctx):
    """the PLNet stereo step's outputs for B0 pairs, on the device"""
    import torch
    dev = torch.device("cuda")
    ls, rs = synth.stereo_batch(B0, H, W, 31)
    L, R = torch.from_numpy(ls).to(dev), torch.from_numpy(rs).to(dev)
    z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    s = dict(fl=z((B0, K, 259)), fr=z((B0, K, 259)), nl=z((B0,), torch.int32), nr=z((B0,), torch.int32), idx=z((B0, K, 2), torch.int32), sc=z((B0, K)),
             nm=z((B0,), torch.int32), lines=z((2 * B0, CL, 4), torch.float64), nlines=z((2 * B0,), torch.int32))
    junc, njunc = z((B0, CJ, 259)), z((B0,), torch.int32)
    ctx.stereo_plnet_batch_dev(L, R, s["fl"], s["fr"], s["nl"], s["nr"], s["lines"], s["nlines"], junc, njunc, s["idx"], s["sc"], s["nm"])
    ctx.sync()
    return s


def batch_of(s, B):
    """B frames of the scene: the first B, or the scene repeated; left and right lines stay the halves of one [2B][capL][4] buffer"""
    import torch
    pick = torch.arange(B, device="cuda") % B0
    t = {k: s[k][pick].contiguous() for k in ("fl", "fr", "nl", "nr", "idx", "nm")}
    t["lines"] = torch.cat([s["lines"][pick], s["lines"][B0 + pick]]).contiguous()
    t["nlines"] = torch.cat([s["nlines"][pick], s["nlines"][B0 + pick]]).contiguous()
    return t


def one_batch(ctx, s, B, reps, emit):
    import torch
    import stereoline_ref as sr
    dev = torch.device("cuda")
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    t = batch_of(s, B)
    rng = np.random.RandomState(B)
    Twc_h = np.stack([sr._pose(rng) for _ in range(B)])
    Twc = torch.from_numpy(Twc_h).to(dev)
    left, right, nL, nR = t["lines"][:B], t["lines"][B:], t["nlines"][:B], t["nlines"][B:]

    def relation():
        return (torch.zeros((B, CL + 1), dtype=torch.int32, device=dev), torch.zeros((B, CE), dtype=torch.int32, device=dev),
                torch.zeros((B, CE), dtype=torch.float64, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev))

    def outputs():
        return dict(lines_right_sel=torch.zeros((B, CL, 4), dtype=torch.float64, device=dev), right_valid=torch.zeros((B, CL), dtype=torch.uint8, device=dev),
                    status=torch.zeros((B, CL), dtype=torch.int32, device=dev), endpoints=torch.zeros((B, CL, 6), dtype=torch.float64, device=dev),
                    plucker=torch.zeros((B, CL, 6), dtype=torch.float64, device=dev), count=torch.zeros((B, 3), dtype=torch.int32, device=dev))
    rel = [relation() for _ in range(4)]                            # composite left / right, by hand left / right
    lm_c, lm_h = (torch.full((B, CL), -1, dtype=torch.int32, device=dev) for _ in range(2))
    out_a, out_b, out_c = outputs(), outputs(), outputs()
    args = lambda o: [o[k] for k in KEYS]  # noqa: E731
    torch.cuda.synchronize()

    def alone():
        ctx.stereo_lines_batch_dev(CAM, left, nL, right, nR, lm_h, Twc, *args(out_a), stream=sp)

    def composite():
        ctx.stereo_line_landmarks_batch_dev(CAM, left, nL, right, nR, t["fl"], t["nl"], t["fr"], t["nr"], t["idx"], t["nm"], Twc, rel[0], rel[1], lm_c,
                                            *args(out_b), stream=sp)

    # the baseline's host side, set up ONCE outside the clock: pinned buffers for the downloads and the uploads, the camera and the poses as C arrays
    import ctypes as C
    pin = lambda shape, dt: torch.zeros(shape, dtype=dt).pin_memory()  # noqa: E731
    p_lines, p_n, p_lm = pin((2 * B, CL, 4), torch.float64), pin((2 * B,), torch.int32), pin((B, CL), torch.int32)
    p_out = {k: pin(tuple(out_c[k].shape), out_c[k].dtype) for k in KEYS}
    v_lines, v_n, v_lm = p_lines.numpy(), p_n.numpy(), p_lm.numpy()
    v_out = {k: p_out[k].numpy() for k in KEYS}
    cam_c = (C.c_double * 8)(*CAM)
    entry, handle = ctx._l.airfe_stereo_lines, ctx._h
    row = lambda v, b: v[b].ctypes.data  # noqa: E731

    def by_hand():
        ctx.assign_points_to_lines_batch_dev(left, nL, t["fl"], t["nl"], *rel[2], stream=sp)
        ctx.assign_points_to_lines_batch_dev(right, nR, t["fr"], t["nr"], *rel[3], stream=sp)
        ctx.match_lines_batch_dev(rel[2][0], rel[2][1], nL, t["nl"], rel[3][0], rel[3][1], nR, t["nr"], t["idx"], t["nm"], lm_h, stereo_filter=CAM[:3],
                                  feat0_t=t["fl"], feat1_t=t["fr"], stream=sp)
        with torch.cuda.stream(st):
            p_lines.copy_(t["lines"], non_blocking=True)           # the line lists, their counts and the line matches, to pinned memory
            p_n.copy_(t["nlines"], non_blocking=True)
            p_lm.copy_(lm_h, non_blocking=True)
            st.synchronize()
            for b in range(B):                                      # the host core per frame, through the C entry, straight into the upload buffers
                if entry(handle, cam_c, row(v_lines, b), int(v_n[b]), row(v_lines, B + b), int(v_n[B + b]), row(v_lm, b), Twc_h[b].ctypes.data,
                         row(v_out["lines_right_sel"], b), row(v_out["right_valid"], b), row(v_out["status"], b), row(v_out["endpoints"], b),
                         row(v_out["plucker"], b), row(v_out["count"], b)):
                    raise RuntimeError("airfe_stereo_lines failed")
            for k in KEYS:
                out_c[k].copy_(p_out[k], non_blocking=True)

    by_hand()
    composite()
    alone()
    torch.cuda.synchronize()
    n_h = t["nlines"].cpu().numpy()
    live = torch.arange(CL, device=dev)[None, :] < nL[:, None]     # the slots the contract speaks of: the first nlines_left of every frame
    for k in KEYS:
        m = live if k != "count" else torch.ones((B,), dtype=torch.bool, device=dev)
        for other, name in ((out_b, "the composite"), (out_a, "the batch entry alone")):
            assert out_c[k][m].cpu().numpy().tobytes() == other[k][m].cpu().numpy().tobytes(), f"{name} and the chain by hand disagree in {k}"
    assert torch.equal(lm_c, lm_h) and all(torch.equal(a, b) for a, b in zip(rel[0] + rel[1], rel[2] + rel[3])), "relations / line matches disagree"
    count = out_b["count"].cpu().numpy().sum(0)
    ta, tb, tc = timed(alone, st, reps), timed(composite, st, reps), timed(by_hand, st, reps)
    emit(what="stereo_lines", B=B, capL=CL, left_lines=int(n_h[:B].sum()), valid_right=int(count[0]), triangulated=int(count[1]), map_lines=int(count[2]),
         reps=reps, batch_entry_ms_median_min_max=ta, composite_ms_median_min_max=tb, by_hand_ms_median_min_max=tc,
         ratio_composite_over_by_hand=round(tb[0] / tc[0], 6), condition_ratio_le_1=bool(tb[0] <= tc[0]))


def main(reps=20, quick=False, out=None):
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)
    ctx = api.Context(superpoint=weights.synthetic_plnet_s0(1234), lightglue=weights.synthetic_lightglue(1234),
                      plnet_s1=os.path.join(ROOT, "tests", "golden", "plnet_s1.airfe"), max_batch=B0, enc_chunk=16, max_keypoints=K, image_width=W,
                      image_height=H)
    s = scene(ctx)
    for B in ((1, 16) if quick else (1, 16, 64)):
        one_batch(ctx, s, B, reps, emit)
    ctx.close()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    arg = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d  # noqa: E731
    main(int(arg("--reps", 20)), "--quick" in sys.argv, arg("--out", None))
